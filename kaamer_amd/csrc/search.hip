// search.hip — gfx950 kernels and the C-ABI entry points of the k-mer search path.
//
// What runs on the device, per batch (all on the caller's stream, no host sync):
//
//   translate_short_kernel / translate_kernel (COUNT + WRITE) + orf_order_kernel
//                         nucleotide input only (translate.hip.inc): GetORFs (dna.go:65-181)
//                         -> ORF batch; a lane per read for reads, a wave per (sequence, frame)
//                         for longer sequences
//   prep_layout_schedule_kernel   protein input (count_group.hip.inc): Query.SizeInKmer etc.
//                         (search.go:290-293; search_protein.go:70-76), the bitmap of positions
//                         that start no k-mer, an LDS table capacity per query, the table
//                         layout E (exclusive scan), the first query of every query group and
//                         the order the groups are handed out in (longest first) -- one launch
//   prep_orf_kernel + layout_kernel + schedule_kernel    the same for an ORF batch
//   probe_kernel          the dominant kernel: flat over residue positions; sliding 7-mer
//                         encode (k_store.go:91-117, search_protein.go:94-98) and bucket
//                         probe (replaces KmerStore.Get, search.go:421) -> vals[pos]
//   count_group_kernel    (count_group.hip.inc) postings expansion + Counter increments
//                         (search.go:427-436, 442-452) in LDS hash tables, one 8-wave
//                         workgroup per query group; a wave per query packs its table into
//                         the query's hit list at E[q]
//   count_global_kernel   G tier: queries whose distinct hits exceed their LDS table count
//                         into an exactly sized table in HBM; its last workgroup finalizes
//                         the batch (counters, status, per-batch state left zeroed)
//   [scan + gather_hits_kernel]   opts.compact: hit lists -> CSR in query order
//   [positions pass]      PositionHits bitmaps when asked for
//   [topn_kernel]         kaamer_topn_device: sortMapByValue order, SetBestStartCodon,
//                         FilterResults (topn.hip.inc)
//   [response text]       behind top-N: the TSV rows, the -aln TSV rows, the JSON objects (the shared
//                         part in out_rows.hip.inc, then tsv_rows, tsv_aln_rows, json_rows.hip.inc; host
//                         side: host_out, host_tsv, host_json, host_out_text.hip.inc)
//
// This is integer hashing/indexing: no MFMA.  The probe is bound by the memory system's
// random-request rate (~51e9 requests/s on MI355X whatever the size up to 128 B,
// tools/random_read_bench.hip), i.e. ~3.3 TB/s for 64-byte buckets.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "kaamer_internal.h"
#include "gcodes.h"

// ------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int kaamer_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return kaamer_fail(KAAMER_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// what devbuf.h reports: a refused allocation of `bytes` (0: the stream wait before a regrow failed)
static int devbuf_fail(hipError_t e, size_t bytes)
{
    (void)hipGetLastError();   // a refused allocation is reported here, not by the next launch check on this thread
    if (!bytes) return kaamer_fail(KAAMER_E_HIP, "hipStreamSynchronize before a regrow failed: %s", hipGetErrorString(e));
    return kaamer_fail(KAAMER_E_NOMEM, "allocation of %zu bytes: %s", bytes, hipGetErrorString(e));
}
#include "devbuf.h"

// an event that is destroyed with its owner
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
    DevEvent &operator=(DevEvent &&o) noexcept
    {
        if (this != &o) { reset(); e = o.e; o.e = nullptr; }
        return *this;
    }
    ~DevEvent() { reset(); }
    void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
};

// the growth rules of the buffers that last from call to call
static constexpr GrowRule GROW_CALL = grow_quarter(64);            // a shard's sequences, offsets and result block (sharded handle)
static constexpr GrowRule GROW_SLOT = grow_quarter(4096);          // a host slot's staging, text and compressed bytes
static constexpr GrowRule GROW_SLOT_SEQS = grow_quarter(4096, 16); // ... its sequences (the kernels read 16 bytes past the end)
static constexpr GrowRule GROW_SLOT_OFF = grow_quarter(16, 1);     // ... its n_seqs + 1 offsets, asked for as n_seqs

// ------------------------------------------------------------------------------------
// device-side structures
// ------------------------------------------------------------------------------------
struct kaamer_workspace;
// the host-buffer calls keep their workspace and device staging buffers between calls
// (creating and freeing ~1 GB of device memory per call cost 10x the search itself)
struct HostSlot {
    kaamer_workspace *ws = nullptr;
    kaamer_workspace_opts opts{};
    DevBuf<uint8_t> d_seqs;
    DevBuf<uint64_t> d_off;
    hipStream_t stream = nullptr;   // every slot works on its own stream
    bool busy = false;              // (under kaamer_index::pool_mu)
};

// `seq_type` as every entry point takes it: the sequence type in bits 0-7, the request's genetic code in bits 8-15
// (KAAMER_SEQ_TYPE).  Workspaces, host slots and sharded sets are matched and sized by the base type alone; the code goes
// with the call into kaamer_search_device and no further.
static inline int32_t seq_base(int32_t seq_type) { return KAAMER_SEQ_TYPE_BASE(seq_type); }
static inline bool is_nucl(int32_t seq_type) { return seq_base(seq_type) == KAAMER_NUCLEOTIDE || seq_base(seq_type) == KAAMER_READS; }

// the entry points' test, before anything is enqueued or a slot is taken
static int check_seq_type(int32_t seq_type, const char *who)
{
    const int32_t base = seq_base(seq_type), code = KAAMER_SEQ_TYPE_GENETIC_CODE(seq_type);
    if ((uint32_t)seq_type >> 16) return kaamer_fail(KAAMER_E_ARG, "%s: sequence type 0x%x has bits above 15 set", who, (unsigned)seq_type);
    if (base != KAAMER_NUCLEOTIDE && base != KAAMER_PROTEIN && base != KAAMER_READS) return kaamer_fail(KAAMER_E_ARG, "%s: unknown sequence type %d", who, base);
    if (kt_gcode_slot(code) < 0) return kaamer_fail(KAAMER_E_ARG, "%s: unknown genetic code %d (one of 1-6, 9-15; 0 = table 11)", who, code);
    return KAAMER_OK;
}
#define SEQ_TYPE_CHK(seq_type, who)                        \
    do {                                                   \
        const int rc_ = check_seq_type((seq_type), (who)); \
        if (rc_) return rc_;                               \
    } while (0)

// the data-dependent bounds of a host-buffer call (0: the library's default for the input size).  The hit count of a
// batch is data dependent: a call starts from an estimate and, while the device reports KAAMER_E_CAPACITY (results are
// never partial), runs the batch again with grown bounds, at most MAX_BOUND_RETRIES times.
struct BatchBounds { uint64_t max_hits, g_slots; uint32_t max_queries; uint32_t pos_scale; /* reported-hit bitmaps: x the default rule (0 = 1) */ };
static const int MAX_BOUND_RETRIES = 6;

// where the full-list calls start (the top-N calls start from 0, the workspace's own default)
static uint64_t full_start_hits(uint64_t seq_bytes) { return seq_bytes * 8 + 65536; }

// the bitmaps of the reported hits alone (a batch that exceeded nothing else)
static void bounds_grow_positions(BatchBounds &b)
{
    b.pos_scale = b.pos_scale ? (b.pos_scale < (1u << 24) ? b.pos_scale * 4 : b.pos_scale) : 4;
}

static void bounds_grow(BatchBounds &b, uint64_t seq_bytes, uint32_t n_seqs, bool nucl)
{
    b.max_hits = b.max_hits ? b.max_hits * 4 : full_start_hits(seq_bytes);
    b.g_slots = b.g_slots ? b.g_slots * 4 : (128ull << 20);
    if (nucl) {  // hard bound: a frame of n codons holds at most n/21 + 1 ORFs
        const uint64_t hard = seq_bytes / 10 + (uint64_t)n_seqs * 6 + 64;
        b.max_queries = (uint32_t)(hard > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : hard);
    }
    bounds_grow_positions(b);
}

struct kaamer_tsv_stage;
struct kaamer_json_stage;
// the response text a text call brings back with its result (host_out_text.hip.inc); 0: none
enum OutFormat { OUT_PLAIN = 0, OUT_TSV = 1, OUT_JSON = 2, OUT_FORMATS = 3 };
// one in-flight call of the pipelined host-buffer boundary (host_top.hip.inc)
struct TopSlot {
    kaamer_workspace *ws = nullptr;
    kaamer_workspace_opts opts{};
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> d_seqs;
    DevBuf<uint64_t> d_off;
    PinnedBuf<uint8_t> h_in;   // the caller's sequences, then (8-byte aligned) its offsets
    DevBuf<uint8_t> d_block;
    size_t block_use = 0;      // bytes of d_block this call may fill: its bound (<= its capacity)
    uint64_t pos_words = 0;    // bitmap words of that bound (calls that ask for PositionHits of the reported hits)
    size_t guess = 1u << 16;   // bytes of the block copied before its size is known (adapts to the previous call)
    uint64_t aln_guess = 0;    // bytes the alignment sections of the previous call needed, plus a quarter (0: none yet)
    // the text calls (host_text.hip.inc), allocated at the slot's first one: the parser and the text's staging
    kaamer_text_parser *parser = nullptr;
    uint64_t parser_text = 0, parser_lines = 0;   // the bounds the parser was created for
    uint32_t parser_recs = 0;
    PinnedBuf<uint8_t> h_text;
    DevBuf<uint8_t> d_text;
    // the BGZF call (kaamer_search_bgzf_top_flat), allocated at the slot's first one: compressed bytes, then (8-byte
    // aligned) the block table -- pinned and device -- and the inflater
    kaamer_inflater *inflater = nullptr;
    uint64_t inflater_comp = 0;
    uint32_t inflater_blocks = 0;
    PinnedBuf<uint8_t> h_comp;
    DevBuf<uint8_t> d_comp;
    // the calls that return response text (host_out_text.hip.inc), allocated at the slot's first one of a kind: the stages
    // with the bounds they were created for, one output buffer (16 bytes more than the text may take), and per format
    // (OutFormat) the bounds the next call starts from: what the previous one needed plus a quarter
    kaamer_tsv_stage *tsv = nullptr;
    kaamer_json_stage *json = nullptr;
    uint32_t stage_queries[OUT_FORMATS] = {};
    uint64_t stage_units[OUT_FORMATS] = {};
    DevBuf<char> d_out;
    uint64_t guess_bytes[OUT_FORMATS] = {}, guess_units[OUT_FORMATS] = {};
    bool busy = false;
};
#define KAAMER_MAX_HOST_SLOTS 8
static void top_slot_free(TopSlot &h);

// protein id -> entry of an attached table (OUT_NONE, TA_NONE: no entry), dense.  The three attaches of one table share one
// map: attach_proteins always builds its own, the subject text takes the alignment table's, the JSON entries the subject
// text's or else the alignment table's -- when that attach holds the same table (host, entries) at that moment.  The buffer
// goes with its last holder, so the last reference must be dropped with the index's device selected, as aln_table_free,
// subject_free and kaamer_index_close arrange.
struct IdMap {
    DevBuf<uint32_t> d;
    uint32_t n = 0;                              // ids the map covers
    const kaamer_proteins *host = nullptr;       // the table it was built from (compared, never read)
    uint32_t entries = 0;
    bool serves(const kaamer_proteins *p, uint32_t n_entries, uint64_t map_n) const { return host == p && entries == n_entries && n == (uint32_t)map_n; }
};

// kaamer_index_attach_proteins: the device copy of the Protein.Sequence table next to the index (top_align.hip.inc)
struct AlnTable {
    const kaamer_proteins *aln_host = nullptr;   // borrowed: the rows of a result with text read the subjects from it
    DevBuf<uint8_t> d_aln_raw, d_aln_codes, d_aln_bad;
    DevBuf<uint64_t> d_aln_off;
    std::shared_ptr<IdMap> aln_idmap;
    DevBuf<int> d_aln_matrix;
    uint32_t aln_entries = 0, aln_max_ns = 0;
    uint64_t aln_bytes = 0, aln_number_of_aa = 0;
    // the *_aln_tsv_flat calls (host_tsv.hip.inc): batches whose rows the host printed because a raw score lay outside the
    // stage's table; raw scores that table holds (0: all of TSV_ALN_RAW_N -- a smaller count is for tests of that path)
    uint64_t tsv_aln_host_batches = 0;
    uint32_t tsv_aln_raw_count = 0;
};
// kaamer_index_attach_subject_text / _json: what a TSV row or a JSON object prints of a hit's entry (tsv_rows.hip.inc,
// json_rows.hip.inc), rendered on the host (host_out.hip.inc).  Entry i is d_bytes[d_off[i], ...):
//   text   up to d_off[i + 1]: EntryId (d_len[i] bytes), then the annotation columns; d_plen[i]: Protein.Length
//   JSON   d_len[i] bytes at a 16-byte boundary: the entry's HitEntries value
struct SubjectTable {
    DevBuf<uint8_t> d_bytes;
    DevBuf<uint64_t> d_off;
    DevBuf<uint32_t> d_len, d_plen;
    std::shared_ptr<IdMap> idmap;
    uint32_t entries = 0, features = 0;
    uint64_t table_bytes = 0, longest = 0;       // longest: the info calls' max_row_suffix / max_entry
};

struct kaamer_index : AlnTable {
    SubjectTable st, sj;          // the subject text, the subject entries in JSON form
    int device;
    kh_image_header hdr;
    kh_bucket *d_buckets;         // raw: taken over from the device build, or uploaded from an image
    uint32_t *d_arena;
    // kaamer_search_batch (full hit lists): a call takes a free slot (workspace + staging + stream) and gives it back;
    // callers beyond the slots wait for one.  Same pool lock as the slots below.
    HostSlot host[4];
    // kaamer_submit_batch_top / kaamer_search_batch_top / kaamer_stream_*: a pool of slots, one per call in flight
    std::mutex pool_mu;
    std::condition_variable pool_cv;
    TopSlot top[KAAMER_MAX_HOST_SLOTS];
    int n_top;
    uint64_t top_pos_words = 0;   // kaamer_index_set_top_positions_bound: first bitmap bound of the host calls (0: the rule)
    int aln_matrix[26 * 26];
    uint64_t aln_budget = 0;                     // kaamer_index_set_align_budget (0: the default)
    uint64_t aln_last[3] = {0, 0, 0};            // the last stage: resident waves, slab bytes, long waves
};

enum { ST_POOL_FULL = 1u, ST_LIST_FULL = 2u, ST_QUERY_CAP = 4u, ST_AA_CAP = 8u, ST_G_ARENA_FULL = 16u, ST_G_TABLE_FULL = 32u,
       ST_POS_UNSUPPORTED = 64u, ST_POS_CAP = 128u, ST_CHAIN_TIMEOUT = 256u, ST_EXCHANGE_CAP = 512u, ST_PEER_FAILED = 1024u,
       ST_IDS_CAP = 2048u /* an ids block of the sharded handle (top_positions_sharded.hip.inc) */,
       ST_ALN_CAP = 4096u /* pair records of kaamer_topn_align_device (top_align.hip.inc) */,
       ST_SEG_CAP = 8192u /* a subject segment of the sharded handle (top_align_sharded.hip.inc) */ };
enum { CTR_IN = 0, CTR_QUERIES, CTR_LOOKUP, CTR_PROBE, CTR_FOUND, CTR_POST, CTR_HITS, CTR_OVERFLOW, CTR_LISTS, CTR_LIST_IDS, CTR_N };
static_assert(sizeof(kaamer_counters) == CTR_N * 8, "counter layout");
#define CTR_REPLICAS 64

// work lists of the counting tiers (device memory)
enum { LIST_S = 0, LIST_L, LIST_SO, LIST_G, N_LISTS };
// small per-batch device state after the list counters (all zeroed by the finalize step)
enum { SLOT_QUEUE_HEAD = N_LISTS, SLOT_STATUS = N_LISTS + 1, SLOT_GROUP_QUEUE = N_LISTS + 2, SLOT_GROUP_QUEUE_POS = N_LISTS + 3,
       SLOT_N_LONG = N_LISTS + 4, SLOT_TILES_DONE = N_LISTS + 5, SLOT_TR_TICKET = N_LISTS + 6,
       SLOT_QUEUE_SUB = N_LISTS + 7 /* 8 words */, SLOT_G_TICKET = N_LISTS + 15, SLOT_PACK_TICKETS = N_LISTS + 16 /* 64 words */,
       SLOT_G_HITS16 = N_LISTS + 80 /* hits the G tier found, in sixteens (saturating) */,
       SLOT_G_MON_HITS16 = N_LISTS + 81 /* those of its monsters (G_MONSTER_HITS) */, SLOT_G_MONSTERS = N_LISTS + 82 /* how many monsters */,
       N_SMALL_SLOTS = N_LISTS + 16 + 64 + 3 };
// a query with more distinct hits than this fits no LDS table at any scale: it says nothing about the tables of the others
#define G_MONSTER_HITS (GRP_MAX_TABLE / 4u * 3u)
static_assert(N_SMALL_SLOTS <= 256, "the finalize step zeroes one slot per thread");
// one entry: everything a tier needs to start on a query, in one 16-byte load
struct alignas(16) WorkItem {
    uint32_t q;
    int32_t size;     // SizeInKmer
    uint64_t aa_off;  // first residue position of the query
};

#define CURSOR_STRIDE 32u  /* unsigned long long words between cursors (256 B) */
#define MAX_TIMED_CALLS 1024u
#define L_WAVES 8
#define L_LOG2CAP 12
#define G_WAVES 8
#ifndef S_MIN_WAVES
#define S_MIN_WAVES 1
#endif
#ifndef L_MIN_WAVES
#define L_MIN_WAVES 1
#endif
#ifndef S_NWIN
#define S_NWIN 3
#endif

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// wave total as a scalar (uniform) value
__device__ __forceinline__ uint32_t wave_total(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum32(v));
}

__device__ __forceinline__ void add_counter(unsigned long long *replicas, uint32_t replica, int which, unsigned long long v)
{
    if (v) atomicAdd(&replicas[(size_t)(replica % CTR_REPLICAS) * CTR_N + which], v);
}

// ====================================================================================
// Kernel P — flat probe over residue positions
// ====================================================================================
// Position i of the packed residue buffer is a k-mer start iff bit (i & 63) of
// valid[i >> 6] is set (prep clears the tail of every query and whole queries that are
// too short).  One wave handles 64 consecutive positions: residue codes are staged in
// LDS, each lane encodes its 7-mer (k_store.go:91-117 in closed form), then the wave
// probes the bucket table with 4 lanes per 64-byte bucket (16 B each, one fabric
// sector per probe) and writes one u32 per position:
//     vals[i] = 0            key absent (or position not a k-mer start)
//             = slot.val     key present: inline protein id or postings-list offset
// This replaces KmerStore.GetValueFromBadger (search.go:421) for the whole batch at
// once; the work is perfectly balanced whatever the query lengths are.
struct ProbeParams {
    const uint4 *table;  // buckets viewed as 4 x uint4 each
    uint64_t n_buckets;
    uint32_t n_shards, shard;
    const uint8_t *residues;
    unsigned long long *invalid;  // one bit per position, set = not a k-mer start; self-cleaning
    const unsigned long long *d_n_pos;  // device scalar: number of residue positions
    uint32_t *vals;
    unsigned long long *counters;
    uint32_t nontemporal;  // bucket loads bypass the caches (small batch against a large table)
};

#define P_WAVES 4
#define P_RING 128u            /* deferred lookups per wave (a power of two): fewer than 64 waiting + the 64 of a window */
#define KH_NO_KEY 0xFFFFFFFDu  /* "no lookup for this position": equals no slot key (valid keys <= 0xE773B9D4, 0xFFFFFFFF = empty) */

// SKIP_IDLE: lanes without a lookup issue no bucket load.  A nucleotide batch has one position in six that starts no
// k-mer (the gaps between ORFs); a load is a request whatever it hits, and the probe runs at the request rate of the
// memory system, so there the exec-masked loads win although their waits are coarser.  Protein batches (1.7 % idle
// positions, a few windows per wave) keep the unconditional, exactly counted loads.
template <bool SKIP_IDLE> __global__ __launch_bounds__(64 * P_WAVES) void probe_kernel(ProbeParams p)
{
    __shared__ uint8_t s_lut[256];
    __shared__ uint8_t s_stage[P_WAVES][80];
    // Lookups whose bucket is full and does not hold the key (about 2 %) go on in the NEXT bucket of the probe sequence.
    // Waiting for that second request inside the window stalls the whole wave (three windows out of four have such a
    // lookup), so they are put on a ring in LDS (key, position, buckets walked) and looked up later, 64 at a time, as an
    // iteration of their own through the same code.  The loop body is ONE straight line for both kinds of iteration, and
    // every global load and store in it is issued unconditionally (idle lanes and idle iterations touch harmless
    // addresses): the compiler's s_waitcnt vmcnt(N) then counts exactly -- a load or store inside a branch or an inner
    // loop anywhere in the body makes every wait of the loop a vmcnt(0).
    __shared__ uint32_t s_ring[P_WAVES][3][P_RING];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));  // wave-uniform: window bases stay scalar
    const unsigned long long n_pos = *p.d_n_pos;
    const unsigned long long n_win = (n_pos + 63) >> 6;
    for (uint32_t i = tid; i < 256; i += 64 * P_WAVES) s_lut[i] = (uint8_t)kh_residue_code((uint8_t)i);
    __syncthreads();  // the only workgroup barrier: the waves run independently from here on
    uint32_t c_lookup = 0, c_probe = 0, c_found = 0;
    uint8_t *stage = s_stage[wv];
    uint32_t *const ring_key = s_ring[wv][0], *const ring_pos = s_ring[wv][1], *const ring_step = s_ring[wv][2];
    uint32_t ring_head = 0, ring_n = 0;  // wave-uniform
    const uint32_t n_buckets = (uint32_t)p.n_buckets;
    const uint32_t mine = 16u * (lane & 3u) + (lane >> 2);  // the lane whose lookup this lane ends up owning (see the rounds)

    const unsigned long long stride = (unsigned long long)gridDim.x * P_WAVES;
    unsigned long long w = (unsigned long long)blockIdx.x * P_WAVES + wv;
    // the bitmap word and the residues of the NEXT window are loaded behind the bucket loads of the current one;
    // windows and reads past the end are clamped (the positions involved are marked invalid or unused)
    unsigned long long mask = 0;
    uint32_t ra = 0, rb = 0;
    auto fetch = [&](unsigned long long win, unsigned long long &m, uint32_t &a, uint32_t &b) {
        const unsigned long long wc = win < n_win ? win : n_win - 1;
        m = p.invalid[wc];
        const unsigned long long i0 = (wc << 6) + lane, last = n_pos - 1;
        a = p.residues[i0 < last ? i0 : last];
        b = p.residues[i0 + 64 < last ? i0 + 64 : last];  // lanes 0..5 hold the halo
    };
    if (n_win) fetch(w, mask, ra, rb);

    while (n_win) {
        const bool ring = ring_n >= 64u || (w >= n_win && ring_n > 0u);  // wave-uniform: this iteration serves the ring
        if (!ring && w >= n_win) break;
        unsigned long long base = 0;
        uint32_t key = KH_NO_KEY, off = lane, step = 0;
        if (ring) {
            const uint32_t n = ring_n < 64u ? ring_n : 64u;
            if (lane < n) {
                const uint32_t slot = (ring_head + lane) & (P_RING - 1u);
                key = ring_key[slot]; off = ring_pos[slot]; step = ring_step[slot];
            }
            ring_head = (ring_head + n) & (P_RING - 1u);
            ring_n -= n;
        } else {
            base = w << 6;
            stage[lane] = s_lut[ra];
            if (lane < 6) stage[64 + lane] = s_lut[rb];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint8_t *st = stage + lane;
            key = kh_key_from_codes(st[0], st[1], st[2], st[3], st[4], st[5], st[6]);
            // not a k-mer start, or (sharded index) a key another device owns: no lookup, the position reads as absent
            const bool own = p.n_shards <= 1 || kh_shard_of(key, p.n_shards) == p.shard;
            key = (((~mask >> lane) & 1ull) && own) ? key : KH_NO_KEY;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            c_lookup += key != KH_NO_KEY ? 1u : 0u;
        }
        c_probe += key != KH_NO_KEY ? 1u : 0u;
        // ---- the next regular window's inputs first (a ring iteration fetches the pending window's again): they are
        // older than the bucket loads, so waiting for the buckets covers them, and the stores at the end of the
        // iteration are younger than every load -- nothing ever waits for a store to be acknowledged
        const unsigned long long w_cur = w;
        if (!ring) w += stride;
        fetch(w, mask, ra, rb);

        // ---- issue: round j serves the lookups of lanes 16j..16j+15, four lanes per 64-byte bucket (16 B each: one
        // fabric sector per probe); nontemporal when the batch is small against the table (a bucket is then read once per
        // batch; a 1 M-read batch touches every bucket several times and wants them cached).  Every lane hashes ITS OWN key
        // once and the rounds pass the bucket index around (the hash per round was computed four times per lookup: 60 of
        // the loop's 270 VALU instructions per window).
        uint32_t my_bucket = 0u;
        if (key != KH_NO_KEY) {
            my_bucket = (uint32_t)kh_home_bucket(key, p.n_shards, p.n_buckets) + step;
            my_bucket = my_bucket >= n_buckets ? my_bucket - n_buckets : my_bucket;
        }
        uint4 ld[4];
        uint32_t rk[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int src = 16 * j + (int)(lane >> 2);
            rk[j] = __shfl(key, src, 64);
            const uint32_t bucket = __shfl(my_bucket, src, 64);
            typedef uint32_t v4u __attribute__((ext_vector_type(4)));
            const v4u *srcp = reinterpret_cast<const v4u *>(p.table) + (uint64_t)bucket * 4 + (lane & 3u);
            if (SKIP_IDLE) {
                ld[j] = make_uint4(KH_EMPTY_KEY, 0u, KH_EMPTY_KEY, 0u);
                if (rk[j] != KH_NO_KEY) {
                    const v4u t = *srcp;
                    ld[j] = make_uint4(t.x, t.y, t.z, t.w);
                }
            } else {
                const v4u t = p.nontemporal ? __builtin_nontemporal_load(srcp) : *srcp;
                ld[j] = make_uint4(t.x, t.y, t.z, t.w);
            }
        }
        // ---- consume: lane 4g+j ends up owning the lookup of lane 16j+g
        uint32_t okey = KH_NO_KEY, oval = 0, oempty = 1u;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t kk = rk[j];
            uint32_t r = (ld[j].x == kk) ? ld[j].y : ((ld[j].z == kk) ? ld[j].w : 0u);
            uint32_t e = (ld[j].x == KH_EMPTY_KEY || ld[j].z == KH_EMPTY_KEY) ? 1u : 0u;
            r |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
            e |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)e, 0xB1, 0xf, 0xf, false);
            r |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
            e |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)e, 0x4E, 0xf, 0xf, false);
            const bool take = (lane & 3u) == (uint32_t)j;
            okey = take ? kk : okey; oval = take ? r : oval; oempty = take ? e : oempty;
        }
        const uint32_t ooff = __shfl(off, (int)mine, 64);  // position of the lookup this lane owns (window offset, or absolute)
        const bool valid = okey != KH_NO_KEY;
        c_found += (valid && oval != 0u) ? 1u : 0u;
        // the key is not in this bucket and the bucket is full: the lookup goes on one bucket further, from the ring
        // (the number of buckets it has walked is fetched only here: a few windows in a hundred get this far)
        const unsigned long long W = __ballot(valid && oval == 0u && oempty == 0u);
        if (W) {  // wave-uniform; LDS only
            const uint32_t ostep = __shfl(step, (int)mine, 64);
            const bool wk = valid && oval == 0u && oempty == 0u && ostep + 1u < n_buckets;
            const unsigned long long W2 = __ballot(wk);
            if (wk) {
                const uint32_t slot = (ring_head + ring_n + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(W2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)W2, 0u))) & (P_RING - 1u);
                ring_key[slot] = okey;
                ring_pos[slot] = (uint32_t)base + ooff;  // positions fit 32 bits (checked on the host)
                ring_step[slot] = ostep + 1u;
            }
            ring_n += (uint32_t)__popcll(W2);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // one coalesced store per window: vals[i] = 0 (key absent, or not a k-mer start) or slot.val; a ring iteration
        // stores only what it found (the regular pass has already written 0 there)
        if (!ring || oval != 0u) p.vals[base + ooff] = oval;
        // leave the bitmap clean for the next batch (a ring iteration stores into the slack word behind the bitmap)
        if (lane == 0) p.invalid[ring ? n_win + 1 : w_cur] = 0ull;
    }
    const uint32_t t_lookup = wave_total(c_lookup), t_probe = wave_total(c_probe), t_found = wave_total(c_found);
    if (lane == 0) {
        const uint32_t rep = blockIdx.x * P_WAVES + wv;
        add_counter(p.counters, rep, CTR_LOOKUP, t_lookup);
        add_counter(p.counters, rep, CTR_PROBE, t_probe);
        add_counter(p.counters, rep, CTR_FOUND, t_found);
    }
}

// ====================================================================================
// Kernel C — per-query counting (postings expansion + Counter increments)
// ====================================================================================
struct QInfo;
struct CountParams {
    const uint32_t *arena;
    const uint32_t *vals;  // from kernel P, indexed like the residue buffer
    // query groups (count_group.hip.inc)
    const struct QInfo *qinfo;
    const uint64_t *slot_off;   // exclusive scan of the table capacities
    uint32_t *group_first;      // first query of each group (self-cleaning)
    const uint32_t *d_n_groups;
    const uint32_t *d_nq;
    uint32_t last_group_pass;   // this launch may clear group_first behind itself
    uint32_t pack_shift;        // count_pack_kernel: a pack = the tables that start in one window of (1 << pack_shift) slots
    uint32_t *pack_tickets;     // count_pack_kernel: PK_TICKETS counters, one per range of packs (zeroed by finalize)
    // PositionHits pass (count_group_kernel MODE 1)
    const uint64_t *pos_base;
    unsigned long long *pos_bits;
    // merge of partial hit lists (count_group_kernel MODE 2)
    const uint32_t *m_pid, *m_km, *m_fp;
    uint32_t merge_fp;  // 0: the partial entries carry no first positions
    // tier input / overflow output lists
    const WorkItem *list;
    const uint32_t *list_count;
    WorkItem *ovf_list;
    uint32_t *ovf_count;
    uint32_t list_cap;
    uint32_t *queue_head;  // workgroups of the last kernel that have finished (zeroed by finalize)
    uint32_t *group_queue; // tickets of the group kernel (zeroed by finalize)
    const uint2 *sched;    // ticket -> (group, first query), longest groups first
    const uint32_t *d_n_sched;
    // results, written straight into their final place: hits of query q are
    // [hit_off[q], hit_off[q] + q_cnt[q]) of the three SoA arrays, with hit_off[q] = E[q], the
    // first slot of the query's counting table in the batch's table layout (a table never holds
    // more distinct ids than its capacity): no allocation, no atomics.  G-tier queries (rare)
    // take space after E[n_queries] from a cursor.  An optional pass packs the lists (CSR).
    // (Measured and dropped: exact reservations on 64 cursors, +1 exposed atomic round trip and a
    // counting pass per group; an ordered layout by look-back over the groups, +30 us.)
    uint64_t *hit_off;
    uint32_t *q_cnt;
    uint32_t *hit_pid, *hit_km, *hit_fp;
    uint64_t hit_cap;                 // entries of the hit arrays
    unsigned long long *tail_cursor;  // entries handed out after E[n_queries] (G tier)
    // G tier arena
    uint32_t *g_keys;  // G-tier tables: 16-byte slots {protein id, count, lowest position, -}
    uint64_t g_slots;
    unsigned long long *g_cursor;
    uint32_t n_proteins;
    unsigned long long *counters;  // [CTR_REPLICAS][CTR_N]
    uint32_t *status;
    // set when count_global_kernel is the last kernel of the batch: its last workgroup finalizes
    kaamer_counters *fin_out;
    uint32_t *fin_small, *fin_status_out;
    uint32_t *fin_g_items;      // entries of LIST_G of this batch, kept for the host (g_tier_grid)
    unsigned long long *fin_cursors;
    uint32_t *fin_slot_scale;   // table capacity scale for the next batch (count_group.hip.inc: table_slots_for)
    uint32_t fin_scale_cap, fin_scale_margin;
};

// G-tier hit lists live after the table layout's total
__device__ __forceinline__ unsigned long long tail_alloc(const CountParams &p, uint32_t total)
{
    const unsigned long long b = p.slot_off[*p.d_nq] + atomicAdd(p.tail_cursor, (unsigned long long)total);
    if (b + total > p.hit_cap) { atomicOr(p.status, (uint32_t)ST_POOL_FULL); return ~0ull; }
    return b;
}

// counting tables: protein id -> (count, lowest matching position)
// A slot is 16 bytes {protein id, count, lowest position, -}: one memory line per table add.  As three arrays an add
// touched three random lines of a table that is megabytes large, and the tier ran at the speed of those line fills and
// write-backs (14 ms per batch on the skewed database, 53 GB of traffic).
struct GlobalTable {
    uint32_t *slots;  // 4 words per slot
    uint32_t *nd;     // nd lives in LDS
    uint32_t log2cap;
    // One workgroup owns the table (its region comes from a cursor, once per batch), so the adds are atomics at
    // WORKGROUP scope: performed in the L2 of the XCD the workgroup runs on, where the plain 16-byte stores of the
    // initialisation went (the L1 is write-through and holds no line of the table: nothing ever loads one before the
    // final read-out).
    __device__ __forceinline__ bool add_n(uint32_t pid, uint32_t pos, uint32_t n, uint32_t &nnew) const
    {
        const uint32_t mask = (1u << log2cap) - 1u;
        uint32_t h = (pid * 0x9E3779B1u) >> (32 - log2cap);
        for (uint32_t t = 0; t <= mask; t++) {
            uint32_t *sl = slots + 4ull * h;
            uint32_t k = KH_EMPTY_PID;  // expected; receives what the slot holds when it is not empty
            if (__hip_atomic_compare_exchange_strong(&sl[0], &k, pid, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                nnew++;
                k = pid;
            }
            if (k == pid) {
                __hip_atomic_fetch_add(&sl[1], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_min(&sl[2], pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                return true;
            }
            h = (h + 1u) & mask;
        }
        return false;
    }
};

// sets bits [b, e) of the not-a-k-mer-start bitmap
__device__ __forceinline__ void mark_invalid_range(unsigned long long *invalid, uint64_t b, uint64_t e)
{
    // sets bits [b, e)
    while (b < e) {
        const uint64_t w = b >> 6;
        const uint64_t hi = ((w + 1) << 6) < e ? ((w + 1) << 6) : e;
        const unsigned nb = (unsigned)(hi - b);
        const unsigned long long m = (nb == 64 ? ~0ull : ((1ull << nb) - 1ull)) << (b & 63);
        atomicOr(&invalid[w], m);
        b = hi;
    }
}

#include "count_window.hip.inc"
#include "count_group.hip.inc"
#ifndef PK_ARENA_ORF
#define PK_ARENA_ORF 640u
#endif
#define PK_ARENA_ORF_LONG 1024u  /* batches of longer sequences (mean > 200 nt): ORFs of a few hundred residues are common */
#include "count_pack.hip.inc"

// Sums the counter replicas, publishes status, and leaves every piece of per-batch device
// state zeroed for the next batch (no memsets in the steady state).  One workgroup.
// IN_FLIGHT: called by the last workgroup of a running kernel.  Everything read here was written
// with device-scope atomics (performed at the memory side), so device-scope atomic loads see
// it without an agent-scope fence -- which on this part writes back the whole L2 (a fence per
// workgroup made the kernel 30x slower).
// g_items_out: a search leaves the entry count of LIST_G there before it is zeroed (kaamer_workspace_finish reads it
// with the status: g_tier_grid); a merge passes nullptr and leaves the word alone.
template <bool IN_FLIGHT>
__device__ __forceinline__ void finalize_body(unsigned long long *replicas, kaamer_counters *out, uint32_t *small_state,
                                              uint32_t *status_out, uint32_t *g_items_out, unsigned long long *cursors,
                                              uint32_t *slot_scale = nullptr, uint32_t scale_cap = 16u, uint32_t margin_q4 = 30u)
{
    // 256 threads: lane <-> replica, wave w sums counters w, w+4, ...
    static_assert(CTR_REPLICAS == 64, "one replica per lane");
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t c = wv; c < CTR_N; c += blockDim.x >> 6) {
        unsigned long long *w = &replicas[(size_t)lane * CTR_N + c];
        unsigned long long s = IN_FLIGHT ? __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *w;
        *w = 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) ((unsigned long long *)out)[c] = s;
    }
    unsigned long long g_hits = 0, g_mon_hits = 0, g_monsters = 0;
    if (threadIdx.x == 0) {
        *status_out = IN_FLIGHT ? __hip_atomic_load(&small_state[SLOT_STATUS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : small_state[SLOT_STATUS];
        if (g_items_out) *g_items_out = IN_FLIGHT ? __hip_atomic_load(&small_state[LIST_G], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : small_state[LIST_G];
        g_hits = 16ull * (IN_FLIGHT ? __hip_atomic_load(&small_state[SLOT_G_HITS16], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : small_state[SLOT_G_HITS16]);
        g_mon_hits = 16ull * (IN_FLIGHT ? __hip_atomic_load(&small_state[SLOT_G_MON_HITS16], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : small_state[SLOT_G_MON_HITS16]);
        g_monsters = IN_FLIGHT ? __hip_atomic_load(&small_state[SLOT_G_MONSTERS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : small_state[SLOT_G_MONSTERS];
    }
    __syncthreads();
    if (threadIdx.x < N_SMALL_SLOTS) small_state[threadIdx.x] = 0;
    if (threadIdx.x < 3) cursors[threadIdx.x * CURSOR_STRIDE] = 0;  // G-tier tail cursor, G arena cursors (count, positions)
    // the next batch's counting tables: 1.5 x SizeInKmer x (distinct proteins per k-mer of THIS batch x the margin), never
    // below 1.5 x SizeInKmer, never above scale_cap (8); the prep kernel of the next batch cuts it to what that batch's
    // positions leave room for in the hit arrays (fit_table_scale)
    if (slot_scale && threadIdx.x == 0) {
        // (written by this workgroup, above).  Queries that left their LDS table are left out on both sides: on a skewed
        // database a few monsters with tens of thousands of hits say nothing about the tables of the others, and tables
        // 1.3 x larger for everybody cost the group kernel more than the few G-tier queries they save (measured: + 13 %
        // per batch on --db zipf).  Unless MANY queries left a table that a larger one would have held (more than an
        // eighth of the batch, the monsters -- more distinct hits than the largest LDS table holds -- not counted): reads
        // whose one coding frame finds all the hits, a dense database at scale 1.  Then only the monsters are left out
        const unsigned long long nq = out->n_queries;
        const unsigned long long n_ovf = out->n_overflow < nq ? out->n_overflow : nq;
        const unsigned long long n_mon = g_monsters < n_ovf ? g_monsters : n_ovf;
        const bool widen = 8ull * (n_ovf - n_mon) > nq;
        const unsigned long long ovf = widen ? n_mon : n_ovf;
        const unsigned long long left_out = widen ? g_mon_hits : g_hits;
        const unsigned long long hits = out->n_hits > left_out ? out->n_hits - left_out : 0ull;
        const unsigned long long lookups = nq ? out->n_lookup / nq * (nq - ovf) + out->n_lookup % nq * (nq - ovf) / nq : 0ull;
        if (lookups) {
            unsigned long long t = (hits * margin_q4 + lookups - 1ull) / lookups;   // sixteenths: 16 x hits / lookups x margin / 16
            if (t < 24ull) t = 16ull;   // (below 1.5 the tables' own slack covers it; measured on the skewed database: a scale
                                        // of ~1.3 cost the group kernel 7 % and saved a tenth of the G-tier queries)
            if (t > scale_cap) t = scale_cap;
            *slot_scale = (uint32_t)t;
        }
    }
}

#include "count_global.hip.inc"

#include "translate.hip.inc"
#include "topn.hip.inc"
#include "top_positions.hip.inc"
#include "top_align.hip.inc"
#include "out_rows.hip.inc"
#include "tsv_rows.hip.inc"
#include "tsv_aln_rows.hip.inc"
#include "json_rows.hip.inc"

// ------------------------------------------------------------------------------------
// exclusive scan of q_cnt[0..nq) -> hit_off[0..nq]
// ------------------------------------------------------------------------------------
#define SCAN_BLOCK 1024
#define SCAN_ITEMS 16
#define SCAN_TILE (SCAN_BLOCK * SCAN_ITEMS)
#define SCAN_SINGLE_MAX (8 * (uint64_t)SCAN_TILE)   // the greatest bound scan_u32_on gives to the one-workgroup form

__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t *total)
{
    __shared__ uint64_t s_w[SCAN_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint64_t t = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint64_t woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < SCAN_BLOCK / 64; i++) {
        if (i < (int)w) woff += s_w[i];
        tot += s_w[i];
    }
    *total = tot;
    return woff + inc - v;
}

// one block walks all tiles with a carry: one launch, for batches of up to ~1e5 queries
__global__ __launch_bounds__(SCAN_BLOCK) void scan_single_kernel(const uint32_t *cnt, const uint32_t *d_nq, uint64_t *hit_off)
{
    const uint32_t nq = *d_nq;
    uint64_t carry = 0;
    for (uint64_t base = 0; base <= nq; base += SCAN_TILE) {
        uint32_t v[SCAN_ITEMS];
        uint64_t s = 0;
#pragma unroll
        for (int i = 0; i < SCAN_ITEMS; i++) {
            const uint64_t idx = base + (uint64_t)threadIdx.x * SCAN_ITEMS + i;
            v[i] = idx < nq ? cnt[idx] : 0u;
            s += v[i];
        }
        uint64_t tot;
        uint64_t ex = block_exclusive_scan(s, &tot) + carry;
#pragma unroll
        for (int i = 0; i < SCAN_ITEMS; i++) {
            const uint64_t idx = base + (uint64_t)threadIdx.x * SCAN_ITEMS + i;
            if (idx <= nq) hit_off[idx] = ex;
            ex += v[i];
        }
        carry += tot;
        __syncthreads();
    }
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_block_sums_kernel(const uint32_t *cnt, const uint32_t *d_nq,
                                                                    uint64_t *bsum)
{
    const uint32_t nq = *d_nq;
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    if (base > nq) { if (threadIdx.x == 0) bsum[blockIdx.x] = 0; return; }
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        const uint64_t idx = base + (uint64_t)threadIdx.x * SCAN_ITEMS + i;
        if (idx < nq) s += cnt[idx];
    }
    uint64_t tot;
    block_exclusive_scan(s, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_top_kernel(uint64_t *bsum, uint32_t n_blocks)
{
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += SCAN_BLOCK) {
        const uint32_t i = b0 + threadIdx.x;
        const uint64_t v = i < n_blocks ? bsum[i] : 0;
        uint64_t tot;
        const uint64_t ex = block_exclusive_scan(v, &tot);
        if (i < n_blocks) bsum[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_apply_kernel(const uint32_t *cnt, const uint32_t *d_nq,
                                                               const uint64_t *bsum, uint64_t *hit_off)
{
    const uint32_t nq = *d_nq;
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    if (base > nq) return;
    uint32_t v[SCAN_ITEMS];
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        const uint64_t idx = base + (uint64_t)threadIdx.x * SCAN_ITEMS + i;
        v[i] = idx < nq ? cnt[idx] : 0u;
        s += v[i];
    }
    uint64_t tot;
    uint64_t ex = block_exclusive_scan(s, &tot) + bsum[blockIdx.x];
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; i++) {
        const uint64_t idx = base + (uint64_t)threadIdx.x * SCAN_ITEMS + i;
        if (idx <= nq) hit_off[idx] = ex;  // index nq receives the grand total
        ex += v[i];
    }
}

#include "exchange.hip.inc"
#include "top_positions_sharded.hip.inc"
#include "top_align_sharded.hip.inc"

// optional compaction: sharded hit arrays -> CSR in query order (one wave per query)
__global__ __launch_bounds__(256) void gather_hits_kernel(const uint32_t *d_nq, const uint64_t *csr_off, const uint64_t *hit_off,
                                                          const uint32_t *q_cnt, const uint32_t *in_pid, const uint32_t *in_km,
                                                          const uint32_t *in_fp, uint32_t *out_pid, uint32_t *out_km,
                                                          uint32_t *out_fp, uint64_t out_cap, uint32_t *status, int firstpos)
{
    const uint32_t nq = *d_nq;
    const uint64_t n_hits = csr_off[nq];
    if (n_hits > out_cap) { if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, (uint32_t)ST_POOL_FULL); return; }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t q = wave; q < nq; q += n_waves) {
        const uint32_t n = q_cnt[q];
        if (n == 0) continue;
        const uint64_t s = hit_off[q], d = csr_off[q];
        for (uint32_t i = lane; i < n; i += 64) {
            out_pid[d + i] = in_pid[s + i];
            out_km[d + i] = in_km[s + i];
            if (firstpos) out_fp[d + i] = in_fp[s + i];
        }
    }
}

__global__ void finalize_kernel(unsigned long long *replicas, kaamer_counters *out, uint32_t *small_state,
                                uint32_t *status_out, uint32_t *g_items_out, unsigned long long *cursors, uint32_t *slot_scale,
                                uint32_t scale_cap, uint32_t margin_q4)
{
    finalize_body<false>(replicas, out, small_state, status_out, g_items_out, cursors, slot_scale, scale_cap, margin_q4);
}

// ------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------
struct kaamer_workspace {
    int device = 0;
    kaamer_workspace_opts opts{};
    uint32_t q_cap = 0;
    uint64_t hit_cap = 0, sparse_cap = 0, g_slots = 0, pos_cap = 0;
    bool compact = false;               // finish with CSR in query order (scan + gather pass)
    DevBuf<uint64_t> d_csr_off;         // compact form: CSR offsets
    DevBuf<uint32_t> d_c_pid, d_c_km, d_c_fp;
    int g_grid = 0, p_grid = 0, n_cu = 0, pack_grid = 0, pack_grid_long = 0;
    uint32_t pack_shift = 0;            // log2 of the group / pack window (slots) of a search: 12 for protein, 9 for ORF batches
    int wide_reads = 0;                 // lane-per-read kernel: 1 the wide one, 0 the narrow one, -1 picked from the mean read length
    bool pack_long = false;             // ORF batches always take the pack kernel's larger arena
    // device buffers
    DevBuf<kaamer_query_meta> d_q;
    DevBuf<uint32_t> d_nq;
    DevBuf<unsigned long long> d_n_pos;
    DevBuf<unsigned long long> d_valid;        // one bit per residue position
    DevBuf<uint32_t> d_vals;                   // probe result per residue position
    DevBuf<uint32_t> d_q_cnt;
    DevBuf<unsigned long long> d_pool_cursor;  // CURSOR_STRIDE apart: G-tier tail cursor, G arena cursor (count), G arena cursor (positions)
    DevBuf<WorkItem> d_lists;                  // [N_LISTS][q_cap] (only the G tier's overflow list is used)
    DevBuf<QInfo> d_qinfo;
    DevBuf<uint32_t> d_slots;
    DevBuf<uint64_t> d_slot_off;
    DevBuf<uint32_t> d_group_first;
    DevBuf<uint32_t> d_n_groups;
    uint32_t groups_cap = 0;
    // the counting stage on a stream of its own (kaamer_workspace_set_count_stream): the caller's stream then carries
    // prep + probe only, so that the probe kernel of batch i + 1 starts while batch i is still counting
    hipStream_t count_stream = nullptr;
    DevEvent ev_probe, ev_count;
    bool split_pending = false;         // the last search's counting stage is on count_stream: consumers wait for ev_count
    int grp_grid = 0;
    // nucleotide / reads input: 6-frame translation products
    bool nucleotide = false;
    uint64_t aa_cap = 0, sa_cap = 0;
    DevBuf<uint32_t> d_cnt3;            // [3][6*max_seqs] ORF / aa / starts counts per (sequence, frame)
    DevBuf<uint64_t> d_off3;            // [3][6*max_seqs+1] their exclusive scans
    DevBuf<uint32_t> d_n6;              // device scalar 6*n_seqs
    // long sequences (> TS_MAX nt) are translated piece-wise: list, pieces per frame, per-piece counts and their scans
    uint32_t max_long = 0;
    uint64_t max_piece_items = 0;
    DevBuf<uint32_t> d_long_seq, d_long_np, d_pcnt3, d_n_piece_items, d_piece_li;
    DevBuf<uint64_t> d_piece_base, d_poff3;
    DevBuf<kaamer_query_meta> d_tmp_meta;
    DevBuf<uint8_t> d_orf_aa;
    DevBuf<int32_t> d_starts_alt;
    uint32_t max_seqs = 0;
    DevBuf<unsigned long long> d_chain;        // layout_kernel: one word per tile, tagged with the batch epoch
    DevBuf<uint2> d_sched;                     // schedule_kernel: ticket -> (group, first query)
    DevBuf<uint64_t> d_group_start;            // layout_kernel: slot at which the group's first table starts
    DevBuf<unsigned long long> d_lay_total;    // total table slots of the batch
    DevBuf<uint32_t> d_slot_scale;             // table capacity scale of the next batch, sixteenths (finalize_body)
    uint32_t slot_scale_cap = 0;        // ceiling of the scale (8: beyond it the tables leave the pack kernel's arena)
    unsigned long long table_room = 0;  // slots of the hit arrays a batch's tables may take (the G tier's lists come after them)
    uint32_t slot_scale_margin = 0;     // sixteenths: tables of (hits per k-mer) x this
    bool dense_tables = false;          // the last finished batch left a table scale of 2 or more: ORF packs take the larger arena
    DevBuf<uint32_t> d_n_sched;
    // post-steps (kaamer_topn_device), allocated on first use
    uint32_t topn_k = 0;
    DevBuf<uint32_t> d_top_cnt, d_top_pid, d_top_km, d_top_fp;
    DevBuf<int32_t> d_top_trim, d_top_start, d_top_size;
    bool last_was_merge = false;
    // PositionHits of the reported hits (kaamer_topn_positions_device), allocated on first use
    DevBuf<uint32_t> d_tp_words;
    DevBuf<int32_t> d_tp_len;
    DevBuf<uint64_t> d_tp_base;
    DevBuf<unsigned long long> d_tp_bits;      // grow-only
    // alignment of the reported hits (top_align.hip.inc), allocated on first use, grow-only
    const uint8_t *last_seqs = nullptr; // the batch input of the last search (protein queries are aligned from it)
    DevBuf<uint8_t> d_ta_qcodes;        // the queries' letter codes, by residue position
    DevBuf<TaLayout> d_ta_lay;
    DevBuf<unsigned long long> d_ta_ctr;
    DevBuf<uint64_t> d_ta_eoff;         // device-resident form: its own scan of top_cnt
    DevBuf<kaamer_align_pair> d_ta_items;      // ... and its pair records
    DevBuf<uint8_t> d_ta_dirs, d_ta_ops, d_ta_ldirs, d_ta_lops;   // per resident wave: direction slab, operations (wave / long form)
    DevBuf<int> d_ta_lbnd;
    XState x;                           // exchange step of the sharded index (kaamer_exchange_pack / _merge; exchange.hip.inc)
    // reported-only packing of the top-N results (kaamer_search_batch_top), allocated on first use
    DevBuf<uint32_t> d_rep_flag, d_rep_aalen;
    DevBuf<uint64_t> d_rep_rank, d_rep_eoff, d_rep_aoff;
    uint32_t lay_epoch = 0;
    DevBuf<unsigned long long> d_tr_chain;     // translate_reads_kernel: three words per 64-sequence chunk, tagged with tr_epoch
    uint32_t tr_epoch = 0;
    DevBuf<uint32_t> d_list_counts;     // [N_LISTS] + queue head + status (zeroed by finalize)
    DevBuf<uint32_t> d_status_out;      // status of the last finished batch; the word after it: its LIST_G entries (a search's)
    int64_t g_last = 0;                 // LIST_G entries of the last batch kaamer_workspace_finish looked at, or G_LAST_UNKNOWN
    int g_floor = 0;                    // workgroups of a G-tier launch behind a batch that had none (g_tier_grid)
    bool clean = false;                 // per-batch device state is known to be zeroed
    bool firstpos = false;              // track the lowest matching position per hit
    bool want_positions = false;        // full PositionHits bitmaps
    uint64_t bits_cap = 0;              // u64 words of bitmap storage
    DevBuf<uint32_t> d_pos_words;       // per query: hits x words per hit
    DevBuf<uint64_t> d_pos_base;        // exclusive scan of the above
    DevBuf<uint64_t> d_pos_off;         // per hit: first word of its bitmap
    DevBuf<unsigned long long> d_pos_bits;
    DevBuf<uint32_t> d_g_keys;
    DevBuf<unsigned long long> d_counter_replicas;
    DevBuf<kaamer_counters> d_counters;
    DevBuf<uint64_t> d_bsum;
    uint32_t n_scan_blocks = 0;
    DevBuf<uint64_t> d_hit_off;
    DevBuf<uint32_t> d_hit_pid, d_hit_km, d_hit_fp;
    std::vector<hipEvent_t> ev;  // 5 events per timed call: total0, probe0, probe1(=count0), count1, total1
    uint32_t n_timed = 0, time_every = 0, call_no = 0;

    // the device is selected before any member goes (a destructor's body runs before its members' destructors)
    ~kaamer_workspace()
    {
        (void)hipSetDevice(device);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};
#define EV_PER_CALL 5
#define G_LAST_UNKNOWN (-1)

static void launch_group(const CountParams &p, int grid, bool firstpos, hipStream_t s)
{
    if (firstpos) hipLaunchKernelGGL((count_group_kernel<true, 0>), dim3(grid), dim3(64 * GRP_WAVES), 0, s, p);
    else hipLaunchKernelGGL((count_group_kernel<false, 0>), dim3(grid), dim3(64 * GRP_WAVES), 0, s, p);
}
static void launch_group_positions(const CountParams &p, int grid, hipStream_t s)
{
    hipLaunchKernelGGL((count_group_kernel<false, 1>), dim3(grid), dim3(64 * GRP_WAVES), 0, s, p);
}
static void launch_group_merge(const CountParams &p, int grid, bool firstpos, hipStream_t s)
{
    // without first positions the merge tables need no third array: three workgroups per CU instead of two
    if (firstpos) hipLaunchKernelGGL((count_group_kernel<true, 2>), dim3(grid), dim3(64 * GRP_WAVES), 0, s, p);
    else hipLaunchKernelGGL((count_group_kernel<false, 2>), dim3(grid), dim3(64 * GRP_WAVES), 0, s, p);
}

// exclusive scan of cnt[0..*d_count) -> off[0..*d_count]; bound: host-side bound of *d_count (which launch, grid sizing)
static void scan_u32_on(kaamer_workspace *ws, const uint32_t *cnt, const uint32_t *d_count, uint64_t bound, uint64_t *off, hipStream_t s)
{
    if (bound <= SCAN_SINGLE_MAX) {
        hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(SCAN_BLOCK), 0, s, cnt, d_count, off);
    } else {
        const uint32_t nsb = (uint32_t)((bound + 1 + SCAN_TILE - 1) / SCAN_TILE);
        hipLaunchKernelGGL(scan_block_sums_kernel, dim3(nsb), dim3(SCAN_BLOCK), 0, s, cnt, d_count, ws->d_bsum);
        hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_BLOCK), 0, s, ws->d_bsum, nsb);
        hipLaunchKernelGGL(scan_apply_kernel, dim3(nsb), dim3(SCAN_BLOCK), 0, s, cnt, d_count, ws->d_bsum, off);
    }
}

// a workspace that is not `clean` (first batch, or a batch that did not run to its finalize kernel) back to the
// per-batch zero state; what becomes of ws->clean is the caller's business
static int ws_reset_if_dirty(kaamer_workspace *ws, hipStream_t s)
{
    if (ws->clean) return KAAMER_OK;
    ws->g_last = G_LAST_UNKNOWN;   // (whatever ran last did not end as a batch does: it says nothing about the next one)
    HIPCHK(hipMemsetAsync(ws->d_pool_cursor, 0, (size_t)3 * CURSOR_STRIDE * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(ws->d_list_counts, 0, N_SMALL_SLOTS * sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(ws->d_counter_replicas, 0, sizeof(unsigned long long) * CTR_REPLICAS * CTR_N, s));
    HIPCHK(hipMemsetAsync(ws->d_valid, 0, (size_t)(ws->pos_cap / 64 + 2) * sizeof(unsigned long long), s));
    return KAAMER_OK;
}

static WorkItem *ws_list(const kaamer_workspace *ws, int which) { return ws->d_lists + (size_t)which * ws->q_cap; }

// what every counting launch of a search and of a merge shares: group / schedule arrays, hit arrays, cursors, G-tier arena,
// counters, status.  Everything else is zero.
static CountParams count_params_base(const kaamer_workspace *ws)
{
    CountParams p;
    memset(&p, 0, sizeof p);
    p.qinfo = ws->d_qinfo;
    p.slot_off = ws->d_slot_off;
    p.group_first = ws->d_group_first;
    p.sched = ws->d_sched;
    p.d_n_sched = ws->d_n_sched;
    p.d_n_groups = ws->d_n_groups;
    p.d_nq = ws->d_nq;
    p.list_cap = ws->q_cap;
    p.group_queue = ws->d_list_counts + SLOT_GROUP_QUEUE;
    p.hit_off = ws->d_hit_off;
    p.q_cnt = ws->d_q_cnt;
    p.hit_pid = ws->d_hit_pid;
    p.hit_km = ws->d_hit_km;
    p.hit_fp = ws->d_hit_fp;
    p.hit_cap = ws->sparse_cap;
    p.tail_cursor = ws->d_pool_cursor;
    p.g_keys = ws->d_g_keys;
    p.g_slots = ws->g_slots;
    p.g_cursor = ws->d_pool_cursor + CURSOR_STRIDE;
    p.counters = ws->d_counter_replicas;
    p.status = ws->d_list_counts + SLOT_STATUS;
    return p;
}

// workgroups of a group-kernel launch over nq tables that hold `items` items in all
static int group_grid(const kaamer_workspace *ws, uint64_t nq, uint64_t items)
{
    const uint64_t g = ((uint64_t)GRP_MIN_TABLE * nq + 3 * items) / GRP_BUDGET + 1;
    return (int)(g > (uint64_t)ws->grp_grid ? (uint64_t)ws->grp_grid : g);
}

// workgroups of a G-tier launch: never more than queries.
// hinted (the G-tier launches of a search): behind a finished batch that sent nothing to the G tier the launch is cut to
// g_floor workgroups (KAAMER_G_FLOOR, shipped: 1).  The kernels are exact at any grid (items go out by ticket, the
// completion count is over the workgroups that take part); every workgroup of the grid has to be PLACED, 80 KB of LDS
// and 8 waves each, and next to the neighbouring batches' kernels the last of them is placed late: with three protein
// batches in flight on DB-SP the empty launch lasts 55-58 us at the full grid and at floors of 16, 32 and 64, 49.5 us at
// 1 (6 us alone; the one workgroup still waits for its 80 KB), and the batch takes 0.1287 instead of 0.1309 ms
// (profiles/r17_gtier_grid.md).  The price is a batch that overflows after a clean one: the floor's workgroups count
// its items alone.  A --db zipf-mid batch (10 000 queries, 7 items) behind a clean one: 0.756 ms at floor 1 against
// 0.605 ms at the full grid, once -- the batch after it is sized from a count above zero.
static int g_tier_grid(const kaamer_workspace *ws, uint32_t nq_bound, bool hinted = false)
{
    int g = ws->g_grid;
    if (hinted && ws->g_last == 0 && ws->g_floor < g) g = ws->g_floor;
    return (uint32_t)g > nq_bound ? (nq_bound > 0 ? (int)nq_bound : 1) : g;
}

// epochs of the chained-tile kernels: 24 bits, never 0
static uint32_t next_epoch(uint32_t &e)
{
    e = (e + 1u) & 0xFFFFFFu;
    if (e == 0) e = 1;
    return e;
}

// The search's environment knobs (tools/README.md), read where a workspace or an index is created and nowhere on the
// per-batch path (a host that calls in through cgo may setenv on another thread).  A knob that is not set leaves the
// shipped value.
struct SearchKnobs {
    int grp_per_cu, p_per_cu, pack_per_cu;  // workgroups per CU of the counting / probe / pack kernels (0: as many as fit)
    int wide_reads;                         // lane-per-read kernel: 1 the wide one, 0 the narrow one, -1 picked per batch
    uint32_t slot_scale_cap;                // ceiling of the table scale, sixteenths
    uint32_t slot_scale_margin;             // sixteenths: tables of (hits per k-mer) x this
    bool pack_long;                         // ORF batches always take the pack kernel's larger arena
    bool ws_trace;                          // a workspace prints its sizes when it is created
    int host_slots;                         // calls in flight through the host-buffer boundary
    int g_floor;                            // G-tier workgroups behind a batch without G-tier items (0: the shipped 1)
};

static SearchKnobs read_knobs()
{
    auto num = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : 0; };
    SearchKnobs k;
    k.grp_per_cu = num("KAAMER_GRP_PER_CU");
    k.p_per_cu = num("KAAMER_P_PER_CU");
    k.pack_per_cu = num("KAAMER_PACK_PER_CU");
    const char *e = getenv("KAAMER_WIDE_READS");
    k.wide_reads = e ? atoi(e) != 0 : -1;
    // (never above 8: at 3e9 residues on one device, 6.6 hits per k-mer, tables of 12 x 1.5 x SizeInKmer leave the pack
    // kernel's arena and the batch takes 92 ms instead of 44; profiles/r03_dense_database.md)
    double cap = 128.0;
    if ((e = getenv("KAAMER_SLOT_SCALE_MAX"))) cap = atof(e) * 16.0;
    k.slot_scale_cap = cap < 16.0 ? 16u : cap > 128.0 ? 128u : (uint32_t)cap;
    k.slot_scale_margin = 30u;   // x 1.9: the hits of a query spread around the batch's mean (measured on DB-UR-lite: 1.2 -> 22.8 ms per
                                 // batch, 1.5 -> 13.9, 1.9 -> 11.9; profiles/r03_dense_database.md)
    if ((e = getenv("KAAMER_SLOT_MARGIN"))) k.slot_scale_margin = (uint32_t)(atof(e) * 16.0);
    k.pack_long = getenv("KAAMER_PACK_LONG") != nullptr;
    k.ws_trace = getenv("KAAMER_WS_TRACE") != nullptr;
    const int hs = num("KAAMER_HOST_SLOTS");
    k.host_slots = hs >= 1 && hs <= KAAMER_MAX_HOST_SLOTS ? hs : 4;
    const int gf = num("KAAMER_G_FLOOR");
    k.g_floor = gf >= 1 ? gf : 0;
    return k;
}

// the attached Protein.Sequence table goes (kaamer_index_attach_proteins, kaamer_index_close; the device is selected)
static void aln_table_free(kaamer_index *ix) { static_cast<AlnTable &>(*ix) = AlnTable(); }

// ... and an attached subject table (ix->st, ix->sj)
static void subject_free(SubjectTable &t) { t = SubjectTable(); }

#include "parse_text.hip.inc"
#include "parse_fasta.hip.inc"
#include "makedb_fasta.hip.inc"
#include "makedb_tsv.hip.inc"
#include "makedb_embl.hip.inc"
#include "makedb_gbk.hip.inc"
#include "inflate.hip.inc"

extern "C" {

const char *kaamer_last_error(void) { return g_err; }
int kaamer_abi_version(void) { return KAAMER_ABI_VERSION; }

#ifdef KAAMER_PHASE_CLOCK
// measurement build only: the phase clocks of count_group_kernel<., 0> since the last reset
// per-workgroup clocks of count_global_kernel: out[b * 16 + i]
int kaamer_debug_gtier_clock(unsigned long long *out, int reset)
{
    HIPCHK(hipDeviceSynchronize());
    static unsigned long long all[2048][16];
    HIPCHK(hipMemcpyFromSymbol(all, HIP_SYMBOL(g_gtier_clock), sizeof all));
    memcpy(out, all, sizeof all);
    if (reset) { memset(all, 0, sizeof all); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_gtier_clock), all, sizeof all)); }
    return KAAMER_OK;
}
int kaamer_debug_phase_clock(unsigned long long out[16], int reset)
{
    HIPCHK(hipDeviceSynchronize());
    static unsigned long long all[2048][16];
    HIPCHK(hipMemcpyFromSymbol(all, HIP_SYMBOL(g_phase_clock), sizeof all));
    for (int i = 0; i < 16; i++) { out[i] = 0; for (int b = 0; b < 2048; b++) out[i] += all[b][i]; }
    if (reset) { memset(all, 0, sizeof all); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_clock), all, sizeof all)); }
    return KAAMER_OK;
}
#endif

int kaamer_index_open_image(const kaamer_image *img, int device, kaamer_index **out)
{
    if (!img || !out) return kaamer_fail(KAAMER_E_ARG, "index_open_image: bad argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(device));
    kaamer_index *ix = new (std::nothrow) kaamer_index();
    if (!ix) return kaamer_fail(KAAMER_E_NOMEM, "index alloc");
    ix->device = device;
    ix->n_top = read_knobs().host_slots;
    ix->hdr = img->hdr;
    DevBuf<kh_bucket> buckets;
    DevBuf<uint32_t> arena;
    const int rc = reserve_group(nullptr, GROW_EXACT, { want(buckets, (size_t)img->hdr.n_buckets),
                                                        want(arena, (size_t)(img->hdr.arena_words < 4 ? 4 : img->hdr.arena_words)) });
    ix->d_buckets = buckets.release();
    ix->d_arena = arena.release();
    if (rc) { kaamer_index_close(ix); return rc; }
    hipError_t e = hipMemcpy(ix->d_buckets, img->buckets, (size_t)img->hdr.n_buckets * sizeof(kh_bucket), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_arena, img->arena, (size_t)img->hdr.arena_words * 4, hipMemcpyHostToDevice);
    // list offset 0 is never handed out (kaamer_layout.h) and reads as "no list": the counting kernel loads it for
    // positions without a list instead of branching around the load (count_pack.hip.inc)
    if (e == hipSuccess) e = hipMemset(ix->d_arena, 0, 16);
    if (e != hipSuccess) { kaamer_index_close(ix); return kaamer_fail(KAAMER_E_HIP, "index upload: %s", hipGetErrorString(e)); }
    *out = ix;
    return KAAMER_OK;
}

// makedb -> serving without an image file in between: the table is built on the device it will be searched on
int kaamer_index_build_proteins(const uint8_t *seqs, const uint64_t *offsets, const uint32_t *ids, uint32_t n_proteins,
                                uint32_t shard, uint32_t n_shards, double load_factor, int device, kaamer_index **out)
{
    if (!out || !offsets || (!seqs && n_proteins) || n_shards == 0 || shard >= n_shards)
        return kaamer_fail(KAAMER_E_ARG, "index_build_proteins: bad argument");
    *out = nullptr;
    kaamer_device_image di;
    const int rc = kaamer_build_on_device(seqs, offsets, ids, n_proteins, shard, n_shards, load_factor, device, &di);
    if (rc) return rc;
    return index_of_device_image(di, device, out);
}

int kaamer_index_open(const char *path, int device, kaamer_index **out)
{
    kaamer_image *img = nullptr;
    int rc = kaamer_image_load(path, &img);
    if (rc) return rc;
    rc = kaamer_index_open_image(img, device, out);
    kaamer_image_free(img);
    return rc;
}

void kaamer_index_close(kaamer_index *ix)
{
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    {   // calls still in flight (a ticket not yet waited for, a caller inside kaamer_search_batch) keep their slot busy:
        // the close waits for them to be given back, then for every slot's stream
        std::unique_lock<std::mutex> lock(ix->pool_mu);
        for (;;) {
            bool busy = false;
            for (const HostSlot &h : ix->host) busy = busy || h.busy;
            for (int i = 0; i < ix->n_top; i++) busy = busy || ix->top[i].busy;
            if (!busy) break;
            ix->pool_cv.wait(lock);
        }
    }
    for (TopSlot &h : ix->top) if (h.stream) (void)hipStreamSynchronize(h.stream);
    for (HostSlot &h : ix->host) {
        if (h.stream) (void)hipStreamSynchronize(h.stream);
        if (h.stream) (void)hipStreamDestroy(h.stream);
        if (h.ws) kaamer_workspace_free(h.ws);
    }
    for (TopSlot &h : ix->top) top_slot_free(h);
    if (ix->d_buckets) (void)hipFree(ix->d_buckets);   // (raw: see kaamer_index)
    if (ix->d_arena) (void)hipFree(ix->d_arena);
    delete ix;   // the slots' buffers and the attached tables go with it: the device is still selected
}

int kaamer_index_get_stats(const kaamer_index *ix, kaamer_image_stats *out)
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "index_get_stats: bad argument");
    kaamer_stats_from_header(&ix->hdr, out);
    return KAAMER_OK;
}

void kaamer_workspace_free(kaamer_workspace *ws) { delete ws; }

uint32_t kaamer_workspace_query_capacity(const kaamer_workspace *ws) { return ws ? ws->q_cap : 0u; }

void kaamer_scan_geometry(uint32_t out[4])
{
    if (!out) return;
    out[0] = SCAN_BLOCK; out[1] = SCAN_ITEMS; out[2] = SCAN_TILE; out[3] = (uint32_t)SCAN_SINGLE_MAX;
}

int kaamer_workspace_create(kaamer_index *ix, const kaamer_workspace_opts *opts, kaamer_workspace **out)
{
    if (!ix || !opts || !out) return kaamer_fail(KAAMER_E_ARG, "workspace_create: bad argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(ix->device));
    kaamer_workspace *ws = new (std::nothrow) kaamer_workspace();
    if (!ws) return kaamer_fail(KAAMER_E_NOMEM, "workspace alloc");
    ws->device = ix->device;
    ws->opts = *opts;
    ws->opts.seq_type = seq_base(opts->seq_type);   // a workspace serves every genetic code: the code is the call's
    ws->nucleotide = is_nucl(opts->seq_type);
    ws->max_seqs = opts->max_seqs ? opts->max_seqs : 1;
    if (ws->nucleotide) {
        // six frames of len/3 codons: at most 2 amino acids per nucleotide, an ORF needs >= 21 of them
        ws->aa_cap = 2 * opts->max_seq_bytes + 64;
        ws->sa_cap = ws->aa_cap;
        uint64_t qc = opts->max_queries ? opts->max_queries : (uint64_t)ws->max_seqs * 4 + opts->max_seq_bytes / 32 + 64;
        if (qc > 0xFFFFFFF0ull) qc = 0xFFFFFFF0ull;
        ws->q_cap = (uint32_t)qc;
        ws->pos_cap = ws->aa_cap + 64;
    } else {
        // one query per protein record: never fewer slots than sequences (the prep kernel writes one
        // descriptor per sequence)
        ws->q_cap = opts->max_queries > ws->max_seqs ? opts->max_queries : ws->max_seqs;
        ws->pos_cap = opts->max_seq_bytes + 64;
    }
    if (ws->q_cap < 1) ws->q_cap = 1;
    // default bound of the (query, protein) pairs: 256 per query, but never more than one per residue position (an ORF
    // batch has millions of queries of ~40 positions: 256 each sized a 1 M-read workspace at 67 GB of hit arrays)
    ws->hit_cap = opts->max_hits ? opts->max_hits : std::min<uint64_t>((uint64_t)ws->q_cap * 256, ws->pos_cap) + (1u << 20);
    ws->g_slots = opts->g_tier_slots ? opts->g_tier_slots : (32ull << 20);
    {
        // hit arrays: the lists sit at the table layout's offsets (<= 1.5 x positions + 64 per query;
        // for a merge the "positions" are partial entries), G-tier lists after them
        const uint64_t items = ws->pos_cap > ws->hit_cap ? ws->pos_cap : ws->hit_cap;
        ws->sparse_cap = items + items / 2 + 64ull * ws->q_cap + GRP_MAX_TABLE + ws->hit_cap / 2 + (1u << 20);
    }
    // the reference fills PositionHits only for nucleotide/reads input or with -pos (search.go:416)
    ws->firstpos = opts->first_pos == 1 || (opts->first_pos == 0 && is_nucl(opts->seq_type));
    const SearchKnobs knobs = read_knobs();
    int grp_per_cu = 0, p_per_cu = 0;
    hipError_t oe = ws->firstpos ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&grp_per_cu, count_group_kernel<true, 0>, 64 * GRP_WAVES, 0)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&grp_per_cu, count_group_kernel<false, 0>, 64 * GRP_WAVES, 0);
    if (oe == hipSuccess)
        oe = ws->nucleotide ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&p_per_cu, probe_kernel<true>, 64 * P_WAVES, 0)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&p_per_cu, probe_kernel<false>, 64 * P_WAVES, 0);
    if (oe != hipSuccess) { delete ws; return kaamer_fail(KAAMER_E_HIP, "occupancy query: %s", hipGetErrorString(oe)); }
    hipDeviceProp_t prop;
    hipError_t pe = hipGetDeviceProperties(&prop, ix->device);
    if (pe != hipSuccess) { delete ws; return kaamer_fail(KAAMER_E_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(pe)); }
    if (grp_per_cu < 1) grp_per_cu = 1;
    if (p_per_cu < 1) p_per_cu = 1;
    // tuning knobs (tools/coresident.sh): workgroups per CU of the counting / probe kernels, never above what fits
    // batches in flight next to this one: ONE counting workgroup per CU (8 waves x 72-80 registers) leaves the CU's other
    // registers and wave slots to the neighbours' probe kernels; three fill the register file and lock them out
    // (tools/r4_sweep.sh: 0.134-0.143 ms per batch against 0.148-0.155 with three batches in flight, 0.26 against 0.20 alone)
    if (opts->concurrent_batches > 1 && !ws->nucleotide) grp_per_cu = 1;
    if (const int v = knobs.grp_per_cu; v >= 1 && v <= 3) grp_per_cu = v < grp_per_cu || opts->concurrent_batches > 1 ? v : grp_per_cu;
    if (const int v = knobs.p_per_cu; v >= 1 && v < p_per_cu) p_per_cu = v;
    ws->n_cu = prop.multiProcessorCount;
    ws->grp_grid = ws->n_cu * grp_per_cu;
    // the G tier is rare on a database like DB-SP, but with a skewed database 15 % of the queries overflow their LDS
    // table: enough workgroups to keep the memory system busy (the last one to finish also finalizes the batch)
    {
        int g_per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&g_per_cu, count_global_kernel, 64 * G_WAVES, 0) != hipSuccess || g_per_cu < 1) g_per_cu = 1;
        ws->g_grid = ws->n_cu * (g_per_cu > 2 ? 2 : g_per_cu);
        ws->g_floor = knobs.g_floor ? knobs.g_floor : 1;
        if (ws->g_floor > ws->g_grid) ws->g_floor = ws->g_grid;
        ws->g_last = G_LAST_UNKNOWN;
    }
    ws->p_grid = ws->n_cu * p_per_cu;
    {
        int pk_per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pk_per_cu, count_pack_kernel<PK_ARENA_ORF>, 64, 0) != hipSuccess || pk_per_cu < 1) pk_per_cu = 1;
        if (const int v = knobs.pack_per_cu; v >= 1 && v < pk_per_cu) pk_per_cu = v;
        ws->pack_grid = ws->n_cu * pk_per_cu;
        int pl = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pl, count_pack_kernel<PK_ARENA_ORF_LONG>, 64, 0) != hipSuccess || pl < 1) pl = 1;
        ws->pack_grid_long = ws->n_cu * pl;
    }
    // Which counting kernel: ORF batches (tables of 64-128 slots, 24 one-wave workgroups per CU) take the pack kernel, 8-16
    // ORFs to a pack window of 512 slots; protein batches the group kernel over UNITS of two group windows
    // (count_group.hip.inc) -- a wave alone on a 700-position query is a 50 us critical path, and with the 11 waves per CU
    // a protein arena allows the pack kernel took 117-156 us against the group kernel's 100 (profiles/r03_count_kernels.md)
    ws->pack_shift = ws->nucleotide ? 9u : GRP_SHIFT + 1u;
    ws->wide_reads = knobs.wide_reads;
    ws->pack_long = knobs.pack_long;
    // a table has at most max(64, 3 x SizeInKmer) slots
    {
        // (a merge counts partial entries instead of positions: as many as max_hits)
        const uint64_t items = ws->pos_cap > ws->hit_cap ? ws->pos_cap : ws->hit_cap;
        const uint64_t gc = (((uint64_t)GRP_MIN_TABLE * ws->q_cap + 3 * items) >> 8) + 4;  // windows of 256 slots at the least
        ws->groups_cap = (uint32_t)(gc > 0x7FFFFFFFull ? 0x7FFFFFFFull : gc);
    }
    int rc = KAAMER_OK;
    {
        uint64_t n = ws->q_cap;
        if (ws->nucleotide && (uint64_t)ws->max_seqs * 6 > n) n = (uint64_t)ws->max_seqs * 6;
        if (ws->nucleotide) {
            const uint64_t ml = opts->max_seq_bytes / (TS_MAX + 1) + 1;
            ws->max_long = (uint32_t)(ml < ws->max_seqs ? ml : ws->max_seqs);
            ws->max_piece_items = 6ull * (opts->max_seq_bytes / 3 / TP_PIECE + ws->max_long + 1);
            if (ws->max_piece_items > n) n = ws->max_piece_items;
        }
        ws->n_scan_blocks = (uint32_t)((n + 1 + SCAN_TILE - 1) / SCAN_TILE);
    }
    auto zero = [&rc](void *p, size_t bytes) { if (!rc && hipMemset(p, 0, bytes) != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "memset"); };
    const size_t qc = ws->q_cap;
    // every batch: queries, probe results, table layout and schedule, counters, the sparse hit arrays
    rc = reserve_group(nullptr, GROW_EXACT, {
        want(ws->d_q, qc), want(ws->d_nq, 1), want(ws->d_n_pos, 1), want(ws->d_valid, (size_t)(ws->pos_cap / 64 + 2)), want(ws->d_vals, (size_t)ws->pos_cap),
        want(ws->d_q_cnt, qc), want(ws->d_pool_cursor, (size_t)3 * CURSOR_STRIDE), want(ws->d_lists, (size_t)N_LISTS * qc),
        want(ws->d_list_counts, N_SMALL_SLOTS), want(ws->d_status_out, 2), want(ws->d_qinfo, qc), want(ws->d_slots, qc), want(ws->d_slot_off, qc + 1),
        want(ws->d_group_first, ws->groups_cap), want(ws->d_sched, ws->groups_cap), want(ws->d_group_start, ws->groups_cap), want(ws->d_lay_total, 1),
        want(ws->d_slot_scale, 4), want(ws->d_n_sched, 1), want(ws->d_n_groups, 1),
        want(ws->d_g_keys, (size_t)(4 * ws->g_slots)),  // 16-byte slots {id, count, lowest position, -}
        want(ws->d_counter_replicas, (size_t)CTR_REPLICAS * CTR_N), want(ws->d_counters, 1), want(ws->d_bsum, ws->n_scan_blocks),
        want(ws->d_chain, qc / PL_TILE + 2), want(ws->d_hit_off, qc + 1),
        want(ws->d_hit_pid, (size_t)ws->sparse_cap), want(ws->d_hit_km, (size_t)ws->sparse_cap), want(ws->d_hit_fp, (size_t)ws->sparse_cap) });
    zero(ws->d_status_out, 2 * sizeof(uint32_t));
    zero(ws->d_chain, (qc / PL_TILE + 2) * sizeof(unsigned long long));
    // first positions are written only when asked for; otherwise the array reads as zeros
    if (!ws->firstpos) zero(ws->d_hit_fp, ws->sparse_cap * sizeof(uint32_t));
    if (!rc) {
        const uint32_t one = SLOT_SCALE_ONE;
        if (hipMemcpy(ws->d_slot_scale, &one, 4, hipMemcpyHostToDevice) != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "workspace init");
        // the tables of a batch may take 70 % of the hit arrays (the G tier's lists come after them).  How far a batch's
        // tables scale inside that room is settled per batch on the device, from the batch's own positions
        // (fit_table_scale): a workspace sized for 2 amino acids per nucleotide holds ORFs of 0.5 per nucleotide at 4 x
        ws->table_room = (unsigned long long)(0.7 * (double)ws->sparse_cap);
        ws->slot_scale_cap = knobs.slot_scale_cap;
        ws->slot_scale_margin = knobs.slot_scale_margin;
        ws->dense_tables = ws->pack_long;
        if (knobs.ws_trace)
            fprintf(stderr, "[kaamer workspace] pos_cap %llu q_cap %u hit_cap %llu sparse_cap %llu table_room %llu slot_scale_cap %u/16\n", (unsigned long long)ws->pos_cap,
                    ws->q_cap, (unsigned long long)ws->hit_cap, (unsigned long long)ws->sparse_cap, ws->table_room, ws->slot_scale_cap);
    }
    if (!rc && ws->nucleotide) {   // the products of the 6-frame translation
        const size_t n6 = (size_t)ws->max_seqs * 6, ml = ws->max_long, mp = (size_t)ws->max_piece_items;
        const size_t tcw = 3 * ((size_t)ws->max_seqs / 64 + 2);
        rc = reserve_group(nullptr, GROW_EXACT, {
            want(ws->d_cnt3, 3 * n6), want(ws->d_off3, 3 * (n6 + 1)), want(ws->d_n6, 1), want(ws->d_long_seq, ml + 1), want(ws->d_piece_li, mp / 6 + 2),
            want(ws->d_long_np, ml + 1), want(ws->d_piece_base, ml + 2), want(ws->d_pcnt3, 3 * mp), want(ws->d_poff3, 3 * (mp + 1)),
            want(ws->d_n_piece_items, 1), want(ws->d_tmp_meta, qc), want(ws->d_tr_chain, tcw),
            want(ws->d_orf_aa, (size_t)ws->aa_cap + 64), want(ws->d_starts_alt, (size_t)ws->sa_cap + 64) });
        zero(ws->d_tr_chain, tcw * sizeof(unsigned long long));
    }
    ws->want_positions = opts->want_positions != 0;
    if (!rc && ws->want_positions) {   // full PositionHits bitmaps
        ws->bits_cap = opts->max_pos_words ? opts->max_pos_words : ws->hit_cap * 8;
        rc = reserve_group(nullptr, GROW_EXACT, { want(ws->d_pos_words, qc), want(ws->d_pos_base, qc + 1), want(ws->d_pos_off, (size_t)ws->sparse_cap),
                                                  want(ws->d_pos_bits, (size_t)ws->bits_cap) });
    }
    ws->compact = opts->compact != 0;
    if (!rc && ws->compact) {   // CSR in query order
        rc = reserve_group(nullptr, GROW_EXACT, { want(ws->d_csr_off, qc + 1), want(ws->d_c_pid, (size_t)ws->hit_cap), want(ws->d_c_km, (size_t)ws->hit_cap),
                                                  want(ws->d_c_fp, (size_t)ws->hit_cap) });
        if (!ws->firstpos) zero(ws->d_c_fp, ws->hit_cap * sizeof(uint32_t));
    }
    if (rc) { delete ws; return rc; }
    *out = ws;
    return KAAMER_OK;
}

// table layout + query groups (count_group.hip.inc): one single-pass kernel
static void launch_layout(kaamer_workspace *ws, uint32_t nq_bound, uint32_t *status, hipStream_t s, uint32_t bshift, bool schedule = true)
{
    const uint32_t cshift = bshift > GRP_SHIFT ? 10u : bshift >= GRP_SHIFT ? 9u : 7u;  // 16 schedule classes over the slots a group / pack can hold
    const uint32_t tiles = (uint32_t)(((uint64_t)nq_bound + 1 + LAY_TILE - 1) / LAY_TILE);
    hipLaunchKernelGGL(layout_kernel, dim3(tiles), dim3(LAY_THREADS), 0, s, ws->d_slots, ws->d_nq, ws->d_slot_off, ws->d_group_first,
                       ws->d_group_start, ws->d_n_groups, ws->groups_cap, ws->d_chain, next_epoch(ws->lay_epoch), status, bshift);
    if (schedule)  // (the pack kernel takes its packs by ticket in layout order: no schedule)
        hipLaunchKernelGGL(schedule_kernel, dim3(1), dim3(1024), 0, s, ws->d_group_first, ws->d_group_start, ws->d_slot_off, ws->d_n_groups,
                           ws->d_nq, ws->d_sched, ws->d_n_sched, cshift);
}

// the hit arrays of the workspace's current result form: CSR in query order (opts.compact), or the sparse arrays
struct WsHits { const uint64_t *off; const uint32_t *pid, *km, *fp; };
static WsHits ws_hits(const kaamer_workspace *ws)
{
    if (ws->compact) return { ws->d_csr_off, ws->d_c_pid, ws->d_c_km, ws->d_c_fp };
    return { ws->d_hit_off, ws->d_hit_pid, ws->d_hit_km, ws->d_hit_fp };
}

// PositionHits layout of the final hit lists: words per query, their scan (d_pos_base), pos_off per hit, bitmaps zeroed.
// sizes: NULL = the search's own QInfo.size; a merge passes the owned queries' SizeInKmer
static void launch_pos_layout(kaamer_workspace *ws, uint32_t nq_bound, const int32_t *sizes, uint32_t *status, hipStream_t s)
{
    uint32_t gb = (nq_bound + 255) / 256;
    if (gb < 1) gb = 1;
    if (gb > (uint32_t)ws->n_cu * 8) gb = (uint32_t)ws->n_cu * 8;
    hipLaunchKernelGGL(pos_words_kernel, dim3(gb), dim3(256), 0, s, ws->d_qinfo, sizes, ws->d_q_cnt, ws->d_nq, ws->d_pos_words);
    scan_u32_on(ws, ws->d_pos_words, ws->d_nq, nq_bound, ws->d_pos_base, s);
    hipLaunchKernelGGL(pos_layout_kernel, dim3(ws->n_cu * 8), dim3(256), 0, s, ws->d_qinfo, sizes, ws->d_q_cnt,
                       ws_hits(ws).off,
                       ws->d_pos_base, ws->d_nq, ws->d_pos_off, ws->d_pos_bits, ws->bits_cap, status);
}

// optional last step of a search / merge: CSR in query order from the sharded hit arrays
static void launch_compaction(kaamer_workspace *ws, uint32_t nq_bound, uint32_t *status, hipStream_t s)
{
    scan_u32_on(ws, ws->d_q_cnt, ws->d_nq, nq_bound, ws->d_csr_off, s);
    uint32_t gb = (nq_bound + 3) / 4;
    if (gb < 1) gb = 1;
    if (gb > (uint32_t)ws->n_cu * 8) gb = (uint32_t)ws->n_cu * 8;
    hipLaunchKernelGGL(gather_hits_kernel, dim3(gb), dim3(256), 0, s, ws->d_nq, ws->d_csr_off, ws->d_hit_off, ws->d_q_cnt, ws->d_hit_pid,
                       ws->d_hit_km, ws->d_hit_fp, ws->d_c_pid, ws->d_c_km, ws->d_c_fp, ws->hit_cap, status, 1);
}

static void fill_result_hits(const kaamer_workspace *ws, kaamer_device_result *out)
{
    out->d_hit_cnt = ws->d_q_cnt;
    out->hit_capacity = ws->compact ? ws->hit_cap : ws->sparse_cap;
    const WsHits h = ws_hits(ws);
    out->d_hit_off = h.off;
    out->d_hit_pid = h.pid;
    out->d_hit_kmatch = h.km;
    out->d_hit_first_pos = h.fp;
}

// whoever consumes the workspace's last search on `stream` first waits for its counting stage, if that ran elsewhere
static int ws_join(kaamer_workspace *ws, hipStream_t stream)
{
    if (ws->split_pending && ws->count_stream && ws->count_stream != stream) HIPCHK(hipStreamWaitEvent(stream, ws->ev_count, 0));
    return KAAMER_OK;
}

int kaamer_workspace_set_count_stream(kaamer_workspace *ws, void *stream)
{
    if (!ws) return kaamer_fail(KAAMER_E_ARG, "workspace_set_count_stream: bad argument");
    HIPCHK(hipSetDevice(ws->device));
    if (ws->split_pending) HIPCHK(hipEventSynchronize(ws->ev_count));
    ws->split_pending = false;
    ws->count_stream = (hipStream_t)stream;
    if (stream && !ws->ev_probe) {
        HIPCHK(hipEventCreateWithFlags(&ws->ev_probe.e, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ws->ev_count.e, hipEventDisableTiming));
    }
    return KAAMER_OK;
}

// ---- the stages of a search, in the order they run: each enqueues its launches on `s` (errors: the caller's hipGetLastError)

// protein batches: prep + table layout + group schedule in one launch (count_group.hip.inc)
static void enqueue_protein_prep(kaamer_workspace *ws, const uint8_t *d_seqs, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t seq_bytes,
                                 uint32_t *status, hipStream_t s)
{
    PrepLayoutParams pl;
    memset(&pl, 0, sizeof pl);
    pl.seqs = d_seqs; pl.pos_bound = seq_bytes; pl.offsets = d_offsets; pl.n_seqs = n_seqs;
    pl.q = ws->d_q; pl.d_nq = ws->d_nq; pl.d_n_pos = ws->d_n_pos; pl.invalid = ws->d_valid; pl.qinfo = ws->d_qinfo;
    pl.hit_off = ws->d_hit_off; pl.q_cnt = ws->d_q_cnt;
    pl.E = ws->d_slot_off; pl.group_first = ws->d_group_first; pl.group_start = ws->d_group_start;
    pl.d_n_groups = ws->d_n_groups; pl.groups_cap = ws->groups_cap; pl.chain = ws->d_chain;
    pl.epoch = next_epoch(ws->lay_epoch);
    pl.status = status; pl.sched = ws->d_sched; pl.d_n_sched = ws->d_n_sched;
    pl.tiles_done = ws->d_list_counts + SLOT_TILES_DONE;
    pl.slots = ws->d_slots; pl.bshift = ws->pack_shift; pl.cshift = ws->pack_shift > GRP_SHIFT ? 10u : ws->pack_shift >= GRP_SHIFT ? 9u : 7u;
    // the group kernel takes the groups longest first (measured with one workgroup per CU and three batches in flight:
    // 0.1381-0.1406 ms per batch, 0.1430-0.1441 with the groups in index order)
    pl.no_sched = 0u;
    pl.d_total = ws->d_lay_total;
    pl.slot_scale = ws->d_slot_scale;
    pl.room_slots = ws->table_room;
    const uint32_t tiles = (uint32_t)(((uint64_t)n_seqs + 1 + PL_TILE - 1) / PL_TILE);
    hipLaunchKernelGGL(prep_layout_schedule_kernel, dim3(tiles), dim3(LAY_THREADS), 0, s, pl);
}

// what the probe and the counting stages work on: the protein records themselves, or the ORFs of a translated batch
struct QueryInput {
    const uint8_t *residues;   // what kernel P reads
    uint64_t pos_bound;        // host-side bound of the residue positions (grid sizing only)
    uint32_t nq_bound;         // host-side bound of the number of queries
};

// the launches that see codon classes, once per GENERIC (translate.hip.inc): the long sequences' COUNT pass, then the reads'
// kernel and the long sequences' WRITE pass
extern "C++" {
template <bool GENERIC>
static void launch_translate_count(const TranslateParams &tp, int tgrid, hipStream_t s)
{
    hipLaunchKernelGGL((translate_kernel<false, GENERIC>), dim3(tgrid), dim3(256), 0, s, tp);
}
template <bool GENERIC>
static void launch_translate_write(const TranslateParams &tp, bool wide_reads, int sgrid, int tgrid, hipStream_t s)
{
    if (wide_reads) hipLaunchKernelGGL((translate_reads_kernel<TS_MAX_WIDE, GENERIC>), dim3(sgrid), dim3(64 * TS_WAVES), 0, s, tp);
    else hipLaunchKernelGGL((translate_reads_kernel<TS_MAX, GENERIC>), dim3(sgrid), dim3(64 * TS_WAVES), 0, s, tp);
    hipLaunchKernelGGL((translate_kernel<true, GENERIC>), dim3(tgrid), dim3(256), 0, s, tp);
}
}  // extern "C++"

// nucleotide batches: 6-frame translation -- count, scan, write, order (translate.hip.inc) -- and the ORFs' prep
// gc_slot: the call's table (kt_gcode_slot); table 11 launches the kernels with compile-time classes
static QueryInput enqueue_translate(kaamer_workspace *ws, const uint8_t *d_seqs, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t seq_bytes,
                                    int gc_slot, uint32_t *status, hipStream_t s)
{
    const size_t cap6 = (size_t)ws->max_seqs * 6;
    TranslateParams tp;
    memset(&tp, 0, sizeof tp);
    tp.seqs = d_seqs; tp.offsets = d_offsets; tp.n_seqs = n_seqs; tp.seq_bound = seq_bytes; tp.max_long = ws->max_long; tp.max_piece_items = ws->max_piece_items;
    tp.cnt_orf = ws->d_cnt3; tp.cnt_aa = ws->d_cnt3 + cap6; tp.cnt_sa = ws->d_cnt3 + 2 * cap6;
    tp.off_orf = ws->d_off3; tp.off_aa = ws->d_off3 + (cap6 + 1); tp.off_sa = ws->d_off3 + 2 * (cap6 + 1);
    tp.tmp_meta = ws->d_tmp_meta; tp.orf_aa = ws->d_orf_aa; tp.starts_alt = ws->d_starts_alt;
    tp.q_cap = ws->q_cap; tp.aa_cap = ws->aa_cap; tp.sa_cap = ws->sa_cap; tp.status = status;
    // which lane-per-read kernel: the wide one (reads up to 384 nt, 2 waves per SIMD) when the batch's mean length says that
    // reads beyond 192 nt are common; a batch of 100-150-nt reads is 4 % slower through it (translate.hip.inc)
    const bool wide_reads = ws->wide_reads >= 0 ? ws->wide_reads != 0 : seq_bytes > 160ull * (n_seqs ? n_seqs : 1u);
    tp.ts_max = wide_reads ? TS_MAX_WIDE : TS_MAX;
    int tgrid = ws->n_cu * 8;  // 256-thread blocks, one (sequence, frame, piece) item per wave at a time
    tp.d_n6 = ws->d_n6;
    int sgrid = ws->n_cu * 8;  // lane-per-read kernel: 2-wave blocks, 13 KB (COUNT) / 30 KB (WRITE) of LDS each
    if ((uint64_t)sgrid * TS_WAVES * 64 > (uint64_t)n_seqs) sgrid = n_seqs > 0 ? (int)(((uint64_t)n_seqs + TS_WAVES * 64 - 1) / (TS_WAVES * 64)) : 1;
    tp.n_long = ws->d_list_counts + SLOT_N_LONG;
    const size_t mpi = (size_t)ws->max_piece_items;
    tp.long_seq = ws->d_long_seq; tp.long_np = ws->d_long_np; tp.piece_base = ws->d_piece_base; tp.piece_li = ws->d_piece_li;
    tp.pcnt_orf = ws->d_pcnt3; tp.pcnt_aa = ws->d_pcnt3 + mpi; tp.pcnt_sa = ws->d_pcnt3 + 2 * mpi;
    tp.poff_orf = ws->d_poff3; tp.poff_aa = ws->d_poff3 + (mpi + 1); tp.poff_sa = ws->d_poff3 + 2 * (mpi + 1);
    tp.d_n_piece_items = ws->d_n_piece_items;
    // reads: a lane each; longer sequences: listed, cut in pieces, a wave per piece
    const uint64_t long_bound = (uint64_t)ws->max_long < n_seqs ? ws->max_long : n_seqs;
    const uint64_t seq_long_max = seq_bytes / (TS_MAX + 1) + 1;
    const uint64_t n_long_bound = long_bound < seq_long_max ? long_bound : seq_long_max;
    const uint64_t piece_bound = 6ull * (seq_bytes / 3 / TP_PIECE + n_long_bound + 1);
    if ((uint64_t)tgrid * 4 > piece_bound) tgrid = (int)((piece_bound + 3) / 4);
    if (tgrid < 1) tgrid = 1;
    tp.ticket = ws->d_list_counts + SLOT_TR_TICKET;
    tp.chain = ws->d_tr_chain;
    tp.epoch = next_epoch(ws->tr_epoch);
    tp.out_meta = ws->d_q; tp.d_nq = ws->d_nq; tp.d_n_pos = ws->d_n_pos;
    tp.w_off_orf = ws->d_off3; tp.w_off_aa = ws->d_off3 + (cap6 + 1); tp.w_off_sa = ws->d_off3 + 2 * (cap6 + 1);
    const bool generic = gc_slot != KT_SLOT_DEFAULT;
    if (generic) {
        const KtTable &kt = kt_tables()[gc_slot];
        tp.gc_slot = (uint32_t)gc_slot;
        for (int i = 0; i < 64; i++) {
            if (kt.start[i] == 'M') tp.gc_start_bits |= 1ull << i;
            if (kt.aa[i] == '*') tp.gc_stop_bits |= 1ull << i;
        }
    }
    // long sequences first (listed, cut in pieces, counted: a wave per piece) -- a reads-only batch falls through
    // these launches; then everything of the reads and the output offsets of both kinds in one kernel
    hipLaunchKernelGGL(list_long_kernel, dim3((unsigned)(((uint64_t)n_seqs + LL_BLOCK - 1) / LL_BLOCK + (n_seqs ? 0 : 1))), dim3(LL_BLOCK), 0, s, tp);
    scan_u32_on(ws, ws->d_long_np, tp.n_long, n_long_bound, ws->d_piece_base, s);
    // (an empty batch -- a text without a record -- still launches one workgroup of each, as list_long_kernel above)
    hipLaunchKernelGGL(piece_li_kernel, dim3((unsigned)((n_long_bound + 255) / 256 + (n_long_bound ? 0 : 1))), dim3(256), 0, s, tp);
    if (generic) launch_translate_count<true>(tp, tgrid, s);
    else launch_translate_count<false>(tp, tgrid, s);
    for (int a = 0; a < 3; a++) scan_u32_on(ws, ws->d_pcnt3 + a * mpi, ws->d_n_piece_items, piece_bound, ws->d_poff3 + a * (mpi + 1), s);
    hipLaunchKernelGGL(long_totals_kernel, dim3((unsigned)((n_long_bound * 6 + 255) / 256 + (n_long_bound ? 0 : 1))), dim3(256), 0, s, tp);
    if (generic) launch_translate_write<true>(tp, wide_reads, sgrid, tgrid, s);
    else launch_translate_write<false>(tp, wide_reads, sgrid, tgrid, s);
    hipLaunchKernelGGL(orf_order_long_kernel, dim3((unsigned)(n_long_bound < (uint64_t)ws->n_cu * 32 ? (n_long_bound + 3) / 4 + 1 : (uint64_t)ws->n_cu * 8)), dim3(256), 0, s,
                       ws->d_tmp_meta, tp.off_orf, ws->d_long_seq, tp.n_long, ws->d_q, ws->d_nq);
    hipLaunchKernelGGL(prep_orf_kernel, dim3(ws->n_cu * 4), dim3(256), 0, s, ws->d_q, ws->d_nq, ws->d_valid, ws->d_n_pos,
                       ws->d_qinfo, ws->d_slots, ws->d_hit_off, ws->d_q_cnt, ws->d_slot_scale, ws->table_room);
    return QueryInput{ ws->d_orf_aa, ws->aa_cap, ws->q_cap };
}

// kernel P: flat probe
static void enqueue_probe(const kaamer_index *ix, kaamer_workspace *ws, const uint8_t *residues, uint64_t pos_bound, hipStream_t s)
{
    ProbeParams pp;
    pp.table = reinterpret_cast<const uint4 *>(ix->d_buckets);
    pp.n_buckets = ix->hdr.n_buckets;
    pp.n_shards = ix->hdr.n_shards;
    pp.shard = ix->hdr.shard;
    pp.residues = residues;
    pp.invalid = ws->d_valid;
    pp.d_n_pos = ws->d_n_pos;
    pp.vals = ws->d_vals;
    pp.counters = ws->d_counter_replicas;
    pp.nontemporal = pos_bound < ix->hdr.n_buckets ? 1u : 0u;
    uint64_t p_blocks = (pos_bound / 64 + 1 + P_WAVES - 1) / P_WAVES;
    if (p_blocks > (uint64_t)ws->p_grid) p_blocks = ws->p_grid;
    if (p_blocks < 1) p_blocks = 1;
    if (ws->nucleotide) hipLaunchKernelGGL(probe_kernel<true>, dim3((unsigned)p_blocks), dim3(64 * P_WAVES), 0, s, pp);
    else hipLaunchKernelGGL(probe_kernel<false>, dim3((unsigned)p_blocks), dim3(64 * P_WAVES), 0, s, pp);
}

// the counting launches of a search share these on top of count_params_base
static CountParams search_count_params(const kaamer_index *ix, const kaamer_workspace *ws)
{
    CountParams p = count_params_base(ws);
    p.arena = ix->d_arena;
    p.vals = ws->d_vals;
    p.queue_head = ws->d_list_counts + SLOT_QUEUE_HEAD;
    p.n_proteins = ix->hdr.max_protein_id + 1u ? ix->hdr.max_protein_id + 1u : 0xFFFFFFFFu;
    return p;
}

// a search finalizes inside the G-tier kernel when nothing follows it
static bool fused_finalize(const kaamer_workspace *ws) { return !ws->compact && !ws->want_positions; }

// kernel C: counting -- group kernel (protein) or pack kernel (ORFs), the G tier behind it, compaction
static void enqueue_count(const kaamer_index *ix, kaamer_workspace *ws, bool nucl, uint64_t seq_bytes, uint32_t n_seqs, uint32_t nq_bound,
                          uint64_t pos_bound, hipStream_t s)
{
    const CountParams p = search_count_params(ix, ws);
    CountParams pc = p;
    pc.ovf_list = ws_list(ws, LIST_G); pc.ovf_count = ws->d_list_counts + LIST_G;
    pc.last_group_pass = ws->want_positions ? 0u : 1u;
    pc.pack_shift = ws->pack_shift;
    pc.pack_tickets = ws->d_list_counts + SLOT_PACK_TICKETS;
    if (!nucl) {
        launch_group(pc, group_grid(ws, nq_bound, pos_bound), ws->firstpos, s);
    } else {
        // one wave per workgroup, packs dealt out statically: never more waves than packs (group_grid's bound, with the
        // pack's own budget 1 << pack_shift)
        uint64_t gb = (((uint64_t)GRP_MIN_TABLE * nq_bound + 3 * pos_bound) >> ws->pack_shift) + 1;
        if (gb > (uint64_t)ws->pack_grid) gb = ws->pack_grid;
        // reads of ~150 nt: ORFs of <= 50 residues, tables of 64-128 slots -> the small arena (20 waves per CU);
        // longer sequences (mixed read lengths, contigs): the arena that holds tables of up to 576 slots, or 66 000
        // ORFs of a 1 M mixed-read batch went to the G tier (measured: 8.19 -> 6.73 ms for the counting stage of
        // that batch, while the 150-nt batch loses 0.4 ms with the larger arena)
        const bool long_orfs = seq_bytes > 200ull * (n_seqs ? n_seqs : 1u) || ws->dense_tables;
        if (long_orfs) {
            if (gb > (uint64_t)ws->pack_grid_long) gb = ws->pack_grid_long;
            hipLaunchKernelGGL((count_pack_kernel<PK_ARENA_ORF_LONG>), dim3((unsigned)gb), dim3(64), 0, s, pc);
        } else {
            hipLaunchKernelGGL((count_pack_kernel<PK_ARENA_ORF>), dim3((unsigned)gb), dim3(64), 0, s, pc);
        }
    }
    CountParams pg = p;
    pg.list = ws_list(ws, LIST_G); pg.list_count = ws->d_list_counts + LIST_G;
    if (fused_finalize(ws)) {
        pg.fin_out = ws->d_counters; pg.fin_small = ws->d_list_counts; pg.fin_status_out = ws->d_status_out;
        pg.fin_g_items = ws->d_status_out + 1; pg.fin_cursors = ws->d_pool_cursor;
        pg.fin_slot_scale = ws->d_slot_scale; pg.fin_scale_cap = ws->slot_scale_cap; pg.fin_scale_margin = ws->slot_scale_margin;
    }
    hipLaunchKernelGGL(count_global_kernel, dim3(g_tier_grid(ws, nq_bound, true)), dim3(64 * G_WAVES), 0, s, pg);
    if (ws->compact) launch_compaction(ws, nq_bound, p.status, s);
}

// PositionHits bitmaps (search.go:442-452): layout from the final hit lists, then one more pass of the group kernel
// that sets one bit per (hit, position)
static void enqueue_positions(const kaamer_index *ix, kaamer_workspace *ws, uint32_t nq_bound, uint64_t pos_bound, hipStream_t s)
{
    const CountParams p = search_count_params(ix, ws);
    launch_pos_layout(ws, nq_bound, nullptr, p.status, s);
    // the PositionHits pass runs on the group kernel: lay the tables out in its groups
    launch_layout(ws, nq_bound, p.status, s, GRP_SHIFT);
    CountParams pp2 = p;
    pp2.pack_shift = GRP_SHIFT;   // (the layout just above)
    pp2.last_group_pass = 1u;
    pp2.pos_base = ws->d_pos_base;
    pp2.pos_bits = ws->d_pos_bits;
    pp2.group_queue = ws->d_list_counts + SLOT_GROUP_QUEUE_POS;
    pp2.ovf_list = ws_list(ws, LIST_SO); pp2.ovf_count = ws->d_list_counts + LIST_SO;
    launch_group_positions(pp2, group_grid(ws, nq_bound, pos_bound), s);
    CountParams pg2 = p;   // the G tier's queries: their hit lists are final, the counting arena is free again
    pg2.list = ws_list(ws, LIST_G); pg2.list_count = ws->d_list_counts + LIST_G;
    pg2.pos_base = ws->d_pos_base;
    pg2.pos_bits = ws->d_pos_bits;
    pg2.g_cursor = ws->d_pool_cursor + 2 * CURSOR_STRIDE;
    hipLaunchKernelGGL(positions_global_kernel, dim3(g_tier_grid(ws, nq_bound, true)), dim3(64 * G_WAVES), 0, s, pg2);
}

int kaamer_search_device(kaamer_index *ix, kaamer_workspace *ws, const uint8_t *d_seqs, const uint64_t *d_offsets,
                         uint32_t n_seqs, uint64_t seq_bytes, int32_t seq_type, void *stream,
                         kaamer_device_result *out)
{
    if (!ix || !ws || !out || (n_seqs && (!d_seqs || !d_offsets))) return kaamer_fail(KAAMER_E_ARG, "search_device: bad argument");
    if (ix->device != ws->device) return kaamer_fail(KAAMER_E_ARG, "workspace belongs to another device");
    SEQ_TYPE_CHK(seq_type, "search_device");
    const bool nucl = is_nucl(seq_type);
    if (nucl != ws->nucleotide) return kaamer_fail(KAAMER_E_ARG, "workspace was created for %s input", ws->nucleotide ? "nucleotide" : "protein");
    if (n_seqs > ws->max_seqs) return kaamer_fail(KAAMER_E_CAPACITY, "batch of %u sequences exceeds workspace max_seqs %u", n_seqs, ws->max_seqs);
    if (ws->pos_cap > 0xFFFFFFF0ull) return kaamer_fail(KAAMER_E_CAPACITY, "a batch holds at most 2^32 residue positions");
    if (seq_bytes > ws->opts.max_seq_bytes) return kaamer_fail(KAAMER_E_CAPACITY, "batch of %llu bytes exceeds workspace max_seq_bytes", (unsigned long long)seq_bytes);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ix->device));
    {   // the previous batch's counting stage may still be reading this workspace on the count stream
        const int jrc = ws_join(ws, s);
        if (jrc) return jrc;
        ws->split_pending = false;
    }
    // kernel timers: an event record costs a few microseconds of stream idle time, so they are
    // off unless asked for, and can sample every k-th call (kaamer_workspace_set_timing)
    const bool timed = ws->time_every && (ws->call_no++ % ws->time_every) == 0;
    hipEvent_t *ev = nullptr;
    if (timed) {
        if (ws->n_timed >= MAX_TIMED_CALLS) ws->n_timed = 0;
        while (ws->ev.size() < (size_t)(ws->n_timed + 1) * EV_PER_CALL) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            ws->ev.push_back(e);
        }
        ev = ws->ev.data() + (size_t)ws->n_timed * EV_PER_CALL;
        HIPCHK(hipEventRecord(ev[0], s));
    }
    {
        const int rrc = ws_reset_if_dirty(ws, s);
        if (rrc) return rrc;
        ws->clean = false;
    }
    uint32_t *status = ws->d_list_counts + SLOT_STATUS;

    // ---- queries: protein records (prep, table layout and group schedule in one launch), or ORFs and their table layout
    QueryInput qin = { d_seqs, seq_bytes, n_seqs };
    if (!nucl) {
        enqueue_protein_prep(ws, d_seqs, d_offsets, n_seqs, seq_bytes, status, s);
    } else {
        qin = enqueue_translate(ws, d_seqs, d_offsets, n_seqs, seq_bytes, kt_gcode_slot(KAAMER_SEQ_TYPE_GENETIC_CODE(seq_type)), status, s);
        launch_layout(ws, qin.nq_bound, status, s, ws->pack_shift, false);
    }
    if (timed) HIPCHK(hipEventRecord(ev[1], s));
    enqueue_probe(ix, ws, qin.residues, qin.pos_bound, s);
    if (timed) HIPCHK(hipEventRecord(ev[2], s));
    const bool split = ws->count_stream && ws->count_stream != s && !timed;
    if (split) {   // everything from here on runs on the count stream, behind the probe kernel
        HIPCHK(hipEventRecord(ws->ev_probe, s));
        HIPCHK(hipStreamWaitEvent(ws->count_stream, ws->ev_probe, 0));
        s = ws->count_stream;
    }
    enqueue_count(ix, ws, nucl, seq_bytes, n_seqs, qin.nq_bound, qin.pos_bound, s);
    if (timed) HIPCHK(hipEventRecord(ev[3], s));
    if (ws->want_positions) enqueue_positions(ix, ws, qin.nq_bound, qin.pos_bound, s);
    if (!fused_finalize(ws))
        hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, ws->d_counter_replicas, ws->d_counters, ws->d_list_counts,
                           ws->d_status_out, ws->d_status_out + 1, ws->d_pool_cursor, ws->d_slot_scale, ws->slot_scale_cap, ws->slot_scale_margin);
    if (timed) HIPCHK(hipEventRecord(ev[4], s));
    HIPCHK(hipGetLastError());
    if (split) {
        HIPCHK(hipEventRecord(ws->ev_count, s));
        ws->split_pending = true;
    }
    ws->clean = true;  // everything up to finalize is enqueued
    ws->last_was_merge = false;
    ws->last_seqs = d_seqs;
    if (timed) ws->n_timed++;

    out->n_queries_cap = ws->q_cap;
    out->d_n_queries = ws->d_nq;
    out->d_q = ws->d_q;
    fill_result_hits(ws, out);
    out->d_orf_aa = nucl ? ws->d_orf_aa : nullptr;
    out->d_starts_alt = nucl ? ws->d_starts_alt : nullptr;
    out->d_counters = ws->d_counters;
    out->d_pos_off = ws->want_positions ? ws->d_pos_off : nullptr;
    out->d_pos_bits = ws->want_positions ? (const uint64_t *)ws->d_pos_bits.get() : nullptr;
    out->d_pos_base = ws->want_positions ? ws->d_pos_base : nullptr;
    return KAAMER_OK;
}

// ---- merge of partial hit lists, in two phases: an exchange merge lays out and ORs its bitmaps between them, so that a
// bitmap bound is reported by the finalize step like every other
// n_queries / n_entries are host-side bounds when d_n_queries (a device scalar) gives the actual number of queries
static int merge_enqueue(kaamer_workspace *ws, const uint64_t *d_ent_off, const uint32_t *d_pid, const uint32_t *d_km, const uint32_t *d_fp,
                         uint32_t n_queries, const uint32_t *d_n_queries, uint64_t n_entries, hipStream_t s)
{
    if (!ws || (n_queries && !d_ent_off) || (n_entries && (!d_pid || !d_km || !d_fp)))
        return kaamer_fail(KAAMER_E_ARG, "merge_device: bad argument");
    if (n_queries > ws->q_cap) return kaamer_fail(KAAMER_E_CAPACITY, "merge of %u queries exceeds the workspace (%u)", n_queries, ws->q_cap);
    if (n_entries > ws->hit_cap) return kaamer_fail(KAAMER_E_CAPACITY, "merge of %llu entries exceeds workspace max_hits", (unsigned long long)n_entries);
    HIPCHK(hipSetDevice(ws->device));
    {
        const int rrc = ws_reset_if_dirty(ws, s);
        if (rrc) return rrc;
        ws->clean = false;
    }
    uint32_t *status = ws->d_list_counts + SLOT_STATUS;
    const uint32_t nq_bound = n_queries;
    const int pb = 256;
    hipLaunchKernelGGL(prep_merge_kernel, dim3((n_queries + pb - 1) / pb > 0 ? (n_queries + pb - 1) / pb : 1), dim3(pb), 0, s, d_ent_off,
                       n_queries, d_n_queries, ws->d_qinfo, ws->d_slots, ws->d_nq, ws->d_hit_off, ws->d_q_cnt);
    // (the merge runs on count_group_kernel<., 2>: units of two group windows, as the search of protein batches)
    launch_layout(ws, nq_bound, status, s, GRP_SHIFT + 1u);
    CountParams p = count_params_base(ws);
    p.last_group_pass = 1u;
    p.pack_shift = GRP_SHIFT + 1u;
    p.m_pid = d_pid; p.m_km = d_km; p.m_fp = d_fp; p.merge_fp = ws->firstpos ? 1u : 0u;
    p.ovf_list = ws_list(ws, LIST_G); p.ovf_count = ws->d_list_counts + LIST_G;
    launch_group_merge(p, group_grid(ws, nq_bound, n_entries), ws->firstpos, s);
    CountParams pg = p;
    pg.list = ws_list(ws, LIST_G); pg.list_count = ws->d_list_counts + LIST_G;
    hipLaunchKernelGGL(merge_global_kernel, dim3(g_tier_grid(ws, nq_bound)), dim3(256), 0, s, pg);
    if (ws->compact) launch_compaction(ws, nq_bound, status, s);
    return KAAMER_OK;
}

// the finalize step and the result; with_positions: the caller has laid the merged bitmaps out behind merge_enqueue
static int merge_finish(kaamer_workspace *ws, hipStream_t s, bool with_positions, kaamer_device_result *out)
{
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, ws->d_counter_replicas, ws->d_counters, ws->d_list_counts,
                       ws->d_status_out, (uint32_t *)nullptr, ws->d_pool_cursor, (uint32_t *)nullptr, 16u, 16u);   // (a merge looks nothing up: the scale
                                                                                                                  // stays, and so does the last search's G-tier count)
    HIPCHK(hipGetLastError());
    ws->clean = true;
    ws->last_was_merge = true;
    memset(out, 0, sizeof *out);
    out->n_queries_cap = ws->q_cap;
    out->d_n_queries = ws->d_nq;
    fill_result_hits(ws, out);
    out->d_counters = ws->d_counters;
    if (with_positions) {
        out->d_pos_off = ws->d_pos_off;
        out->d_pos_bits = (const uint64_t *)ws->d_pos_bits.get();
        out->d_pos_base = ws->d_pos_base;
    }
    return KAAMER_OK;
}

int kaamer_merge_device(kaamer_workspace *ws, const uint64_t *d_ent_off, const uint32_t *d_pid, const uint32_t *d_km,
                        const uint32_t *d_fp, uint32_t n_queries, uint64_t n_entries, void *stream, kaamer_device_result *out)
{
    if (!out) return kaamer_fail(KAAMER_E_ARG, "merge_device: bad argument");
    const int rc = merge_enqueue(ws, d_ent_off, d_pid, d_km, d_fp, n_queries, nullptr, n_entries, (hipStream_t)stream);
    return rc ? rc : merge_finish(ws, (hipStream_t)stream, false, out);
}

#include "exchange_host.hip.inc"

// FilterResults / top-N (and SetBestStartCodon for nucleotide input) of the workspace's last
// search or merge, on the device; see topn.hip.inc.
int kaamer_topn_device(kaamer_workspace *ws, const kaamer_topn_opts *opts, void *stream, kaamer_topn_result *out)
{
    if (!ws || !opts || !out || opts->max_results < 1) return kaamer_fail(KAAMER_E_ARG, "topn_device: bad argument");
    const bool best_start = opts->best_start_codon != 0;
    const kaamer_workspace *src = opts->orf_source ? opts->orf_source : ws;  // whose queries (ORFs) the results belong to
    if (best_start && (!src->nucleotide || (ws->last_was_merge && !opts->orf_source)))
        return kaamer_fail(KAAMER_E_ARG, "topn_device: SetBestStartCodon needs the ORFs of a nucleotide/reads search");
    if (opts->orf_source && opts->orf_source->device != ws->device) return kaamer_fail(KAAMER_E_ARG, "topn_device: orf_source lives on another device");
    if (ws->last_was_merge && !opts->d_size_in_kmer && !opts->orf_source)
        return kaamer_fail(KAAMER_E_ARG, "topn_device: merged results need d_size_in_kmer or orf_source (the owner's queries)");
    if (best_start && !ws->firstpos) return kaamer_fail(KAAMER_E_ARG, "topn_device: SetBestStartCodon needs first positions (first_pos != 2)");
    HIPCHK(hipSetDevice(ws->device));
    // a search whose counting stage ran on the count stream: the post-steps follow it there (the caller's stream is the probe
    // stream of the next batches), and consumers keep waiting for ev_count
    const bool on_count_stream = ws->split_pending && ws->count_stream;
    hipStream_t ts = on_count_stream ? ws->count_stream : (hipStream_t)stream;
    {   // the result arrays: q_cap rows of the largest max_results so far, and the per-query ones
        const size_t n = (size_t)ws->q_cap * opts->max_results, qc = ws->q_cap;
        int rc = reserve_group(ts, GROW_EXACT, { want(ws->d_top_pid, n), want(ws->d_top_km, n), want(ws->d_top_fp, n) });
        if (!rc) rc = reserve_group(ts, GROW_EXACT, { want(ws->d_top_cnt, qc), want(ws->d_top_trim, qc), want(ws->d_top_start, qc), want(ws->d_top_size, qc) });
        if (rc) { ws->topn_k = 0; return rc; }
        if (ws->topn_k < opts->max_results) ws->topn_k = opts->max_results;
    }
    TopnParams p;
    memset(&p, 0, sizeof p);
    p.d_nq = ws->d_nq;
    p.q = src->d_q;
    p.src_nq = src->d_nq;
    p.q_first = opts->orf_source ? opts->q_first : 0u;
    p.q_stride = opts->orf_source ? (opts->q_stride ? opts->q_stride : 1u) : 1u;
    p.size_in = opts->d_size_in_kmer;
    p.hit_cnt = ws->d_q_cnt;
    const WsHits h = ws_hits(ws);
    p.hit_off = h.off;
    p.pid = h.pid;
    p.km = h.km;
    // without first positions top_first_pos is zeros (kaamer_hip.h), whatever the counting tiers left in the hit arrays
    p.fp = ws->firstpos ? h.fp : nullptr;
    p.orf_aa = src->d_orf_aa;
    p.starts_alt = src->d_starts_alt;
    p.min_k_ratio = opts->min_k_ratio;
    p.min_k_match = opts->min_k_match;
    p.K = opts->max_results;
    p.best_start = best_start ? 1 : 0;
    p.top_cnt = ws->d_top_cnt; p.top_pid = ws->d_top_pid; p.top_km = ws->d_top_km; p.top_fp = ws->d_top_fp;
    p.trim = ws->d_top_trim; p.start_pos = ws->d_top_start; p.size_out = ws->d_top_size;
    // lanes per query: a protein query has ~190 hits (a wave), an ORF ~15 (16 lanes: four ORFs per wave)
    if (src->nucleotide) hipLaunchKernelGGL(topn_kernel<16>, dim3(ws->n_cu * 8), dim3(256), 0, ts, p);
    else hipLaunchKernelGGL(topn_kernel<64>, dim3(ws->n_cu * 8), dim3(256), 0, ts, p);
    if (on_count_stream) HIPCHK(hipEventRecord(ws->ev_count, ts));
    HIPCHK(hipGetLastError());
    out->max_results = opts->max_results;
    out->d_top_cnt = ws->d_top_cnt;
    out->d_top_pid = ws->d_top_pid;
    out->d_top_kmatch = ws->d_top_km;
    out->d_top_first_pos = ws->d_top_fp;
    out->d_trim = ws->d_top_trim;
    out->d_start_position = ws->d_top_start;
    out->d_size_in_kmer = ws->d_top_size;
    return KAAMER_OK;
}

// ---- PositionHits of the reported hits (top_positions.hip.inc) -------------------------------------------------------
// Storage rule.  A reported hit of query q takes ceil(S_q / 64) words, so a batch needs at most
//     K x sum_q ceil(S_q / 64)  <=  K x (pos_cap / 64 + q_cap)          (the hard bound: every query reports K hits)
// words.  The default provisions f hits per query instead of K: f = min(K, 16) for protein batches (a protein query of
// the flagship database reports its MaxResults = 10), f = 1 for ORF batches (most ORFs of a reads batch report nothing;
// 1 M reads: 4.2 M ORFs, a few per cent reported).  A batch beyond the bound is an ST_POS_CAP / KAAMER_E_CAPACITY like
// any other bound; the host calls repeat it with 4 x the words (BatchBounds::pos_scale), never beyond the hard bound.
static uint64_t tp_hard_words(const kaamer_workspace *ws, uint32_t K)
{
    const uint64_t per_hit = ws->pos_cap / 64 + ws->q_cap + 1;
    const uint64_t lim = 0xFFFFFFF0ull;   // the per-query word counts saturate at 32 bits (top_pos_words_kernel)
    return per_hit > lim / K ? lim : per_hit * K;
}
static uint64_t tp_default_words(const kaamer_workspace *ws, uint32_t K, uint32_t scale)
{
    const uint32_t f = ws->nucleotide ? 1u : (K < 16u ? K : 16u);
    const uint64_t hard = tp_hard_words(ws, K);
    uint64_t w = (ws->pos_cap / 64 + ws->q_cap + 1) * f;
    if (scale > 1) w = w > hard / scale ? hard : w * scale;
    return w > hard ? hard : w;
}

static int tp_prepare(kaamer_workspace *ws)
{
    const size_t qc = ws->q_cap;   // (fixed per workspace: nothing to wait for, the group is made once)
    return reserve_group(nullptr, GROW_EXACT, { want(ws->d_tp_words, qc), want(ws->d_tp_len, qc), want(ws->d_tp_base, qc + 1) });
}

static TopPosParams tp_params(const kaamer_index *ix, const kaamer_workspace *ws, const kaamer_topn_result *top)
{
    TopPosParams p;
    memset(&p, 0, sizeof p);
    p.d_nq = ws->d_nq; p.qinfo = ws->d_qinfo; p.vals = ws->d_vals; p.arena = ix->d_arena;
    p.top_cnt = top->d_top_cnt; p.top_pid = top->d_top_pid; p.K = top->max_results;
    p.words = ws->d_tp_words; p.bits_len = ws->d_tp_len; p.base = ws->d_tp_base;
    p.status = ws->d_status_out;
    return p;
}

// per-query words and their scan: everything the bitmap kernel and the block layout need to know
static void tp_enqueue_layout(kaamer_workspace *ws, const TopPosParams &p, hipStream_t s)
{
    uint32_t gb = (ws->q_cap + 255) / 256;
    if (gb > (uint32_t)ws->n_cu * 8) gb = (uint32_t)ws->n_cu * 8;
    hipLaunchKernelGGL(top_pos_words_kernel, dim3(gb), dim3(256), 0, s, p);
    scan_u32_on(ws, ws->d_tp_words, ws->d_nq, ws->q_cap, ws->d_tp_base, s);
}

static int tp_check(const kaamer_index *ix, const kaamer_workspace *ws, const kaamer_topn_result *top, const char *who)
{
    if (!ix || !ws || !top) return kaamer_fail(KAAMER_E_ARG, "%s: bad argument", who);
    if (ix->device != ws->device) return kaamer_fail(KAAMER_E_ARG, "%s: workspace belongs to another device", who);
    if (ws->last_was_merge) return kaamer_fail(KAAMER_E_ARG, "%s: the workspace's last result is a merge: the probe results live on the shards", who);
    if (!ws->d_top_cnt || top->d_top_cnt != ws->d_top_cnt || top->d_top_pid != ws->d_top_pid || top->max_results < 1 || top->max_results > ws->topn_k)
        return kaamer_fail(KAAMER_E_ARG, "%s: not the result of this workspace's last kaamer_topn_device", who);
    return KAAMER_OK;
}

int kaamer_topn_positions_device(kaamer_index *ix, kaamer_workspace *ws, const kaamer_topn_result *top, uint64_t max_pos_words,
                                 void *stream, kaamer_topn_positions *out)
{
    if (!out) return kaamer_fail(KAAMER_E_ARG, "topn_positions_device: bad argument");
    int rc = tp_check(ix, ws, top, "topn_positions_device");
    if (rc) return rc;
    HIPCHK(hipSetDevice(ws->device));
    const uint64_t hard = tp_hard_words(ws, top->max_results);
    uint64_t cap = max_pos_words ? max_pos_words : tp_default_words(ws, top->max_results, 1);
    if (cap > hard) cap = hard;
    // the post-steps of a search whose counting stage ran on the count stream follow it there (kaamer_topn_device)
    const bool on_count_stream = ws->split_pending && ws->count_stream;
    hipStream_t s = on_count_stream ? ws->count_stream : (hipStream_t)stream;
    rc = tp_prepare(ws);
    if (rc) return rc;
    rc = reserve(ws->d_tp_bits, (size_t)cap, GROW_EXACT, s);   // (an earlier batch may still be writing it)
    if (rc) return rc;
    TopPosParams p = tp_params(ix, ws, top);
    p.bits = ws->d_tp_bits; p.cap = cap;
    tp_enqueue_layout(ws, p, s);
    hipLaunchKernelGGL(top_pos_bits_kernel, dim3(ws->n_cu * 8), dim3(64 * TP_WAVES), 0, s, p);
    if (on_count_stream) HIPCHK(hipEventRecord(ws->ev_count, s));
    HIPCHK(hipGetLastError());
    out->d_pos_base = ws->d_tp_base;
    out->d_pos_bits_len = ws->d_tp_len;
    out->d_pos_bits = (const uint64_t *)ws->d_tp_bits.get();
    out->pos_words_capacity = cap;
    return KAAMER_OK;
}

int kaamer_index_set_top_positions_bound(kaamer_index *ix, uint64_t words)
{
    if (!ix) return kaamer_fail(KAAMER_E_ARG, "index_set_top_positions_bound: bad argument");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    ix->top_pos_words = words;
    return KAAMER_OK;
}

// What the device's finalize step left as the next batch's table scale, worked out again on the host from the same
// counters: from a scale of 2 on, ORF batches take the pack kernel with the larger arena (tables of 200-500 slots).
static void ws_note_density(kaamer_workspace *ws, const kaamer_counters &c)
{
    if (!c.n_lookup || ws->pack_long) return;
    unsigned long long t = (c.n_hits * ws->slot_scale_margin + c.n_lookup - 1ull) / c.n_lookup;
    if (t > ws->slot_scale_cap) t = ws->slot_scale_cap;
    ws->dense_tables = t >= 2u * SLOT_SCALE_ONE;
}

int kaamer_workspace_finish(kaamer_workspace *ws, void *stream, kaamer_counters *out)
{
    if (!ws) return kaamer_fail(KAAMER_E_ARG, "workspace_finish: bad argument");
    HIPCHK(hipSetDevice(ws->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (ws->split_pending) HIPCHK(hipEventSynchronize(ws->ev_count));   // (the counting stage ran on the count stream)
    uint32_t st_g[2] = { 0, 0 };   // status, LIST_G entries of the last search
    HIPCHK(hipMemcpy(st_g, ws->d_status_out, sizeof st_g, hipMemcpyDeviceToHost));
    const uint32_t status = st_g[0];
    kaamer_counters c;
    HIPCHK(hipMemcpy(&c, ws->d_counters, sizeof c, hipMemcpyDeviceToHost));
    if (out) *out = c;
    if (!ws->last_was_merge) {
        ws_note_density(ws, c);
        ws->g_last = st_g[1];   // sizes the next search's G-tier launches (g_tier_grid)
    }
    if (status) { ws->clean = false; ws->g_last = G_LAST_UNKNOWN; }  // an aborted batch may leave per-batch state behind
    if (status & ST_POOL_FULL) return kaamer_fail(KAAMER_E_CAPACITY, "hit pool exhausted: raise workspace max_hits (now %llu)", (unsigned long long)ws->hit_cap);
    if (status & ST_LIST_FULL) return kaamer_fail(KAAMER_E_CAPACITY, "tier work list exhausted");
    if (status & ST_CHAIN_TIMEOUT) return kaamer_fail(KAAMER_E_HIP, "table layout: a tile never published its total");
    if (status & (ST_QUERY_CAP | ST_AA_CAP))
        return kaamer_fail(KAAMER_E_CAPACITY, "more ORFs than the workspace holds: raise workspace max_queries (now %u)", ws->q_cap);
    if (status & ST_EXCHANGE_CAP) return kaamer_fail(KAAMER_E_CAPACITY, "exchange block capacity exceeded (or the blocks do not describe one batch): raise max_entries_per_peer / max_queries of the exchange layout");
    if (status & ST_PEER_FAILED) return kaamer_fail(KAAMER_E_CAPACITY, "a peer's search of this batch exceeded one of its workspace bounds: nothing was merged (that rank's kaamer_workspace_finish says which bound)");
    if (status & ST_ALN_CAP) return kaamer_fail(KAAMER_E_CAPACITY, "more reported (query, hit) pairs than kaamer_topn_align_device provisioned: raise kaamer_topn_align_opts.max_pairs");
    if (status & ST_POS_CAP) return kaamer_fail(KAAMER_E_CAPACITY, "position bitmaps exceed the workspace: raise max_pos_words (now %llu)", (unsigned long long)ws->bits_cap);
    if (status & ST_G_ARENA_FULL)
        return kaamer_fail(KAAMER_E_CAPACITY, "global counting arena exhausted: raise workspace g_tier_slots (now %llu)", (unsigned long long)ws->g_slots);
    if (status) return kaamer_fail(KAAMER_E_CAPACITY, "device status 0x%x", status);
    return KAAMER_OK;
}

int kaamer_workspace_kernel_ms_sum(kaamer_workspace *ws, double *probe_ms, double *count_ms, double *total_ms,
                                   uint32_t *n_calls)
{
    if (!ws) return kaamer_fail(KAAMER_E_ARG, "kernel_ms_sum: bad argument");
    HIPCHK(hipSetDevice(ws->device));
    double a = 0, b = 0, c = 0;
    for (uint32_t i = 0; i < ws->n_timed; i++) {
        hipEvent_t *ev = ws->ev.data() + (size_t)i * EV_PER_CALL;
        float x = 0, y = 0, z = 0;
        HIPCHK(hipEventElapsedTime(&x, ev[1], ev[2]));
        HIPCHK(hipEventElapsedTime(&y, ev[2], ev[3]));
        HIPCHK(hipEventElapsedTime(&z, ev[0], ev[4]));
        a += x;
        b += y;
        c += z;
    }
    if (probe_ms) *probe_ms = a;
    if (count_ms) *count_ms = b;
    if (total_ms) *total_ms = c;
    if (n_calls) *n_calls = ws->n_timed;
    return KAAMER_OK;
}

void kaamer_workspace_reset_timers(kaamer_workspace *ws)
{
    if (ws) { ws->n_timed = 0; ws->call_no = 0; }
}

void kaamer_workspace_set_timing(kaamer_workspace *ws, uint32_t every)
{
    if (ws) { ws->time_every = every; ws->call_no = 0; }
}

// ------------------------------------------------------------------------------------
// host-buffer form
// ------------------------------------------------------------------------------------
// The hit arrays of kaamer_search_batch (tens of MB) land in pinned host memory: a D2H copy into fresh
// pageable memory runs at 2-3 GB/s here.  Pinned buffers are kept in a small process-wide cache.
extern "C++" {
namespace {
struct PinnedCache {
    std::mutex mu;
    std::vector<std::pair<void *, size_t>> free_list;
};
PinnedCache g_pinned;

void *pinned_get(size_t bytes, size_t *cap)
{
    {
        std::lock_guard<std::mutex> lock(g_pinned.mu);
        size_t best = (size_t)-1;
        for (size_t i = 0; i < g_pinned.free_list.size(); i++)
            if (g_pinned.free_list[i].second >= bytes && (best == (size_t)-1 || g_pinned.free_list[i].second < g_pinned.free_list[best].second)) best = i;
        if (best != (size_t)-1) {
            void *p = g_pinned.free_list[best].first;
            *cap = g_pinned.free_list[best].second;
            g_pinned.free_list.erase(g_pinned.free_list.begin() + (long)best);
            return p;
        }
    }
    void *p = nullptr;
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return nullptr;
    *cap = want;
    return p;
}

void pinned_put(void *p, size_t cap)
{
    std::lock_guard<std::mutex> lock(g_pinned.mu);
    if (g_pinned.free_list.size() < 32) g_pinned.free_list.emplace_back(p, cap);   // (four full-list callers hold twelve arrays at once)
    else (void)hipHostFree(p);
}

template <class T> struct PinnedArr {
    T *p = nullptr;
    size_t cap = 0;
    PinnedArr() = default;
    PinnedArr(const PinnedArr &) = delete;
    PinnedArr &operator=(const PinnedArr &) = delete;
    ~PinnedArr() { if (p) pinned_put(p, cap); }
    bool resize(size_t n)
    {
        if (p) { pinned_put(p, cap); p = nullptr; }
        p = (T *)pinned_get((n ? n : 1) * sizeof(T), &cap);
        return p != nullptr;
    }
    T *data() { return p; }
};
}  // namespace
}  // extern "C++"

struct batch_out_owner {
    kaamer_batch_out pub;
    std::vector<kaamer_query_meta> q;
    std::vector<uint64_t> hit_off;
    std::vector<uint32_t> hit_cnt;
    PinnedArr<uint32_t> pid, km, fp;
    std::vector<uint8_t> orf_aa;
    std::vector<int32_t> starts_alt;
    std::vector<uint64_t> pos_off, pos_bits;
};

// workspace + staging buffers of a host-buffer call: reused while they are large enough
static int host_slot_acquire(kaamer_index *ix, HostSlot &h, const kaamer_workspace_opts &need, uint64_t seq_bytes, uint32_t n_seqs)
{
    const kaamer_workspace_opts &o = h.opts;
    const bool fits = h.ws && o.seq_type == need.seq_type && o.first_pos == need.first_pos && o.want_positions == need.want_positions &&
                      o.compact == need.compact && o.max_seq_bytes >= need.max_seq_bytes && o.max_seqs >= need.max_seqs &&
                      o.max_hits >= need.max_hits && o.g_tier_slots >= need.g_tier_slots && o.max_queries >= need.max_queries &&
                      o.max_pos_words >= need.max_pos_words && (need.max_hits != 0 || o.max_hits == 0);
    if (!fits) {
        if (h.ws) { kaamer_workspace_free(h.ws); h.ws = nullptr; }
        kaamer_workspace_opts g = need;  // some headroom so that slightly larger batches do not rebuild it
        g.max_seq_bytes = need.max_seq_bytes + need.max_seq_bytes / 4 + 4096;
        g.max_seqs = need.max_seqs + need.max_seqs / 4 + 16;
        if (need.max_hits) g.max_hits = need.max_hits + need.max_hits / 4;
        if (need.max_pos_words) g.max_pos_words = need.max_pos_words + need.max_pos_words / 4;
        const int rc = kaamer_workspace_create(ix, &g, &h.ws);
        if (rc) { h.ws = nullptr; return rc; }
        h.opts = g;
    }
    const int rc = reserve(h.d_seqs, (size_t)seq_bytes, GROW_SLOT_SEQS, h.stream);
    return rc ? rc : reserve(h.d_off, (size_t)n_seqs, GROW_SLOT_OFF, h.stream);
}

// host buffers -> device, search enqueued on the slot's stream; nothing is waited for
static int search_batch_enqueue(kaamer_index *ix, HostSlot &slot, const kaamer_batch_in *in, const BatchBounds &b, kaamer_device_result *dr)
{
    const uint64_t seq_bytes = in->offsets[in->n_seqs];
    kaamer_workspace_opts o;
    memset(&o, 0, sizeof o);
    o.max_seq_bytes = seq_bytes;
    o.max_seqs = in->n_seqs ? in->n_seqs : 1;
    o.max_hits = b.max_hits;
    o.g_tier_slots = b.g_slots;
    o.seq_type = seq_base(in->seq_type);
    o.first_pos = 1;  // kaamer_batch_out always carries hit_first_pos
    o.want_positions = in->want_positions ? 1u : 0u;
    o.compact = 1u;  // the host form is CSR
    o.max_pos_words = b.max_hits * 8;
    o.max_queries = b.max_queries;
    int rc = host_slot_acquire(ix, slot, o, seq_bytes, in->n_seqs);
    if (rc) return rc;
    if (!slot.stream) HIPCHK(hipStreamCreateWithFlags(&slot.stream, hipStreamNonBlocking));
    hipStream_t s = slot.stream;
    hipError_t e = hipSuccess;
    if (seq_bytes) e = hipMemcpyAsync(slot.d_seqs, in->seqs, (size_t)seq_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(slot.d_off, in->offsets, ((size_t)in->n_seqs + 1) * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return kaamer_fail(KAAMER_E_HIP, "H2D: %s", hipGetErrorString(e));
    return kaamer_search_device(ix, slot.ws, slot.d_seqs, slot.d_off, in->n_seqs, seq_bytes, in->seq_type, s, dr);
}

// waits for the slot's stream and brings the full hit lists to the host
static int search_batch_collect(HostSlot &slot, const kaamer_batch_in *in, const kaamer_device_result &dr, kaamer_batch_out **out)
{
    kaamer_workspace *ws = slot.ws;
    batch_out_owner *bo = nullptr;
    hipStream_t s = slot.stream;
    kaamer_counters c;
    uint32_t nq = 0;
    uint64_t n_hits = 0, n_words = 0, n_sa = 0;
    unsigned long long n_aa = 0;
    hipError_t e;
    int rc = kaamer_workspace_finish(ws, s, &c);
    if (rc) goto done;
    bo = new (std::nothrow) batch_out_owner();
    if (!bo) { rc = kaamer_fail(KAAMER_E_NOMEM, "batch_out"); goto done; }
    // every copy on the slot's own stream (a plain hipMemcpy goes through the null stream, where concurrent callers
    // would queue behind each other); the host waits where it needs a value to size the next copy
    e = hipMemcpyAsync(&nq, dr.d_n_queries, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) { bo->q.resize(nq); bo->hit_off.resize((size_t)nq + 1); bo->hit_cnt.resize((size_t)nq + 1); }
    if (e == hipSuccess && nq) e = hipMemcpyAsync(bo->hit_cnt.data(), dr.d_hit_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && nq) e = hipMemcpyAsync(bo->q.data(), dr.d_q, (size_t)nq * sizeof(kaamer_query_meta), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(bo->hit_off.data(), dr.d_hit_off, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && ws->want_positions) e = hipMemcpyAsync(&n_words, ws->d_pos_base + nq, sizeof n_words, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && ws->nucleotide) {
        const size_t cap6 = (size_t)ws->max_seqs * 6;
        e = hipMemcpyAsync(&n_aa, ws->d_n_pos, sizeof n_aa, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&n_sa, ws->d_off3 + 2 * (cap6 + 1) + (size_t)in->n_seqs * 6, sizeof n_sa, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) {
        n_hits = bo->hit_off[nq];
        if (!bo->pid.resize(n_hits) || !bo->km.resize(n_hits) || !bo->fp.resize(n_hits)) e = hipErrorOutOfMemory;
        if (e == hipSuccess && n_hits) {
            e = hipMemcpyAsync(bo->pid.data(), dr.d_hit_pid, n_hits * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(bo->km.data(), dr.d_hit_kmatch, n_hits * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(bo->fp.data(), dr.d_hit_first_pos, n_hits * 4, hipMemcpyDeviceToHost, s);
        }
    }
    if (e == hipSuccess && ws->want_positions) {
        bo->pos_off.resize(n_hits + 1); bo->pos_bits.resize(n_words + 1);
        if (n_hits) e = hipMemcpyAsync(bo->pos_off.data(), dr.d_pos_off, n_hits * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && n_words) e = hipMemcpyAsync(bo->pos_bits.data(), dr.d_pos_bits, n_words * 8, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess && ws->nucleotide) {
        bo->orf_aa.resize(n_aa + 1); bo->starts_alt.resize(n_sa + 1);
        if (n_aa) e = hipMemcpyAsync(bo->orf_aa.data(), dr.d_orf_aa, n_aa, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && n_sa) e = hipMemcpyAsync(bo->starts_alt.data(), dr.d_starts_alt, n_sa * sizeof(int32_t), hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { rc = kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(e)); goto done; }
    memset(&bo->pub, 0, sizeof bo->pub);
    bo->pub.n_queries = nq;
    bo->pub.q = bo->q.data();
    bo->pub.hit_off = bo->hit_off.data();
    bo->pub.hit_cnt = bo->hit_cnt.data();
    bo->pub.hit_pid = bo->pid.data();
    bo->pub.hit_kmatch = bo->km.data();
    bo->pub.hit_first_pos = bo->fp.data();
    if (ws->nucleotide) { bo->pub.orf_aa = bo->orf_aa.data(); bo->pub.starts_alt = bo->starts_alt.data(); }
    if (ws->want_positions) { bo->pub.pos_off = bo->pos_off.data(); bo->pub.pos_bits = bo->pos_bits.data(); }
    bo->pub.counters = c;
    *out = &bo->pub;
    bo = nullptr;
done:
    delete bo;
    return rc;
}

static int search_batch_once(kaamer_index *ix, HostSlot &slot, const kaamer_batch_in *in, const BatchBounds &b, kaamer_batch_out **out)
{
    kaamer_device_result dr;
    const int rc = search_batch_enqueue(ix, slot, in, b, &dr);
    if (rc) return rc;
    return search_batch_collect(slot, in, dr, out);
}

// ---- the same call in two halves (the worker pool of search_protein.go:58-118 without a blocked thread per batch when
// the full hit lists are wanted: -pos, PositionHits).  submit copies the caller's buffers (they are borrowed for the call
// only), takes a slot, enqueues; wait collects, repeating the batch from the copy when a bound was too small.
struct kaamer_full_ticket {
    kaamer_index *ix;
    HostSlot *slot;
    std::vector<uint8_t> *seqs;
    std::vector<uint64_t> *offs;
    kaamer_batch_in in;
    kaamer_device_result dr;
    BatchBounds b;
    int attempt;
};

// a free slot (one whose workspace already serves this kind of batch, if there is one); callers beyond the slots wait
static HostSlot *host_slot_take(kaamer_index *ix, int32_t seq_type)
{
    seq_type = seq_base(seq_type);
    HostSlot *slot = nullptr;
    std::unique_lock<std::mutex> lock(ix->pool_mu);
    for (;;) {
        for (HostSlot &h : ix->host)
            if (!h.busy && (!slot || (h.ws && h.opts.seq_type == seq_type && !(slot->ws && slot->opts.seq_type == seq_type)))) slot = &h;
        if (slot) break;
        ix->pool_cv.wait(lock);
    }
    slot->busy = true;
    return slot;
}

static void host_slot_give(kaamer_index *ix, HostSlot *h)
{
    { std::lock_guard<std::mutex> lock(ix->pool_mu); h->busy = false; }
    ix->pool_cv.notify_all();
}

int kaamer_submit_batch_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                             int32_t want_positions, kaamer_full_ticket **ticket)
{
    if (!ix || !ticket || !offsets || (n_seqs && !seqs)) return kaamer_fail(KAAMER_E_ARG, "submit_batch: bad argument");
    *ticket = nullptr;
    SEQ_TYPE_CHK(seq_type, "submit_batch");
    HIPCHK(hipSetDevice(ix->device));
    kaamer_full_ticket *t = new (std::nothrow) kaamer_full_ticket();
    if (!t) return kaamer_fail(KAAMER_E_NOMEM, "ticket");
    memset(t, 0, sizeof *t);
    t->ix = ix;
    t->seqs = new (std::nothrow) std::vector<uint8_t>(seqs, seqs + offsets[n_seqs]);
    t->offs = new (std::nothrow) std::vector<uint64_t>(offsets, offsets + n_seqs + 1);
    if (!t->seqs || !t->offs) { delete t->seqs; delete t->offs; delete t; return kaamer_fail(KAAMER_E_NOMEM, "ticket"); }
    t->in.seqs = t->seqs->data(); t->in.offsets = t->offs->data(); t->in.n_seqs = n_seqs; t->in.seq_type = seq_type;
    t->in.want_positions = want_positions;
    t->b.max_hits = full_start_hits(offsets[n_seqs]);
    t->slot = host_slot_take(ix, seq_type);
    const int rc = search_batch_enqueue(ix, *t->slot, &t->in, t->b, &t->dr);
    if (rc && rc != KAAMER_E_CAPACITY) {
        if (t->slot->stream) (void)hipStreamSynchronize(t->slot->stream);
        host_slot_give(ix, t->slot);
        delete t->seqs; delete t->offs; delete t;
        return rc;
    }
    if (rc) t->attempt = -1;   // (a bound refused on the host already: wait starts with the retry)
    *ticket = t;
    return KAAMER_OK;
}

int kaamer_wait_batch(kaamer_full_ticket *t, kaamer_batch_out **out)
{
    if (!t || !out) return kaamer_fail(KAAMER_E_ARG, "wait_batch: bad argument");
    *out = nullptr;
    kaamer_index *ix = t->ix;
    int rc = hipSetDevice(ix->device) == hipSuccess ? KAAMER_OK : kaamer_fail(KAAMER_E_HIP, "hipSetDevice");
    while (!rc) {
        rc = t->attempt < 0 ? KAAMER_E_CAPACITY : search_batch_collect(*t->slot, &t->in, t->dr, out);
        if (t->attempt < 0) t->attempt = 0;
        if (rc != KAAMER_E_CAPACITY || t->attempt >= MAX_BOUND_RETRIES) break;
        t->attempt++;
        bounds_grow(t->b, t->in.offsets[t->in.n_seqs], t->in.n_seqs, is_nucl(t->in.seq_type));
        rc = search_batch_enqueue(ix, *t->slot, &t->in, t->b, &t->dr);   // (an error here, E_CAPACITY included, ends the loop: kept as it was)
    }
    if (rc && t->slot->stream) (void)hipStreamSynchronize(t->slot->stream);
    host_slot_give(ix, t->slot);
    delete t->seqs; delete t->offs; delete t;
    return rc;
}

void kaamer_full_ticket_discard(kaamer_full_ticket *t)
{
    if (!t) return;
    (void)hipSetDevice(t->ix->device);
    if (t->slot->stream) (void)hipStreamSynchronize(t->slot->stream);
    if (t->slot->ws) t->slot->ws->clean = false;
    host_slot_give(t->ix, t->slot);
    delete t->seqs; delete t->offs; delete t;
}

int kaamer_search_batch(kaamer_index *ix, const kaamer_batch_in *in, kaamer_batch_out **out)
{
    if (!ix || !in || !out || !in->offsets || (in->n_seqs && !in->seqs)) return kaamer_fail(KAAMER_E_ARG, "search_batch: bad argument");
    *out = nullptr;
    SEQ_TYPE_CHK(in->seq_type, "search_batch");
    HIPCHK(hipSetDevice(ix->device));
    HostSlot *slot = host_slot_take(ix, in->seq_type);
    struct Release {
        kaamer_index *ix; HostSlot *h;
        ~Release() { host_slot_give(ix, h); }
    } release{ ix, slot };
    BatchBounds b = { full_start_hits(in->offsets[in->n_seqs]), 0, 0 };
    for (int attempt = 0;; attempt++) {
        const int rc = search_batch_once(ix, *slot, in, b, out);
        if (rc != KAAMER_E_CAPACITY || attempt >= MAX_BOUND_RETRIES) return rc;
        bounds_grow(b, in->offsets[in->n_seqs], in->n_seqs, is_nucl(in->seq_type));
    }
}

#include "host_top.hip.inc"
#include "host_top_align.hip.inc"
#include "host_text.hip.inc"
#include "host_out.hip.inc"
#include "host_tsv.hip.inc"
#include "host_json.hip.inc"
#include "host_out_text.hip.inc"
#include "host_sharded.hip.inc"
#include "host_sharded_submit.hip.inc"
#include "host_sharded_collect.hip.inc"
#include "host_replicas.hip.inc"
#include "host_text_file.hip.inc"
#include "host_sharded_stream.hip.inc"

void kaamer_batch_free(kaamer_batch_out *out)
{
    if (!out) return;
    delete reinterpret_cast<batch_out_owner *>(out);  // pub is the first member
}

}  // extern "C"
