// count_global.hip.inc — the G tier: the queries whose distinct hits exceed their LDS table (count_group.hip.inc,
// count_pack.hip.inc) and the ORFs count_pack_kernel sends on uncounted (a "fresh" item, wi.size < 0).  Included by
// search.hip after count_window.hip.inc and finalize_body.  One workgroup of G_WAVES waves per item, items by ticket.
//
// The stages of an item; each is a function below and count_global_kernel's item loop is this list:
//   g_count_postings   a sweep that only sums the query's postings (post): it sizes everything that follows
//   g_lds_attempt      the WHOLE query in the LDS table.  Holds with at most BigLdsTable::LIMIT distinct hits and no id
//                      walking 128 slots; a query of 65 535 k-mers or more (a position is 16 bits of a table word) skips it
//   g_partitioned      else: the postings are scattered into R id-range buckets in the G arena and every bucket is counted
//                      in the LDS table on its own.  Bucket sizes are GUESSED first and COUNTED by one more sweep when a
//                      guessed bucket was full (bucket_full)
//   g_hbm_table        else (a bucket with more distinct ids than the LDS table holds): a table in the G arena
//   g_publish          q_cnt, hit_off, the hit and monster tallies -- once, whatever stage ended the item
// A stage's GOutcome is the same in every thread: G_DONE, G_NO_SPACE (an arena or the hit arrays are full: the status bit
// is set and the query publishes no hits, never a partial list) or G_TABLE_FULL (on to the next stage).
//
// LDS is ONE struct, GShared, declared once, its size pinned by a static_assert (two workgroups per CU); its members say
// which stage owns them.  g_reset_attempt zeroes nd, fail, out_cursor, bucket_full and sink.n -- thread 0, before a
// barrier -- when an item and when an attempt (a table, a partition) begins.  Functions take `GShared &` or pointers to
// members and are inlined: the compiler sees the __shared__ object and the accesses stay ds_* (count_window.hip.inc).
//
// BARRIER RULE.  Every __syncthreads() is reached by all 64 * G_WAVES threads.  Whatever decides whether one is reached --
// a branch, a loop exit, a GOutcome -- comes from LDS words read AFTER a barrier that follows their last write (fail, nd,
// off, base, bucket_full, sink.n) or from values equal in every thread (size, fresh, R, attempt), never from a lane's or
// a wave's own `ok`: a wave whose add found no slot sets `fail` and goes on to the same barriers.
//
// Memory: buckets and HBM table are regions of the G arena that g_cursor hands to ONE workgroup, once per launch, written
// by its stores and workgroup-scope atomics and read back by it after a barrier (which drains vmcnt); the reasoning is next
// to the code (GlobalTable in search.hip, g_partitioned, g_hbm_table).  No agent-scope fence: a full L2 write-back here.
//
// count_windows is NOT count_window.hip.inc's flatten (a head carries three ids, runs are merged per head slot, long lists
// go to the sink); it shares the wave scan, the owner search and the work counters.

#ifndef G_MIN_BLOCKS
#define G_MIN_BLOCKS 1
#endif
#ifndef G_NWIN
#define G_NWIN 2   /* windows of 64 positions a wave has in flight in the G tier's sweeps */
#endif
#ifndef G_EXPAND_UNROLL
#define G_EXPAND_UNROLL 8  /* measured on the skewed batch: 4 -> 5.28 ms, 8 -> 4.36, 16 -> 4.42, 32 -> 4.55 */
#endif

// ---- the tables a sweep adds to: add_n(id, position, n, nnew) ---------------------------------------------------------
// `nnew` counts the entries this lane created, for tables whose distinct-hit counter (nd) is bumped once per wave

// The G tier's first attempt: a table of 8192 slots in LDS (64 KB: protein id | count in the low and lowest position in the
// high 16 bits of one word, so the query must be shorter than 65 535 k-mers).  A query of a skewed database that overflows
// its group table typically has a few thousand distinct hits behind tens of thousands of postings: here those postings
// are LDS atomics instead of line fills and write-backs of a multi-megabyte table in HBM.
#define BIG_LOG2CAP 13
struct BigLdsTable {
    uint32_t *keys, *val, *nd;
    static constexpr uint32_t CAP = 1u << BIG_LOG2CAP;
    static constexpr uint32_t LIMIT = CAP - CAP / 4;  // keep 25 % free
    __device__ __forceinline__ bool add_n(uint32_t pid, uint32_t pos, uint32_t n, uint32_t &nnew) const
    {
        uint32_t h = (pid * 0x9E3779B1u) >> (32 - BIG_LOG2CAP);
        for (uint32_t t = 0; t < 128u; t++) {  // a table this crowded is handed to the HBM path
            uint32_t k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (k == KH_EMPTY_PID) {
                const uint32_t old = atomicCAS(&keys[h], KH_EMPTY_PID, pid);
                // the distinct hits are counted as they come (at most 8192 bumps of one LDS word per query): the attempt is
                // given up the moment the table is three quarters full, not after every further id has walked a full table
                if (old == KH_EMPTY_PID) { k = pid; if (atomicAdd(nd, 1u) >= LIMIT) return false; }
                else k = old;
            }
            if (k == pid) {
                atomicAdd(&val[h], n);  // counts stay below 65 536: one per position of the query at most
                uint32_t old = __hip_atomic_load(&val[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                while (pos < (old >> 16)) {
                    const uint32_t seen = atomicCAS(&val[h], old, (old & 0xFFFFu) | (pos << 16));
                    if (seen == old) break;
                    old = seen;
                }
                return true;
            }
            h = (h + 1u) & (CAP - 1u);
        }
        return false;
    }
};

// A query with more distinct hits than the LDS table holds is partitioned by protein-id range (g_partitioned):
// these two "tables" take the place of a counting table in the postings sweep -- the first counts the items per range,
// the second writes them to their range's bucket.  An item is (protein id, position | run length << 16).
#define G_MAX_RANGES 64u
__device__ __forceinline__ uint32_t g_range_of(uint32_t pid, uint32_t R) { return (uint32_t)(((uint64_t)(pid * 0x85EBCA6Bu) * R) >> 32); }
struct RangeHist {
    uint32_t *cnt, *nd;
    uint32_t R;
    __device__ __forceinline__ bool add_n(uint32_t pid, uint32_t, uint32_t, uint32_t &) const { atomicAdd(&cnt[g_range_of(pid, R)], 1u); return true; }
};
struct RangeScatter {
    uint32_t *cur, *nd;
    uint2 *items;
    uint32_t R;
    const uint32_t *first;  // first item of every bucket
    uint32_t cap;           // items a bucket holds (guessed sizes: the same for all; counted sizes: no limit)
    uint32_t *full;         // set when a bucket is full
    __device__ __forceinline__ bool add_n(uint32_t pid, uint32_t pos, uint32_t n, uint32_t &) const
    {
        const uint32_t r = g_range_of(pid, R);
        const uint32_t at = atomicAdd(&cur[r], 1u);
        if (at - first[r] < cap) items[at] = make_uint2(pid, pos | (n << 16));
        else *full = 1u;
        return true;
    }
};

// the sizing sweep adds nothing
struct NullTable {
    uint32_t *nd;
    __device__ __forceinline__ bool add_n(uint32_t, uint32_t, uint32_t, uint32_t &) const { return true; }
};

// PositionHits of the G-tier queries (search.go:442-452): the query's final hit list goes into a
// table in HBM (id -> index in the list), then every (position, id) sets one bit of that hit's bitmap.
struct BitsTable {
    const uint32_t *slots;  // 4 words per slot: {protein id, index in the hit list, -, -}
    uint32_t *nd;
    uint32_t log2cap, words;
    unsigned long long *bits;  // first bitmap of the query
    __device__ __forceinline__ bool add_n(uint32_t pid, uint32_t pos, uint32_t n, uint32_t &) const
    {
        const uint32_t mask = (1u << log2cap) - 1u;
        uint32_t h = (pid * 0x9E3779B1u) >> (32 - log2cap);
        for (uint32_t t = 0; t <= mask; t++) {
            const uint32_t k = __hip_atomic_load(&slots[4ull * h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == pid) {
                unsigned long long *bm = bits + (unsigned long long)__hip_atomic_load(&slots[4ull * h + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * words;
                const uint32_t w0 = pos >> 6, b0 = pos & 63u;
                const uint32_t n0 = n < 64u - b0 ? n : 64u - b0;
                atomicOr(&bm[w0], (n0 == 64u ? ~0ull : ((1ull << n0) - 1ull)) << b0);
                if (n > n0) atomicOr(&bm[w0 + 1], (1ull << (n - n0)) - 1ull);
                return true;
            }
            if (k == KH_EMPTY_PID) return false;  // cannot happen: every id of the postings is a hit
            h = (h + 1u) & mask;
        }
        return false;
    }
};

// ---- the window -------------------------------------------------------------------------------------------------------
// Adjacent positions of a query mostly hit the same proteins (a homologous stretch), so
// lane i and lane i+1 usually carry the same id in the same head slot.  Sixty-four lanes
// adding to one LDS word serialise; instead the first lane of every run of equal ids adds
// the whole run at once (run length from a ballot of the change points).
template <class Table>
__device__ __forceinline__ bool add_runs(const Table &tab, uint32_t x, uint32_t pos, uint32_t &nnew)
{
    const uint32_t lane = lane_id();
    const uint32_t prev = __shfl_up(x, 1, 64);
    const bool change = (lane == 0) || (prev != x);
    const unsigned long long cm = __ballot(change);
    bool ok = true;
    if (change && x != KH_EMPTY_PID) {
        const unsigned long long above = (lane == 63) ? 0ull : (cm >> (lane + 1));
        const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : 64u - lane;
        ok = tab.add_n(x, pos, len, nnew);
    }
    return ok;
}

// Postings lists of more than LONG_LIST ids are not expanded by the wave that meets them: they go on a list in
// LDS and the whole workgroup expands them afterwards, FLAT -- item t of all the lists together belongs to the list found
// by binary search in the prefix of their lengths -- a thread per id (g_expand_sink).  One wave walking a 9 000-protein
// list 64 ids at a time, for each of the 21 positions of a shared motif, is 3 000 dependent round trips while the other
// waves wait.
#define LONG_LIST 8u
#define LONG_SINK_CAP 960u   /* 15 entries per lane; with 1024 the kernel's LDS was 56 bytes over half a CU's: one workgroup per CU */
#define LONG_SINK_LIFT 512u  /* first step of the binary lifting over the prefix: the largest power of two below the capacity */
struct LongSink {
    uint32_t n;
    uint32_t off[LONG_SINK_CAP], pos[LONG_SINK_CAP], cnt[LONG_SINK_CAP];  // cnt becomes the exclusive prefix
    uint32_t total;
};

// NWIN 64-position windows of one query, processed by one wave with all their memory
// round trips overlapped: (1) the probe results of every window, (2) the 16-byte heads of
// every postings list (count + first three ids), (3) the remaining ids of all lists,
// spread evenly over the 64 lanes whatever the individual list lengths are (per-window
// prefix sum of the leftovers, owner found by binary search in LDS), then the counter
// increments (KCombStore.Get + the id loop of search.go:427-436).  Window k starts at
// c0 + k*stride.  `pref` is NWIN * 64 words of LDS private to the wave.  No workgroup
// barriers inside.  COUNT_ONLY: only sum the postings (the sizing sweep).  With a `sink`, long lists go there while it
// has room.  -> false (in every lane) when an add of this wave found no slot.
template <class Table, int NWIN, bool COUNT_ONLY>
__device__ __forceinline__ bool count_windows(const CountParams &p, const uint32_t *vals,
                                              int32_t size, int32_t c0, int32_t stride, const Table &tab, WorkCount &c,
                                              uint32_t *pref, LongSink *sink = nullptr)
{
    const uint32_t lane = lane_id();
    uint32_t v[NWIN];
    uint4 h[NWIN];
#pragma unroll
    for (int k = 0; k < NWIN; k++) {
        const int32_t pos = c0 + k * stride + (int32_t)lane;
        v[k] = 0u;
        h[k] = make_uint4(0, 0, 0, 0);
        if (pos < size) {
            v[k] = vals[pos];
            if (v[k] & KH_INLINE_BIT) h[k] = make_uint4(1u, v[k] & ~KH_INLINE_BIT, 0, 0);
            else if (v[k] != 0u) h[k] = reinterpret_cast<const uint4 *>(p.arena)[v[k]];  // {count, id0, id1, id2}
        }
        if (!COUNT_ONLY && sink && h[k].x > LONG_LIST) {
            const uint32_t slot = atomicAdd(&sink->n, 1u);
            if (slot < LONG_SINK_CAP) {  // (a full list: the wave expands it itself, below)
                sink->off[slot] = v[k]; sink->pos[slot] = (uint32_t)pos; sink->cnt[slot] = h[k].x;
                c.list(v[k], h[k].x);
                h[k] = make_uint4(0, 0, 0, 0);
                v[k] = 0u;
            }
        }
    }
    bool ok = true;
    uint32_t nnew = 0;
    // leftovers (ids beyond the three that came with the head): all their loads are issued
    // before anything is consumed
    constexpr int XIT = 2;  // leftover rounds kept in registers per window (64 ids each)
    uint32_t xid[NWIN][XIT], xpos[NWIN][XIT];
    uint32_t xtotal[NWIN];
    if (!COUNT_ONLY) {
#pragma unroll
        for (int k = 0; k < NWIN; k++) {
            const uint32_t lcnt = h[k].x;
            const uint32_t extra = lcnt > 3u ? lcnt - 3u : 0u;
            const uint32_t inc = wave_inclusive_scan_dpp(extra);
            xtotal[k] = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            pref[k * 64 + lane] = inc - extra;  // exclusive prefix
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < NWIN; k++) {
            const uint32_t *wpref = pref + k * 64;
#pragma unroll
            for (int it = 0; it < XIT; it++) {
                const uint32_t t = (uint32_t)it * 64u + lane;
                const bool act = t < xtotal[k];
                const uint32_t lo = act ? flatten_owner(wpref, t) : 0u;  // largest lane with pref[lane] <= t owns leftover t
                // executed by all lanes: the owner may be a lane that is idle in this round
                const uint32_t off = __shfl(v[k], (int)lo, 64);
                xid[k][it] = KH_EMPTY_PID;
                xpos[k][it] = (uint32_t)(c0 + k * stride) + lo;
                if (act) xid[k][it] = p.arena[(uint64_t)off * 4 + 4 + (t - wpref[lo])];
            }
        }
        // very long lists (more than XIT*64 leftovers in one window): counted as they arrive
#pragma unroll
        for (int k = 0; k < NWIN; k++) {
            const uint32_t *wpref = pref + k * 64;
            for (uint32_t t0 = XIT * 64u; t0 < xtotal[k]; t0 += 64) {
                const uint32_t t = t0 + lane;
                const bool act = t < xtotal[k];
                const uint32_t lo = act ? flatten_owner(wpref, t) : 0u;
                const uint32_t off = __shfl(v[k], (int)lo, 64);
                if (act) ok = ok && tab.add_n(p.arena[(uint64_t)off * 4 + 4 + (t - wpref[lo])], (uint32_t)(c0 + k * stride) + lo, 1u, nnew);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // heads: inline ids and the first three ids of every list
#pragma unroll
    for (int k = 0; k < NWIN; k++) {
        const uint32_t pos = (uint32_t)(c0 + k * stride) + lane;
        const uint32_t lcnt = h[k].x;
        c.list(v[k], lcnt);
        if (!COUNT_ONLY) {  // all lanes take part: run heads add for their whole run
            ok = add_runs(tab, lcnt > 0 ? h[k].y : KH_EMPTY_PID, pos, nnew) && ok;
            ok = add_runs(tab, lcnt > 1 ? h[k].z : KH_EMPTY_PID, pos, nnew) && ok;
            ok = add_runs(tab, lcnt > 2 ? h[k].w : KH_EMPTY_PID, pos, nnew) && ok;
        }
    }
    if (!COUNT_ONLY) {
#pragma unroll
        for (int k = 0; k < NWIN; k++)
#pragma unroll
            for (int it = 0; it < XIT; it++)
                if (xid[k][it] != KH_EMPTY_PID) ok = ok && tab.add_n(xid[k][it], xpos[k][it], 1u, nnew);
        const uint32_t wave_new = wave_total(nnew);
        if (lane == 0 && wave_new) atomicAdd(tab.nd, wave_new);
    }
    return __all(ok);
}

// One sweep of the query by the workgroup: every wave takes NWIN windows per round.  -> false when an add of THIS wave
// found no slot (a wave's own view: it must not steer a barrier); `fail`, when given, is set as well, and with STOP the
// wave gives the rest of the sweep up once anybody has set it.
template <class Table, bool COUNT_ONLY, bool STOP = false, int NWIN = G_NWIN>
__device__ __forceinline__ bool g_sweep(const CountParams &p, const uint32_t *vals, int32_t size, const Table &tab, WorkCount &c,
                                        uint32_t *wave_pref, LongSink *sink = nullptr, uint32_t *fail = nullptr)
{
    const int32_t wv = (int32_t)(threadIdx.x >> 6);
    bool all_ok = true;
    for (int32_t r0 = 0; r0 < size; r0 += 64 * G_WAVES * NWIN) {
        if (STOP && *fail) break;
        const bool ok = count_windows<Table, NWIN, COUNT_ONLY>(p, vals, size, r0 + 64 * wv, 64 * G_WAVES, tab, c, wave_pref, sink);
        if (!ok) {
            all_ok = false;
            if (fail) *fail = 1;
        }
    }
    return all_ok;
}

// Thread 0: `slots` 16-byte slots of the G arena for this workgroup alone -> *out, ~0 (and ST_G_ARENA_FULL) when the
// arena has no room.  The others read *out after a barrier.
__device__ __forceinline__ void g_arena_take(const CountParams &p, unsigned long long slots, unsigned long long *out)
{
    const unsigned long long off = atomicAdd(p.g_cursor, slots);
    if (off + slots > p.g_slots) { atomicOr(p.status, (uint32_t)ST_G_ARENA_FULL); *out = ~0ull; }
    else *out = off;
}

// Writes the occupied slots of a table of `cap` slots (a multiple of 64) to the hit arrays from entry `base` on, in the
// order the waves get to them: slot(i, id, count, lowest position) reads slot i.  STRIPES stripes of 64 * G_WAVES slots
// are read per round trip.  `cursor` (LDS, zero on entry) counts the entries written.
template <int STRIPES, class Idx, class Slot>
__device__ __forceinline__ void g_read_out(const CountParams &p, unsigned long long base, Idx cap, uint32_t *cursor, Slot slot)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (Idx i0 = (Idx)wv * 64; i0 < cap; i0 += (Idx)STRIPES * 64 * G_WAVES) {
        uint32_t k[STRIPES], c[STRIPES], m[STRIPES];
#pragma unroll
        for (int u = 0; u < STRIPES; u++) {
            const Idx i = i0 + (Idx)u * 64 * G_WAVES + lane;
            slot(i < cap ? i : cap - 1, k[u], c[u], m[u]);
            if (i >= cap) k[u] = KH_EMPTY_PID;
        }
#pragma unroll
        for (int u = 0; u < STRIPES; u++) {
            const bool has = k[u] != KH_EMPTY_PID;
            const unsigned long long bm = __ballot(has);
            uint32_t wbase = 0;
            if (lane == 0 && bm) wbase = atomicAdd(cursor, (uint32_t)__popcll(bm));
            wbase = __shfl(wbase, 0, 64);
            if (has) {
                const unsigned long long idx = base + wbase + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
                p.hit_pid[idx] = k[u];
                p.hit_km[idx] = c[u];
                p.hit_fp[idx] = m[u];
            }
        }
    }
}

// ---- count_global_kernel: state, clock, stages ------------------------------------------------------------------------
struct GShared {
    uint32_t keys[BigLdsTable::CAP], val[BigLdsTable::CAP];  // the LDS table: g_table_clear, the adds, g_table_flush
    uint32_t pref[G_WAVES][G_NWIN * 64];                     // count_windows: private to a wave, rewritten by every window
    LongSink sink;                                           // count_windows pushes, g_expand_sink reads
    uint32_t roff[G_MAX_RANGES], rcur[G_MAX_RANGES];         // g_partitioned: first item / cursor (after the scatter: end) of every bucket
    unsigned long long post;                                 // g_count_postings writes, every later stage reads
    unsigned long long off;                                  // g_arena_take's answer (buckets, HBM table)
    unsigned long long base;                                 // first entry of the query's hit list (~0: none yet): g_table_flush, g_hbm_table
    uint32_t rtotal, reserved;                               // items in all buckets; entries the list may take (<= n_proteins: 32 bits)
    uint32_t nd, fail;                                       // the table being filled: distinct ids / "an add found no slot" (2: no space for the list)
    uint32_t out_cursor;                                     // g_read_out: entries written from the table being read
    uint32_t bucket_full;                                    // RangeScatter: a guessed bucket had no room
    uint32_t item, last;                                     // the next ticket; "this workgroup finalizes the batch"
};
static_assert(sizeof(GShared) <= 81728, "count_global_kernel: more LDS than this and a CU holds one workgroup instead of two");

enum GOutcome { G_DONE, G_NO_SPACE, G_TABLE_FULL };

// fresh: the query was sent here unseen (its table does not fit a wave's arena, count_pack.hip.inc), so its postings have not
// been counted anywhere yet; otherwise it overflowed its table and they have
struct GItem { uint32_t q; int32_t size; bool fresh; const uint32_t *vals; };

// what a workgroup adds to the batch's counters when it has run out of items (lane-private; wave 0 holds the hits)
struct GTally {
    unsigned long long hits = 0, mon_hits = 0, post = 0, lists = 0, lids = 0;
    uint32_t monsters = 0;
};

// tools/phase_clock_gtier.py: where the G tier's time goes, per workgroup (thread 0): the named laps and tallies of
// g_gtier_clock's columns.  In normal builds the struct is empty and every call below is an empty inline function.
enum GLap { GL_POSTINGS = 0, GL_LDS = 1, GL_PARTITION = 2, GL_BUCKETS = 3, GL_TOTAL = 4, GL_N_IN_LDS = 5, GL_N_PARTITIONED = 6,
            GL_POST_PARTITIONED = 7, GL_LONGEST = 8, GL_LONGEST_POST = 9, GL_LONGEST_TOTAL = 10 };
#ifdef KAAMER_PHASE_CLOCK
__device__ unsigned long long g_gtier_clock[2048][16];
#define G_CLOCKED(...) { if (threadIdx.x == 0) { __VA_ARGS__ } }
#else
#define G_CLOCKED(...) { }
#endif
struct GClock {
#ifdef KAAMER_PHASE_CLOCK
    unsigned long long acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, start = 0, t = 0, t0 = 0;
#endif
    __device__ __forceinline__ void begin() G_CLOCKED(start = wall_clock64();)
    __device__ __forceinline__ void begin_item() G_CLOCKED(t = t0 = wall_clock64();)
    __device__ __forceinline__ void lap(GLap i) G_CLOCKED(const unsigned long long now = wall_clock64(); acc[i] += now - t; t = now;)
    __device__ __forceinline__ void partitioned(unsigned long long post) G_CLOCKED(acc[GL_N_PARTITIONED] += 1; acc[GL_POST_PARTITIONED] += post;)
    __device__ __forceinline__ void done_in_lds(unsigned long long post) G_CLOCKED(
        const unsigned long long d = wall_clock64() - t0;
        acc[GL_N_IN_LDS] += 1;
        if (d > acc[GL_LONGEST]) { acc[GL_LONGEST] = d; acc[GL_LONGEST_POST] = post; })
    __device__ __forceinline__ void end() G_CLOCKED(
        if (blockIdx.x >= 2048) return;
        unsigned long long *out = g_gtier_clock[blockIdx.x];
        acc[GL_TOTAL] = wall_clock64() - start;
        for (int i = 0; i < 8; i++) out[i] += acc[i];
        if (acc[GL_LONGEST] > out[GL_LONGEST]) { out[GL_LONGEST] = acc[GL_LONGEST]; out[GL_LONGEST_POST] = acc[GL_LONGEST_POST]; }
        if (acc[GL_TOTAL] > out[GL_LONGEST_TOTAL]) out[GL_LONGEST_TOTAL] = acc[GL_TOTAL];)
};
#undef G_CLOCKED

// thread 0, before a barrier: the words an attempt (a table, a partition) starts from
__device__ __forceinline__ void g_reset_attempt(GShared &s)
{
    if (threadIdx.x == 0) { s.nd = 0; s.fail = 0; s.out_cursor = 0; s.bucket_full = 0; s.sink.n = 0; }
}

// The long postings lists a sweep set aside, expanded by all threads into `tab`.  Called after a barrier that follows the
// sweep; has one barrier inside.
template <class Table>
__device__ __forceinline__ void g_expand_sink(const CountParams &p, GShared &s, const Table &tab)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    LongSink &sk = s.sink;
    const uint32_t nl = sk.n < LONG_SINK_CAP ? sk.n : LONG_SINK_CAP;
    if (wv == 0 && nl) {  // lengths -> exclusive prefix (15 entries per lane)
        constexpr uint32_t PER = LONG_SINK_CAP / 64;
        uint32_t sum = 0;
        for (uint32_t i = 0; i < PER; i++) { const uint32_t e = lane * PER + i; sum += e < nl ? sk.cnt[e] : 0u; }
        const uint32_t inc = wave_inclusive_scan_dpp(sum);
        uint32_t run = inc - sum;
        for (uint32_t i = 0; i < PER; i++) {
            const uint32_t e = lane * PER + i;
            if (e < nl) { const uint32_t c = sk.cnt[e]; sk.cnt[e] = run; run += c; }
        }
        if (lane == 63) sk.total = inc;
    }
    __syncthreads();
    uint32_t nnew = 0;
    bool ok = true;
    const uint32_t total = nl ? sk.total : 0u;
    // Eight items per thread and round, their arena loads all issued before the first id is used, and the list of an
    // item found from the previous item's (the next item of a thread is 512 further on: the same list, or the one
    // after it) instead of a ten-step search in LDS per id.  One dependent (search -> load -> add) chain per id made
    // a monster query's sweep ~1 500 cycles per id and thread: 0.6 ms for half a million postings, three sweeps per
    // query, and the tier ended when the slowest workgroup had done two of them (4.5 ms per skewed batch).
    constexpr int EU = G_EXPAND_UNROLL;
    uint32_t e = 0;  // largest e with prefix[e] <= the thread's current item
    auto find_list = [&](uint32_t t) {
        if (e + 1u < nl && sk.cnt[e + 1u] <= t) {      // not in the current list any more
            e++;
            if (e + 1u < nl && sk.cnt[e + 1u] <= t) {  // nor in the next one: search
                e = 0;
#pragma unroll
                for (uint32_t sft = LONG_SINK_LIFT; sft > 0; sft >>= 1)
                    if (e + sft < nl && sk.cnt[e + sft] <= t) e += sft;
            }
        }
    };
    for (uint32_t t0 = tid; t0 < total; t0 += EU * 64 * G_WAVES) {
        if (s.fail) break;  // (the table gave up: no point in the rest)
        uint32_t ids[EU], pos_[EU];
#pragma unroll
        for (int u = 0; u < EU; u++) {
            const uint32_t t = t0 + (uint32_t)u * 64 * G_WAVES;
            const uint32_t tt = t < total ? t : total - 1u;  // (clamped: the load is issued whatever; used only if t < total)
            find_list(tt);
            ids[u] = p.arena[(uint64_t)sk.off[e] * 4 + 1 + (tt - sk.cnt[e])];
            pos_[u] = sk.pos[e];
        }
#pragma unroll
        for (int u = 0; u < EU; u++)
            if (t0 + (uint32_t)u * 64 * G_WAVES < total)
                if (!tab.add_n(ids[u], pos_[u], 1u, nnew)) { ok = false; s.fail = 1; }
    }
    const uint32_t wn = wave_total(nnew);
    if (lane == 0 && wn) atomicAdd(&s.nd, wn);
    if (!ok) s.fail = 1;
}

// One pass over the query into `tab` by the whole workgroup: the sweep, then the long lists it set aside.  One barrier
// inside; the caller's barriers before and after.  (What it meets was counted already: by the kernel that sent the query
// here, or by g_count_postings.)  STOP: the waves give the sweep up once `fail` is set.
template <class Table, bool STOP = false>
__device__ __forceinline__ void g_pass(const CountParams &p, GShared &s, const GItem &it, const Table &tab)
{
    WorkCount wc;
    g_sweep<Table, false, STOP>(p, it.vals, it.size, tab, wc, s.pref[threadIdx.x >> 6], &s.sink, &s.fail);
    __syncthreads();
    g_expand_sink(p, s, tab);
}

// the item's words, and the workgroup's next item by ticket (after the first one): a query here costs anything from
// microseconds to milliseconds, and two expensive ones on the same workgroup's static share were the tier's tail
__device__ __forceinline__ uint32_t g_begin_item(const CountParams &p, GShared &s, uint32_t n_part)
{
    g_reset_attempt(s);
    if (threadIdx.x == 0) {
        s.post = 0;
        s.item = atomicAdd(p.queue_head + (SLOT_G_TICKET - SLOT_QUEUE_HEAD), 1u) + n_part;
    }
    __syncthreads();
    return s.item;
}

// exact number of postings (an upper bound of the distinct proteins) -> s.post; a fresh item's work counters -> tl
__device__ __forceinline__ void g_count_postings(const CountParams &p, GShared &s, const GItem &it, GTally &tl)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    WorkCount wc;
    g_sweep<NullTable, true>(p, it.vals, it.size, NullTable{&s.nd}, wc, s.pref[wv]);
    const unsigned long long wp = wave_total(wc.post);
    if (lane == 0 && wp) atomicAdd(&s.post, wp);
    if (it.fresh) {
        const uint32_t wl = wave_total(wc.lists), wi = wave_total(wc.lids);
        if (lane == 0) { tl.post += wp; tl.lists += wl; tl.lids += wi; }
    }
    __syncthreads();
}

// an empty LDS table and a fresh attempt (barrier, clear, barrier)
__device__ __forceinline__ void g_table_clear(GShared &s)
{
    __syncthreads();
    g_reset_attempt(s);
    for (uint32_t i = threadIdx.x; i < BigLdsTable::CAP; i += 64 * G_WAVES) { s.keys[i] = KH_EMPTY_PID; s.val[i] = 0xFFFF0000u; }
    __syncthreads();
}

// After the barrier that ends the adds: appends the LDS table's hits to the query's list.  The list's space is taken with
// the first hits: exactly the hits when the table held the whole query, else (`bucketed`) the bound min(postings, proteins)
// for all buckets together.
__device__ __forceinline__ GOutcome g_table_flush(const CountParams &p, GShared &s, bool bucketed, uint32_t &written)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t total = s.nd;
    if (s.fail != 0u || total > BigLdsTable::LIMIT) return G_TABLE_FULL;
    if (s.base == ~0ull && total > 0) {  // (workgroup-uniform: read after a barrier)
        __syncthreads();
        if (tid == 0) {
            unsigned long long want = total;
            if (bucketed) want = s.post < p.n_proteins ? s.post : p.n_proteins;
            s.base = tail_alloc(p, (uint32_t)(want > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : want));
            s.reserved = (uint32_t)want;  // (<= n_proteins or total: 32 bits)
            if (s.base == ~0ull) s.fail = 2;
        }
        __syncthreads();
        if (s.fail == 2u) return G_NO_SPACE;
    }
    if (total > 0) {
        if ((unsigned long long)written + total > s.reserved) { if (tid == 0) atomicOr(p.status, (uint32_t)ST_POOL_FULL); return G_NO_SPACE; }
        const uint32_t *keys = s.keys, *val = s.val;
        g_read_out<1>(p, s.base + written, (uint32_t)BigLdsTable::CAP, &s.out_cursor, [&](uint32_t i, uint32_t &k, uint32_t &c, uint32_t &m) {
            k = keys[i];
            const uint32_t v = val[i];
            c = v & 0xFFFFu; m = v >> 16;
        });
        written += total;
    }
    return G_DONE;
}

// ---- in LDS: the whole query in the big table first.  A query with more distinct hits than it holds (a skewed
// database: tens of thousands of proteins behind a few motifs) has its postings PARTITIONED by protein-id range
// (a hash of the id) into R buckets in the G arena -- one counting sweep for the bucket sizes, one sweep that
// scatters (id, position, run length) -- and then every bucket is counted in the LDS table on its own and its
// hits appended to the query's list (space for min(postings, proteins) entries is taken once).  Three sweeps of
// the query and sequential bucket reads instead of one random line fill and write-back per posting in a
// multi-megabyte table in HBM (6.5 of the skewed batch's 8.3 ms); counting the ranges by re-sweeping the whole
// query per range (tried first) costs R sweeps and lost for the monsters (profiles/r03_count_kernels.md).
__device__ __forceinline__ GOutcome g_lds_attempt(const CountParams &p, GShared &s, const GItem &it, uint32_t &written)
{
    const BigLdsTable bt{s.keys, s.val, &s.nd};
    g_table_clear(s);
    g_pass<BigLdsTable, true>(p, s, it, bt);
    __syncthreads();
    return g_table_flush(p, s, false, written);
}

// Guessed sizes: the ranges are a hash of the protein id, so every bucket gets postings / R items give or take a few per
// cent, and buckets of 5/4 of that (+ 2 048) spare the sweep that counts them -- one of a monster's three sweeps over
// hundreds of thousands of postings.  -> the items a bucket holds; 0: too many postings to guess.  Ends with a barrier
// unless it returns 0 (workgroup-uniform: s.post and R are).
__device__ __forceinline__ uint32_t g_guess_sizes(GShared &s, uint32_t R)
{
    const uint32_t tid = threadIdx.x;
    const unsigned long long per = s.post / R;
    const unsigned long long c = per + per / 4ull + 2048ull;
    if (c * R > 0x7FFFFFFFull) return 0u;
    const uint32_t cap_items = (uint32_t)c;
    if (tid < G_MAX_RANGES) { s.roff[tid] = tid * cap_items; s.rcur[tid] = tid * cap_items; }
    if (tid == 0) s.rtotal = R * cap_items;
    __syncthreads();
    return cap_items;
}

// Counted sizes: one sweep that counts the items of every range, then their exclusive prefix.  Ends with a barrier.
__device__ __forceinline__ void g_count_sizes(const CountParams &p, GShared &s, const GItem &it, uint32_t R)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid < G_MAX_RANGES) s.roff[tid] = 0;
    __syncthreads();
    g_pass(p, s, it, RangeHist{s.roff, &s.nd, R});
    __syncthreads();
    if (wv == 0) {  // exclusive prefix of the bucket sizes (R <= 64: one lane each); cursors start at the offsets
        const uint32_t v = lane < R ? s.roff[lane] : 0u;
        const uint32_t inc = wave_inclusive_scan_dpp(v);
        s.roff[lane] = inc - v;
        s.rcur[lane] = inc - v;
        if (lane == 63) s.rtotal = inc;
    }
    __syncthreads();
}

// every bucket in the LDS table on its own, its hits appended to the query's list
__device__ __forceinline__ GOutcome g_count_buckets(const CountParams &p, GShared &s, uint32_t R, const uint2 *items, uint32_t &written)
{
    const BigLdsTable bt{s.keys, s.val, &s.nd};
    for (uint32_t r = 0; r < R; r++) {
        g_table_clear(s);
        uint32_t nnew = 0;
        const uint32_t b0 = s.roff[r], b1 = s.rcur[r];   // (the scatter sweep left every cursor at its bucket's end)
        for (uint32_t i = b0 + threadIdx.x; i < b1; i += 64 * G_WAVES) {
            if (s.fail) break;
            const uint2 it = items[i];
            if (!bt.add_n(it.x, it.y & 0xFFFFu, it.y >> 16, nnew)) s.fail = 1;
        }
        __syncthreads();
        const GOutcome o = g_table_flush(p, s, true, written);
        if (o != G_DONE) return o;   // (workgroup-uniform)
    }
    return G_DONE;
}

// The partition: bucket sizes (guessed, then counted), offsets, scatter, buckets.  A guessed bucket that is full after all
// (a few ids with very many positions in one range) sends the query through the counted sizes (attempt 1).
// G_TABLE_FULL: a bucket with more distinct ids than the LDS table holds.
__device__ __forceinline__ GOutcome g_partitioned(const CountParams &p, GShared &s, const GItem &it, uint32_t &written, GClock &clk)
{
    const uint32_t tid = threadIdx.x;
    uint32_t R = (uint32_t)(s.post / 16384ull) + 2u;  // ~3 000 distinct ids per bucket when ids repeat ~6 times
    if (R > G_MAX_RANGES) R = G_MAX_RANGES;
    for (int attempt = 0; attempt < 2; attempt++) {
        uint32_t cap_items = 0xFFFFFFFFu;
        __syncthreads();
        g_reset_attempt(s);
        if (attempt == 0) {
            cap_items = g_guess_sizes(s, R);
            if (cap_items == 0u) continue;   // (workgroup-uniform) too many postings to guess: count them
        } else {
            g_count_sizes(p, s, it, R);
        }
        if (tid == 0) {  // 8 bytes per item: half a 16-byte slot of the arena
            g_arena_take(p, ((unsigned long long)s.rtotal + 1ull) / 2ull + 1ull, &s.off);
            s.sink.n = 0;
        }
        __syncthreads();
        if (s.off == ~0ull) return G_NO_SPACE;
        uint2 *items = reinterpret_cast<uint2 *>(p.g_keys + 4ull * s.off);
        g_pass(p, s, it, RangeScatter{s.rcur, &s.nd, items, R, s.roff, cap_items, &s.bucket_full});
        // the buckets were written by this workgroup's own stores into a region nobody has loaded from (g_cursor
        // never hands a region out twice within a launch): after the barrier (which drains vmcnt) the loads
        // of g_count_buckets miss the L1 and find them in the L2
        __syncthreads();
        clk.lap(GL_PARTITION);
        if (s.bucket_full != 0u) continue;   // (workgroup-uniform: read after a barrier) a guessed bucket was too small
        const GOutcome o = g_count_buckets(p, s, R, items, written);
        clk.lap(GL_BUCKETS);
        clk.partitioned(s.post);
        if (o == G_TABLE_FULL) written = 0;  // (what the buckets before it wrote is left behind: the HBM table starts over)
        return o;
    }
    return G_TABLE_FULL;
}

// The counting table in HBM, sized from the query's exact postings count.  Leaves the list's start in s.base (~0: none).
__device__ __forceinline__ GOutcome g_hbm_table(const CountParams &p, GShared &s, const GItem &it, uint32_t &written)
{
    const uint32_t tid = threadIdx.x;
    unsigned long long bound = s.post;
    if (bound > p.n_proteins) bound = p.n_proteins;
    uint32_t log2cap = 10;
    while ((1ull << log2cap) < 2 * bound && log2cap < 31) log2cap++;
    const unsigned long long cap = 1ull << log2cap;
    if (tid == 0) g_arena_take(p, cap, &s.off);
    __syncthreads();
    const unsigned long long off = s.off;
    if (off == ~0ull) return G_NO_SPACE;
    const GlobalTable gt{p.g_keys + 4ull * off, &s.nd, log2cap};
    // The table belongs to this workgroup alone (g_cursor never hands out a region twice within one launch) and is
    // touched with plain 16-byte initialisation stores, workgroup-scope atomics and, at the end, plain read-out
    // loads.  Nothing loads from it before the read-out, so no stale line can sit in the L1 (write-through, holds
    // no line of the table); the atomics are performed in the XCD's L2, where the initialisation stores went.  A
    // workgroup barrier (which drains vmcnt) between the phases is enough: no agent-scope fence -- a full L2
    // write-back on this part.
    for (unsigned long long i = tid; i < cap; i += 64 * G_WAVES)
        reinterpret_cast<uint4 *>(gt.slots)[i] = make_uint4(KH_EMPTY_PID, 0u, 0xFFFFFFFFu, 0u);
    __syncthreads();
    g_pass(p, s, it, gt);
    __syncthreads();
    const uint32_t total = s.nd;
    const bool failed = s.fail != 0;
    if (tid == 0) {
        if (failed) { atomicOr(p.status, (uint32_t)ST_G_TABLE_FULL); s.base = ~0ull; }
        else if (total == 0) s.base = 0;
        else s.base = tail_alloc(p, total);
    }
    __syncthreads();
    const unsigned long long base = s.base;
    if (base == ~0ull) return G_NO_SPACE;
    if (total > 0) {
        // four stripes of the table per round trip, a 16-byte slot per lane
        const uint4 *slots = reinterpret_cast<const uint4 *>(gt.slots);
        g_read_out<4>(p, base, cap, &s.out_cursor, [&](unsigned long long i, uint32_t &k, uint32_t &c, uint32_t &m) {
            const uint4 sv = slots[i];
            k = sv.x; c = sv.y; m = sv.z;
        });
    }
    written = total;
    return G_DONE;
}

// the query's result: `written` entries from s.base on, or nothing (no space anywhere: the status says so).  s.base is
// read after the barrier that followed its last write.  Ends with a barrier: the next item resets the words.
__device__ __forceinline__ void g_publish(const CountParams &p, GShared &s, uint32_t q, GOutcome o, uint32_t written, GTally &tl)
{
    const unsigned long long base = o == G_DONE ? s.base : ~0ull;
    if ((threadIdx.x >> 6) == 0 && base != ~0ull) {
        tl.hits += written;
        if (written > G_MONSTER_HITS) { tl.mon_hits += written; tl.monsters++; }
    }
    if (threadIdx.x == 0) { p.q_cnt[q] = (base != ~0ull) ? written : 0u; p.hit_off[q] = (base == ~0ull || written == 0) ? 0 : base; }
    __syncthreads();
}

__global__ __launch_bounds__(64 * G_WAVES, G_MIN_BLOCKS) void count_global_kernel(CountParams p)
{
    __shared__ GShared s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t n_items = *p.list_count < p.list_cap ? *p.list_count : p.list_cap;
    // the grid is sized for a batch full of overflowing queries; most batches have none, and the workgroups beyond the
    // items (all but one when there are none) leave at once -- they take no part in the completion count either
    const uint32_t n_part = n_items < gridDim.x ? (n_items ? n_items : 1u) : gridDim.x;
    if (blockIdx.x >= n_part) return;
    GTally tl;
    GClock clk;
    clk.begin();
    for (uint32_t item = blockIdx.x; item < n_items;) {
        const WorkItem wi = p.list[item];
        GItem it;
        it.q = wi.q; it.fresh = wi.size < 0; it.size = it.fresh ? -wi.size : wi.size; it.vals = p.vals + wi.aa_off;
        item = g_begin_item(p, s, n_part);
        clk.begin_item();
        g_count_postings(p, s, it, tl);
        GOutcome o = G_TABLE_FULL;
        uint32_t written = 0;
        if (it.size < 65535) {
            if (tid == 0) s.base = ~0ull;
            clk.lap(GL_POSTINGS);
            o = g_lds_attempt(p, s, it, written);
            clk.lap(GL_LDS);
            if (o == G_TABLE_FULL) o = g_partitioned(p, s, it, written, clk);
            __syncthreads();
            if (o == G_TABLE_FULL) {   // (a bucket overflowed: the table in HBM)
                g_reset_attempt(s);
                __syncthreads();
            }
        }
        const bool in_lds = o != G_TABLE_FULL;
        if (!in_lds) o = g_hbm_table(p, s, it, written);
        g_publish(p, s, it.q, o, written, tl);
        if (in_lds) clk.done_in_lds(s.post);
    }
    clk.end();
    if (lane == 0) {
        const uint32_t rep = blockIdx.x * G_WAVES + wv;
        add_counter(p.counters, rep, CTR_HITS, tl.hits);
        // (what the queries that left their LDS tables found, and the monsters among them: finalize_body works the next
        // batch's table scale out without the ones or the others)
        if (tl.hits) atomicAdd(p.queue_head + (SLOT_G_HITS16 - SLOT_QUEUE_HEAD), (uint32_t)((tl.hits + 15ull) >> 4 > 0x0FFFFFFFull ? 0x0FFFFFFFull : (tl.hits + 15ull) >> 4));
        if (tl.monsters) {
            atomicAdd(p.queue_head + (SLOT_G_MON_HITS16 - SLOT_QUEUE_HEAD), (uint32_t)((tl.mon_hits + 15ull) >> 4 > 0x0FFFFFFFull ? 0x0FFFFFFFull : (tl.mon_hits + 15ull) >> 4));
            atomicAdd(p.queue_head + (SLOT_G_MONSTERS - SLOT_QUEUE_HEAD), tl.monsters);
        }
        add_counter(p.counters, rep, CTR_POST, tl.post);
        add_counter(p.counters, rep, CTR_LISTS, tl.lists);
        add_counter(p.counters, rep, CTR_LIST_IDS, tl.lids);
    }
    if (p.fin_out) {
        // the batch ends here: the last workgroup to arrive does the finalize step
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's counter atomics are done
        __syncthreads();
        // two levels: 512 workgroups bumping ONE word serialise at ~90 per microsecond (6 us of a 0.2 ms batch);
        // eight sub-counters (workgroup index mod 8), and the last arrival of each bumps the top one
        if (tid == 0) {
            const uint32_t sub = blockIdx.x & 7u, n_sub = (n_part - sub + 7u) >> 3, n_top = n_part < 8u ? n_part : 8u;
            s.last = 0;
            if (atomicAdd(p.queue_head + (SLOT_QUEUE_SUB - SLOT_QUEUE_HEAD) + sub, 1u) == n_sub - 1u)
                s.last = atomicAdd(p.queue_head, 1u) == n_top - 1u;
        }
        __syncthreads();
        if (s.last) {
            finalize_body<true>(p.counters, p.fin_out, p.fin_small, p.fin_status_out, p.fin_g_items, p.fin_cursors, p.fin_slot_scale, p.fin_scale_cap, p.fin_scale_margin);
        }
    }
}

// ---- PositionHits of the G-tier queries -------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * G_WAVES) void positions_global_kernel(CountParams p)
{
    constexpr int NWIN = 2;
    __shared__ uint32_t s_nd;
    __shared__ uint32_t s_pref[G_WAVES][NWIN * 64];
    __shared__ unsigned long long s_off;
    const uint32_t tid = threadIdx.x, wv = tid >> 6;
    const uint32_t n_items = *p.list_count < p.list_cap ? *p.list_count : p.list_cap;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const WorkItem wi = p.list[item];
        const uint32_t q = wi.q, cnt = p.q_cnt[q];
        const int32_t size = wi.size < 0 ? -wi.size : wi.size;  // (negative: sent to the G tier unseen, see count_global_kernel)
        const unsigned long long hoff = p.hit_off[q];
        uint32_t log2cap = 10;
        while ((1ull << log2cap) < 2ull * cnt && log2cap < 31) log2cap++;
        const unsigned long long cap = 1ull << log2cap;
        if (tid == 0) {
            s_nd = 0;
            g_arena_take(p, cap, &s_off);
        }
        __syncthreads();
        const unsigned long long off = s_off;
        if (off == ~0ull || cnt == 0 || size <= 0) { __syncthreads(); continue; }
        uint32_t *slots = p.g_keys + 4ull * off;
        for (unsigned long long i = tid; i < cap; i += 64 * G_WAVES) __hip_atomic_store(&slots[4 * i], KH_EMPTY_PID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const uint32_t mask = (uint32_t)cap - 1u;
        for (uint32_t i = tid; i < cnt; i += 64 * G_WAVES) {
            const uint32_t pid = p.hit_pid[hoff + i];
            uint32_t h = (pid * 0x9E3779B1u) >> (32 - log2cap);
            while (atomicCAS(&slots[4ull * h], KH_EMPTY_PID, pid) != KH_EMPTY_PID) h = (h + 1u) & mask;  // ids are distinct, load <= 0.5
            __hip_atomic_store(&slots[4ull * h + 1], i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        BitsTable bt;
        bt.slots = slots; bt.nd = &s_nd; bt.log2cap = log2cap;
        bt.words = ((uint32_t)size + 63u) >> 6;
        bt.bits = p.pos_bits + p.pos_base[q];
        WorkCount wc;
        const bool ok = g_sweep<BitsTable, false, false, NWIN>(p, p.vals + wi.aa_off, size, bt, wc, s_pref[wv]);
        if (!ok && (tid & 63u) == 0) atomicOr(p.status, (uint32_t)ST_G_TABLE_FULL);
        __syncthreads();
    }
}
