// out_rows.hip.inc — what the three response writers behind top-N share on the device (included by search.hip after
// top_align.hip.inc, before tsv_rows.hip.inc, tsv_aln_rows.hip.inc and json_rows.hip.inc; the host side is host_out.hip.inc).
//
// A writer prints UNITS -- a TSV row per reported hit, a JSON object per reported query -- into one byte range, in query
// order, and says where every unit starts.  All of them work on tiles of OUT_TILE queries and in the same passes:
//   a length pass   per tile: the bytes and the units of its queries (the writer's own kernel)
//   out_scan_kernel one workgroup: the tiles' two sums scanned in 64 bits, the totals, the capacity check, the status word
//   a write pass    per tile: its units, at the tile's prefix (the writer's own kernels; nothing is written when the status
//                   word is set)
// Every writer clears the counts before its first pass: a length pass may set status bits, the scan kernel adds its own.
#define OUT_TILE 256u
#define OUT_NONE 0xFFFFFFFFu
// counts[]: what the host reads after a call (kaamer_*_rows_result.d_counts); OUT_C_RAW: tsv_aln_rows.hip.inc
enum { OUT_C_UNITS = 0, OUT_C_BYTES = 1, OUT_C_STATUS = 2, OUT_C_RAW = 3, OUT_C_N = 4 };
enum { OUT_ST_OUT_CAP = 1u, OUT_ST_UNIT_CAP = 2u, OUT_ST_UPSTREAM = 4u /* the batch's own status, or no bitmaps in its block */,
       OUT_ST_OBJECT = 8u /* json_rows.hip.inc: an object of 4 GB */, OUT_ST_MISMATCH = 16u /* ... its two passes disagreed */ };

struct OutParams {
    const uint32_t *d_nq;
    uint32_t nq_cap;
    const kaamer_query_meta *q;
    const uint32_t *top_cnt, *top_pid, *top_km;
    const int32_t *start_pos, *size_out;
    uint32_t K;
    const uint8_t *names;
    uint64_t names_len;
    const kaamer_text_span *spans;
    uint32_t n_names;
    const uint64_t *pos_base;      // the three of kaamer_topn_positions; NULL unless positions
    const int32_t *pos_len;
    const uint64_t *pos_bits;
    int positions;
    // the host-buffer calls: the packed result block of the same batch (topn.hip.inc).  A block whose status word is set is
    // refused by the host whatever follows, so the stage writes nothing; with positions the bitmaps are the block's section
    // (top_positions.hip.inc: per query at pos_base[q], as in the workspace's own storage)
    const uint8_t *block;
    const uint32_t *idmap;         // protein id -> entry of the attached subject table, OUT_NONE: no entry
    uint32_t idmap_n;
    // the stage's own
    unsigned long long *tile_bytes, *tile_units;   // per tile: sums, then exclusive prefixes
    unsigned long long *unit_off;                  // where every unit starts, and the total behind the last
    uint64_t unit_cap;
    char *out;
    uint64_t out_cap;
    unsigned long long *counts;    // OUT_C_*
};

__device__ __forceinline__ uint32_t out_digits(uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u
         : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}

// the id -> entry map, as kaamer_fetch_hits resolves an id
__device__ __forceinline__ uint32_t out_entry(const OutParams &p, uint32_t pid)
{
    return pid < p.idmap_n ? p.idmap[pid] : OUT_NONE;
}

// inclusive scan of one value per thread of an OUT_TILE-thread workgroup (sh: OUT_TILE words); every thread gets its own
// inclusive prefix, *total the workgroup's sum
__device__ __forceinline__ unsigned long long out_block_scan(unsigned long long v, unsigned long long *sh, unsigned long long *total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < OUT_TILE; o <<= 1) {
        const unsigned long long add = t >= o ? sh[t - o] : 0ull;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const unsigned long long mine = sh[t];
    *total = sh[OUT_TILE - 1];
    __syncthreads();
    return mine;
}

__device__ __forceinline__ uint32_t out_nq(const OutParams &p)
{
    const uint32_t nq = *p.d_nq;
    return nq < p.nq_cap ? nq : p.nq_cap;
}

// false: the batch's block is flagged (or holds no bitmaps although they are wanted) -- nothing of the batch is read;
// else, with positions, the bitmaps are taken from the block.  Every thread computes the same.
__device__ __forceinline__ bool out_upstream(OutParams &p)
{
    if (!p.block) return true;
    const RepBlockHdr *hdr = reinterpret_cast<const RepBlockHdr *>(p.block);
    if (hdr->status) return false;
    if (p.positions) {
        const uint64_t at = rep_pos_ext(hdr)->off_pos_bits;
        if (!at) return false;
        p.pos_bits = reinterpret_cast<const uint64_t *>(p.block + at);
    }
    return true;
}

// one workgroup: exclusive scan of the tiles' two sums in place, OUT_TILE tiles per round; totals and status.  sep: the
// bytes between two units that no unit counts (0: rows, 1: the comma between two objects)
__global__ __launch_bounds__(OUT_TILE) void out_scan_kernel(OutParams p, uint32_t sep)
{
    __shared__ unsigned long long sh[OUT_TILE];
    if (!out_upstream(p)) {
        if (threadIdx.x == 0) { p.counts[OUT_C_UNITS] = 0; p.counts[OUT_C_BYTES] = 0; p.counts[OUT_C_STATUS] = OUT_ST_UPSTREAM; }
        return;
    }
    const uint32_t nq = out_nq(p);
    const uint32_t tiles = (nq + OUT_TILE - 1u) / OUT_TILE;
    unsigned long long base_b = 0, base_u = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += OUT_TILE) {
        const uint32_t t = t0 + threadIdx.x;
        const unsigned long long b = t < tiles ? p.tile_bytes[t] : 0ull, u = t < tiles ? p.tile_units[t] : 0ull;
        unsigned long long tb = 0, tu = 0;
        const unsigned long long ib = out_block_scan(b, sh, &tb), iu = out_block_scan(u, sh, &tu);
        if (t < tiles) { p.tile_bytes[t] = base_b + ib - b; p.tile_units[t] = base_u + iu - u; }
        base_b += tb; base_u += tu;
    }
    if (threadIdx.x == 0) {
        const unsigned long long bytes = base_b + (base_u ? (base_u - 1ull) * sep : 0ull);
        unsigned long long st = p.counts[OUT_C_STATUS];   // (the length pass may have set a bit)
        if (bytes > p.out_cap) st |= OUT_ST_OUT_CAP;
        if (base_u + 1ull > p.unit_cap) st |= OUT_ST_UNIT_CAP;
        p.counts[OUT_C_UNITS] = base_u; p.counts[OUT_C_BYTES] = bytes; p.counts[OUT_C_STATUS] = st;
        if (!st) p.unit_off[base_u] = bytes;
    }
}

// [lo, hi) of the output from the LDS window that starts at `w`, by the whole workgroup: 16 bytes per lane, consecutive
// lanes consecutive addresses; a chunk the range covers only in part goes out in bytes
__device__ __forceinline__ void out_store_window(char *out, const char *win, unsigned long long w, unsigned long long lo, unsigned long long hi)
{
    for (unsigned long long c = (lo - w) / 16ull + threadIdx.x; c * 16ull < hi - w; c += OUT_TILE) {
        const unsigned long long at = w + c * 16ull;
        if (at >= lo && at + 16ull <= hi) {
            *reinterpret_cast<uint4 *>(out + at) = *reinterpret_cast<const uint4 *>(win + c * 16ull);
        } else {
            const unsigned long long a = at > lo ? at : lo, b = at + 16ull < hi ? at + 16ull : hi;
            for (unsigned long long i = a; i < b; i++) out[i] = win[i - w];
        }
    }
}
