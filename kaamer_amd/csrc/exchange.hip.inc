// exchange.hip.inc — the exchange step of the sharded index as device code (included by search.hip).
//
// SURVEY 8e / BASELINE north_star: the table is split by hash prefix, every rank searches the whole
// batch against its shard, query q is owned by rank q mod W, and ONE exchange step brings each
// partial hit list (protein id, partial Kmatch, first position) to the owner, which merges.  The
// reference has nothing like it (one process, search_fastq.go:94-118 is the per-query block whose
// result the merge must reproduce).
//
// To keep the step free of host synchronisation the exchange uses EQUAL-SIZE blocks: rank r sends
// one block of `block_words` u32 words to every rank d:
//     [0] entries in the block   [1] status (bit 0: the block's capacity was exceeded; bit 1: first positions inside;
//                                    bit 2: the SENDER's search of the batch failed -- its lists are not to be trusted;
//                                    bit 3: some block of this sender exceeded its capacity: the batch fails on EVERY rank)
//     [2] queries of the batch   [3] queries owned by d = ceil((nq - d) / W)
//     [4] entries this block NEEDED (= [0] unless it overflowed)
//     [5] the largest [4] over the sender's W blocks   [6], [7] zero (arrays = 4: see below)
//     [8 .. 8+q_cap)             per owned query i (global query d + i W): number of entries
//     (XWord and XStatus below name these words and bits; tests/blockfmt.py restates the format under the same names)
//     then pid[e_cap], kmatch[e_cap], first_pos[e_cap]   (structure of arrays)
// Blocks with PositionHits bitmaps (arrays = 4; search.go:442-452) add, after the counts, SizeInKmer[q_cap] (the entry
// arrays follow it), and after the entry arrays, from the even word bits_off = 8 + 2 q_cap + 3 e_cap (rounded up), a
// section of p_cap = (block_words - bits_off) / 2 u64 words: entry j of owned query i has ceil(SizeInKmer_i / 64) words at
// bbase[i] + j words_i (bbase: the scan of entries_i x words_i).  [6] = bitmap words this block needed, [7] = the largest
// [6] of the sender's W blocks, status bit 4 = bitmaps inside; a section that does not fit sets bits 0 / 3 as the entries do.
// so the transport is an all-to-all with equal splits (grouped ncclSend / ncclRecv over xGMI: all
// seven links busy at once), whatever the data-dependent sizes are.  The block size of a batch is the
// caller's choice within the buffers' capacity (kaamer_exchange_layout_fit): word [5] of the W received
// headers gives every rank the SAME figure -- the largest block any pair of ranks needed -- so all ranks
// size the blocks of a later batch alike (the previous need + a margin) without a collective of their
// own, and what travels is payload, not capacity.  A block that does not fit fails the batch on every
// rank (KAAMER_E_CAPACITY, never a partial result); the caller repeats it with the full capacity.
//
//   kaamer_exchange_pack   per destination, tiled scan of the owned queries' hit counts (3 small launches);
//                          copy of the hit lists into the blocks (16 lanes per query)
//   kaamer_exchange_merge  per source, tiled scan of the received counts + totals per owned query;
//                          copy into per-query contiguous entries; then the merge
//                          (count_group_kernel MODE 2) on the owner's workspace
//   arrays = 4             the same scans over bitmap words (modes 2, 3), x_pack_bits_kernel / x_unpack_bits_kernel,
//                          and after the merge's bitmap layout x_or_bits_kernel (the bitmaps of one hit, OR-merged)
#define X_BLOCK 1024
#define X_ITEMS 8
#define X_TILE (X_BLOCK * X_ITEMS)
#define X_SMALL_TILES 4u  /* up to this many tiles per row a single workgroup per row scans them (one launch) */

enum XWord : uint32_t {       // the header words of a block
    X_ENTRIES = 0, X_STATUS, X_NQ, X_OWNED, X_NEED, X_NEED_MAX, X_BITS_NEED, X_BITS_NEED_MAX,
    X_HDR                     // the header's length: the counts start here
};
enum XStatus : uint32_t {     // the bits of blk[X_STATUS]
    XS_OVERFLOW = 1u, XS_FIRST_POS = 2u, XS_SENDER_FAILED = 4u, XS_SENDER_OVERFLOW = 8u, XS_BITMAPS = 16u
};

struct XParams {
    uint32_t world, rank, q_cap;
    uint64_t e_cap, block_words;
    // pack: the search workspace's last result
    const uint32_t *d_nq;
    const uint32_t *src_status;  // status word of the search that produced the lists (written by its finalize step, same stream)
    const uint64_t *hit_off;
    const uint32_t *hit_cnt, *pid, *km, *fp;
    uint32_t *send;
    uint32_t *dst_off;  // [world][q_cap]
    // unpack
    const uint32_t *recv;
    uint32_t *src_off;  // [world][q_cap]
    uint64_t *ent_off;  // [q_cap + 1]
    uint32_t *d_nq_owned;
    uint32_t *m_pid, *m_km, *m_fp;
    uint64_t m_cap;
    uint32_t *status;
    unsigned long long *stats;  // unpack: {queries of the batch, largest block any pair of ranks needed, a block overflowed, 0}
    uint64_t *tile_sum; // [rows][n_tiles] scratch of the tiled scans
    uint32_t n_tiles;
    uint32_t with_fp;   // 0: first positions are not wanted (protein search without -pos): their third of the entries stays untouched
    // blocks with PositionHits bitmaps (arrays = 4)
    uint64_t p_cap;     // u64 words of a block's bitmap section
    uint64_t bits_off;  // u32 word at which the bitmap section starts (even: 8-byte aligned)
    uint32_t ent_base;  // u32 word at which the entry arrays start: 8 + q_cap, or 8 + 2 q_cap with the SizeInKmer section
    const QInfo *qinfo; // pack: the search's queries (QInfo.size = the SizeInKmer its bitmaps were laid out with)
    const uint64_t *pos_off;
    const unsigned long long *pos_bits;
    uint64_t *dst_boff; // pack: [world][q_cap] bitmap word offset of each owned query inside its block
    uint64_t *src_boff; // unpack: [world][q_cap] the same inside each received block
    uint64_t *ent_boff; // unpack: [q_cap + 1] first bitmap word of each owned query in m_bits (aligned with ent_off)
    int32_t *m_size;    // unpack: SizeInKmer of each owned query (as every block carried it)
    unsigned long long *m_bits;
    uint64_t mb_cap;
    unsigned long long *pstats;  // unpack: {largest bitmap need between any pair of ranks, a bitmap section overflowed}
    // OR-merge: the merge workspace's result
    const uint32_t *r_nq, *r_cnt, *r_pid;
    const uint64_t *r_off, *r_pos_off, *r_pos_base;
    unsigned long long *r_pos_bits;
    uint64_t r_bits_cap;
    uint64_t *m_dst;    // [m_cap] per received entry: first word of its merged hit's bitmap
    unsigned long long *g_tab;  // [2 m_cap] hash tables of the queries whose merged hits exceed the LDS table
};

__device__ __forceinline__ uint32_t x_words(int32_t size) { return size > 0 ? ((uint32_t)size + 63u) >> 6 : 0u; }
__device__ __forceinline__ unsigned long long *x_bits(uint32_t *blk, const XParams &p) { return reinterpret_cast<unsigned long long *>(blk + p.bits_off); }
__device__ __forceinline__ const unsigned long long *x_bits(const uint32_t *blk, const XParams &p)
{
    return reinterpret_cast<const unsigned long long *>(blk + p.bits_off);
}
__device__ __forceinline__ uint32_t x_sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

__device__ __forceinline__ uint32_t *x_block(uint32_t *base, const XParams &p, uint32_t peer) { return base + (uint64_t)peer * p.block_words; }
__device__ __forceinline__ const uint32_t *x_block(const uint32_t *base, const XParams &p, uint32_t peer) { return base + (uint64_t)peer * p.block_words; }
// the per-query sections of a block: entry counts, and (arrays = 4) SizeInKmer
__device__ __forceinline__ uint32_t *x_counts(uint32_t *blk) { return blk + X_HDR; }
__device__ __forceinline__ const uint32_t *x_counts(const uint32_t *blk) { return blk + X_HDR; }
__device__ __forceinline__ uint32_t *x_sizes(uint32_t *blk, const XParams &p) { return blk + X_HDR + p.q_cap; }
__device__ __forceinline__ const uint32_t *x_sizes(const uint32_t *blk, const XParams &p) { return blk + X_HDR + p.q_cap; }
// queries of a batch of nq that rank `peer` owns: peer, peer + W, ...
__device__ __forceinline__ uint32_t x_owned_by(uint32_t nq, uint32_t peer, uint32_t world) { return nq > peer ? (nq - peer + world - 1) / world : 0u; }

// exclusive scan of one tile of a block-wide loop (1024 threads, X_ITEMS each); returns the tile total
__device__ __forceinline__ uint64_t x_tile_scan(const uint32_t (&v)[X_ITEMS], uint64_t (&ex)[X_ITEMS])
{
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < X_ITEMS; i++) s += v[i];
    uint64_t tot;
    uint64_t e = block_exclusive_scan(s, &tot);
#pragma unroll
    for (int i = 0; i < X_ITEMS; i++) { ex[i] = e; e += v[i]; }
    return tot;
}

// Every source must describe the same batch: X_NQ equal in all blocks and X_OWNED (queries this rank owns) =
// ceil((nq - rank) / W) <= q_cap.  Otherwise nothing is unpacked (0 owned queries) and the batch fails.
__device__ __forceinline__ bool x_headers_agree(const XParams &p)
{
    const uint32_t nq = x_block(p.recv, p, 0)[X_NQ];
    const uint32_t want = x_owned_by(nq, p.rank, p.world);
    bool ok = want <= p.q_cap;
    for (uint32_t t = 0; t < p.world; t++) {
        const uint32_t *b = x_block(p.recv, p, t);
        ok = ok && b[X_NQ] == nq && b[X_OWNED] == want;
    }
    return ok;
}
__device__ __forceinline__ uint32_t x_owned_checked(const XParams &p)
{
    return x_headers_agree(p) ? x_block(p.recv, p, 0)[X_OWNED] : 0u;
}

// ---- scans over ROWS of per-query counts, tiled over the grid (a single workgroup per row took 5 ms for the 4.2 M ORFs
// of a 1 M-read batch at W = 1).  Three small launches: tile sums (grid: tiles x rows), one workgroup that scans the
// tile sums of every row and writes the totals, and the apply pass (grid: tiles x rows) that redoes a tile's local scan
// on top of its base.
//   MODE 0 (pack):   row d = destination rank; item i = hit count of query d + i W; n_items = queries owned by d
//   MODE 1 (unpack): row s < W = source rank, item i = entries block s holds for owned query i; row W = their sum over
//                    the sources; n_items = owned queries
//   MODE 2 (pack, arrays = 4):   as MODE 0, item = bitmap words of query d + i W (hits x ceil(SizeInKmer / 64))
//   MODE 3 (unpack, arrays = 4): as MODE 1, item = bitmap words block s holds for owned query i; row W = their sum
template <int MODE> __device__ __forceinline__ uint32_t x_items(const XParams &p, uint32_t row)
{
    if (MODE == 0 || MODE == 2) {
        const uint32_t n = x_owned_by(*p.d_nq, row, p.world);
        return n < p.q_cap ? n : p.q_cap;
    }
    return x_owned_checked(p);
}
template <int MODE> __device__ __forceinline__ uint32_t x_value(const XParams &p, uint32_t row, uint64_t idx)
{
    if (MODE == 0) return p.hit_cnt[row + idx * p.world];
    if (MODE == 2) {
        const uint64_t q = row + idx * p.world;
        return x_sat32((uint64_t)p.hit_cnt[q] * x_words(p.qinfo[q].size));
    }
    if (MODE == 3) {
        uint64_t v = 0;
        for (uint32_t t = (row < p.world ? row : 0u); t < (row < p.world ? row + 1u : p.world); t++) {
            const uint32_t *b = x_block(p.recv, p, t);
            v += (uint64_t)x_counts(b)[idx] * x_words((int32_t)x_sizes(b, p)[idx]);
        }
        return x_sat32(v);
    }
    if (row < p.world) return x_counts(x_block(p.recv, p, row))[idx];
    uint32_t v = 0;
    for (uint32_t t = 0; t < p.world; t++) v += x_counts(x_block(p.recv, p, t))[idx];
    return v;
}
// item idx of a row and its exclusive offset o within the row: where the copy kernels will find the query's data
template <int MODE> __device__ __forceinline__ void x_store(const XParams &p, uint32_t row, uint64_t idx, uint32_t v, uint64_t o)
{
    if (MODE == 0) {
        x_counts(x_block(p.send, p, row))[idx] = v;
        p.dst_off[(uint64_t)row * p.q_cap + idx] = x_sat32(o);
    } else if (MODE == 2) {
        x_sizes(x_block(p.send, p, row), p)[idx] = (uint32_t)p.qinfo[row + idx * p.world].size;
        p.dst_boff[(uint64_t)row * p.q_cap + idx] = o;
    } else if (row < p.world) {
        if (MODE == 1) p.src_off[(uint64_t)row * p.q_cap + idx] = x_sat32(o);
        else p.src_boff[(uint64_t)row * p.q_cap + idx] = o;
    } else if (MODE == 1) {
        p.ent_off[idx] = o;
    } else {
        p.ent_boff[idx] = o;
        // all shards translate alike: every block must carry the same SizeInKmer, or they are not one batch
        const uint32_t sz = x_sizes(x_block(p.recv, p, 0), p)[idx];
        bool same = true;
        for (uint32_t t = 1; t < p.world; t++) same = same && x_sizes(x_block(p.recv, p, t), p)[idx] == sz;
        p.m_size[idx] = (int32_t)sz;
        if (!same) { atomicOr(p.status, (uint32_t)ST_EXCHANGE_CAP); *p.d_nq_owned = 0u; }
    }
}
// one tile of a row on top of `tbase`: the items' offsets stored; returns the tile's total
template <int MODE> __device__ __forceinline__ uint64_t x_tile_apply(const XParams &p, uint32_t row, uint32_t n, uint64_t base, uint64_t tbase)
{
    uint32_t v[X_ITEMS];
    uint64_t ex[X_ITEMS];
#pragma unroll
    for (int i = 0; i < X_ITEMS; i++) {
        const uint64_t idx = base + (uint64_t)threadIdx.x * X_ITEMS + i;
        v[i] = idx < n ? x_value<MODE>(p, row, idx) : 0u;
    }
    const uint64_t tot = x_tile_scan(v, ex);
#pragma unroll
    for (int i = 0; i < X_ITEMS; i++) {
        const uint64_t idx = base + (uint64_t)threadIdx.x * X_ITEMS + i;
        if (idx < n) x_store<MODE>(p, row, idx, v[i], tbase + ex[i]);
    }
    return tot;
}

// ---- what one thread writes once a row's total is known -----------------------------------------------------------------
// pack: the header of destination d's block from its entry total.  (X_NEED_MAX: x_pack_copy_kernel, once all W blocks have
// their X_NEED; the bitmap words: x_pack_bits_headers.)
__device__ __forceinline__ void x_pack_header(const XParams &p, uint32_t d, uint64_t total)
{
    const uint32_t nq = *p.d_nq;
    uint32_t n_owned = x_owned_by(nq, d, p.world);
    uint32_t st = 0;
    if (n_owned > p.q_cap) { n_owned = p.q_cap; st = XS_OVERFLOW; }
    if (total > p.e_cap) st = XS_OVERFLOW;
    uint32_t *blk = x_block(p.send, p, d);
    blk[X_ENTRIES] = total > p.e_cap ? 0u : (uint32_t)total;
    // a search that ran out of a workspace bound (hit pool, G-tier arena or table) has written empty lists for the
    // queries it could not finish: every owner must know, or it would merge them into a result that looks complete
    blk[X_STATUS] = st | (p.with_fp ? XS_FIRST_POS : 0u) | ((p.src_status && *p.src_status) ? XS_SENDER_FAILED : 0u);
    blk[X_NQ] = nq;
    blk[X_OWNED] = n_owned;
    blk[X_NEED] = x_sat32(total);
    blk[X_NEED_MAX] = blk[X_BITS_NEED] = blk[X_BITS_NEED_MAX] = 0u;
}
// pack, arrays = 4: the bitmap sections' words of all W headers from their totals; a section that does not fit sets the
// overflow bit as the entries do (x_pack_copy_kernel spreads it to XS_SENDER_OVERFLOW in every block of this sender)
__device__ __forceinline__ void x_pack_bits_headers(const XParams &p, const uint64_t *total)
{
    uint32_t mx = 0;
    for (uint32_t d = 0; d < p.world; d++) {
        uint32_t *blk = x_block(p.send, p, d);
        blk[X_BITS_NEED] = x_sat32(total[d]);
        blk[X_STATUS] |= XS_BITMAPS | (total[d] > p.p_cap ? XS_OVERFLOW : 0u);
        mx = blk[X_BITS_NEED] > mx ? blk[X_BITS_NEED] : mx;
    }
    for (uint32_t d = 0; d < p.world; d++) x_block(p.send, p, d)[X_BITS_NEED_MAX] = mx;
}
// unpack: everything the owner derives from the W received headers and the entry total -- the statistics, the batch's
// status, and how many owned queries the merge may read
__device__ __forceinline__ void x_owner_verdict(const XParams &p, uint64_t total)
{
    const uint32_t n_owned = x_owned_checked(p);
    p.ent_off[n_owned] = total;
    uint32_t st = total > p.m_cap ? 1u : 0u, peer = 0u, need = 0;
    for (uint32_t t = 0; t < p.world; t++) {
        const uint32_t *bh = x_block(p.recv, p, t);
        const uint32_t b1 = bh[X_STATUS];
        if (b1 & (XS_OVERFLOW | XS_SENDER_OVERFLOW)) st = 1u;  // this block, or another block of the same sender, did not fit
        peer |= b1 & XS_SENDER_FAILED;
        need = bh[X_NEED_MAX] > need ? bh[X_NEED_MAX] : need;
        if (p.with_fp && !(b1 & XS_FIRST_POS)) st = 1u;  // the owner wants first positions the sender did not pack: an error, not zeros
    }
    if (p.stats) { p.stats[0] = x_block(p.recv, p, 0)[X_NQ]; p.stats[1] = need; p.stats[2] = st; p.stats[3] = 0; }
    if (!x_headers_agree(p)) st = 1u;  // ranks on different batches, or a stale / garbled block
    if (st) atomicOr(p.status, (uint32_t)ST_EXCHANGE_CAP);
    if (peer) atomicOr(p.status, (uint32_t)ST_PEER_FAILED);
    // a block that overflowed carries counts without entries: nothing is merged (the batch fails with
    // KAAMER_E_CAPACITY at kaamer_workspace_finish), and nothing may be read past the buffers
    *p.d_nq_owned = (st | peer) ? 0u : n_owned;
}
// unpack, arrays = 4: the same over the bitmap words of the headers (after x_owner_verdict: it may only take d_nq_owned back)
__device__ __forceinline__ void x_owner_verdict_bits(const XParams &p, uint64_t total)
{
    p.ent_boff[x_owned_checked(p)] = total;
    uint32_t need = 0, povf = 0, bad = total > p.mb_cap ? 1u : 0u;
    for (uint32_t t = 0; t < p.world; t++) {
        const uint32_t *bh = x_block(p.recv, p, t);
        need = bh[X_BITS_NEED_MAX] > need ? bh[X_BITS_NEED_MAX] : need;
        if (bh[X_BITS_NEED] > p.p_cap || bh[X_BITS_NEED_MAX] > p.p_cap) povf = 1u;
        if (!(bh[X_STATUS] & XS_BITMAPS)) bad = 1u;  // the owner wants bitmaps the sender did not pack: an error, not empty bitmaps
    }
    if (p.pstats) { p.pstats[0] = need; p.pstats[1] = povf; }
    if (bad | povf) {
        atomicOr(p.status, (uint32_t)ST_EXCHANGE_CAP);
        *p.d_nq_owned = 0u;
    }
}

template <int MODE> __global__ __launch_bounds__(X_BLOCK) void x_scan_sums_kernel(XParams p)
{
    const uint32_t row = blockIdx.y, tile = blockIdx.x;
    const uint32_t n = x_items<MODE>(p, row);
    const uint64_t base = (uint64_t)tile * X_TILE;
    uint64_t sum = 0;
    if (base < n) {
#pragma unroll
        for (int i = 0; i < X_ITEMS; i++) {
            const uint64_t idx = base + (uint64_t)threadIdx.x * X_ITEMS + i;
            if (idx < n) sum += x_value<MODE>(p, row, idx);
        }
    }
    uint64_t tot;
    block_exclusive_scan(sum, &tot);
    if (threadIdx.x == 0) p.tile_sum[(uint64_t)row * p.n_tiles + tile] = tot;
}

// one workgroup: tile sums -> tile bases (exclusive, per row); row totals -> the block headers (pack) / the entry
// total, the status and the number of owned queries (unpack)
template <int MODE> __global__ __launch_bounds__(X_BLOCK) void x_scan_top_kernel(XParams p)
{
    const uint32_t rows = (MODE & 1) ? p.world + 1u : p.world;
    __shared__ uint64_t s_total[65];
    for (uint32_t row = 0; row < rows; row++) {
        uint64_t carry = 0;
        uint64_t *ts = p.tile_sum + (uint64_t)row * p.n_tiles;
        for (uint32_t t0 = 0; t0 < p.n_tiles; t0 += X_BLOCK) {
            const uint32_t t = t0 + threadIdx.x;
            const uint64_t v = t < p.n_tiles ? ts[t] : 0;
            uint64_t tot;
            const uint64_t ex = block_exclusive_scan(v, &tot);
            if (t < p.n_tiles) ts[t] = carry + ex;
            carry += tot;
            __syncthreads();
        }
        if (threadIdx.x == 0) s_total[row < 65 ? row : 64] = carry;
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (MODE == 0) for (uint32_t d = 0; d < p.world; d++) x_pack_header(p, d, s_total[d]);
    if (MODE == 1) x_owner_verdict(p, s_total[p.world]);
    if (MODE == 2) x_pack_bits_headers(p, s_total);
    if (MODE == 3) x_owner_verdict_bits(p, s_total[p.world]);
}

template <int MODE> __global__ __launch_bounds__(X_BLOCK) void x_scan_apply_kernel(XParams p)
{
    const uint32_t row = blockIdx.y, tile = blockIdx.x;
    const uint32_t n = x_items<MODE>(p, row);
    const uint64_t base = (uint64_t)tile * X_TILE;
    if (base < n) x_tile_apply<MODE>(p, row, n, base, p.tile_sum[(uint64_t)row * p.n_tiles + tile]);
}

// small batches (up to X_SMALL_TILES tiles per row), modes 0 and 1: one workgroup per row walks its tiles with a carry --
// one launch instead of three
template <int MODE> __global__ __launch_bounds__(X_BLOCK) void x_scan_small_kernel(XParams p)
{
    static_assert(SCAN_BLOCK == X_BLOCK, "block_exclusive_scan is written for 1024 threads");
    const uint32_t row = blockIdx.x;
    const uint32_t n = x_items<MODE>(p, row);
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n; base += X_TILE) {
        carry += x_tile_apply<MODE>(p, row, n, base, carry);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (MODE == 0) x_pack_header(p, row, carry);
    else if (row == p.world) x_owner_verdict(p, carry);
}

// X_GROUP lanes per query: its hit list into the block of its owner.  (A whole wave per query left 49 of 64 lanes
// idle on an ORF batch -- 4.2 M lists of ~15 entries -- and the pass took 7.3 ms per 1 M reads.)
// Protein batches (thousands of queries, lists of a few hundred entries) take a wave per query: with 16 lanes a list
// of 186 entries is twelve dependent round trips, and the two copies were 42 + 57 us of the 460 us sharded protein step.
#define X_GROUP 16u
#define X_GROUP_WIDE 64u
#define X_WIDE_QUERIES 262144u   /* batches of at most this many queries use the wide form */
#define X_COPY_BLOCK 256
// this thread's place in a copy kernel: the first query of its group of LANES lanes, the stride to the group's next
// query, and its lane within the group
template <uint32_t LANES> struct XLanes {
    uint64_t first, stride;
    uint32_t lane;
    __device__ __forceinline__ XLanes()
        : first(((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / LANES), stride(((uint64_t)gridDim.x * blockDim.x) / LANES),
          lane(threadIdx.x & (LANES - 1u)) {}
};

template <uint32_t LANES>
__global__ __launch_bounds__(X_COPY_BLOCK) void x_pack_copy_kernel(XParams p)
{
    const uint32_t nq = *p.d_nq, W = p.world;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the scans (earlier launches) have left every block's need in X_NEED: the sender's largest goes into every header,
        // and so does the fact that one of its blocks did not fit (no thread of this kernel reads these words)
        uint32_t mx = 0, any = 0;
        for (uint32_t d = 0; d < W; d++) {
            const uint32_t *b = x_block(p.send, p, d);
            mx = b[X_NEED] > mx ? b[X_NEED] : mx;
            any |= b[X_STATUS] & XS_OVERFLOW;
        }
        for (uint32_t d = 0; d < W; d++) {
            uint32_t *b = x_block(p.send, p, d);
            b[X_NEED_MAX] = mx;
            if (any) b[X_STATUS] |= XS_SENDER_OVERFLOW;
        }
    }
    const XLanes<LANES> g;
    for (uint64_t q = g.first; q < nq; q += g.stride) {
        const uint32_t d = (uint32_t)(q % W);
        const uint64_t i = q / W;
        if (i >= p.q_cap) continue;
        const uint32_t n = p.hit_cnt[q];
        if (n == 0) continue;
        const uint64_t o = p.dst_off[(uint64_t)d * p.q_cap + i];
        if (o + n > p.e_cap) continue;  // over capacity: flagged by the scan kernel
        const uint64_t s = p.hit_off[q];
        uint32_t *blk = x_block(p.send, p, d) + p.ent_base;
        for (uint32_t t = g.lane; t < n; t += LANES) {
            blk[o + t] = p.pid[s + t];
            blk[p.e_cap + o + t] = p.km[s + t];
            if (p.with_fp) blk[2 * p.e_cap + o + t] = p.fp[s + t];
        }
    }
}

// X_GROUP lanes per owned query: the entries of all sources, source after source
template <uint32_t LANES>
__global__ __launch_bounds__(X_COPY_BLOCK) void x_unpack_copy_kernel(XParams p)
{
    const uint32_t W = p.world;
    const uint32_t n_owned = x_owned_checked(p);
    const XLanes<LANES> g;
    for (uint64_t i = g.first; i < n_owned; i += g.stride) {
        uint64_t dst = p.ent_off[i];
        for (uint32_t s = 0; s < W; s++) {
            const uint32_t *blk = x_block(p.recv, p, s);
            const uint32_t n = x_counts(blk)[i];
            const uint64_t o = p.src_off[(uint64_t)s * p.q_cap + i];
            if (o + n > p.e_cap || dst + n > p.m_cap) break;  // flagged by the scan kernel
            const uint32_t *ent = blk + p.ent_base;
            for (uint32_t t = g.lane; t < n; t += LANES) {
                p.m_pid[dst + t] = ent[o + t];
                p.m_km[dst + t] = ent[p.e_cap + o + t];
                if (p.with_fp) p.m_fp[dst + t] = ent[2 * p.e_cap + o + t];
            }
            dst += n;
        }
    }
}

// ---- PositionHits bitmaps through the exchange (arrays = 4) ------------------------------------------------------------
// X_GROUP lanes per query: the bitmaps of its hits, in hit-list order, after the bitmaps of the query before it in the
// block (hit j of owned query i at dst_boff[i] + j * ceil(SizeInKmer_i / 64)).  The search laid a query's bitmaps out at
// pos_off[hit], words = ceil(QInfo.size / 64).
template <uint32_t LANES>
__global__ __launch_bounds__(X_COPY_BLOCK) void x_pack_bits_kernel(XParams p)
{
    // a search that failed (its bitmap storage included: then pos_off was never laid out) sends no bitmaps; its blocks
    // carry XS_SENDER_FAILED and the batch fails on every rank
    if (p.src_status && *p.src_status) return;
    const uint32_t nq = *p.d_nq, W = p.world;
    const XLanes<LANES> g;
    for (uint64_t q = g.first; q < nq; q += g.stride) {
        const uint32_t d = (uint32_t)(q % W);
        const uint64_t i = q / W;
        if (i >= p.q_cap) continue;
        const uint32_t n = p.hit_cnt[q], w = x_words(p.qinfo[q].size);
        const uint64_t tot = (uint64_t)n * w;
        if (tot == 0) continue;
        const uint64_t o = p.dst_boff[(uint64_t)d * p.q_cap + i];
        if (o + tot > p.p_cap) continue;  // over capacity: flagged by the scan kernel
        const uint64_t s = p.hit_off[q];
        unsigned long long *dst = x_bits(x_block(p.send, p, d), p) + o;
        for (uint64_t t = g.lane; t < tot; t += LANES) {
            const uint64_t h = t / w;
            dst[t] = p.pos_bits[p.pos_off[s + h] + (t - h * w)];
        }
    }
}

// X_GROUP lanes per owned query: the bitmaps of all sources, source after source -- entry k of the query's unpacked
// entries (ent_off) has its bitmap at ent_boff[i] + k * words.  Nothing when the headers, the sizes or a section failed
// (d_nq_owned = 0).
template <uint32_t LANES>
__global__ __launch_bounds__(X_COPY_BLOCK) void x_unpack_bits_kernel(XParams p)
{
    const uint32_t W = p.world;
    const uint32_t n_owned = *p.d_nq_owned;
    const XLanes<LANES> g;
    for (uint64_t i = g.first; i < n_owned; i += g.stride) {
        const uint32_t w = x_words(p.m_size[i]);
        uint64_t dst = p.ent_boff[i];
        for (uint32_t s = 0; s < W && w; s++) {
            const uint32_t *blk = x_block(p.recv, p, s);
            const uint64_t tot = (uint64_t)x_counts(blk)[i] * w;
            const uint64_t o = p.src_boff[(uint64_t)s * p.q_cap + i];
            if (o + tot > p.p_cap || dst + tot > p.mb_cap) break;  // flagged by the scan kernel
            const unsigned long long *src = x_bits(blk, p) + o;
            for (uint64_t t = g.lane; t < tot; t += LANES) p.m_bits[dst + t] = src[t];
            dst += tot;
        }
    }
}

// One wave per owned query, after the merge (count_group_kernel MODE 2) and the layout of the merged bitmaps
// (pos_words_kernel / scan / pos_layout_kernel, which zeroed them): every received entry's bitmap is ORed into the bitmap
// of its merged hit.  A hash of the merged ids gives each entry its hit: in LDS (sized to the query), or -- for queries
// with more merged hits than half the LDS table -- in HBM (2 x entries slots at 2 ent_off[i], as the G tier keeps its
// tables); each entry's destination is kept in LDS, or in HBM (m_dst) for queries with more entries than that holds.
// Only a query that touches HBM scratch pays a device-scope fence (an agent-scope release writes L2 back: with one
// per query the pass took 148 ms of a 1 M-read batch).
// Every k-mer key is owned by exactly one shard, so the bitmaps one (query, protein) receives from different shards are
// DISJOINT: the 64-bit atomicOr of one word by several lanes sets each bit once, whatever the order, and the merged
// bitmap equals the unsharded search's bit for bit.
#define XO_LDS_SLOTS 1024u
__device__ __forceinline__ uint32_t xo_hash(uint32_t pid) { return pid * 2654435761u; }

__global__ __launch_bounds__(64) void x_or_bits_kernel(XParams p)
{
    __shared__ uint32_t s_key[XO_LDS_SLOTS], s_val[XO_LDS_SLOTS];
    __shared__ uint64_t s_dst[XO_LDS_SLOTS];
    const uint32_t lane = threadIdx.x;
    const uint32_t nq = *p.r_nq;
    if (p.r_pos_base[nq] > p.r_bits_cap) return;   // pos_layout_kernel flagged ST_POS_CAP and laid nothing out
    for (uint32_t i = blockIdx.x; i < nq; i += gridDim.x) {
        const uint32_t m = p.r_cnt[i];
        const uint64_t e0 = p.ent_off[i], ne = p.ent_off[i + 1] - e0;
        const uint32_t w = x_words(p.m_size[i]);
        if (m == 0 || ne == 0 || w == 0) continue;
        const uint64_t hb = p.r_off[i];
        const bool lds = m <= XO_LDS_SLOTS / 2, lds_dst = ne <= XO_LDS_SLOTS;
        uint32_t lg = 6;
        while ((1u << lg) < 2u * m && (1u << lg) < XO_LDS_SLOTS) lg++;
        const uint32_t lcap = 1u << lg;
        const uint64_t gcap = 2 * ne;   // >= 2 m: the merged ids are a subset of the entries' ids
        unsigned long long *gt = p.g_tab + 2 * e0;
        if (lds) for (uint32_t t = lane; t < lcap; t += 64) s_key[t] = KH_EMPTY_PID;
        else for (uint64_t t = lane; t < gcap; t += 64) gt[t] = ~0ull;
        if (!lds) __threadfence();
        __syncthreads();
        for (uint32_t j = lane; j < m; j += 64) {   // the merged ids are distinct
            const uint32_t pid = p.r_pid[hb + j];
            if (lds) {
                uint32_t h = xo_hash(pid) >> (32 - lg);
                while (atomicCAS(&s_key[h], KH_EMPTY_PID, pid) != KH_EMPTY_PID) h = (h + 1u) & (lcap - 1u);
                s_val[h] = j;
            } else {
                const unsigned long long v = ((unsigned long long)pid << 32) | j;
                uint64_t h = (uint64_t)xo_hash(pid) % gcap;
                while (atomicCAS(&gt[h], ~0ull, v) != ~0ull) h = h + 1 == gcap ? 0 : h + 1;
            }
        }
        if (!lds) __threadfence();
        __syncthreads();
        for (uint64_t k = lane; k < ne; k += 64) {
            const uint32_t pid = p.m_pid[e0 + k];
            uint64_t dst = ~0ull;
            if (lds) {
                uint32_t h = xo_hash(pid) >> (32 - lg);
                for (uint32_t probe = 0; probe < lcap; probe++) {
                    const uint32_t key = s_key[h];
                    if (key == pid) { dst = p.r_pos_off[hb + s_val[h]]; break; }
                    if (key == KH_EMPTY_PID) break;
                    h = (h + 1u) & (lcap - 1u);
                }
            } else {
                uint64_t h = (uint64_t)xo_hash(pid) % gcap;
                for (uint64_t probe = 0; probe < gcap; probe++) {
                    const unsigned long long v = __hip_atomic_load(&gt[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (v == ~0ull) break;
                    if ((uint32_t)(v >> 32) == pid) { dst = p.r_pos_off[hb + (uint32_t)v]; break; }
                    h = h + 1 == gcap ? 0 : h + 1;
                }
            }
            // (~0: the merge lost this query -- its status already fails the batch)
            if (lds_dst) s_dst[k] = dst;
            else p.m_dst[e0 + k] = dst;
        }
        if (!lds_dst) __threadfence();
        __syncthreads();
        const uint64_t b0 = p.ent_boff[i], tot = ne * w;
        for (uint64_t t = lane; t < tot; t += 64) {
            const unsigned long long bits = p.m_bits[b0 + t];
            if (!bits) continue;
            const uint64_t k = t / w;
            const uint64_t dst = lds_dst ? s_dst[k] : __hip_atomic_load(&p.m_dst[e0 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (dst != ~0ull) atomicOr(&p.r_pos_bits[dst + (t - k * w)], bits);
        }
        __syncthreads();
    }
}

// ---- the step's state in a workspace (host): what XParams points at, allocated on first use ------------------------------
// The block layout may change from batch to batch within the buffers' capacity, so the buffers only ever grow.
struct XStatsSlot {             // what the W headers of one merge said, as kaamer_exchange_stats(_positions) return it
    unsigned long long stats[4];   // {queries of the batch, largest block any pair of ranks needed, a block overflowed, 0}
    unsigned long long pstats[2];  // {largest bitmap need between any pair of ranks, a bitmap section overflowed}
};
struct XState {
    // pack: where each query's entries / bitmaps start inside its block
    DevBuf<uint32_t> dst_off;
    DevBuf<uint64_t> dst_boff;
    // unpack: offsets per (source, owned query), the owned queries' entries in one piece, the header statistics
    DevBuf<uint32_t> src_off, nq_owned, pid, km, fp;
    DevBuf<uint64_t> ent_off;
    DevBuf<unsigned long long> stats;
    // unpack with bitmaps: offsets, sizes, the bitmaps, the OR-merge's scratch
    DevBuf<uint64_t> src_boff, ent_boff, mdst;
    DevBuf<int32_t> msize;
    DevBuf<unsigned long long> mbits, gtab, pstats;
    DevBuf<uint64_t> tiles;           // tile sums of the tiled scans
    PinnedBuf<XStatsSlot> h_stats;    // two slots, slot = merge sequence number & 1
    DevEvent ev_stats[2];
    uint64_t merge_seq = 0;           // merges enqueued on this workspace
};
