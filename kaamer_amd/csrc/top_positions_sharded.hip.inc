// top_positions_sharded.hip.inc — PositionHits bitmaps of the REPORTED hits on a sharded index (included by search.hip
// after exchange.hip.inc).
//
// The reported hits of a query are known at its owner only after the merge and the top-N step, while the probe's vals[]
// (top_positions.hip.inc) live on the shards: each shard's vals[] hold the keys that shard owns.  One more round trip
// after search -> pack -> pull -> merge -> top-N therefore makes the bitmaps of the reported hits, and only those cross
// devices (the reference fills PositionHits for every hit, search.go:442-452, and prints them for the hits it reports,
// search.go:520-522,540-543,591-594):
//
//   tps_ids_pack_kernel   owner d, behind rep_block_kernel: the reported queries of the owner as a compact IDS BLOCK
//                         (u32 words; rq_cap / ent_cap: the bounds the block was sized with)
//                           [0] batch sequence  [1] n_rep  [2],[3] n_ent (u64)  [4] status (the owner's failure bits;
//                           ST_IDS_CAP: the block cannot hold the reported ids)  [5..7] zero
//                           rep_query u32[rq_cap] (owned-query indices, ascending) | off u64[rq_cap + 1]
//                           | pid u32[ent_cap] (sortMapByValue order, as reported)
//                         Every shard pulls all W ids blocks.
//   tps_words_kernel      shard s, per owner d: checks the header, then per reported query i (batch query
//                         q = d + rep_query[i] W): cnt_i x ceil(size_q / 64) words, size_q = the shard's own QInfo.size
//                         (every shard translates the batch alike: the untrimmed SizeInKmer, as top_pos_words_kernel).
//                         The caller scans them (scan_u32_on) into per-query word offsets: every shard and the owner
//                         compute the same offsets and the same total.
//   tps_bits_kernel       shard s, per owner d: one wave per reported query, tp_query_bits on the shard's vals[]: its
//                         PARTIAL bitmaps (the unsharded bitmap restricted to the positions whose keys the shard owns;
//                         the W partials of a hit are disjoint) into SEGMENT d of the shard's send buffer:
//                           u64 [0] = batch sequence | status << 32, then the words in exactly the pos_bits layout of
//                           owner d's packed block (contiguous per reported query, in reported order).
//   tps_or_kernel         owner d, after pulling segment d of every shard: checks the W headers, lays out the bitmap
//                         sections of its packed block (tp_block_sections), writes pos_bits_len / pos_off and ORs the W
//                         segments word by word into pos_bits.  No hash, no atomics: all W segments have one layout.
// Sizes are bounds like every other: an ids block or a segment that is too small is seen by every shard and the owner
// (same totals), flagged in the headers and in the packed block's status (ST_IDS_CAP / ST_POS_CAP); the caller
// repeats the batch with larger ones and never gets a partial block.
#define TPS_HDR 8u

struct TpsIdsLayout {
    uint32_t rq_cap;     // reported queries the block holds
    uint64_t ent_cap;    // reported ids it holds
};
__host__ __device__ __forceinline__ uint64_t tps_ids_off_at(const TpsIdsLayout &L) { return ((uint64_t)TPS_HDR + L.rq_cap + 1u) & ~1ull; }   // even: u64 aligned
__host__ __device__ __forceinline__ uint64_t tps_ids_pid_at(const TpsIdsLayout &L) { return tps_ids_off_at(L) + 2ull * ((uint64_t)L.rq_cap + 1); }
__host__ __device__ __forceinline__ uint64_t tps_ids_words(const TpsIdsLayout &L) { return (tps_ids_pid_at(L) + L.ent_cap + 1ull) & ~1ull; }

struct TpsIdsHdr {   // words [0..7] of an ids block
    uint32_t seq, n_rep;
    uint64_t n_ent;
    uint32_t status, zero[3];
};
static_assert(sizeof(TpsIdsHdr) == 4 * TPS_HDR && offsetof(TpsIdsHdr, n_ent) == 8 && offsetof(TpsIdsHdr, status) == 16, "ids block header");

struct TpsIds {   // an ids block as its readers see it
    uint32_t seq, n_rep, status;
    uint64_t n_ent;
    const uint32_t *rq;
    const uint64_t *off;
    const uint32_t *pid;
};
__host__ __device__ __forceinline__ TpsIds tps_ids_view(const uint32_t *ids, const TpsIdsLayout &L)
{
    const TpsIdsHdr *h = reinterpret_cast<const TpsIdsHdr *>(ids);
    TpsIds v;
    v.seq = h->seq; v.n_rep = h->n_rep; v.n_ent = h->n_ent; v.status = h->status;
    v.rq = ids + TPS_HDR;
    v.off = reinterpret_cast<const uint64_t *>(ids + tps_ids_off_at(L));
    v.pid = ids + tps_ids_pid_at(L);
    return v;
}

struct TpsParams {
    uint32_t world, owner, seq;
    TpsIdsLayout ids_layout;
    // owner side: the merge workspace's top-N result and the scans topn_pack_block made
    const uint32_t *m_nq;
    const uint32_t *top_cnt, *top_pid;
    uint32_t K;
    const uint64_t *rank, *eoff, *aoff;
    const uint32_t *m_status;        // the merge workspace's status word
    uint8_t *block;                  // the owner's packed result block
    uint64_t block_cap;
    uint32_t *ids_out;               // pack: the owner's ids block
    // shard side
    const uint32_t *ids;             // the ids block of `owner` as this shard (or the owner itself) holds it
    const uint32_t *s_nq;            // the search workspace: queries, QInfo, vals[], its status word
    const QInfo *qinfo;
    const uint32_t *vals, *arena;
    const uint32_t *s_status;
    uint32_t *n_out;                 // [0] reported queries of this owner after the checks, [1] status of the checks
    uint32_t *words;                 // per reported query: hits x words per hit (saturating)
    const uint64_t *base;            // exclusive scan of words[], [n] = total
    unsigned long long *seg;         // bits: this shard's segment for `owner`; OR: the W received segments
    uint64_t seg_cap, seg_stride;    // bitmap words a segment holds; u64 words between received segments
};

__device__ __forceinline__ uint64_t tps_seg_header(uint32_t seq, uint32_t status) { return (uint64_t)seq | ((uint64_t)status << 32); }

__global__ __launch_bounds__(256) void tps_ids_pack_kernel(TpsParams p)
{
    const uint32_t nq = *p.m_nq;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const uint64_t n_rep = p.rank[nq], n_ent = p.eoff[nq];
    RepBlockHdr *hdr = reinterpret_cast<RepBlockHdr *>(p.block);
    // the owner's failure bits: its merge status (a failed shard is in there: the exchange blocks carry it) and a packed
    // block that overflowed.  (hdr->status gains at most the bit set below, by the one thread, when `fits` is false.)
    const uint32_t failed = *p.m_status | (hdr->status & 0x80000000u ? (uint32_t)ST_EXCHANGE_CAP : 0u);
    const bool fits = n_rep <= p.ids_layout.rq_cap && n_ent <= p.ids_layout.ent_cap;
    const bool ok = !failed && fits;
    if (first) {
        TpsIdsHdr h;
        h.seq = p.seq;
        h.n_rep = ok ? (uint32_t)n_rep : 0u;
        h.n_ent = ok ? n_ent : 0ull;
        h.status = failed | (fits ? 0u : (uint32_t)ST_IDS_CAP);
        h.zero[0] = h.zero[1] = h.zero[2] = 0u;
        *reinterpret_cast<TpsIdsHdr *>(p.ids_out) = h;
        if (!fits) hdr->status |= (uint32_t)ST_IDS_CAP;
    }
    if (!ok) return;
    uint32_t *rq = p.ids_out + TPS_HDR;
    uint64_t *off = reinterpret_cast<uint64_t *>(p.ids_out + tps_ids_off_at(p.ids_layout));
    uint32_t *pid = p.ids_out + tps_ids_pid_at(p.ids_layout);
    if (first) off[n_rep] = n_ent;
    for (uint64_t q = wave; q < nq; q += n_waves) {
        const uint32_t cnt = p.top_cnt[q];
        if (cnt == 0) continue;
        const uint64_t r = p.rank[q], e = p.eoff[q];
        if (lane == 0) { rq[r] = (uint32_t)q; off[r] = e; }
        for (uint32_t i = lane; i < cnt; i += 64) pid[e + i] = p.top_pid[q * p.K + i];
    }
}

// 0: the block describes this batch, no failure, within its bounds; s_nq, s_status: the reader's own search workspace's
__device__ __forceinline__ uint32_t tps_ids_check(const TpsIds &v, uint32_t seq, const TpsIdsLayout &L, uint32_t s_nq, uint32_t s_status)
{
    uint32_t st = v.status | s_status;
    if (v.seq != seq || v.n_rep > L.rq_cap || v.n_rep > s_nq || v.n_ent > L.ent_cap) st |= (uint32_t)ST_PEER_FAILED;
    return st;
}

// the W received segment headers (seq | status << 32), stride bytes apart, folded into a status word
__device__ __forceinline__ uint32_t tps_segs_status(const void *segs, uint64_t stride, uint32_t world, uint32_t seq)
{
    uint32_t st = 0;
    for (uint32_t s = 0; s < world; s++) {
        const uint64_t h = *reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(segs) + (uint64_t)s * stride);
        if ((uint32_t)h != seq) st |= (uint32_t)ST_PEER_FAILED;
        st |= (uint32_t)(h >> 32);
    }
    return st;
}

__global__ __launch_bounds__(256) void tps_words_kernel(TpsParams p)
{
    const TpsIds v = tps_ids_view(p.ids, p.ids_layout);
    const uint32_t nq = *p.s_nq;
    const uint32_t st = tps_ids_check(v, p.seq, p.ids_layout, nq, *p.s_status);
    const uint32_t n = st ? 0u : v.n_rep;
    if (blockIdx.x == 0 && threadIdx.x == 0) { p.n_out[0] = n; p.n_out[1] = st; }
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = (uint64_t)p.owner + (uint64_t)v.rq[i] * p.world;
        const int32_t size = q < nq ? p.qinfo[q].size : 0;
        const uint64_t cnt = v.off[i + 1] - v.off[i];
        const uint64_t w = cnt <= p.K ? cnt * x_words(size) : 0ull;
        p.words[i] = x_sat32(w);
    }
}

__global__ __launch_bounds__(64 * TP_WAVES) void tps_bits_kernel(TpsParams p)
{
    __shared__ uint32_t s_pid[TP_WAVES][64];
    const uint32_t n = p.n_out[0];
    const uint64_t total = p.base[n];
    const uint32_t st = p.n_out[1] | (total > p.seg_cap ? (uint32_t)ST_POS_CAP : 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) p.seg[0] = tps_seg_header(p.seq, st);
    if (st) return;
    const uint32_t nq = *p.s_nq;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *pid = s_pid[wv];
    const TpsIds v = tps_ids_view(p.ids, p.ids_layout);
    unsigned long long *bits = p.seg + 1;
    const uint64_t wave = (uint64_t)blockIdx.x * TP_WAVES + wv, n_waves = (uint64_t)gridDim.x * TP_WAVES;
    for (uint64_t i = wave; i < n; i += n_waves) {
        const uint64_t q = (uint64_t)p.owner + (uint64_t)v.rq[i] * p.world;
        if (q >= nq) continue;
        const QInfo qi = p.qinfo[q];
        const uint32_t size = qi.size > 0 ? (uint32_t)qi.size : 0u;
        const uint64_t e = v.off[i], cnt = v.off[i + 1] - e;
        if (size == 0 || cnt == 0 || cnt > p.K) continue;   // (no words were counted for it)
        tp_query_bits(pid, v.pid + e, (uint32_t)cnt, p.vals + qi.aa_off, size, p.arena, bits + p.base[i], lane);
    }
}

__global__ __launch_bounds__(256) void tps_or_kernel(TpsParams p)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    RepBlockHdr *hdr = reinterpret_cast<RepBlockHdr *>(p.block);
    // a batch that failed earlier (on the owner, on a shard, or in the ids block): refused as it is.  The checks below
    // depend on the received headers only, so every thread takes the same way whatever it reads here.
    const TpsIds v = tps_ids_view(p.ids, p.ids_layout);
    if (hdr->status || v.status) return;
    uint32_t st = tps_segs_status(p.seg, 8 * p.seg_stride, p.world, p.seq);
    const uint32_t nq = *p.m_nq;
    const uint64_t n_rep = p.rank[nq], n_ent = p.eoff[nq], n_aa = p.aoff[nq];
    if (p.n_out[0] != n_rep) st |= (uint32_t)ST_PEER_FAILED;   // the owner's own shard walked the same ids block
    if (st) {
        if (first) hdr->status |= st;
        return;
    }
    const uint64_t total = p.base[n_rep];
    RepPosExt x;
    if (tp_block_sections(p.block, p.block_cap, n_rep, n_ent, n_aa, total, p.seg_cap, first, &x) <= 0) return;
    int32_t *rep_len = reinterpret_cast<int32_t *>(p.block + x.off_pos_len);
    uint64_t *rep_poff = reinterpret_cast<uint64_t *>(p.block + x.off_pos_off);
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(p.block + x.off_pos_bits);
    const uint32_t s_nq = *p.s_nq;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wave; i < n_rep; i += n_waves) {
        const uint64_t q = (uint64_t)p.owner + (uint64_t)v.rq[i] * p.world;
        const int32_t size = q < s_nq ? p.qinfo[q].size : 0;
        const uint32_t nw = x_words(size);
        const uint64_t e = v.off[i], cnt = v.off[i + 1] - e, b = p.base[i];
        if (lane == 0) rep_len[i] = size > 0 ? size : 0;
        for (uint64_t j = lane; j < cnt; j += 64) rep_poff[e + j] = b + j * nw;
    }
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long v = 0ull;
        for (uint32_t s = 0; s < p.world; s++) v |= p.seg[(uint64_t)s * p.seg_stride + 1 + w];
        bits[w] = v;
    }
}
