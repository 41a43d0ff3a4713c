// top_positions.hip.inc — PositionHits bitmaps of the REPORTED hits only (included by search.hip after topn.hip.inc).
//
// The reference fills PositionHits for every hit of a query (search.go:442-452) and prints them for the hits it reports
// (search.go:520-522,540-543,591-594: at most MaxResults per query).  Once kaamer_topn_device has run, everything the
// bitmaps of those few hits need is resident: the probe's vals[] (one word per residue position: 0, an inline protein id,
// or the offset of a postings list in the arena, kaamer_layout.h), the queries' QInfo (SizeInKmer as searched -- for an
// ORF the untrimmed one, as top_first_pos is -- and the first residue position) and top_cnt / top_pid.  No counting
// table, no LDS bitmap, no atomics:
//
//   top_pos_words_kernel   per query: reported hits x ceil(SizeInKmer / 64) words (saturating at 32 bits, as
//                          pos_words_kernel does) and the bit length; the caller scans the words into per-query bases
//   top_pos_bits_kernel    one wave per reported query, 64 positions (one output word per hit) at a time: lane = position.
//                          The lane walks the ids under its k-mer and keeps a mask with bit r set when an id is reported
//                          hit r (the reported ids of the query sit in LDS, 64 at a time: MaxResults > 64 takes rounds).
//                          Postings lists longer than TP_COOP_MIN ids are not walked by their lane (10^4 ids would stall
//                          the wave behind one lane): the whole wave scans such a list with coalesced loads and ORs the
//                          lanes' masks together.  No order of the ids inside a list is assumed.
//                          Word `stripe` of hit r is then __ballot(bit r of the masks); lane r stores hit r's word.
// Layout as pos_layout_kernel's: the bitmaps of a query are contiguous, in reported order, ceil(SizeInKmer / 64) words
// each; every word of every bitmap is stored (nothing needs zeroing first).
// The same kernel serves both forms of the call: the device-resident one writes into the workspace's own storage, the
// host-buffer one appends three sections to the packed result block (topn.hip.inc) behind rep_block_kernel:
//   ... | pos_bits_len i32[n_rep] | pos_off u64[n_ent + 1] (CSR, in words) | pos_bits u64[pos_off[n_ent]]
// tp_query_bits (the bitmaps of one reported query) and tp_block_sections (where the three sections go) are shared with
// the sharded handle's kernels (top_positions_sharded.hip.inc), where every shard makes the part its own vals[] gives.
#define TP_WAVES 4
#define TP_COOP_MIN 16u   /* ids; longer lists are scanned by the whole wave */

struct TopPosParams {
    const uint32_t *d_nq;
    const QInfo *qinfo;
    const uint32_t *vals;
    const uint32_t *arena;
    const uint32_t *top_cnt, *top_pid;
    uint32_t K;
    uint32_t *words;               // per query: reported hits x words per hit (saturating)
    int32_t *bits_len;             // per query: SizeInKmer of a query that reports, else 0
    const uint64_t *base;          // exclusive scan of words[], [nq] = total
    unsigned long long *bits;      // device-resident form: the workspace's storage
    uint64_t cap;                  // ... and its capacity in words
    uint32_t *status;              // ST_POS_CAP goes here (the status of the last finished batch)
    // host-buffer form: the packed block and the scans rep_block_kernel laid it out from
    uint8_t *block;
    uint64_t block_cap;
    const uint64_t *rank, *eoff, *aoff;
};

__global__ void top_pos_words_kernel(TopPosParams p)
{
    const uint32_t nq = *p.d_nq;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * blockDim.x) {
        const int32_t size = p.qinfo[q].size;
        const uint32_t cnt = p.top_cnt[q];
        const uint64_t w = size > 0 ? (uint64_t)cnt * (((uint32_t)size + 63u) >> 6) : 0;
        p.words[q] = w > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)w;
        p.bits_len[q] = (cnt && size > 0) ? size : 0;
    }
}

__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// bit r set iff `id` is the r-th of the n reported ids in LDS (all lanes read the same address: a broadcast)
__device__ __forceinline__ unsigned long long tp_match(const uint32_t *pid, uint32_t n, uint32_t id)
{
    unsigned long long m = 0ull;
    for (uint32_t r = 0; r < n; r++) m |= (unsigned long long)(pid[r] == id) << r;
    return m;
}

// The bitmap sections behind a block that rep_block_kernel laid out from the three totals (n_rep, n_ent, n_aa); `total`
// bitmap words are wanted, `cap` is the bound.  Every thread computes the same; `first` (one thread of the grid) writes
// the header.  0: rep_block_kernel flagged the block, nothing was laid out; -1: the words do not fit (ST_POS_CAP is set:
// a bound like every other, the whole batch is repeated with a larger one, never a partial block); 1: laid out.
__device__ __forceinline__ int tp_block_sections(uint8_t *block, uint64_t block_cap, uint64_t n_rep, uint64_t n_ent, uint64_t n_aa,
                                                 uint64_t total, uint64_t cap, bool first, RepPosExt *xo)
{
    RepBlockHdr l;
    rep_block_layout(l, n_rep, n_ent, n_aa);
    const uint64_t base_total = l.total_bytes;
    if (base_total > block_cap) return 0;
    RepPosExt x;
    x.off_pos_len = base_total;
    x.off_pos_off = rep_align8(x.off_pos_len + 4 * n_rep);
    x.off_pos_bits = x.off_pos_off + 8 * (n_ent + 1);
    x.n_pos_words = total;
    RepBlockHdr *hdr = reinterpret_cast<RepBlockHdr *>(block);
    const bool fits = total <= cap && x.off_pos_bits <= block_cap && total <= (block_cap - x.off_pos_bits) / 8;
    if (!fits) {
        if (first) hdr->status |= (uint32_t)ST_POS_CAP;
        return -1;
    }
    if (first) {
        *rep_pos_ext(hdr) = x;
        hdr->total_bytes = x.off_pos_bits + 8 * total;
        reinterpret_cast<uint64_t *>(block + x.off_pos_off)[n_ent] = total;   // CSR end
    }
    *xo = x;
    return 1;
}

// The bitmaps of ONE reported query, by one wave: `ids[0..cnt)` its reported protein ids, `vals[0..size)` the probe's
// words of its residue positions, out[r * nw + stripe] word `stripe` of reported hit r (nw = ceil(size / 64) > 0).
// `pid`: 64 words of LDS of this wave.  vals[] of a shard image hold the keys that shard owns: the result is then the
// bitmap restricted to those positions.
__device__ __forceinline__ void tp_query_bits(uint32_t *pid, const uint32_t *ids, uint32_t cnt, const uint32_t *vals, uint32_t size,
                                              const uint32_t *arena, unsigned long long *out, uint32_t lane)
{
    const uint32_t nw = (size + 63u) >> 6;
    for (uint32_t r0 = 0; r0 < cnt; r0 += 64) {   // cnt <= K; K may exceed 64
        const uint32_t nr = cnt - r0 < 64u ? cnt - r0 : 64u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the previous round's readers are done
        __builtin_amdgcn_wave_barrier();
        pid[lane] = lane < nr ? ids[r0 + lane] : KH_EMPTY_PID;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t st = 0; st < nw; st++) {
            const uint32_t pos = (st << 6) + lane;
            const uint32_t v = pos < size ? vals[pos] : 0u;
            unsigned long long mask = 0ull;
            uint32_t n_ids = 0;
            if (v & KH_INLINE_BIT) mask = tp_match(pid, nr, v & ~KH_INLINE_BIT);
            else if (v) {
                const uint32_t *l = arena + (uint64_t)v * 4;   // {count, ids...}
                n_ids = l[0];
                if (n_ids <= TP_COOP_MIN)
                    for (uint32_t t = 0; t < n_ids; t++) mask |= tp_match(pid, nr, l[1 + t]);
            }
            unsigned long long todo = __ballot(n_ids > TP_COOP_MIN);
            while (todo) {   // wave-uniform: the long lists of this stripe, one after the other
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const uint32_t lv = (uint32_t)__shfl((int)v, src, 64), ln = (uint32_t)__shfl((int)n_ids, src, 64);
                const uint32_t *lids = arena + (uint64_t)lv * 4 + 1;
                unsigned long long m = 0ull;
                for (uint32_t t = lane; t < ln; t += 64) m |= tp_match(pid, nr, lids[t]);
                m = wave_or_u64(m);
                if ((int)lane == src) mask = m;
            }
            unsigned long long mine = 0ull;
            for (uint32_t j = 0; j < nr; j++) {
                const unsigned long long b = __ballot((mask >> j) & 1ull);
                if (lane == j) mine = b;
            }
            if (lane < nr) out[(uint64_t)(r0 + lane) * nw + st] = mine;
        }
    }
}

__global__ __launch_bounds__(64 * TP_WAVES) void top_pos_bits_kernel(TopPosParams p)
{
    __shared__ uint32_t s_pid[TP_WAVES][64];
    if (*p.status) return;   // the batch exceeded a bound earlier: its result is refused, whatever is left of it is not read
    const uint32_t nq = *p.d_nq;
    const uint64_t total = p.base[nq];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    unsigned long long *bits = p.bits;
    uint64_t cap = p.cap;
    int32_t *rep_len = nullptr;
    uint64_t *rep_poff = nullptr;
    if (p.block) {
        // the sections rep_block_kernel wrote, from the same three totals (every thread computes the same)
        RepPosExt x;
        if (tp_block_sections(p.block, p.block_cap, p.rank[nq], p.eoff[nq], p.aoff[nq], total, cap, first, &x) <= 0) return;
        rep_len = reinterpret_cast<int32_t *>(p.block + x.off_pos_len);
        rep_poff = reinterpret_cast<uint64_t *>(p.block + x.off_pos_off);
        bits = reinterpret_cast<unsigned long long *>(p.block + x.off_pos_bits);
    } else if (total > cap) {
        if (first) atomicOr(p.status, (uint32_t)ST_POS_CAP);
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *pid = s_pid[wv];
    const uint64_t wave = (uint64_t)blockIdx.x * TP_WAVES + wv, n_waves = (uint64_t)gridDim.x * TP_WAVES;
    for (uint64_t q = wave; q < nq; q += n_waves) {
        const uint32_t cnt = p.top_cnt[q];
        if (cnt == 0) continue;   // most ORFs of a reads batch: no words, no work
        const QInfo qi = p.qinfo[q];
        const uint32_t size = qi.size > 0 ? (uint32_t)qi.size : 0u;
        const uint32_t nw = (size + 63u) >> 6;
        const uint64_t qbase = p.base[q];
        if (rep_len) {
            if (lane == 0) rep_len[p.rank[q]] = (int32_t)size;
            const uint64_t e = p.eoff[q];
            for (uint32_t i = lane; i < cnt; i += 64) rep_poff[e + i] = qbase + (uint64_t)i * nw;
        }
        if (nw == 0) continue;
        const uint32_t *vals = p.vals + qi.aa_off;
        unsigned long long *out = bits + qbase;
        tp_query_bits(pid, p.top_pid + q * p.K, cnt, vals, size, p.arena, out, lane);
    }
}
