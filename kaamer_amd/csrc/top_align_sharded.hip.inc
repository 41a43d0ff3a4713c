// top_align_sharded.hip.inc — the alignment (`-aln`) of the REPORTED hits on a sharded index (included by search.hip after
// top_align.hip.inc and top_positions_sharded.hip.inc).
//
// After merge and top-N the reported hits of a query are known at its owner only (device q mod W), where the query's
// residues are too (every shard translates the whole batch).  The Protein.Sequence table is PARTITIONED over the handle's
// devices like the keys (kaamer_sharded_index_attach_proteins): device s holds the entries whose id mod W == s.  One more
// round trip brings the subjects of the reported hits, and only those, to the owner:
//
//   owner d -> holders    the compact ids block of tps_ids_pack_kernel (top_positions_sharded.hip.inc), as it is: a call
//                         that wants positions AND alignments packs and pulls it once
//   tas_len_kernel        holder s, per owner d: checks the block's header, then one wave per reported query: per reported
//                         id, in block order, one u32 into the length array of SEGMENT d of the holder's send buffer -- the
//                         stored length, TAS_NOT_MINE (id mod W != s), TAS_NO_ENTRY (mine, no entry in the table) or
//                         TAS_TOO_LONG -- and the bytes the query's held subjects take.  The caller scans those
//                         (scan_u32_on) straight into the segment's base array.
//   tas_gather_kernel     holder s, per owner d: one wave per reported query copies the stored bytes of its held subjects
//                         behind one another, in pair order, with 16-byte loads and stores.  The segment:
//                           u64 [0] = batch sequence | status << 32   [1] = payload bytes the segment needed
//                           base u64[rq_cap + 1]   first payload byte of each reported query's held subjects
//                           len  u32[ent_cap]      per reported id
//                           bytes u8[byte_cap]     (16-byte aligned)
//                         A subject reported for several queries of one owner travels once per pair.
//   tas_check_kernel      owner d, after pulling segment d of every holder: the W headers; a failure lands in the packed
//                         block's status (ST_SEG_CAP: a segment was too small)
//   tas_pairs_kernel      owner d: the sharded sibling of ta_pairs_kernel.  One wave per owned query i (batch query
//                         d + i W: meta and residues on the owner's search workspace, trim in the merge workspace's top-N
//                         result): folds the query's letters, takes every pair's length and byte offset from the ONE
//                         segment whose holder is id mod W, derives the subject's letter codes and its bad-letter flag from
//                         the raw bytes (aln_code) into a codes buffer at the same offsets, and classifies the pair by the
//                         rules ta_pairs_kernel follows (ta_pair).  entry = the pair's own index; pair_off[] holds its byte offset:
//                         TaTable { raw = the received segments, codes, off = pair_off } describes the gathered subjects.
// ta_layout_kernel, ta_wave_kernel<false> / <true> and ta_finish_kernel then run unchanged on the owner.
#define TAS_NOT_MINE 0xFFFFFFFFu
#define TAS_NO_ENTRY 0xFFFFFFFEu
#define TAS_TOO_LONG 0xFFFFFFFDu
#define TAS_MAX_LEN 0x3FFFFFFFu   /* a stored length that travels; beyond it the pair fails with status 3 (ta_pair) */

struct TasLayout {
    uint32_t rq_cap;      // reported queries the segment describes
    uint64_t ent_cap;     // reported ids
    uint64_t byte_cap;    // payload bytes
};
__host__ __device__ __forceinline__ uint64_t tas_align16(uint64_t x) { return (x + 15ull) & ~15ull; }
__host__ __device__ __forceinline__ uint64_t tas_base_at() { return 16; }
__host__ __device__ __forceinline__ uint64_t tas_len_at(const TasLayout &L) { return 16 + 8ull * ((uint64_t)L.rq_cap + 1); }
__host__ __device__ __forceinline__ uint64_t tas_bytes_at(const TasLayout &L) { return tas_align16(tas_len_at(L) + 4ull * L.ent_cap); }
__host__ __device__ __forceinline__ uint64_t tas_seg_bytes(const TasLayout &L) { return tas_align16(tas_bytes_at(L) + L.byte_cap); }

struct TasParams {
    uint32_t world, owner, self, seq, K;
    TpsIdsLayout ids_layout;
    TasLayout lay;
    const uint32_t *ids;             // the ids block of `owner` as this device holds it
    // holder side: its search workspace's query count and status word, its part of the table
    const uint32_t *s_nq, *s_status;
    const uint8_t *raw;
    const uint64_t *off;
    const uint32_t *idmap;           // id / W -> entry, TA_NONE: no entry
    uint32_t idmap_n;
    uint32_t *n_out;                 // [0] reported queries of this owner after the checks, [1] status of the checks
    uint32_t *qbytes;                // per reported query: bytes of its held subjects (saturating)
    uint8_t *seg;                    // this holder's segment for `owner`
    unsigned long long *need_out;    // [0] payload bytes the segment needed, [1] its status (read by the host)
    // owner side
    const uint32_t *m_nq;
    const kaamer_query_meta *q;
    const uint32_t *top_cnt, *top_pid;
    const int32_t *trim;
    const uint64_t *rank, *eoff;
    const uint8_t *qraw;
    uint8_t *qcodes;
    const uint8_t *segs;             // the W received segments, seg_stride bytes apart
    uint64_t seg_stride;
    uint8_t *codes;                  // the subjects' letter codes, at the offsets of `segs`
    uint64_t *pair_off;              // per pair: byte offset of its subject in `segs`
    uint8_t *block;
    const TaLayout *tlay;
};

__device__ __forceinline__ uint64_t tas_shfl64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t tas_incl_scan(uint64_t v, uint32_t lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
        if (lane >= (uint32_t)d) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(256) void tas_len_kernel(TasParams p)
{
    const TpsIds v = tps_ids_view(p.ids, p.ids_layout);
    uint32_t st = tps_ids_check(v, p.seq, p.ids_layout, *p.s_nq, *p.s_status);
    if (!st && (v.n_rep > p.lay.rq_cap || v.n_ent > p.lay.ent_cap)) st |= (uint32_t)ST_SEG_CAP;   // ... and within the segment's
    const uint32_t n = st ? 0u : v.n_rep;
    if (blockIdx.x == 0 && threadIdx.x == 0) { p.n_out[0] = n; p.n_out[1] = st; }
    uint32_t *len = reinterpret_cast<uint32_t *>(p.seg + tas_len_at(p.lay));
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wave; i < n; i += n_waves) {
        const uint64_t e = v.off[i], e1 = v.off[i + 1];
        uint64_t sum = 0;
        if (e <= e1 && e1 <= v.n_ent) {
            for (uint64_t j = e + lane; j < e1; j += 64) {
                const uint32_t pid = v.pid[j];
                uint32_t l = TAS_NOT_MINE;
                if (pid % p.world == p.self) {
                    const uint32_t local = pid / p.world;
                    const uint32_t ent = local < p.idmap_n ? p.idmap[local] : TA_NONE;
                    if (ent == TA_NONE) l = TAS_NO_ENTRY;
                    else {
                        const uint64_t ns = p.off[ent + 1] - p.off[ent];
                        l = ns > TAS_MAX_LEN ? TAS_TOO_LONG : (uint32_t)ns;
                    }
                }
                len[j] = l;
                if (l <= TAS_MAX_LEN) sum += l;
            }
        }
        sum = tas_incl_scan(sum, lane);
        // (saturating: a query whose held subjects reach 4 GiB makes the total exceed every segment -- the host keeps byte_cap
        // below 2^32 - 1 -- so tas_gather_kernel refuses the segment with ST_SEG_CAP before any base[] is used)
        if (lane == 63) p.qbytes[i] = x_sat32(sum);
    }
}

// n bytes from src to dst by one wave: 16-byte stores to the aligned middle, one byte per lane at the two ends
__device__ __forceinline__ void tas_wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane)
{
    uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    if (head > n) head = n;
    if (lane < head) dst[lane] = src[lane];
    const uint32_t chunks = (n - head) / 16u, done = head + 16u * chunks;
    for (uint32_t k = lane; k < chunks; k += 64) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16u * k, 16);      // (the source's alignment is whatever the table gave it)
        *reinterpret_cast<uint4 *>(dst + head + 16u * k) = v;
    }
    if (lane < n - done) dst[done + lane] = src[done + lane];
}

__global__ __launch_bounds__(256) void tas_gather_kernel(TasParams p)
{
    const uint32_t n = p.n_out[0];
    const uint64_t *base = reinterpret_cast<const uint64_t *>(p.seg + tas_base_at());
    const uint64_t total = n ? base[n] : 0ull;
    const uint32_t st = p.n_out[1] | (total > p.lay.byte_cap ? (uint32_t)ST_SEG_CAP : 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long *h = reinterpret_cast<unsigned long long *>(p.seg);
        h[0] = tps_seg_header(p.seq, st);
        h[1] = total;
        p.need_out[0] = total; p.need_out[1] = st;
    }
    if (st) return;
    const TpsIds v = tps_ids_view(p.ids, p.ids_layout);
    const uint32_t *len = reinterpret_cast<const uint32_t *>(p.seg + tas_len_at(p.lay));
    uint8_t *bytes = p.seg + tas_bytes_at(p.lay);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wave; i < n; i += n_waves) {
        const uint64_t e = v.off[i], e1 = v.off[i + 1];
        if (e > e1 || e1 > v.n_ent) continue;   // (as tas_len_kernel: nothing was counted for it)
        uint64_t run = base[i];
        const uint64_t end = base[i + 1];
        for (uint64_t j0 = e; j0 < e1; j0 += 64) {
            const uint64_t j = j0 + lane;
            uint32_t l = TAS_NOT_MINE;
            uint64_t src = 0;
            if (j < e1) {
                l = len[j];
                if (l <= TAS_MAX_LEN) src = p.off[p.idmap[v.pid[j] / p.world]];
            }
            const uint32_t c = l <= TAS_MAX_LEN ? l : 0u;
            const uint64_t incl = tas_incl_scan(c, lane);
            const uint64_t mine = run + incl - c;
            unsigned long long todo = __ballot(c != 0u);
            while (todo) {
                const int b = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const uint32_t lb = (uint32_t)__shfl((int)c, b, 64);
                const uint64_t ob = tas_shfl64(mine, b), sb = tas_shfl64(src, b);
                if (ob + lb <= end) tas_wave_copy(bytes + ob, p.raw + sb, lb, lane);   // (within what the scan gave the query)
            }
            run += tas_shfl64(incl, 63);
        }
    }
}

__global__ void tas_check_kernel(TasParams p)
{
    RepBlockHdr *hdr = reinterpret_cast<RepBlockHdr *>(p.block);
    if (hdr->status || tps_ids_view(p.ids, p.ids_layout).status) return;   // a batch that failed earlier: refused as it is
    const uint32_t st = tps_segs_status(p.segs, p.seg_stride, p.world, p.seq);
    if (st) hdr->status |= st;
}

__global__ __launch_bounds__(256) void tas_pairs_kernel(TasParams p)
{
    if (!p.tlay->ok) return;
    kaamer_align_pair *items = p.tlay->items;
    const uint32_t nq = *p.m_nq;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t bytes_at = tas_bytes_at(p.lay), len_at = tas_len_at(p.lay);
    for (uint64_t q = wave; q < nq; q += n_waves) {
        const uint32_t cnt = p.top_cnt[q];
        if (cnt == 0) continue;
        const kaamer_query_meta m = p.q[(uint64_t)p.owner + q * p.world];
        const uint32_t tr = (uint32_t)p.trim[q];
        const uint32_t qlen = m.aa_len - tr;            // Query.Sequence as the handler holds it: the trimmed ORF
        const uint64_t qoff = m.aa_off + tr;
        const bool qbad = ta_wave_codes(p.qraw + qoff, p.qcodes + qoff, qlen, lane);
        const uint64_t e0 = p.eoff[q], rk = p.rank[q];
        // the length of reported id r, as its holder h = id mod W stored it in its segment
        auto len_of = [&](uint32_t h, uint32_t r) { return reinterpret_cast<const uint32_t *>(p.segs + (uint64_t)h * p.seg_stride + len_at)[e0 + r]; };
        // a holder that did not answer for its own id (never, with checked headers) counts as an id without an entry
        const uint32_t first_missing = ta_first_missing(cnt, lane, [&](uint32_t r) {
            const uint32_t l = len_of(p.top_pid[q * p.K + r] % p.world, r);
            return l == TAS_NO_ENTRY || l == TAS_NOT_MINE;
        });
        // lane h: where the query's next subject lies in holder h's payload
        uint64_t run = 0, run_end = 0;
        if (lane < p.world) {
            const uint64_t *base = reinterpret_cast<const uint64_t *>(p.segs + (uint64_t)lane * p.seg_stride + tas_base_at());
            run = base[rk]; run_end = base[rk + 1];
        }
        for (uint32_t r0 = 0; r0 < cnt; r0 += 64) {
            const uint32_t r = r0 + lane;
            const bool valid = r < cnt;
            uint32_t h = 0xFFFFFFFFu, l = TAS_NOT_MINE;
            if (valid) { h = p.top_pid[q * p.K + r] % p.world; l = len_of(h, r); }
            const uint32_t c = l <= TAS_MAX_LEN ? l : 0u;
            uint64_t soff = 0;
            bool inside = true;
            for (uint32_t hh = 0; hh < p.world; hh++) {
                if (!__ballot(valid && h == hh)) continue;
                const uint64_t incl = tas_incl_scan(h == hh ? (uint64_t)c : 0ull, lane);
                const uint64_t b = tas_shfl64(run, (int)hh), e = tas_shfl64(run_end, (int)hh), tot = tas_shfl64(incl, 63);
                if (h == hh) {
                    const uint64_t at = b + incl - c;
                    inside = at + c <= e && e <= p.lay.byte_cap;
                    soff = (uint64_t)hh * p.seg_stride + bytes_at + at;
                }
                if (lane == hh) run += tot;
            }
            if (!inside) l = TAS_TOO_LONG;   // (never, with checked headers: nothing is read outside a segment)
            if (valid) p.pair_off[e0 + r] = soff;
            // the subjects' letter codes and bad-letter flags, pair by pair
            bool sbad = false;
            const uint32_t in_chunk = cnt - r0 < 64u ? cnt - r0 : 64u;
            for (uint32_t j = 0; j < in_chunk && r0 + j < first_missing; j++) {
                const uint32_t lj = (uint32_t)__shfl((int)l, (int)j, 64);
                if (lj > TAS_MAX_LEN) continue;
                const uint64_t oj = tas_shfl64(soff, (int)j);
                const bool any = ta_wave_codes(p.segs + oj, p.codes + oj, lj, lane);
                if (lane == j) sbad = any;
            }
            if (!valid) continue;
            items[e0 + r] = ta_pair(qlen, qoff, qbad, r >= first_missing, (uint32_t)(e0 + r), l <= TAS_MAX_LEN ? l : TA_NS_TOO_LONG, sbad);
        }
    }
}
