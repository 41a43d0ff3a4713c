// top_align.hip.inc — the alignment step (`-aln`) of the REPORTED hits, behind kaamer_topn_device on the same stream
// (included by search.hip after top_positions.hip.inc).
//
// QueryResultHandler (search.go:483-494) aligns every reported hit with its query -- align.Align(query.Sequence,
// HitEntries[hit.Key].Sequence, ...) -- and re-sorts the hits by BitScore.  Once kaamer_topn_device has run, both sides
// of every pair are resident: the query residues (the batch input, or the ORF buffer; the ORF after SetBestStartCodon's
// trim) and the database's Protein.Sequence table (kaamer_index_attach_proteins).  No host round trip in between:
//
//   ta_layout_kernel   one thread: where the pair records and the operations go (two sections behind the packed result
//                      block of topn.hip.inc / top_positions.hip.inc, or the workspace's own array), tickets to zero
//   ta_pairs_kernel    one wave per reported query: folds the query's letters to the aligner's codes ([uU] -> '*', case
//                      folded; a letter outside the alphabet fails the query's pairs, status 2), resolves every reported
//                      id through the table's id map and classifies the pair: wave-per-pair, long subject (beyond
//                      ALN_WAVE_NS), empty (no cell), failed (2 bad letter, 3 too long, 4 no entry in the table: the
//                      reference's FetchHitsInformation stops a query's loop at the first such id, search.go:461-463, so
//                      that hit and the query's later ones keep the empty AlignmentResult)
//   ta_wave_kernel     a grid of PERSISTENT waves, each the owner of one direction slab, takes pairs by ticket until none
//                      are left and runs align_wave_pair (align_wave.hip.inc: the recurrence of align_wave_kernel, not a
//                      copy) with the tallies of align.go:87-133 stepped inside the traceback.  The slab is sized on the
//                      host from the batch's longest query and the table's longest subject (capped at ALN_WAVE_NS), the
//                      number of waves from a byte budget: no rounds, no retry, no partial result.  <true>: the few
//                      pairs with a longer subject, boundary row and subject in HBM, slabs of the table's longest subject.
//                      With text wanted a pair's n_ops operations go to the compact section at an atomically taken offset.
//   ta_finish_kernel   one thread: the block's final size
// Floats (Identity, Similarity, BitScore, EValue), the <= MaxResults-element sort and the three rows stay on the host
// (host_top_align.hip.inc), through the same code kaamer_align_pairs uses.
#include "align_wave.hip.inc"

#define TA_NONE 0xFFFFFFFFu
#define TA_WAVE (-1)   /* status of a pair that waits for ta_wave_kernel<false> */
#define TA_LONG (-2)   /* ... for ta_wave_kernel<true> */

static_assert(sizeof(kaamer_align_pair) == 64, "pair record");

struct TaTable {   // the attached Protein.Sequence table on the device
    const uint8_t *raw, *codes;    // stored bytes; the aligner's letter codes
    const uint64_t *off;           // n_entries + 1
    const uint8_t *bad;            // per entry: a letter outside the alphabet
    const uint32_t *idmap;         // protein id -> entry, TA_NONE: no entry
    uint32_t idmap_n;
};

struct TaLayout {
    kaamer_align_pair *items;
    uint8_t *ops;
    uint64_t ops_cap, n_ent, items_bytes;
    uint32_t ok, pad;
};

struct TaParams {
    const uint32_t *d_nq;
    const kaamer_query_meta *q;
    const uint32_t *top_cnt, *top_pid;
    const int32_t *trim;
    uint32_t K;
    const uint64_t *eoff;          // exclusive scan of top_cnt: pair e = eoff[q] + r
    const uint8_t *qraw;           // the queries' residues (batch input / ORF buffer)
    uint8_t *qcodes;               // their codes, at the same offsets
    TaTable tab;
    const int *matrix;
    int dp_open, gap_open, gap_extend;
    TaLayout *lay;
    unsigned long long *ctr;       // [0] ticket of the wave kernel, [1] of the long one, [2] operations cursor
    uint8_t *block;                // host-buffer form: the packed block, its capacity, the bytes the two sections may take
    uint64_t block_cap, aln_cap;
    int want_text;
    kaamer_align_pair *items;      // device-resident form: the workspace's array
    uint64_t items_cap;
    uint32_t *status;
    uint8_t *dirs, *opsbuf;        // per resident wave: direction slab, operations
    uint64_t slab_bytes, ops_bytes;
    int *bnd;                      // long form: boundary rows per wave
    uint64_t bnd_ints;
};

__global__ void ta_layout_kernel(TaParams p)
{
    TaLayout l;
    l.items = nullptr; l.ops = nullptr; l.ops_cap = 0; l.n_ent = 0; l.items_bytes = 0; l.ok = 0; l.pad = 0;
    p.ctr[0] = 0; p.ctr[1] = 0; p.ctr[2] = 0;
    if (p.block) {
        RepBlockHdr *hdr = reinterpret_cast<RepBlockHdr *>(p.block);
        RepAlnExt x;
        x.off_items = x.off_ops = x.ops_bytes = x.need_bytes = 0; x.cap_bytes = p.aln_cap;
        if (hdr->status == 0) {   // (a refused batch: nothing of it is read)
            const uint64_t n_ent = p.eoff[*p.d_nq];
            const uint64_t at = rep_align8(hdr->total_bytes), ib = sizeof(kaamer_align_pair) * n_ent;
            const uint64_t room = p.block_cap > at ? p.block_cap - at : 0;
            const uint64_t cap = room < p.aln_cap ? room : p.aln_cap;
            x.cap_bytes = cap;
            x.need_bytes = ib;
            if (ib <= cap) {
                x.off_items = at; x.off_ops = at + ib;
                l.items = reinterpret_cast<kaamer_align_pair *>(p.block + at);
                l.ops = p.block + at + ib;
                l.ops_cap = p.want_text ? cap - ib : 0;
                l.n_ent = n_ent; l.items_bytes = ib; l.ok = 1;
                hdr->total_bytes = at + ib;
            }
        }
        *rep_aln_ext(hdr) = x;
    } else if (*p.status == 0) {
        const uint64_t n_ent = p.eoff[*p.d_nq];
        if (n_ent > p.items_cap) atomicOr(p.status, (uint32_t)ST_ALN_CAP);
        else { l.items = p.items; l.n_ent = n_ent; l.items_bytes = sizeof(kaamer_align_pair) * n_ent; l.ok = 1; }
    }
    *p.lay = l;
}

// by one wave: n letters to the aligner's codes, at the same offsets; true: a letter outside the alphabet (its code is 0)
__device__ __forceinline__ bool ta_wave_codes(const uint8_t *raw, uint8_t *codes, uint32_t n, uint32_t lane)
{
    bool bad = false;
    for (uint32_t i = lane; i < n; i += 64) {
        int c = aln_code(raw[i]);
        if (c < 0) { bad = true; c = 0; }
        codes[i] = (uint8_t)c;
    }
    return __ballot(bad) != 0ull;
}

// by one wave: the first of a query's cnt reported hits for which miss(r) holds, cnt when there is none.  That id without
// an entry ends the query's HitEntries (search.go:461-463)
template <class Miss> __device__ __forceinline__ uint32_t ta_first_missing(uint32_t cnt, uint32_t lane, Miss miss)
{
    uint32_t first_missing = cnt;
    for (uint32_t r0 = 0; r0 < cnt && first_missing == cnt; r0 += 64) {
        const uint32_t r = r0 + lane;
        const unsigned long long mm = __ballot(r < cnt && miss(r));
        if (mm) first_missing = r0 + (uint32_t)__ffsll((long long)mm) - 1u;
    }
    return first_missing;
}

// The pair record of one reported hit, before any kernel aligns it.  missing: the hit lies at or behind the query's
// first_missing.  ns: the subject's stored length (TA_NS_TOO_LONG: one too long to have travelled); sbad: it holds a
// letter outside the alphabet.
#define TA_NS_TOO_LONG 0xFFFFFFFFull
__device__ __forceinline__ kaamer_align_pair ta_pair(uint32_t qlen, uint64_t qoff, bool qbad, bool missing, uint32_t entry, uint64_t ns, bool sbad)
{
    kaamer_align_pair it;
    it.n_ops = it.start_i = it.start_j = it.end_i = it.end_j = 0;
    it.identical = it.similar = it.mismatches = it.gap_openings = it.raw = 0;
    it.query_len = qlen; it.off = qoff; it.entry = TA_NONE; it.subject_len = 0;
    if (missing) it.status = 4;
    else {
        it.entry = entry;
        it.subject_len = ns > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)ns;
        if (qbad || sbad) it.status = 2;
        else if (qlen > 0x3FFFFFFFu || ns > 0x3FFFFFFFull) it.status = 3;
        else if (qlen == 0 || ns == 0) it.status = 0;                       // no cell: the empty alignment
        else it.status = ns <= ALN_WAVE_NS ? TA_WAVE : TA_LONG;
    }
    return it;
}

__global__ __launch_bounds__(256) void ta_pairs_kernel(TaParams p)
{
    if (!p.lay->ok) return;
    kaamer_align_pair *items = p.lay->items;
    const uint32_t nq = *p.d_nq;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t q = wave; q < nq; q += n_waves) {
        const uint32_t cnt = p.top_cnt[q];
        if (cnt == 0) continue;
        const kaamer_query_meta m = p.q[q];
        const uint32_t tr = (uint32_t)p.trim[q];
        const uint32_t qlen = m.aa_len - tr;            // Query.Sequence as the handler holds it: the trimmed ORF
        const uint64_t qoff = m.aa_off + tr;
        const bool qbad = ta_wave_codes(p.qraw + qoff, p.qcodes + qoff, qlen, lane);
        const uint32_t first_missing = ta_first_missing(cnt, lane, [&](uint32_t r) {
            const uint32_t pid = p.top_pid[q * p.K + r];
            return pid >= p.tab.idmap_n || p.tab.idmap[pid] == TA_NONE;
        });
        const uint64_t e0 = p.eoff[q];
        for (uint32_t r = lane; r < cnt; r += 64) {
            const bool missing = r >= first_missing;
            uint32_t ent = TA_NONE;
            uint64_t ns = 0;
            bool sbad = false;
            if (!missing) {
                ent = p.tab.idmap[p.top_pid[q * p.K + r]];
                ns = p.tab.off[ent + 1] - p.tab.off[ent];
                sbad = !qbad && p.tab.bad[ent];   // (read as the rules read it: only where it decides)
            }
            items[e0 + r] = ta_pair(qlen, qoff, qbad, missing, ent, ns, sbad);
        }
    }
}

template <bool LONG>
__global__ __launch_bounds__(64) void ta_wave_kernel(TaParams p)
{
    __shared__ AlnWaveLds L;
    __shared__ unsigned long long s_u64;
    __shared__ uint32_t s_n;
    if (!p.lay->ok) return;
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < ALN_NL * ALN_NL; i += 64) L.m[i] = p.matrix[i];
    __syncthreads();
    kaamer_align_pair *items = p.lay->items;
    const uint64_t n_ent = p.lay->n_ent, ops_cap = p.lay->ops_cap;
    uint8_t *const out_ops = p.lay->ops;
    uint8_t *const dirs = p.dirs + (uint64_t)blockIdx.x * p.slab_bytes;
    uint8_t *const ops = p.opsbuf + (uint64_t)blockIdx.x * p.ops_bytes;
    int *const bnd = LONG ? p.bnd + (uint64_t)blockIdx.x * p.bnd_ints : nullptr;
    for (;;) {
        if (lane == 0) s_u64 = atomicAdd(&p.ctr[LONG ? 1 : 0], LONG ? 64ull : 1ull);
        __syncthreads();
        const uint64_t t = s_u64;
        __syncthreads();
        if (t >= n_ent) break;
        // the pairs of this ticket that are this kernel's (one for the wave form; of 64 for the long form, nearly always none)
        const uint64_t mine_e = LONG ? t + lane : t;
        const bool want = mine_e < n_ent && items[mine_e].status == (LONG ? TA_LONG : TA_WAVE);
        unsigned long long todo = __ballot(want);
        if (!LONG) todo &= 1ull;
        while (todo) {
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint64_t e = t + (uint64_t)b;
            const uint32_t nq = items[e].query_len, ns = items[e].subject_len;
            const uint64_t qoff = items[e].off, soff = p.tab.off[items[e].entry];
            const uint64_t need = (uint64_t)((nq + 63u) / 64u) * ((uint64_t)ns + 63u) * 64u;
            if (need > p.slab_bytes || (uint64_t)nq + ns > p.ops_bytes || (LONG && 3ull * ((uint64_t)ns + 1) > p.bnd_ints)) {
                if (lane == 0) items[e].status = 3;   // beyond the slab the host sized: never written out of bounds
                continue;
            }
            PairOut o;
            AlnTally ty;
            align_wave_pair<LONG, true>(L, p.qcodes + qoff, nq, p.tab.codes + soff, ns, p.dp_open, dirs, ops, bnd, p.qraw + qoff,
                                        p.tab.raw + soff, p.gap_open, p.gap_extend, o, ty);
            if (lane == 0) {
                unsigned long long at = 0;
                if (ops_cap) at = atomicAdd(&p.ctr[2], (unsigned long long)o.n_ops);
                kaamer_align_pair it = items[e];
                it.status = 0; it.n_ops = o.n_ops; it.start_i = o.start_i; it.start_j = o.start_j; it.end_i = o.end_i; it.end_j = o.end_j;
                it.identical = ty.identical; it.similar = ty.similar; it.mismatches = ty.mismatches; it.gap_openings = ty.gap_openings;
                it.raw = ty.raw; it.off = at;
                items[e] = it;
                s_u64 = at; s_n = (uint32_t)o.n_ops;
            }
            __threadfence_block();
            __syncthreads();
            if (ops_cap) {
                const uint64_t at = s_u64, n = s_n;
                if (at + n <= ops_cap)
                    for (uint64_t i = lane; i < n; i += 64) out_ops[at + i] = ops[i];
            }
            __syncthreads();
        }
    }
}

__global__ void ta_finish_kernel(TaParams p)
{
    if (!p.block || !p.lay->ok) return;
    RepBlockHdr *hdr = reinterpret_cast<RepBlockHdr *>(p.block);
    RepAlnExt *x = rep_aln_ext(hdr);
    const uint64_t used = p.ctr[2];
    x->need_bytes = p.lay->items_bytes + used;
    if (used <= p.lay->ops_cap) {
        x->ops_bytes = used;
        hdr->total_bytes = rep_align8(x->off_ops + used);
    }
}
