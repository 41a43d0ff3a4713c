// topn.hip.inc — the post-steps of a query on the device (included by search.hip):
//   sortMapByValue     (search.go:132-152)  Kmatch descending; ties, unordered in the reference,
//                                           by ascending protein id
//   SetBestStartCodon  (dna.go:198-272)     reads / nucleotide only, before the filter
//                                           (search_fastq.go:119-123, search_nucleotide.go:116-120)
//   FilterResults      (search.go:189-220)  MinKRatio / MinKMatch prefix, at most MaxResults
// A group of lanes per query.  A hit is the 64-bit key (Kmatch << 32 | ~protein id): the largest key is
// the first hit of the reference's order, and since ids are unique "the next hit" is the largest
// key below the previous one -- no removal bookkeeping.  Up to 512 hits of a query stay in
// registers (8 per lane); longer lists are re-scanned from HBM (L2) every round.
#define TOPN_R 8

struct TopnParams {
    const uint32_t *d_nq;
    const kaamer_query_meta *q;
    const uint32_t *src_nq;  // queries q[] holds (the orf_source's last search)
    uint32_t q_first, q_stride;  // result i belongs to query q_first + i * q_stride of q[] (merged results: the owner's queries)
    const int32_t *size_in;  // SizeInKmer per query instead of q[] (merged results of a sharded index)
    const uint64_t *hit_off;
    const uint32_t *hit_cnt;
    const uint32_t *pid, *km, *fp;
    const uint8_t *orf_aa;
    const int32_t *starts_alt;
    double min_k_ratio;
    long long min_k_match;
    uint32_t K;
    int best_start;  // apply SetBestStartCodon and its gate (hits[0].Kmatch >= MinKMatch)
    uint32_t *top_cnt, *top_pid, *top_km, *top_fp;
    int32_t *trim, *start_pos, *size_out;
};

// maximum over the G lanes of a query's group (xor shuffles below G stay inside the group)
template <int G> __device__ __forceinline__ unsigned long long group_max_u64(unsigned long long v)
{
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// G lanes per query: 64 for protein batches (a query has ~190 hits), 16 for ORF batches (4.2 M ORFs of ~15 hits per
// 1 M reads: a whole wave per ORF took 2.8 ms).  Up to G * TOPN_R hits of a query stay in registers; longer lists are
// re-scanned from HBM (L2) every round.  The groups of a wave run their own loops: every cross-lane step below reads
// lanes of the own group only.
template <int G>
__global__ __launch_bounds__(256) void topn_kernel(TopnParams p)
{
    const uint32_t nq = *p.d_nq;
    const uint32_t lane = threadIdx.x & 63u, gl = lane & (uint32_t)(G - 1), gbase = lane - gl;
    const unsigned long long gmask = G == 64 ? ~0ull : (((1ull << (G & 63)) - 1ull) << gbase);
    const uint64_t grp = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const uint64_t n_grp = ((uint64_t)gridDim.x * blockDim.x) / G;
    for (uint64_t qi = grp; qi < nq; qi += n_grp) {
        kaamer_query_meta m;
        if (p.size_in) { m.size_in_kmer = p.size_in[qi]; m.start_position = 0; m.plus_strand = 1; m.aa_len = 0; m.aa_off = 0; m.sa_off = 0; m.sa_len = 0; }
        else {
            const uint64_t qsrc = (uint64_t)p.q_first + qi * p.q_stride;
            if (qsrc >= *p.src_nq) {  // results that belong to no query of the source (inconsistent exchange headers): nothing reported
                if (gl == 0) { p.top_cnt[qi] = 0; p.trim[qi] = 0; p.start_pos[qi] = 0; p.size_out[qi] = 0; }
                continue;
            }
            m = p.q[qsrc];
        }
        const uint32_t n = p.hit_cnt[qi];
        const uint64_t base = p.hit_off[qi];
        int32_t size = m.size_in_kmer, start_pos = m.start_position, trimmed = 0;
        uint32_t kept = 0;
        const bool cached = n <= (uint32_t)G * TOPN_R;
        unsigned long long key[TOPN_R];
#pragma unroll
        for (int r = 0; r < TOPN_R; r++) {
            const uint32_t i = (uint32_t)r * G + gl;
            key[r] = 0ull;
            if (cached && i < n) key[r] = ((unsigned long long)p.km[base + i] << 32) | (unsigned long long)(0xFFFFFFFFu - p.pid[base + i]);
        }
        // largest key below `prev` and the index of its hit (in the lane that holds it)
        auto next_below = [&](unsigned long long prev, uint32_t &idx) {
            unsigned long long best = 0ull;
            idx = 0;
            if (cached) {
#pragma unroll
                for (int r = 0; r < TOPN_R; r++)
                    if (key[r] < prev && key[r] > best) { best = key[r]; idx = (uint32_t)r * G + gl; }
            } else {
                for (uint32_t i = gl; i < n; i += G) {
                    const unsigned long long k = ((unsigned long long)p.km[base + i] << 32) | (unsigned long long)(0xFFFFFFFFu - p.pid[base + i]);
                    if (k < prev && k > best) { best = k; idx = i; }
                }
            }
            return best;
        };
        uint32_t idx = 0;
        unsigned long long mine = n ? next_below(~0ull, idx) : 0ull;
        unsigned long long win = group_max_u64<G>(mine);
        bool report = win != 0ull;
        if (report && p.best_start) {
            const long long kmax = (long long)(win >> 32);
            if (kmax < p.min_k_match) report = false;  // search_fastq.go:120
            else if (m.sa_len >= 1) {                   // dna.go:210-212
                // first matching position of the first best hit; a later best hit only counts if
                // it matches at position 0 (dna.go:224-237: `exit` is never reset)
                const unsigned long long own = __ballot(mine == win) & gmask;
                const uint32_t owner = (uint32_t)__ffsll((long long)own) - 1u;  // a lane of this group
                const uint32_t fp_mine = mine == win ? p.fp[base + idx] : 0u;
                long long first_best = (long long)__shfl(fp_mine, (int)owner, 64);
                bool zero = false;
                if (cached) {
#pragma unroll
                    for (int r = 0; r < TOPN_R; r++) {
                        const uint32_t i = (uint32_t)r * G + gl;
                        if (key[r] != win && (long long)(key[r] >> 32) == kmax && key[r] != 0ull && p.fp[base + i] == 0u) zero = true;
                    }
                } else {
                    for (uint32_t i = gl; i < n; i += G)
                        if ((long long)p.km[base + i] == kmax && (0xFFFFFFFFu - p.pid[base + i]) != (uint32_t)win && p.fp[base + i] == 0u) zero = true;
                }
                if (__ballot(zero) & gmask) first_best = 0;
                // the last alternative start at or before it (dna.go:240-249), the group's first lane walks the list
                int32_t best = 0, first = 0;
                if (gl == 0) {
                    const int32_t *sa = p.starts_alt + m.sa_off;
                    first = best = sa[0];
                    for (uint32_t s = 0; s < m.sa_len; s++) {
                        if ((long long)sa[s] <= first_best) best = sa[s];
                        else break;
                    }
                }
                best = __shfl(best, (int)gbase, 64);
                first = __shfl(first, (int)gbase, 64);
                if (best != first) {                    // dna.go:252-267
                    trimmed = best;
                    start_pos = m.plus_strand ? start_pos + 3 * best : start_pos - 3 * best;
                    const long long new_len = (long long)m.aa_len - best;
                    size = (int32_t)(new_len - KAAMER_KMER_SIZE + 1);
                    if (new_len > 0 && p.orf_aa[m.aa_off + m.aa_len - 1] == '*') size--;
                }
            }
        }
        // FilterResults: the passing hits are a prefix of the sorted order
        while (report && win != 0ull && kept < p.K) {
            const long long km = (long long)(win >> 32);
            if (((double)km / (double)size) < p.min_k_ratio || km < p.min_k_match) break;
            if (mine == win) {
                const uint64_t o = qi * p.K + kept;
                p.top_pid[o] = 0xFFFFFFFFu - (uint32_t)win;
                p.top_km[o] = (uint32_t)km;
                p.top_fp[o] = p.fp ? p.fp[base + idx] : 0u;
            }
            kept++;
            mine = next_below(win, idx);
            win = group_max_u64<G>(mine);
        }
        if (gl == 0) {
            p.top_cnt[qi] = kept;
            p.trim[qi] = trimmed;
            p.start_pos[qi] = start_pos;
            p.size_out[qi] = size;
        }
    }
}

// ---- only what is reported leaves the device (kaamer_search_batch_top / kaamer_submit_batch_top): the queries
// FilterResults left with at least one hit, their hits as CSR, their (trimmed) ORF residues, packed in query order
// into ONE block, so that a call costs one device-to-host copy (the block starts with its own size: the host copies a
// guess, reads the header, and fetches the rest only when the guess was short):
//   RepBlockHdr (256 B) | rep_query u32[n_rep] | trim i32[n_rep] | q kaamer_query_meta[n_rep] | top_off u64[n_rep + 1]
//   | pid u32[n_ent] | kmatch u32[n_ent] | first_pos u32[n_ent] | orf_aa u8[n_aa]        (every section 8-byte aligned)
struct RepBlockHdr {
    uint64_t total_bytes;
    uint32_t n_queries, n_rep;
    uint64_t n_ent, n_aa;
    uint32_t status;      // the batch's device status word (0 = fine); bit 31: the block's capacity was exceeded
    uint32_t pad;
    uint64_t off_rep_query, off_trim, off_q, off_top_off, off_pid, off_km, off_fp, off_aa;  // byte offsets of the sections
    kaamer_counters counters;
    uint8_t reserved[256 - 40 - 64 - sizeof(kaamer_counters)];
};
static_assert(sizeof(RepBlockHdr) == 256, "block header is 256 bytes");

// what the bitmaps of the reported hits add to the header, in its reserved bytes (top_positions.hip.inc; zero in a block
// without bitmaps)
struct RepPosExt {
    uint64_t off_pos_len, off_pos_off, off_pos_bits;   // byte offsets of the three sections
    uint64_t n_pos_words;
};
// ... and their alignments, behind RepPosExt (top_align.hip.inc; zero in a block without alignments)
struct RepAlnExt {
    uint64_t off_items, off_ops;   // byte offsets of the two sections
    uint64_t ops_bytes;            // operations stored
    uint64_t need_bytes, cap_bytes;   // both sections: what the batch needed, what this call ran with
};
static_assert(sizeof(RepPosExt) + sizeof(RepAlnExt) <= sizeof(((RepBlockHdr *)nullptr)->reserved), "the header's reserved bytes hold both extensions");
static_assert(offsetof(RepBlockHdr, reserved) % 8 == 0, "aligned");
__host__ __device__ __forceinline__ RepPosExt *rep_pos_ext(RepBlockHdr *h) { return reinterpret_cast<RepPosExt *>(h->reserved); }
__host__ __device__ __forceinline__ const RepPosExt *rep_pos_ext(const RepBlockHdr *h) { return reinterpret_cast<const RepPosExt *>(h->reserved); }
__host__ __device__ __forceinline__ RepAlnExt *rep_aln_ext(RepBlockHdr *h) { return reinterpret_cast<RepAlnExt *>(h->reserved + sizeof(RepPosExt)); }
__host__ __device__ __forceinline__ const RepAlnExt *rep_aln_ext(const RepBlockHdr *h) { return reinterpret_cast<const RepAlnExt *>(h->reserved + sizeof(RepPosExt)); }

__host__ __device__ __forceinline__ uint64_t rep_align8(uint64_t x) { return (x + 7ull) & ~7ull; }

// the section offsets and the size of a block, from its three totals
__host__ __device__ __forceinline__ void rep_block_layout(RepBlockHdr &h, uint64_t n_rep, uint64_t n_ent, uint64_t n_aa)
{
    h.off_rep_query = sizeof(RepBlockHdr);
    h.off_trim = rep_align8(h.off_rep_query + 4 * n_rep);
    h.off_q = rep_align8(h.off_trim + 4 * n_rep);
    h.off_top_off = rep_align8(h.off_q + sizeof(kaamer_query_meta) * n_rep);
    h.off_pid = h.off_top_off + 8 * (n_rep + 1);
    h.off_km = rep_align8(h.off_pid + 4 * n_ent);
    h.off_fp = rep_align8(h.off_km + 4 * n_ent);
    h.off_aa = rep_align8(h.off_fp + 4 * n_ent);
    h.total_bytes = rep_align8(h.off_aa + n_aa);
}

struct RepParams {
    const uint32_t *d_nq;
    const kaamer_query_meta *q;     // the queries the results belong to: result i is query q_first + i * q_stride
    uint32_t q_first, q_stride;
    const uint32_t *top_cnt;
    const int32_t *trim, *start_pos, *size_out;
    uint32_t K;
    const uint32_t *top_pid, *top_km, *top_fp;
    const uint8_t *orf_aa;  // NULL for protein input
    uint32_t *flag, *aalen;                 // per query, scanned by the caller
    const uint64_t *rank, *eoff, *aoff;     // exclusive scans of flag, top_cnt, aalen (n + 1 entries each)
    uint8_t *block;                         // the result block
    uint64_t block_cap;
    const kaamer_counters *ctr;             // written by the batch's finalize step, earlier on the stream
    const uint32_t *status_out;
};

__global__ void rep_flags_kernel(RepParams p)
{
    const uint32_t nq = *p.d_nq;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * blockDim.x) {
        const bool f = p.top_cnt[q] > 0;
        p.flag[q] = f ? 1u : 0u;
        p.aalen[q] = (f && p.orf_aa) ? p.q[(uint64_t)p.q_first + q * p.q_stride].aa_len - (uint32_t)p.trim[q] : 0u;
    }
}

__global__ __launch_bounds__(256) void rep_block_kernel(RepParams p)
{
    const uint32_t nq = *p.d_nq;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    // section offsets from the three totals (every thread computes the same)
    const uint64_t n_rep = p.rank[nq], n_ent = p.eoff[nq], n_aa = p.aoff[nq];
    RepBlockHdr h;
    rep_block_layout(h, n_rep, n_ent, n_aa);
    const bool fits = h.total_bytes <= p.block_cap;
    if (wave == 0 && lane == 0) {
        RepBlockHdr *out = reinterpret_cast<RepBlockHdr *>(p.block);
        h.n_queries = nq; h.n_rep = (uint32_t)n_rep; h.n_ent = n_ent; h.n_aa = n_aa;
        h.status = *p.status_out | (fits ? 0u : 0x80000000u);
        h.pad = 0;
        h.counters = *p.ctr;
        if (!fits) h.total_bytes = sizeof(RepBlockHdr);
        for (uint32_t i = 0; i < sizeof h.reserved; i++) h.reserved[i] = 0;
        *out = h;
    }
    if (!fits) return;
    uint32_t *rep_query = reinterpret_cast<uint32_t *>(p.block + h.off_rep_query);
    int32_t *rep_trim = reinterpret_cast<int32_t *>(p.block + h.off_trim);
    kaamer_query_meta *rep_q = reinterpret_cast<kaamer_query_meta *>(p.block + h.off_q);
    uint64_t *rep_off = reinterpret_cast<uint64_t *>(p.block + h.off_top_off);
    uint32_t *rep_pid = reinterpret_cast<uint32_t *>(p.block + h.off_pid);
    uint32_t *rep_km = reinterpret_cast<uint32_t *>(p.block + h.off_km);
    uint32_t *rep_fp = reinterpret_cast<uint32_t *>(p.block + h.off_fp);
    uint8_t *rep_aa = p.block + h.off_aa;
    if (wave == 0 && lane == 0) rep_off[n_rep] = n_ent;  // CSR end
    for (uint64_t q = wave; q < nq; q += n_waves) {
        const uint32_t cnt = p.top_cnt[q];
        if (cnt == 0) continue;
        const uint64_t r = p.rank[q], e = p.eoff[q];
        kaamer_query_meta m = p.q[(uint64_t)p.q_first + q * p.q_stride];
        const uint32_t tr = (uint32_t)p.trim[q];
        const uint64_t src_aa = m.aa_off + tr;
        const uint32_t n_aa_q = p.orf_aa ? m.aa_len - tr : 0u;
        if (lane == 0) {
            m.start_position = p.start_pos[q];      // the query as the reference reports it after
            m.size_in_kmer = p.size_out[q];         // SetBestStartCodon (dna.go:252-270)
            m.aa_len -= tr;
            m.aa_off = p.orf_aa ? p.aoff[q] : src_aa;   // protein input: still into the caller's buffer
            m.sa_off = 0; m.sa_len = 0;             // StartsAlternative is emptied (dna.go:270)
            rep_query[r] = (uint32_t)q;
            rep_q[r] = m;
            rep_trim[r] = (int32_t)tr;
            rep_off[r] = e;
        }
        for (uint32_t i = lane; i < cnt; i += 64) {  // cnt <= K; K may exceed 64
            rep_pid[e + i] = p.top_pid[q * p.K + i];
            rep_km[e + i] = p.top_km[q * p.K + i];
            rep_fp[e + i] = p.top_fp[q * p.K + i];
        }
        const uint64_t dst_aa = p.aoff[q];
        for (uint32_t i = lane; i < n_aa_q; i += 64) rep_aa[dst_aa + i] = p.orf_aa[src_aa + i];
    }
}
