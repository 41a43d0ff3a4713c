// tsv_aln_rows.hip.inc — the -aln TSV rows of the reported hits, written on the device (included by search.hip after
// tsv_rows.hip.inc: the row form TsvAln for that file's passes, over its sinks, row head and row tail; the host side is in
// host_tsv.hip.inc, the contract and the host formatter in tsv_format.cpp, the two number formats in fmt_double.h).
//
// QueryResultHandler aligns every reported hit, sorts a query's hits by BitScore and prints a row per hit
// (search.go:483-494, :556-604).  Behind kaamer_topn_align_device the pair records are resident; the rest is what the plain
// rows need.
//
//   tsv_aln_order_kernel   a lane per query: the order of its hits by BitScore descending, stable (insertion: a query has
//                          at most max_results hits), kept as order[q * K + row] = hit; counts the pairs whose raw score lies
//                          outside the table (the batch is then the host formatter's: nothing of the rows is to be read)
//   tsv_len_kernel<TsvAln>, out_scan_kernel, tsv_off_kernel<TsvAln>, tsv_write_kernel<TsvAln>
//                          the four passes of the rows (tsv_rows.hip.inc) over this form
//
// Floats.  Identity is float32(identical) / float32(columns) * 100, each step IEEE-rounded.  BitScore is a function of the
// raw score alone and EValue = len(query) * NumberOfAA / 2^BitScore: the device's pow is not the host's, so BitScore and
// 2^BitScore come from a table per raw score that the host fills with kaamer_align_finish's own arithmetic for the call's
// (lambda, K); the product and the quotient are IEEE-rounded here as they are there.
// Numbers.  "%.2f" of Identity and BitScore is 64-bit integer arithmetic (the table holds no BitScore of 2^63 or more);
// "%e" of EValue is exact for every double (fmt_double.h), its limbs in LDS, limb-major: lane t's limb i is word
// i * OUT_TILE + t, consecutive lanes in consecutive banks.
#include "fmt_double.h"

// The raw score is the reference's own tally with the request's gap penalties over an alignment made with the aligner's
// fixed ones: long gaps make it negative (a few pairs in a thousand on reads).  The table holds both signs.
#define TSV_ALN_RAW_N (1u << 17)    /* raw scores the table holds: [TSV_ALN_RAW_MIN, TSV_ALN_RAW_MIN + TSV_ALN_RAW_N) */
#define TSV_ALN_RAW_MIN (-65536)

struct TsvAlnParams : TsvParams {    // top_km and size_out are not read
    const uint64_t *pair_off;      // kaamer_topn_alignments
    const kaamer_align_pair *pairs;
    uint64_t pair_cap;
    // the host-buffer calls: the pair records are the section the alignment stage laid out in the packed block (lay->items,
    // lay->n_ent; nothing of them when it did not fit: the call repeats the batch).  unaligned: options without a row in
    // AllMatrixScores -- no stage ran, every hit keeps the empty AlignmentResult with status 1, in sortMapByValue order
    const TaLayout *lay;
    int unaligned;
    uint16_t *order;               // [nq_cap * K]
    const double *tab_bits, *tab_pow;   // per raw score, at raw - TSV_ALN_RAW_MIN: BitScore, 2^BitScore
    uint32_t tab_n;
    int protein;                   // the base sequence type: fields 7 and 8 are the alignment's
    double number_of_aa;
};

// a lane's limbs in LDS
struct TsvLimbs {
    uint32_t *base;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return base[i * OUT_TILE]; }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) { base[i * OUT_TILE] = v; }
};

// Every thread computes the same: where the pair records are.
__device__ __forceinline__ void tsv_aln_setup(TsvAlnParams &p)
{
    if (!p.lay) return;
    const bool ok = p.lay->ok != 0;
    p.pairs = ok ? p.lay->items : nullptr;
    p.pair_cap = ok ? p.lay->n_ent : 0ull;
}

// hit h of query q
__device__ __forceinline__ kaamer_align_pair tsv_aln_pair(const TsvAlnParams &p, uint64_t q, uint32_t h)
{
    if (p.unaligned) {
        kaamer_align_pair it;
        memset(&it, 0, sizeof it);
        it.status = 1;
        return it;
    }
    return p.pairs[p.pair_off[q] + h];
}

// where the table holds a raw score; tab_n: outside it
__device__ __forceinline__ uint32_t tsv_aln_slot(const TsvAlnParams &p, int32_t raw)
{
    const int64_t at = (int64_t)raw - TSV_ALN_RAW_MIN;
    return at >= 0 && at < (int64_t)p.tab_n ? (uint32_t)at : p.tab_n;
}

__device__ __forceinline__ bool tsv_aln_in_table(const TsvAlnParams &p, const kaamer_align_pair &it)
{
    return it.status != 0 || tsv_aln_slot(p, it.raw) < p.tab_n;
}

// the BitScore a hit is sorted by: the empty AlignmentResult's is 0
__device__ __forceinline__ double tsv_aln_bits(const TsvAlnParams &p, uint64_t q, uint32_t h)
{
    if (p.unaligned) return 0.0;
    const kaamer_align_pair *it = p.pairs + p.pair_off[q] + h;
    const uint32_t at = tsv_aln_slot(p, it->raw);
    return it->status == 0 && at < p.tab_n ? p.tab_bits[at] : 0.0;
}

// the hits of query q, or 0 when its pair records lie beyond what the alignment stage provisioned (that stage has flagged
// the batch then)
__device__ __forceinline__ uint32_t tsv_aln_cnt(const TsvAlnParams &p, uint64_t q, uint32_t nq)
{
    if (q >= nq) return 0u;
    uint32_t cnt = p.top_cnt[q];
    if (cnt > p.K) cnt = p.K;
    return p.unaligned || p.pair_off[q] + cnt <= p.pair_cap ? cnt : 0u;
}

__global__ __launch_bounds__(OUT_TILE) void tsv_aln_order_kernel(TsvAlnParams p)
{
    tsv_aln_setup(p);
    const uint32_t nq = out_nq(p);
    const uint64_t q = (uint64_t)blockIdx.x * OUT_TILE + threadIdx.x;
    const uint32_t cnt = tsv_aln_cnt(p, q, nq);
    if (!cnt) return;
    uint16_t *order = p.order + q * p.K;
    uint32_t outside = 0;
    for (uint32_t r = 0; r < cnt; r++) {
        outside += tsv_aln_in_table(p, tsv_aln_pair(p, q, r)) ? 0u : 1u;
        const double b = tsv_aln_bits(p, q, r);
        uint32_t j = r;
        for (; j > 0; j--) {   // sort.Slice's less is `>`: a hit passes only hits with a strictly smaller BitScore
            const uint16_t before = order[j - 1];
            if (!(tsv_aln_bits(p, q, before) < b)) break;
            order[j] = before;
        }
        order[j] = (uint16_t)r;
    }
    if (outside) atomicAdd(&p.counts[OUT_C_RAW], (unsigned long long)outside);
}

// a row of query q: hit h = order[row] of its reported hits; ent: the hit's entry or OUT_NONE (tsv_aln_entry)
template <class Sink> __device__ __forceinline__ void tsv_aln_row(const TsvAlnParams &p, Sink &o, uint32_t q, uint32_t h, uint32_t ent, TsvLimbs &X)
{
    const kaamer_query_meta m = p.q[q];
    const TsvEntry e = tsv_row_head(p, o, m, ent);
    const kaamer_align_pair it = tsv_aln_pair(p, q, h);
    const bool ok = it.status == 0;                 // else the empty AlignmentResult: zeros
    const bool cols = ok && it.n_ops != 0;
    const float identity = ok ? __fmul_rn(__fdiv_rn((float)it.identical, (float)it.n_ops), 100.0f) : 0.0f;   // align.go:101 (NaN without columns)
    (void)kfmt_fixed2_small(o, (double)identity);
    o.put('\t');
    tsv_put_i32(o, ok ? it.n_ops : 0);
    o.put('\t');
    tsv_put_i32(o, ok ? it.mismatches : 0);
    o.put('\t');
    tsv_put_i32(o, ok ? it.gap_openings : 0);
    o.put('\t');
    tsv_put_i32(o, p.protein ? (cols ? it.start_i + 1 : (ok ? 1 : 0)) : p.start_pos[q]);   // align.go:153-156
    o.put('\t');
    tsv_put_i32(o, p.protein ? (cols ? it.end_i : 0) : m.end_position);
    o.put('\t');
    tsv_put_i32(o, cols ? it.start_j + 1 : (ok ? 1 : 0));
    o.put('\t');
    tsv_put_i32(o, cols ? it.end_j : 0);
    o.put('\t');
    const uint32_t at = tsv_aln_slot(p, it.raw);
    const bool tab = ok && at < p.tab_n;   // (outside the table: the batch is flagged, the bytes are not read)
    const double bits = tab ? p.tab_bits[at] : 0.0;
    const double evalue = tab ? __ddiv_rn(__dmul_rn((double)it.query_len, p.number_of_aa), p.tab_pow[at]) : 0.0;   // align.go:142
    kfmt_exp6(o, evalue, X);
    o.put('\t');
    (void)kfmt_fixed2_small(o, bits);
    tsv_row_tail<(uint32_t)KAAMER_KMER_SIZE - 1u>(p, o, q, h, ent, e);   // FormatPositionsToString(bitmap, true)
}

// The entry of hit h of query q.  FetchHitsInformation stops at a missing id BEFORE the sort (search.go:461-463): the hits
// from there on in sortMapByValue order carry status 4, wherever the sort puts them (a negative BitScore goes behind
// them and keeps its entry).  gone: a row before this one had no entry -- it decides for the hits of an unaligned batch
// (status 1: the text calls with options that have no row in AllMatrixScores), which are still in that order.
__device__ __forceinline__ uint32_t tsv_aln_entry(const TsvAlnParams &p, uint64_t q, uint32_t h, bool gone)
{
    const int32_t status = p.unaligned ? 1 : p.pairs[p.pair_off[q] + h].status;
    if (status == 4 || (gone && status == 1)) return OUT_NONE;
    return out_entry(p, p.top_pid[q * p.K + h]);
}

// the -aln rows as a form of the passes in tsv_rows.hip.inc: the hits in BitScore order, the write passes return on a raw
// score outside the table too
struct TsvAln {
    using Params = TsvAlnParams;
    struct Lds { uint32_t limbs[KFMT_LIMBS * OUT_TILE]; };
    using Lane = TsvLimbs;
    static __device__ __forceinline__ void setup(Params &p) { tsv_aln_setup(p); }
    static __device__ __forceinline__ Lane lane(Lds &lds) { return Lane{ lds.limbs + threadIdx.x }; }
    static __device__ __forceinline__ uint32_t count(const Params &p, uint64_t q, uint32_t nq) { return tsv_aln_cnt(p, q, nq); }
    static __device__ __forceinline__ uint32_t hit(const Params &p, uint64_t q, uint32_t r) { return p.order[q * p.K + r]; }
    static __device__ __forceinline__ uint32_t entry(const Params &p, uint64_t q, uint32_t h, bool &gone)
    {
        const uint32_t ent = tsv_aln_entry(p, q, h, gone);
        gone = gone || ent == OUT_NONE;
        return ent;
    }
    static __device__ __forceinline__ bool refused(const Params &p) { return p.counts[OUT_C_STATUS] || p.counts[OUT_C_RAW]; }
    template <class Sink> static __device__ __forceinline__ void row(const Params &p, Sink &o, uint32_t q, uint32_t h, uint32_t ent, Lane &X)
    {
        tsv_aln_row(p, o, q, h, ent, X);
    }
};

// kaamer_tsv_format_doubles_device: a lane per value, its text into a 32-byte slot (NUL-padded; a longer text is cut at 31
// bytes) through the device functions the rows use
struct TsvSlot {
    char *p;
    uint32_t n;
    __device__ __forceinline__ void put(char c) { if (n < 31u) p[n] = c; n++; }
};

__global__ __launch_bounds__(OUT_TILE) void tsv_format_doubles_kernel(const double *values, uint64_t n, int mode, char *out)
{
    __shared__ uint32_t limbs[KFMT_LIMBS * OUT_TILE];
    const uint64_t i = (uint64_t)blockIdx.x * OUT_TILE + threadIdx.x;
    if (i >= n) return;
    TsvLimbs X = { limbs + threadIdx.x };
    TsvSlot o = { out + i * 32ull, 0u };
    if (mode == 0) kfmt_exp6(o, values[i], X);
    else kfmt_fixed2(o, values[i], X);
    for (uint32_t k = o.n; k < 32u; k++) o.p[k] = '\0';
    if (o.n >= 32u) o.p[31] = '\0';
}
