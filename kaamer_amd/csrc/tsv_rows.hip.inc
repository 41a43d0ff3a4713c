// tsv_rows.hip.inc — the TSV response rows of the reported hits, written on the device (included by search.hip after
// out_rows.hip.inc, whose tiles, scans, scan kernel and window store it uses; the -aln rows are tsv_aln_rows.hip.inc, the host
// side is host_tsv.hip.inc, the contract and the host formatter are in tsv_format.cpp).
//
// QueryResultHandler builds a row with `output += ...` per field (search.go:505-554).  Behind kaamer_topn_device all a row
// needs is resident: the text with the records' name spans, the reported hits, SizeInKmer / StartPosition after
// SetBestStartCodon, the bitmaps of the reported hits and the subject text (kaamer_index_attach_subject_text).
//
// The passes are written once, over a row FORM (TsvPlain here, TsvAln in tsv_aln_rows.hip.inc); every instantiation is a
// kernel of its own:
//   tsv_len_kernel     a lane per query: the bytes of its rows (the form's row into a counting sink: digits, field lengths,
//                      the runs of the bitmap words), summed per tile of OUT_TILE queries
//   out_scan_kernel    (out_rows.hip.inc)
//   tsv_off_kernel     a workgroup per tile, a lane per query: the first byte of every row (unit_off, in CSR order), from the
//                      tiles' prefixes, a scan inside the tile and the rows' lengths once more (nothing per row is kept
//                      between the passes: a batch has up to max_results rows per query, nearly all of them absent)
//   tsv_write_kernel   a workgroup per tile, a lane per query.  The rows of a tile are one contiguous byte range of the
//                      output.  Rows are short, many and uneven, and names, ids and annotation values are byte copies at
//                      arbitrary alignment, so no lane writes a row to memory itself: the workgroup builds the range in LDS,
//                      TSV_WINDOW bytes at a time (windows lie on multiples of TSV_WINDOW in the output), every lane putting
//                      the part of its rows that falls into the window (the row into a clipping sink), and then stores the
//                      window with 16 bytes per lane, consecutive lanes at consecutive addresses.  Only the first and the last
//                      16 bytes of a tile's range, which it may share with its neighbours, go out as single bytes.
// The same row body serves the length passes and the write pass, so they cannot disagree about a row.  (Two kernels instead
// of one behind the scan, and a kernel per form: with two row bodies in one kernel the compiler needed scratch memory for
// scalar registers; apart they need none.)
// Nothing is written beyond out_cap or unit_cap: the scan kernel sets the status word and the write kernel returns.
//
// A form supplies: Params (a TsvParams) and setup(p) (what every thread derives from it first); Lds and Lane, the form's
// per-workgroup LDS and a lane's handle on it; count(p, q, nq), the rows of a query; hit(p, q, r), the hit printed r-th;
// entry(p, q, h, gone), the hit's entry under the missing-entry rule, with `gone` carried from row to row; refused(p),
// whether the write passes return; row(p, o, q, h, ent, X), the row itself.
#define TSV_WINDOW 16384u

// the rows' own: the subject text.  Entry i is st_bytes[st_off[i], st_off[i + 1]), its first st_idlen[i] bytes the EntryId,
// the rest the annotation columns ('\t' + value each)
struct TsvParams : OutParams {
    int annotations;
    const uint8_t *st_bytes;
    const uint64_t *st_off;
    const uint32_t *st_idlen, *st_length;
    uint32_t n_features;
};

// counts the bytes of a row
struct TsvCount {
    uint64_t n = 0;
    __device__ __forceinline__ void put(char) { n++; }
    __device__ __forceinline__ void copy(const uint8_t *, uint64_t len) { n += len; }
    __device__ __forceinline__ void fill(char, uint32_t len) { n += len; }
    __device__ __forceinline__ void put_u32(uint32_t v) { n += out_digits(v); }
};

// puts the bytes of a row that fall into [lo, hi) of the output into the LDS window that starts at `w`
struct TsvWindow {
    char *lds;
    uint64_t pos, w, lo, hi;
    __device__ __forceinline__ void put(char c)
    {
        if (pos >= lo && pos < hi) lds[pos - w] = c;
        pos++;
    }
    __device__ __forceinline__ void copy(const uint8_t *src, uint64_t len)
    {
        const uint64_t a = pos > lo ? pos : lo, b = pos + len < hi ? pos + len : hi;
        uint64_t i = a;
        for (; i + 8 <= b; i += 8) {   // eight loads in flight, then the eight stores: a lane's copies are latency, not bandwidth
            uint8_t t[8];
#pragma unroll
            for (int k = 0; k < 8; k++) t[k] = src[i - pos + k];
#pragma unroll
            for (int k = 0; k < 8; k++) lds[i - w + k] = (char)t[k];
        }
        for (; i < b; i++) lds[i - w] = (char)src[i - pos];
        pos += len;
    }
    __device__ __forceinline__ void fill(char c, uint32_t len)
    {
        const uint64_t a = pos > lo ? pos : lo, b = pos + len < hi ? pos + len : hi;
        for (uint64_t i = a; i < b; i++) lds[i - w] = c;
        pos += len;
    }
    __device__ __forceinline__ void put_u32(uint32_t v)
    {
        uint32_t div = 1;
        for (uint32_t d = out_digits(v); d > 1; d--) div *= 10u;
        for (; div; div /= 10u) { put((char)('0' + v / div)); v %= div; }
    }
};

template <class Sink> __device__ __forceinline__ void tsv_put_i32(Sink &o, int32_t v)   // strconv.Itoa
{
    if (v < 0) { o.put('-'); o.put_u32(0u - (uint32_t)v); }
    else o.put_u32((uint32_t)v);
}

template <class Sink> __device__ __forceinline__ void tsv_put_u64(Sink &o, unsigned long long v)
{
    if (v <= 0xFFFFFFFFull) { o.put_u32((uint32_t)v); return; }
    unsigned long long div = 1;
    while (v / div >= 10ull) div *= 10ull;
    for (; div; div /= 10ull) { o.put((char)('0' + (uint32_t)(v / div))); v %= div; }
}

// "%.2f" of float32(kmatch) / float32(size) * float32(100) (search.go:514).  The division and the multiplication are each
// IEEE-rounded float32 (the intrinsics: no contraction, no fast division); strconv prints the float32's exact value rounded
// half-even at the second decimal.  A float32 times 100 is exact in double (24 + 7 bits): floor, fraction, parity.
template <class Sink> __device__ __forceinline__ void tsv_put_identity(Sink &o, uint32_t kmatch, int32_t size)
{
    const float x = __fmul_rn(__fdiv_rn((float)kmatch, (float)size), 100.0f);
    if (x != x) { o.put('N'); o.put('a'); o.put('N'); return; }
    if (isinf(x)) { o.put(x > 0 ? '+' : '-'); o.put('I'); o.put('n'); o.put('f'); return; }
    const double v = fabs((double)x) * 100.0;
    const double fl = floor(v), frac = v - fl;
    unsigned long long cents = (unsigned long long)fl;
    if (frac > 0.5 || (frac == 0.5 && (cents & 1ull))) cents++;
    if (x < 0.0f) o.put('-');   // (a negative SizeInKmer: never from a search)
    tsv_put_u64(o, cents / 100ull);
    const uint32_t c = (uint32_t)(cents % 100ull);
    o.put('.');
    o.put((char)('0' + c / 10u));
    o.put((char)('0' + c % 10u));
}

// a word of a bitmap of n bits, the bits from n on cleared
__device__ __forceinline__ unsigned long long tsv_word(const uint64_t *bits, uint32_t wi, uint32_t n)
{
    unsigned long long w = bits[wi];
    const uint32_t left = n - wi * 64u;
    if (left < 64u) w &= (1ull << left) - 1ull;
    return w;
}

// runs of set bits: where a run starts, bits & ~(bits << 1 | carry)
__device__ __forceinline__ uint32_t tsv_runs(const uint64_t *bits, uint32_t n)
{
    uint32_t runs = 0;
    unsigned long long carry = 0;
    for (uint32_t wi = 0, words = (n + 63u) >> 6; wi < words; wi++) {
        const unsigned long long w = tsv_word(bits, wi, n);
        runs += (uint32_t)__popcll(w & ~((w << 1) | carry));
        carry = w >> 63;
    }
    return runs;
}

// FormatPositionsToString(bitmap, false), search.go:694-742, as kaamer_format_positions prints it: "start-end" per run,
// start = first set position + 1, end = the first unset position + 1, or n for a run that reaches the end
// (ADD: what every run's end gains -- 0 here, KMER_SIZE - 1 in the -aln form, FormatPositionsToString(bitmap, true))
template <uint32_t ADD, class Sink> __device__ __forceinline__ void tsv_put_positions_add(Sink &o, const uint64_t *bits, uint32_t n)
{
    bool in_run = false, first = true;
    uint32_t start = 0;
    for (uint32_t wi = 0, words = (n + 63u) >> 6; wi < words; wi++) {
        const unsigned long long w = tsv_word(bits, wi, n);
        uint32_t cur = 0;
        while (cur < 64u) {
            const unsigned long long m = (in_run ? ~w : w) >> cur;
            if (!m) break;
            cur += (uint32_t)__builtin_ctzll(m);
            const uint32_t at = wi * 64u + cur;
            if (!in_run) { start = at; in_run = true; continue; }
            if (!first) o.put(',');
            first = false;
            o.put_u32(start + 1u);
            o.put('-');
            o.put_u32((at >= n ? n : at + 1u) + ADD);
            in_run = false;
        }
    }
    if (in_run) {
        if (!first) o.put(',');
        o.put_u32(start + 1u);
        o.put('-');
        o.put_u32(n + ADD);
    }
}

template <class Sink> __device__ __forceinline__ void tsv_put_positions(Sink &o, const uint64_t *bits, uint32_t n)
{
    tsv_put_positions_add<0u>(o, bits, n);
}

// the bytes of a name before its first 0x20
__device__ __forceinline__ uint32_t tsv_query_id_len(const uint8_t *name, uint32_t name_len)
{
    uint32_t len = 0;
    bool found = false;
    while (len < name_len && !found) {   // eight bytes at a time: one wait per eight loads, not one per byte
        const uint32_t n = name_len - len < 8u ? name_len - len : 8u;
        uint8_t t[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) t[k] = k < n ? name[len + k] : (uint8_t)' ';
        uint32_t take = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            found = found || t[k] == (uint8_t)' ';
            take += found ? 0u : 1u;
        }
        len += take;
    }
    return len;
}


// where an entry's bytes are; OUT_NONE: nowhere, every length 0
struct TsvEntry {
    uint64_t s0, s1;
    uint32_t idlen;
};

// the head of a row of either form: the query's id (strings.Split(Query.Name, " ")[0]) and the hit's EntryId, a tab behind
// each -> where the entry's bytes are, for the tail
template <class Sink> __device__ __forceinline__ TsvEntry tsv_row_head(const TsvParams &p, Sink &o, const kaamer_query_meta &m, uint32_t ent)
{
    if (m.src_seq < p.n_names) {
        const kaamer_text_span sp = p.spans[m.src_seq];
        if ((uint64_t)sp.name_off + sp.name_len <= p.names_len) {
            const uint8_t *name = p.names + sp.name_off;
            o.copy(name, tsv_query_id_len(name, sp.name_len));
        }
    }
    o.put('\t');
    TsvEntry e;
    e.s0 = ent != OUT_NONE ? p.st_off[ent] : 0; e.s1 = ent != OUT_NONE ? p.st_off[ent + 1] : 0;
    e.idlen = ent != OUT_NONE ? p.st_idlen[ent] : 0;
    o.copy(p.st_bytes + e.s0, e.idlen);
    o.put('\t');
    return e;
}

// the bitmap of hit h of query q -> its bits
__device__ __forceinline__ const uint64_t *tsv_hit_bits(const TsvParams &p, uint32_t q, uint32_t h, uint32_t *n_bits)
{
    const int32_t n = p.pos_len[q];
    *n_bits = n > 0 ? (uint32_t)n : 0u;
    return p.pos_bits + p.pos_base[q] + (uint64_t)h * ((*n_bits + 63u) >> 6);
}

// the tail of a row of either form: with positions the runs of hit h's bitmap behind a tab (ADD: tsv_put_positions_add),
// with annotations the entry's columns (a tab each for a hit without entry), the newline
template <uint32_t ADD, class Sink> __device__ __forceinline__ void tsv_row_tail(const TsvParams &p, Sink &o, uint32_t q, uint32_t h, uint32_t ent, const TsvEntry &e)
{
    if (p.positions) {
        uint32_t n_bits;
        const uint64_t *bits = tsv_hit_bits(p, q, h, &n_bits);
        o.put('\t');
        tsv_put_positions_add<ADD>(o, bits, n_bits);
    }
    if (p.annotations) {
        if (ent != OUT_NONE) o.copy(p.st_bytes + e.s0 + e.idlen, e.s1 - e.s0 - e.idlen);
        else o.fill('\t', p.n_features);
    }
    o.put('\n');
}

// the plain rows (search.go:505-554): the hits in reporting order
struct TsvPlain {
    using Params = TsvParams;
    struct Lds {};
    struct Lane {};
    static __device__ __forceinline__ void setup(Params &) {}
    static __device__ __forceinline__ Lane lane(Lds &) { return Lane(); }
    static __device__ __forceinline__ uint32_t count(const Params &p, uint64_t q, uint32_t nq)
    {
        if (q >= nq) return 0u;
        const uint32_t cnt = p.top_cnt[q];
        return cnt > p.K ? p.K : cnt;
    }
    static __device__ __forceinline__ uint32_t hit(const Params &, uint64_t, uint32_t r) { return r; }
    // OUT_NONE from the query's first missing entry on
    static __device__ __forceinline__ uint32_t entry(const Params &p, uint64_t q, uint32_t h, bool &gone)
    {
        const uint32_t ent = gone ? OUT_NONE : out_entry(p, p.top_pid[q * p.K + h]);
        gone = ent == OUT_NONE;
        return ent;
    }
    static __device__ __forceinline__ bool refused(const Params &p) { return p.counts[OUT_C_STATUS] != 0; }
    template <class Sink> static __device__ __forceinline__ void row(const Params &p, Sink &o, uint32_t q, uint32_t r, uint32_t ent, Lane &)
    {
        const kaamer_query_meta m = p.q[q];
        const TsvEntry e = tsv_row_head(p, o, m, ent);
        const uint32_t km = p.top_km[(uint64_t)q * p.K + r];
        const int32_t size = p.size_out[q];
        tsv_put_identity(o, km, size);
        o.put('\t');
        tsv_put_i32(o, size);
        o.put('\t');
        o.put_u32(km);
        o.put('\t');
        if (p.positions) {
            uint32_t n_bits;
            const uint64_t *bits = tsv_hit_bits(p, q, r, &n_bits);
            const uint32_t runs = tsv_runs(bits, n_bits);
            o.put_u32(runs ? runs - 1u : 0u);   // strings.Count(posString, ",")
        } else {
            o.put('N'); o.put('/'); o.put('A');
        }
        o.put('\t');
        tsv_put_i32(o, p.start_pos[q]);
        o.put('\t');
        tsv_put_i32(o, m.end_position);
        o.put('\t'); o.put('1'); o.put('\t');
        if (p.annotations) o.put_u32(ent != OUT_NONE ? p.st_length[ent] : 0u);
        else { o.put('N'); o.put('/'); o.put('A'); }
        tsv_row_tail<0u>(p, o, q, r, ent, e);
    }
};

template <class Form> __global__ __launch_bounds__(OUT_TILE) void tsv_len_kernel(typename Form::Params p)
{
    __shared__ unsigned long long sh[OUT_TILE];
    __shared__ typename Form::Lds lds;
    Form::setup(p);
    const uint32_t nq = out_nq(p);
    if ((uint64_t)blockIdx.x * OUT_TILE >= nq || !out_upstream(p)) return;
    const uint64_t q = (uint64_t)blockIdx.x * OUT_TILE + threadIdx.x;
    const uint32_t cnt = Form::count(p, q, nq);
    typename Form::Lane X = Form::lane(lds);
    TsvCount o;
    bool gone = false;
    for (uint32_t r = 0; r < cnt; r++) {
        const uint32_t h = Form::hit(p, q, r);
        const uint32_t ent = Form::entry(p, q, h, gone);
        Form::row(p, o, (uint32_t)q, h, ent, X);
    }
    unsigned long long bytes = 0, lines = 0;
    (void)out_block_scan(o.n, sh, &bytes);
    (void)out_block_scan(cnt, sh, &lines);
    if (threadIdx.x == 0) { p.tile_bytes[blockIdx.x] = bytes; p.tile_units[blockIdx.x] = lines; }
}

// a workgroup per tile, a lane per query: where every row starts (the tiles' prefixes, a scan of the queries' rows and bytes
// inside the tile, the rows' lengths once more)
template <class Form> __global__ __launch_bounds__(OUT_TILE) void tsv_off_kernel(typename Form::Params p)
{
    __shared__ unsigned long long sh[OUT_TILE];
    __shared__ typename Form::Lds lds;
    Form::setup(p);
    const uint32_t nq = out_nq(p);
    if ((uint64_t)blockIdx.x * OUT_TILE >= nq) return;
    if (Form::refused(p)) return;   // (uniform: written before this kernel started)
    (void)out_upstream(p);
    const uint64_t q = (uint64_t)blockIdx.x * OUT_TILE + threadIdx.x;
    const uint32_t cnt = Form::count(p, q, nq);
    typename Form::Lane X = Form::lane(lds);
    unsigned long long tile_total = 0;
    const unsigned long long e0 = p.tile_units[blockIdx.x] + out_block_scan(cnt, sh, &tile_total) - cnt;
    unsigned long long mine = 0;
    bool gone = false;
    for (uint32_t r = 0; r < cnt; r++) {
        const uint32_t h = Form::hit(p, q, r);
        const uint32_t ent = Form::entry(p, q, h, gone);
        TsvCount o;
        Form::row(p, o, (uint32_t)q, h, ent, X);
        p.unit_off[e0 + r] = mine;   // relative to the query's first byte for now
        mine += o.n;
    }
    const unsigned long long q0 = p.tile_bytes[blockIdx.x] + out_block_scan(mine, sh, &tile_total) - mine;
    for (uint32_t r = 0; r < cnt; r++) p.unit_off[e0 + r] += q0;
}

template <class Form> __global__ __launch_bounds__(OUT_TILE) void tsv_write_kernel(typename Form::Params p)
{
    __shared__ unsigned long long sh[OUT_TILE];
    __shared__ typename Form::Lds lds;
    __shared__ __attribute__((aligned(16))) char win[TSV_WINDOW];
    Form::setup(p);
    const uint32_t nq = out_nq(p);
    if ((uint64_t)blockIdx.x * OUT_TILE >= nq) return;
    if (Form::refused(p)) return;   // (uniform: written before this kernel started)
    (void)out_upstream(p);
    const uint64_t q = (uint64_t)blockIdx.x * OUT_TILE + threadIdx.x;
    const uint32_t cnt = Form::count(p, q, nq);
    typename Form::Lane X = Form::lane(lds);
    unsigned long long tile_total = 0;
    const unsigned long long e0 = p.tile_units[blockIdx.x] + out_block_scan(cnt, sh, &tile_total) - cnt;
    // the tile's rows are [b0, b1) of the output; unit_off[rows] is the total, so every row's end is the next entry
    const unsigned long long b0 = p.tile_bytes[blockIdx.x], b1 = p.unit_off[p.tile_units[blockIdx.x] + tile_total];
    const unsigned long long q0 = cnt ? p.unit_off[e0] : 0ull, q1 = cnt ? p.unit_off[e0 + cnt] : 0ull;
    for (unsigned long long w = b0 - b0 % TSV_WINDOW; w < b1; w += TSV_WINDOW) {
        const unsigned long long lo = w > b0 ? w : b0, hi = w + TSV_WINDOW < b1 ? w + TSV_WINDOW : b1;
        if (q0 < hi && q1 > lo) {
            bool gone = false;
            for (uint32_t r = 0; r < cnt; r++) {
                const uint32_t h = Form::hit(p, q, r);
                const uint32_t ent = Form::entry(p, q, h, gone);
                const unsigned long long s = p.unit_off[e0 + r], e = p.unit_off[e0 + r + 1];
                if (e <= lo) continue;
                if (s >= hi) break;
                TsvWindow o = { win, s, w, lo, hi };
                Form::row(p, o, (uint32_t)q, h, ent, X);
            }
        }
        __syncthreads();
        out_store_window(p.out, win, w, lo, hi);
        __syncthreads();
    }
}
