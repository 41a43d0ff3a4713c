// tsv_rows.hip.inc — the TSV response rows of the reported hits, written on the device (included by search.hip after
// top_align.hip.inc; the host side is host_tsv.hip.inc, the contract and the host formatter are in tsv_format.cpp).
//
// QueryResultHandler builds a row with `output += ...` per field (search.go:505-554).  Behind kaamer_topn_device all a row
// needs is resident: the text with the records' name spans, the reported hits, SizeInKmer / StartPosition after
// SetBestStartCodon, the bitmaps of the reported hits and the subject text (kaamer_index_attach_subject_text).
//
//   tsv_len_kernel     a lane per query: the bytes of its rows (tsv_row into a counting sink: digits, field lengths, for
//                      field 11 the runs of the bitmap words), summed per tile of TSV_TILE queries
//   tsv_scan_kernel    one workgroup: the tiles' bytes and rows, scanned in 64 bits; the totals, the capacity check
//   tsv_off_kernel     a workgroup per tile, a lane per query: the first byte of every row (line_off, in CSR order), from the
//                      tiles' prefixes, a scan inside the tile and the rows' lengths once more (nothing per row is kept
//                      between the passes: a batch has up to max_results rows per query, nearly all of them absent)
//   tsv_write_kernel   a workgroup per tile, a lane per query.  The rows of a tile are one contiguous byte range of the
//                      output.  Rows are short, many and uneven, and names, ids and annotation values are byte copies at
//                      arbitrary alignment, so no lane writes a row to memory itself: the workgroup builds the range in LDS,
//                      TSV_WINDOW bytes at a time (windows lie on multiples of TSV_WINDOW in the output), every lane putting
//                      the part of its rows that falls into the window (tsv_row into a clipping sink), and then stores the
//                      window with 16 bytes per lane, consecutive lanes at consecutive addresses.  Only the first and the last
//                      16 bytes of a tile's range, which it may share with its neighbours, go out as single bytes.
// The same tsv_row serves the length passes and the write pass, so they cannot disagree about a row.  (Two kernels instead
// of one behind the scan: with both instances of tsv_row in one kernel the compiler needed scratch memory for scalar
// registers; apart they need none.)
// Nothing is written beyond out_cap or line_cap: the scan kernel sets the status word and the write kernel returns.
#define TSV_TILE 256u
#define TSV_WINDOW 16384u
#define TSV_NONE 0xFFFFFFFFu
enum { TSV_C_LINES = 0, TSV_C_BYTES = 1, TSV_C_STATUS = 2, TSV_C_RAW = 3 /* tsv_aln_rows.hip.inc */, TSV_C_N = 4 };
enum { TSV_ST_OUT_CAP = 1u, TSV_ST_LINE_CAP = 2u, TSV_ST_UPSTREAM = 4u /* the batch's own status, or no bitmaps in its block */ };

struct TsvParams {
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
    int positions, annotations;
    // the host-buffer calls: the packed result block of the same batch (topn.hip.inc).  A block whose status word is set is
    // refused by the host whatever follows, so the stage writes nothing; with positions the bitmaps are the block's section
    // (top_positions.hip.inc: per query at pos_base[q], as in the workspace's own storage)
    const uint8_t *block;
    // the subject text: entry i is st_bytes[st_off[i], st_off[i + 1]), its first st_idlen[i] bytes the EntryId, the rest the
    // annotation columns ('\t' + value each)
    const uint8_t *st_bytes;
    const uint64_t *st_off;
    const uint32_t *st_idlen, *st_length, *idmap;
    uint32_t idmap_n, n_features;
    // the stage's own
    unsigned long long *tile_bytes, *tile_lines;   // per tile: sums, then exclusive prefixes
    unsigned long long *line_off;
    uint64_t line_cap;
    char *out;
    uint64_t out_cap;
    unsigned long long *counts;    // TSV_C_*
};

__device__ __forceinline__ uint32_t tsv_digits(uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u
         : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}

// counts the bytes of a row
struct TsvCount {
    uint64_t n = 0;
    __device__ __forceinline__ void put(char) { n++; }
    __device__ __forceinline__ void copy(const uint8_t *, uint64_t len) { n += len; }
    __device__ __forceinline__ void fill(char, uint32_t len) { n += len; }
    __device__ __forceinline__ void put_u32(uint32_t v) { n += tsv_digits(v); }
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
        for (uint32_t d = tsv_digits(v); d > 1; d--) div *= 10u;
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

// the id -> entry map, as kaamer_fetch_hits resolves an id
__device__ __forceinline__ uint32_t tsv_entry(const TsvParams &p, uint32_t pid)
{
    return pid < p.idmap_n ? p.idmap[pid] : TSV_NONE;
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

// row r of query q; ent: the hit's entry, TSV_NONE from the query's first missing entry on
template <class Sink> __device__ __forceinline__ void tsv_row(const TsvParams &p, Sink &o, uint32_t q, uint32_t r, uint32_t ent)
{
    const kaamer_query_meta m = p.q[q];
    if (m.src_seq < p.n_names) {   // strings.Split(Query.Name, " ")[0]
        const kaamer_text_span sp = p.spans[m.src_seq];
        if ((uint64_t)sp.name_off + sp.name_len <= p.names_len) {
            const uint8_t *name = p.names + sp.name_off;
            o.copy(name, tsv_query_id_len(name, sp.name_len));
        }
    }
    o.put('\t');
    const uint64_t s0 = ent != TSV_NONE ? p.st_off[ent] : 0, s1 = ent != TSV_NONE ? p.st_off[ent + 1] : 0;
    const uint32_t idlen = ent != TSV_NONE ? p.st_idlen[ent] : 0;
    o.copy(p.st_bytes + s0, idlen);
    o.put('\t');
    const uint32_t km = p.top_km[(uint64_t)q * p.K + r];
    const int32_t size = p.size_out[q];
    tsv_put_identity(o, km, size);
    o.put('\t');
    tsv_put_i32(o, size);
    o.put('\t');
    o.put_u32(km);
    o.put('\t');
    const uint64_t *bits = nullptr;
    uint32_t n_bits = 0;
    if (p.positions) {
        const int32_t n = p.pos_len[q];
        n_bits = n > 0 ? (uint32_t)n : 0u;
        bits = p.pos_bits + p.pos_base[q] + (uint64_t)r * ((n_bits + 63u) >> 6);
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
    if (p.annotations) o.put_u32(ent != TSV_NONE ? p.st_length[ent] : 0u);
    else { o.put('N'); o.put('/'); o.put('A'); }
    if (p.positions) {
        o.put('\t');
        tsv_put_positions(o, bits, n_bits);
    }
    if (p.annotations) {
        if (ent != TSV_NONE) o.copy(p.st_bytes + s0 + idlen, s1 - s0 - idlen);
        else o.fill('\t', p.n_features);
    }
    o.put('\n');
}

// inclusive scan of one value per thread of a TSV_TILE-thread workgroup (sh: TSV_TILE words); every thread gets its own
// inclusive prefix, *total the workgroup's sum
__device__ __forceinline__ unsigned long long tsv_block_scan(unsigned long long v, unsigned long long *sh, unsigned long long *total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < TSV_TILE; o <<= 1) {
        const unsigned long long add = t >= o ? sh[t - o] : 0ull;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const unsigned long long mine = sh[t];
    *total = sh[TSV_TILE - 1];
    __syncthreads();
    return mine;
}

__device__ __forceinline__ uint32_t tsv_nq(const TsvParams &p)
{
    const uint32_t nq = *p.d_nq;
    return nq < p.nq_cap ? nq : p.nq_cap;
}

// false: the batch's block is flagged (or holds no bitmaps although they are wanted) -- nothing of the batch is read;
// else, with positions, the bitmaps are taken from the block.  Every thread computes the same.
__device__ __forceinline__ bool tsv_upstream(TsvParams &p)
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

__global__ __launch_bounds__(TSV_TILE) void tsv_len_kernel(TsvParams p)
{
    __shared__ unsigned long long sh[TSV_TILE];
    const uint32_t nq = tsv_nq(p);
    if ((uint64_t)blockIdx.x * TSV_TILE >= nq || !tsv_upstream(p)) return;
    const uint64_t q = (uint64_t)blockIdx.x * TSV_TILE + threadIdx.x;
    TsvCount o;
    uint32_t cnt = 0;
    if (q < nq) {
        cnt = p.top_cnt[q];
        if (cnt > p.K) cnt = p.K;
        bool gone = false;
        for (uint32_t r = 0; r < cnt; r++) {
            const uint32_t ent = gone ? TSV_NONE : tsv_entry(p, p.top_pid[q * p.K + r]);
            gone = ent == TSV_NONE;
            tsv_row(p, o, (uint32_t)q, r, ent);
        }
    }
    unsigned long long bytes = 0, lines = 0;
    (void)tsv_block_scan(o.n, sh, &bytes);
    (void)tsv_block_scan(cnt, sh, &lines);
    if (threadIdx.x == 0) { p.tile_bytes[blockIdx.x] = bytes; p.tile_lines[blockIdx.x] = lines; }
}

// one workgroup: exclusive scan of the tiles' two sums in place, TSV_TILE tiles per round; totals and status
__global__ __launch_bounds__(TSV_TILE) void tsv_scan_kernel(TsvParams p)
{
    __shared__ unsigned long long sh[TSV_TILE];
    if (!tsv_upstream(p)) {
        if (threadIdx.x == 0) { p.counts[TSV_C_LINES] = 0; p.counts[TSV_C_BYTES] = 0; p.counts[TSV_C_STATUS] = TSV_ST_UPSTREAM; }
        return;
    }
    const uint32_t nq = tsv_nq(p);
    const uint32_t tiles = (nq + TSV_TILE - 1u) / TSV_TILE;
    unsigned long long base_b = 0, base_l = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += TSV_TILE) {
        const uint32_t t = t0 + threadIdx.x;
        const unsigned long long b = t < tiles ? p.tile_bytes[t] : 0ull, l = t < tiles ? p.tile_lines[t] : 0ull;
        unsigned long long tb = 0, tl = 0;
        const unsigned long long ib = tsv_block_scan(b, sh, &tb), il = tsv_block_scan(l, sh, &tl);
        if (t < tiles) { p.tile_bytes[t] = base_b + ib - b; p.tile_lines[t] = base_l + il - l; }
        base_b += tb; base_l += tl;
    }
    if (threadIdx.x == 0) {
        unsigned long long st = 0;
        if (base_b > p.out_cap) st |= TSV_ST_OUT_CAP;
        if (base_l + 1ull > p.line_cap) st |= TSV_ST_LINE_CAP;
        p.counts[TSV_C_LINES] = base_l; p.counts[TSV_C_BYTES] = base_b; p.counts[TSV_C_STATUS] = st;
        if (!st) p.line_off[base_l] = base_b;
    }
}

// a workgroup per tile, a lane per query: where every row starts (the tiles' prefixes, a scan of the queries' rows and bytes
// inside the tile, the rows' lengths once more)
__global__ __launch_bounds__(TSV_TILE) void tsv_off_kernel(TsvParams p)
{
    __shared__ unsigned long long sh[TSV_TILE];
    const uint32_t nq = tsv_nq(p);
    if ((uint64_t)blockIdx.x * TSV_TILE >= nq) return;
    if (p.counts[TSV_C_STATUS]) return;   // (uniform: written by the scan kernel before this one started)
    (void)tsv_upstream(p);
    const uint64_t q = (uint64_t)blockIdx.x * TSV_TILE + threadIdx.x;
    uint32_t cnt = 0;
    if (q < nq) {
        cnt = p.top_cnt[q];
        if (cnt > p.K) cnt = p.K;
    }
    unsigned long long tile_total = 0;
    const unsigned long long e0 = p.tile_lines[blockIdx.x] + tsv_block_scan(cnt, sh, &tile_total) - cnt;
    unsigned long long mine = 0;
    bool gone = false;
    for (uint32_t r = 0; r < cnt; r++) {
        const uint32_t ent = gone ? TSV_NONE : tsv_entry(p, p.top_pid[q * p.K + r]);
        gone = ent == TSV_NONE;
        TsvCount o;
        tsv_row(p, o, (uint32_t)q, r, ent);
        p.line_off[e0 + r] = mine;   // relative to the query's first byte for now
        mine += o.n;
    }
    const unsigned long long q0 = p.tile_bytes[blockIdx.x] + tsv_block_scan(mine, sh, &tile_total) - mine;
    for (uint32_t r = 0; r < cnt; r++) p.line_off[e0 + r] += q0;
}

// [lo, hi) of the output from the LDS window that starts at `w`, by the whole workgroup: 16 bytes per lane, consecutive
// lanes consecutive addresses; a chunk the range covers only in part goes out in bytes
__device__ __forceinline__ void tsv_store_window(char *out, const char *win, unsigned long long w, unsigned long long lo, unsigned long long hi)
{
    for (unsigned long long c = (lo - w) / 16ull + threadIdx.x; c * 16ull < hi - w; c += TSV_TILE) {
        const unsigned long long at = w + c * 16ull;
        if (at >= lo && at + 16ull <= hi) {
            *reinterpret_cast<uint4 *>(out + at) = *reinterpret_cast<const uint4 *>(win + c * 16ull);
        } else {
            const unsigned long long a = at > lo ? at : lo, b = at + 16ull < hi ? at + 16ull : hi;
            for (unsigned long long i = a; i < b; i++) out[i] = win[i - w];
        }
    }
}

__global__ __launch_bounds__(TSV_TILE) void tsv_write_kernel(TsvParams p)
{
    __shared__ unsigned long long sh[TSV_TILE];
    __shared__ __attribute__((aligned(16))) char win[TSV_WINDOW];
    const uint32_t nq = tsv_nq(p);
    if ((uint64_t)blockIdx.x * TSV_TILE >= nq) return;
    if (p.counts[TSV_C_STATUS]) return;   // (uniform: written by the scan kernel before this one started)
    (void)tsv_upstream(p);
    const uint64_t q = (uint64_t)blockIdx.x * TSV_TILE + threadIdx.x;
    uint32_t cnt = 0;
    if (q < nq) {
        cnt = p.top_cnt[q];
        if (cnt > p.K) cnt = p.K;
    }
    unsigned long long tile_total = 0;
    const unsigned long long e0 = p.tile_lines[blockIdx.x] + tsv_block_scan(cnt, sh, &tile_total) - cnt;
    // the tile's rows are [b0, b1) of the output; line_off[lines] is the total, so every row's end is the next entry
    const unsigned long long b0 = p.tile_bytes[blockIdx.x], b1 = p.line_off[p.tile_lines[blockIdx.x] + tile_total];
    const unsigned long long q0 = cnt ? p.line_off[e0] : 0ull, q1 = cnt ? p.line_off[e0 + cnt] : 0ull;
    for (unsigned long long w = b0 - b0 % TSV_WINDOW; w < b1; w += TSV_WINDOW) {
        const unsigned long long lo = w > b0 ? w : b0, hi = w + TSV_WINDOW < b1 ? w + TSV_WINDOW : b1;
        if (q0 < hi && q1 > lo) {
            bool gone = false;
            for (uint32_t r = 0; r < cnt; r++) {
                const uint32_t ent = gone ? TSV_NONE : tsv_entry(p, p.top_pid[q * p.K + r]);
                gone = ent == TSV_NONE;
                const unsigned long long s = p.line_off[e0 + r], e = p.line_off[e0 + r + 1];
                if (e <= lo) continue;
                if (s >= hi) break;
                TsvWindow o = { win, s, w, lo, hi };
                tsv_row(p, o, (uint32_t)q, r, ent);
            }
        }
        __syncthreads();
        tsv_store_window(p.out, win, w, lo, hi);
        __syncthreads();
    }
}
