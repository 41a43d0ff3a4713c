// parse_text.hip.inc — GetQueriesFastq (search.go:324-412) on the device: raw FASTQ text in HBM -> the packed batch
// kaamer_search_device takes (sequence bytes + u64 offsets) plus one span per record (included by search.hip).
//
// The rules, stated per line (the header repeats them next to kaamer_parse_fastq_device; RecordParser in
// host_search.cpp is the host's statement of the same reader):
//   lines    split at '\n'; a last piece without '\n' is a line; one trailing '\r' is dropped (bufio.ScanLines)
//   class    X  empty after the '\r' drop, or anything that is neither H nor S (ignored)
//            H  the first byte is '@' (search.go:380: also a quality line that happens to start with '@')
//            S  every byte is one of ATGCNatgcn (search.go:340,386: also a quality line made of those letters)
//   records  an S line whose next non-X line is an H, or that has no next non-X line (of a run of S lines the last one
//            wins: search.go:386-388 replaces the pending sequence); its name is what follows the '@' of the nearest
//            preceding H line, empty when there is none; no case change; SizeInKmer = len - 6 (search.go:395,407)
//
// Seven launches on one stream, ordered by nothing but the end of each grid (no workgroup ever waits on another):
//   pt_count_kernel      per PT_TILE bytes: the number of '\n'
//   pt_tile_scan_kernel  one workgroup: exclusive scan of those counts, the line totals, the first status check
//   pt_lines_kernel      per tile again: where every line starts, and which lines hold a byte outside the S alphabet.
//                        Lines are classified BY POSITION: every lane looks at its own 16 bytes whatever line they
//                        belong to, so a line as long as the whole text costs what the same bytes in short lines cost
//   pt_records_kernel<0> per PT_LINES lines: class of every line, the records that are decided inside the block,
//                        the block's summary (first non-X class, last H line, an undecided last S line)
//   pt_block_scan_kernel one workgroup: what follows / precedes every block of lines, record and byte bases, totals
//   pt_records_kernel<1> per PT_LINES lines again, now with its bases: offsets[] and spans[]
//   pt_gather_kernel     BY DESTINATION: every lane fills 16 bytes of the packed buffer, finding its record by binary
//                        search in offsets[] -- again no per-line work, a read of any length is spread over the grid
enum {
    PT_PIECE = 16,                              // bytes a lane reads at once
    PT_BLOCK = 256,                             // threads of the two tile kernels
    PT_PIECES = 4,                              // pieces per lane and tile
    PT_WAVE_STEP = 64 * PT_PIECE,               // bytes one wave reads with one instruction
    PT_TILE = PT_BLOCK * PT_PIECE * PT_PIECES,  // bytes of text per workgroup: 16 KiB
    PT_LINES = 1024,                            // lines per workgroup of pt_records_kernel (= its threads)
};
enum { PT_ST_RECORDS = 1u, PT_ST_LINES = 2u };
enum { PT_X = 0, PT_H = 1, PT_S = 2 };
// the words of the result block (u64 each)
enum { PT_R_RECORDS = 0, PT_R_LINES, PT_R_SEQ_BYTES, PT_R_STATUS, PT_R_NL /* lines as the kernels count them: '\n's + 1 */, PT_R_N };

struct PtParams {
    const uint8_t *text;     // 16-byte aligned
    uint32_t n;              // bytes of text
    uint32_t n_tiles;
    uint32_t line_cap;       // line_start holds line_cap + 2 entries, bad line_cap + 1
    uint32_t rec_cap;
    uint32_t *tile_nl;       // n_tiles + 1: counts, then (in place) exclusive bases
    uint32_t *line_start;    // line i = [line_start[i], line_start[i + 1] - 1): the '\n' excluded; u32 arithmetic wraps on purpose
    uint32_t *bad;           // line i holds a byte outside ATGCNatgcn (the dropped '\r' apart)
    // per block of PT_LINES lines
    uint32_t *blk_first, *blk_last_h, *blk_cnt, *blk_next, *blk_rec_base, *blk_h_before;
    uint64_t *blk_bytes, *blk_tail, *blk_byte_base;
    uint8_t *seqs;
    uint64_t *offsets;
    kaamer_text_span *spans;
    unsigned long long *res; // PT_R_*
};

// ^[ATGCNatgcn]$ for one byte: letters only (0x41-0x5A, 0x61-0x7A share bits 7-6 = 01), then a 32-bit table over bits 4-0
__device__ __forceinline__ bool pt_is_nt(uint32_t c)
{
    const uint32_t table = (1u << 1) | (1u << 3) | (1u << 7) | (1u << 14) | (1u << 20);   // a c g n t
    return (c & 0xC0u) == 0x40u && ((table >> (c & 31u)) & 1u);
}

// the piece at `pos` (a multiple of 16): bytes beyond the text read as 0 and are never looked at (nv = valid bytes)
__device__ __forceinline__ uint4 pt_load_piece(const uint8_t *text, uint32_t n, uint32_t pos, uint32_t &nv)
{
    uint4 v = make_uint4(0, 0, 0, 0);
    nv = 0;
    if (pos >= n) return v;
    nv = n - pos < (uint32_t)PT_PIECE ? n - pos : (uint32_t)PT_PIECE;
    if (nv == PT_PIECE) return *reinterpret_cast<const uint4 *>(text + pos);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < PT_PIECE; b++)
        if ((uint32_t)b < nv) w[b >> 2] |= (uint32_t)text[pos + b] << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t pt_piece_byte(const uint4 &v, int b)
{
    const uint32_t w = (b >> 2) == 0 ? v.x : (b >> 2) == 1 ? v.y : (b >> 2) == 2 ? v.z : v.w;
    return (w >> (8 * (b & 3))) & 0xFFu;
}

__device__ __forceinline__ uint32_t pt_count_nl(const uint4 &v, uint32_t nv)
{
    uint32_t c = 0;
#pragma unroll
    for (int b = 0; b < PT_PIECE; b++) c += ((uint32_t)b < nv && pt_piece_byte(v, b) == '\n') ? 1u : 0u;
    return c;
}

// inclusive sum over the 256 threads of a tile kernel (a lane's 16 bytes may hold several '\n', so the ranks come from
// a shuffle scan of the per-lane counts, not from a ballot); block_total: the sum over all.  `wsum`: 4 words of LDS
__device__ __forceinline__ uint32_t pt_block_incl_sum(uint32_t v, uint32_t *wsum, uint32_t &block_total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(s, d, 64);
        if (lane >= d) s += o;
    }
    __syncthreads();   // (wsum of the previous piece has been read)
    if (lane == 63) wsum[w] = s;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < PT_BLOCK / 64; i++) {
        const uint32_t x = wsum[i];
        if (i < w) before += x;
        total += x;
    }
    block_total = total;
    return s + before;
}

__global__ __launch_bounds__(PT_BLOCK) void pt_count_kernel(PtParams p)
{
    __shared__ uint32_t wsum[PT_BLOCK / 64];
    const uint32_t tile = blockIdx.x;
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < PT_PIECES; j++) {
        const uint64_t pos = (uint64_t)tile * PT_TILE + (uint64_t)(j * PT_BLOCK + threadIdx.x) * PT_PIECE;
        if (pos >= p.n) continue;
        uint32_t nv;
        const uint4 v = pt_load_piece(p.text, p.n, (uint32_t)pos, nv);
        // most pieces of a FASTQ hold no '\n': a word-wide test (a zero byte in v ^ 0x0A0A0A0A; it may say yes wrongly,
        // never no) before the byte loop
        const uint32_t has = ((v.x ^ 0x0A0A0A0Au) - 0x01010101u) & ~(v.x ^ 0x0A0A0A0Au) & 0x80808080u;
        const uint32_t has2 = ((v.y ^ 0x0A0A0A0Au) - 0x01010101u) & ~(v.y ^ 0x0A0A0A0Au) & 0x80808080u;
        const uint32_t has3 = ((v.z ^ 0x0A0A0A0Au) - 0x01010101u) & ~(v.z ^ 0x0A0A0A0Au) & 0x80808080u;
        const uint32_t has4 = ((v.w ^ 0x0A0A0A0Au) - 0x01010101u) & ~(v.w ^ 0x0A0A0A0Au) & 0x80808080u;
        if (has | has2 | has3 | has4) cnt += pt_count_nl(v, nv);
    }
    uint32_t total;
    (void)pt_block_incl_sum(cnt, wsum, total);
    if (threadIdx.x == 0) p.tile_nl[tile] = total;
}

// ---- scans of one workgroup of PT_LINES threads over an LDS array (Hillis-Steele: log2 steps, two barriers each) ----
// REV = false: v[t] = op(v[t - d], v[t]);  REV = true: v[t] = op(v[t], v[t + d]) (a suffix scan).  On return lds[] holds the
// scanned values of every thread, valid until the next call.
template <bool REV, class T, class Op> __device__ __forceinline__ T pt_scan(T v, T *lds, Op op)
{
    const int t = threadIdx.x;
    __syncthreads();   // (the previous user of lds is done)
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < PT_LINES; d <<= 1) {
        T o = v;
        if (!REV) { if (t >= d) o = op(lds[t - d], v); }
        else { if (t + d < PT_LINES) o = op(v, lds[t + d]); }
        __syncthreads();
        lds[t] = v = o;
        __syncthreads();
    }
    return v;
}
struct PtAdd32 { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct PtAdd64 { __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; } };
struct PtMax32 { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct PtFirst { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a ? a : b; } };   // the nearer non-X class

__global__ __launch_bounds__(PT_LINES) void pt_tile_scan_kernel(PtParams p)
{
    __shared__ uint32_t lds[PT_LINES];
    __shared__ uint32_t carry_s;
    const int t = threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < p.n_tiles; base += PT_LINES) {
        const uint32_t i = base + t;
        const uint32_t v = i < p.n_tiles ? p.tile_nl[i] : 0u;
        const uint32_t incl = pt_scan<false>(v, lds, PtAdd32());
        const uint32_t carry = carry_s;
        if (i < p.n_tiles) p.tile_nl[i] = carry + incl - v;
        __syncthreads();
        if (t == PT_LINES - 1) carry_s = carry + incl;
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t total_nl = carry_s;   // < 2^32: the text has fewer bytes than that
        p.tile_nl[p.n_tiles] = total_nl;
        // lines as the reader counts them: a last piece without '\n' is one, an empty one is not
        p.res[PT_R_LINES] = (unsigned long long)total_nl + ((p.n && p.text[p.n - 1] != '\n') ? 1ull : 0ull);
        const unsigned long long nl = (unsigned long long)total_nl + 1;   // ... and as the kernels do: the last may be empty (class X)
        p.res[PT_R_NL] = nl;
        p.line_start[0] = 0;
        if (nl > p.line_cap) p.res[PT_R_STATUS] = PT_ST_LINES;
        else p.line_start[nl] = p.n + 1u;   // the text's end as one more '\n' (wraps to 0 at 2^32 - 1 bytes: see PtParams)
    }
}

__global__ __launch_bounds__(PT_BLOCK) void pt_lines_kernel(PtParams p)
{
    __shared__ uint32_t wsum[PT_BLOCK / 64];
    if (p.res[PT_R_STATUS]) return;
    const uint32_t tile = blockIdx.x;
    uint32_t carry = p.tile_nl[tile];
#pragma unroll 1
    for (int j = 0; j < PT_PIECES; j++) {
        const uint64_t pos64 = (uint64_t)tile * PT_TILE + (uint64_t)(j * PT_BLOCK + threadIdx.x) * PT_PIECE;
        uint32_t nv = 0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (pos64 < p.n) v = pt_load_piece(p.text, p.n, (uint32_t)pos64, nv);
        const uint32_t pos = (uint32_t)pos64;
        const uint32_t cnt = pt_count_nl(v, nv);
        uint32_t total;
        const uint32_t incl = pt_block_incl_sum(cnt, wsum, total);
        uint32_t line = carry + incl - cnt;   // the line this piece's first byte belongs to
        carry += total;
        bool bad = false;
#pragma unroll
        for (int b = 0; b < PT_PIECE; b++) {
            const uint32_t c = pt_piece_byte(v, b);
            if ((uint32_t)b >= nv) {
                // (beyond the text)
            } else if (c == '\n') {
                if (bad && line < p.line_cap + 1u) __hip_atomic_store(&p.bad[line], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bad = false;
                line++;
                if (line <= p.line_cap) p.line_start[line] = pos + (uint32_t)b + 1u;
            } else if (!pt_is_nt(c)) {
                bool dropped = false;   // one '\r' right before the '\n' or the text's end is not part of the line
                if (c == '\r') {
                    const uint32_t q = pos + (uint32_t)b + 1u;
                    dropped = q >= p.n || (b + 1 < PT_PIECE ? pt_piece_byte(v, (b + 1) & 15) : (uint32_t)p.text[q]) == '\n';
                }
                if (!dropped) bad = true;
            }
        }
        if (bad && line < p.line_cap + 1u) __hip_atomic_store(&p.bad[line], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// bytes of line i after the '\r' drop
__device__ __forceinline__ uint32_t pt_line_len(const PtParams &p, uint32_t i, uint32_t &start)
{
    start = p.line_start[i];
    const uint32_t end = p.line_start[i + 1] - 1u;
    uint32_t len = end - start;
    if (len && p.text[end - 1u] == '\r') len--;
    return len;
}

template <bool EMIT> __global__ __launch_bounds__(PT_LINES) void pt_records_kernel(PtParams p)
{
    __shared__ unsigned long long lds64[PT_LINES];
    uint32_t *lds = reinterpret_cast<uint32_t *>(lds64);
    if (p.res[PT_R_STATUS]) return;
    const unsigned long long nl = p.res[PT_R_NL];
    const uint32_t blk = blockIdx.x;
    if ((unsigned long long)blk * PT_LINES >= nl) return;
    const int t = threadIdx.x;
    const unsigned long long i64 = (unsigned long long)blk * PT_LINES + t;
    const uint32_t i = (uint32_t)i64;
    uint32_t cls = PT_X, start = 0, len = 0;
    if (i64 < nl) {
        len = pt_line_len(p, i, start);
        if (len) cls = p.text[start] == '@' ? PT_H : (p.bad[i] ? PT_X : PT_S);
    }
    // the class of the next non-X line: inside the block, else what follows the block (known on the second pass)
    (void)pt_scan<true>(cls, lds, PtFirst());
    uint32_t next = t + 1 < PT_LINES ? lds[t + 1] : 0u;
    const bool undecided = cls == PT_S && next == 0;   // at most the block's last non-X line
    if (EMIT && next == 0) next = p.blk_next[blk];
    const uint32_t first_in_block = lds[0];
    const bool rec = cls == PT_S && (EMIT ? next != PT_S : next == PT_H);
    // the nearest H line at or before this one, as line index + 1 (0: none)
    uint32_t h = pt_scan<false>(cls == PT_H ? i + 1u : 0u, lds, PtMax32());
    const uint32_t last_h_in_block = lds[PT_LINES - 1];
    const uint32_t cnt_incl = pt_scan<false>(rec ? 1u : 0u, lds, PtAdd32());
    const uint32_t cnt_total = lds[PT_LINES - 1];
    const unsigned long long bytes_incl = pt_scan<false>((unsigned long long)(rec ? len : 0u), lds64, PtAdd64());
    const unsigned long long bytes_total = lds64[PT_LINES - 1];
    if (!EMIT) {
        if (t == 0) {
            p.blk_first[blk] = first_in_block;
            p.blk_last_h[blk] = last_h_in_block;
            p.blk_cnt[blk] = cnt_total;
            p.blk_bytes[blk] = bytes_total;
            p.blk_tail[blk] = 0;
        }
        __syncthreads();
        if (undecided) p.blk_tail[blk] = (1ull << 32) | len;
        return;
    }
    if (!rec) return;
    if (h == 0) h = p.blk_h_before[blk];
    const unsigned long long r = (unsigned long long)p.blk_rec_base[blk] + cnt_incl - 1u;
    if (r >= p.rec_cap) return;   // (the status word is set: pt_block_scan_kernel)
    kaamer_text_span sp;
    sp.name_off = 0; sp.name_len = 0; sp.seq_off = start; sp.seq_len = len;
    if (h) {
        uint32_t hs;
        const uint32_t hl = pt_line_len(p, h - 1u, hs);   // (an H line has at least its '@')
        sp.name_off = hs + 1u; sp.name_len = hl - 1u;
    }
    p.spans[r] = sp;
    p.offsets[r] = p.blk_byte_base[blk] + bytes_incl - len;
}

__global__ __launch_bounds__(PT_LINES) void pt_block_scan_kernel(PtParams p)
{
    __shared__ unsigned long long lds64[PT_LINES];
    __shared__ unsigned long long carry64_s;
    __shared__ uint32_t carry_s, carry_h_s;
    uint32_t *lds = reinterpret_cast<uint32_t *>(lds64);
    if (p.res[PT_R_STATUS]) return;
    const unsigned long long nl = p.res[PT_R_NL];
    const uint32_t nb = (uint32_t)((nl + PT_LINES - 1) / PT_LINES);
    const int t = threadIdx.x;
    // what follows every block: a suffix scan, chunk by chunk from the end
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = (nb - 1) / PT_LINES * PT_LINES;; base -= PT_LINES) {
        const uint32_t b = base + t;
        const uint32_t v = b < nb ? p.blk_first[b] : 0u;
        (void)pt_scan<true>(v, lds, PtFirst());
        const uint32_t carry = carry_s;
        uint32_t next = t + 1 < PT_LINES ? lds[t + 1] : 0u;
        if (!next) next = carry;
        if (b < nb) p.blk_next[b] = next;
        const uint32_t head = lds[0];
        __syncthreads();
        if (t == 0) carry_s = head ? head : carry;
        __syncthreads();
        if (base == 0) break;
    }
    // record and byte bases, the nearest H line before every block
    if (t == 0) { carry_s = 0; carry_h_s = 0; carry64_s = 0; }
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += PT_LINES) {
        const uint32_t b = base + t;
        uint32_t cnt = 0, lh = 0;
        unsigned long long bytes = 0;
        if (b < nb) {
            cnt = p.blk_cnt[b]; bytes = p.blk_bytes[b]; lh = p.blk_last_h[b];
            const unsigned long long tail = p.blk_tail[b];
            if ((tail >> 32) && p.blk_next[b] != PT_S) { cnt++; bytes += (uint32_t)tail; }   // its last S line is a record after all
        }
        const uint32_t cnt_incl = pt_scan<false>(cnt, lds, PtAdd32());
        const uint32_t c0 = carry_s;
        const uint32_t h_incl = pt_scan<false>(lh, lds, PtMax32());
        const uint32_t h_excl = t ? lds[t - 1] : 0u;
        const uint32_t h0 = carry_h_s;
        const unsigned long long bytes_incl = pt_scan<false>(bytes, lds64, PtAdd64());
        const unsigned long long b0 = carry64_s;
        if (b < nb) {
            p.blk_rec_base[b] = c0 + cnt_incl - cnt;
            p.blk_byte_base[b] = b0 + bytes_incl - bytes;
            p.blk_h_before[b] = h_excl > h0 ? h_excl : h0;
        }
        __syncthreads();
        if (t == PT_LINES - 1) { carry_s = c0 + cnt_incl; carry_h_s = h_incl > h0 ? h_incl : h0; carry64_s = b0 + bytes_incl; }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t n_rec = carry_s;   // < 2^31: a record takes two bytes of text
        p.res[PT_R_RECORDS] = n_rec;
        p.res[PT_R_SEQ_BYTES] = carry64_s;
        if (n_rec > p.rec_cap) p.res[PT_R_STATUS] = PT_ST_RECORDS;
        else p.offsets[n_rec] = carry64_s;
    }
}

// 16 bytes of the packed buffer per lane.  The buffer holds 16 bytes more than the text, so the last piece is stored whole.
__global__ __launch_bounds__(PT_BLOCK) void pt_gather_kernel(PtParams p)
{
    if (p.res[PT_R_STATUS]) return;
    const uint32_t n_rec = (uint32_t)p.res[PT_R_RECORDS];
    const unsigned long long total = p.res[PT_R_SEQ_BYTES];
    const unsigned long long n_pieces = (total + PT_PIECE - 1) / PT_PIECE;
    for (unsigned long long k = (unsigned long long)blockIdx.x * PT_BLOCK + threadIdx.x; k < n_pieces; k += (unsigned long long)gridDim.x * PT_BLOCK) {
        const unsigned long long d = k * PT_PIECE;
        // the record that holds byte d: the last r with offsets[r] <= d (records are never empty)
        uint32_t lo = 0, hi = n_rec - 1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (p.offsets[mid] <= d) lo = mid; else hi = mid - 1;
        }
        uint32_t r = lo;
        unsigned long long r_end = p.offsets[r + 1];
        uint32_t src = p.spans[r].seq_off + (uint32_t)(d - p.offsets[r]);
        uint32_t w[4] = {0, 0, 0, 0};
        const uint32_t a = src & ~3u;
        if (r_end >= d + PT_PIECE && (unsigned long long)a + 20 <= p.n) {
            // the whole piece comes out of one read: five aligned words, shifted into place
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p.text + a);
            const uint32_t x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3], x4 = q[4];
            const uint32_t sh = (src & 3u) * 8u;
            w[0] = __funnelshift_r(x0, x1, sh); w[1] = __funnelshift_r(x1, x2, sh);
            w[2] = __funnelshift_r(x2, x3, sh); w[3] = __funnelshift_r(x3, x4, sh);
        } else {
#pragma unroll
            for (int b = 0; b < PT_PIECE; b++) {
                const unsigned long long at = d + (unsigned long long)b;
                if (at < total) {
                    if (at >= r_end) { r++; r_end = p.offsets[r + 1]; src = p.spans[r].seq_off; }
                    w[b >> 2] |= (uint32_t)p.text[src] << (8 * (b & 3));
                    src++;
                }
            }
        }
        *reinterpret_cast<uint4 *>(p.seqs + d) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ------------------------------------------------------------------------------------------------------------------
struct kaamer_text_parser {
    int device = 0;
    uint64_t max_text = 0;
    uint32_t rec_cap = 0, line_cap = 0, n_tiles_cap = 0, n_blk_cap = 0;
    int n_cu = 0;
    DevBuf<uint32_t> d_u32;                    // every u32 array, one allocation
    DevBuf<unsigned long long> d_u64;          // every u64 array
    DevBuf<uint8_t> d_seqs;
    DevBuf<kaamer_text_span> d_spans;
    DevBuf<uint32_t> d_fa;                     // what only FASTA needs (parse_fasta.hip.inc), allocated at the first FASTA text
    PinnedBuf<unsigned long long> h_res;
    PtParams p{};                              // the device pointers, laid out once
    bool parsed = false;
    bool fasta = false;                        // the last parse was kaamer_parse_fasta_device
    ~kaamer_text_parser() { (void)hipSetDevice(device); }   // (before the buffers go)
};

static uint64_t pt_default_line_cap(uint64_t max_text, uint32_t max_records)
{
    // a FASTQ record is four lines; anything beyond this rule sets PT_ST_LINES (KAAMER_E_CAPACITY), never a partial result
    uint64_t cap = max_text / 16 + (uint64_t)max_records * 4 + 1024;
    if (cap > max_text + 1) cap = max_text + 1;   // a text cannot hold more lines than that
    return cap;
}

extern "C" {

void kaamer_text_parser_free(kaamer_text_parser *ps) { delete ps; }

static int text_parser_create_lines(int device, uint64_t max_text_bytes, uint32_t max_records, uint64_t line_cap, kaamer_text_parser **out)
{
    if (!out) return kaamer_fail(KAAMER_E_ARG, "text_parser_create: bad argument");
    *out = nullptr;
    if (max_text_bytes > 0xFFFFFFFFull)
        return kaamer_fail(KAAMER_E_ARG, "text_parser_create: a text holds at most 2^32 - 1 bytes (spans are 32-bit): cut it (kaamer_text_cut_fastq)");
    if (line_cap < 1) line_cap = 1;
    if (line_cap > max_text_bytes + 1) line_cap = max_text_bytes + 1;
    HIPCHK(hipSetDevice(device));
    kaamer_text_parser *ps = new (std::nothrow) kaamer_text_parser();
    if (!ps) return kaamer_fail(KAAMER_E_NOMEM, "text parser");
    ps->device = device;
    ps->max_text = max_text_bytes;
    ps->rec_cap = max_records;
    ps->line_cap = (uint32_t)(line_cap > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : line_cap);
    ps->n_tiles_cap = (uint32_t)((max_text_bytes + PT_TILE - 1) / PT_TILE);
    ps->n_blk_cap = (uint32_t)(((uint64_t)ps->line_cap + PT_LINES - 1) / PT_LINES);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    ps->n_cu = e == hipSuccess ? prop.multiProcessorCount : 256;
    const size_t lc = ps->line_cap, nb = (size_t)ps->n_blk_cap + 1, nt = (size_t)ps->n_tiles_cap + 1;
    const size_t n32 = nt + (lc + 2) + (lc + 1) + 6 * nb;
    const size_t n64 = 3 * nb + ((size_t)max_records + 1) + PT_R_N;
    const int rc = reserve_group(nullptr, GROW_EXACT, { want(ps->d_u32, n32), want(ps->d_u64, n64), want(ps->d_seqs, (size_t)max_text_bytes + 2 * PT_PIECE),
                                                        want(ps->d_spans, (size_t)max_records + 1), want(ps->h_res, (size_t)PT_R_N) });
    if (rc) { delete ps; return rc; }
    PtParams &p = ps->p;
    uint32_t *a = ps->d_u32;
    p.tile_nl = a; a += nt;
    p.line_start = a; a += lc + 2;
    p.bad = a; a += lc + 1;
    p.blk_first = a; a += nb; p.blk_last_h = a; a += nb; p.blk_cnt = a; a += nb;
    p.blk_next = a; a += nb; p.blk_rec_base = a; a += nb; p.blk_h_before = a; a += nb;
    unsigned long long *b = ps->d_u64;
    p.blk_bytes = reinterpret_cast<uint64_t *>(b); b += nb;
    p.blk_tail = reinterpret_cast<uint64_t *>(b); b += nb;
    p.blk_byte_base = reinterpret_cast<uint64_t *>(b); b += nb;
    p.offsets = reinterpret_cast<uint64_t *>(b); b += (size_t)max_records + 1;
    p.res = b;
    p.seqs = ps->d_seqs; p.spans = ps->d_spans;
    p.line_cap = ps->line_cap; p.rec_cap = ps->rec_cap;
    *out = ps;
    return KAAMER_OK;
}

int kaamer_text_parser_create(int device, uint64_t max_text_bytes, uint32_t max_records, kaamer_text_parser **out)
{
    return text_parser_create_lines(device, max_text_bytes, max_records, pt_default_line_cap(max_text_bytes, max_records), out);
}

void kaamer_text_parser_geometry(uint32_t out[4])
{
    if (!out) return;
    out[0] = PT_PIECE; out[1] = PT_WAVE_STEP; out[2] = PT_TILE; out[3] = PT_LINES;
}

int kaamer_parse_fastq_device(kaamer_text_parser *ps, const uint8_t *d_text, uint64_t n_bytes, void *stream)
{
    if (!ps || (!d_text && n_bytes)) return kaamer_fail(KAAMER_E_ARG, "parse_fastq_device: bad argument");
    if (n_bytes > ps->max_text) return kaamer_fail(KAAMER_E_ARG, "parse_fastq_device: %llu bytes of text, the parser was created for %llu",
                                                   (unsigned long long)n_bytes, (unsigned long long)ps->max_text);
    if ((uintptr_t)d_text & (PT_PIECE - 1)) return kaamer_fail(KAAMER_E_ARG, "parse_fastq_device: the text must start at a 16-byte boundary (any hipMalloc'd buffer does)");
    HIPCHK(hipSetDevice(ps->device));
    hipStream_t s = (hipStream_t)stream;
    PtParams p = ps->p;
    p.text = d_text;
    p.n = (uint32_t)n_bytes;
    p.n_tiles = (uint32_t)((n_bytes + PT_TILE - 1) / PT_TILE);
    // lines this text can have at most, within the parser's bound: sizes the flag reset and the per-line grids
    const uint64_t line_bound = n_bytes + 1 < ps->line_cap ? n_bytes + 1 : ps->line_cap;
    const uint32_t n_blk = (uint32_t)((line_bound + PT_LINES - 1) / PT_LINES);
    HIPCHK(hipMemsetAsync(p.res, 0, PT_R_N * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(p.bad, 0, (size_t)(line_bound + 1) * sizeof(uint32_t), s));
    if (p.n_tiles) hipLaunchKernelGGL(pt_count_kernel, dim3(p.n_tiles), dim3(PT_BLOCK), 0, s, p);
    hipLaunchKernelGGL(pt_tile_scan_kernel, dim3(1), dim3(PT_LINES), 0, s, p);
    if (p.n_tiles) hipLaunchKernelGGL(pt_lines_kernel, dim3(p.n_tiles), dim3(PT_BLOCK), 0, s, p);
    hipLaunchKernelGGL(pt_records_kernel<false>, dim3(n_blk), dim3(PT_LINES), 0, s, p);
    hipLaunchKernelGGL(pt_block_scan_kernel, dim3(1), dim3(PT_LINES), 0, s, p);
    hipLaunchKernelGGL(pt_records_kernel<true>, dim3(n_blk), dim3(PT_LINES), 0, s, p);
    if (n_bytes) {
        uint64_t g = (n_bytes / PT_PIECE + PT_BLOCK - 1) / PT_BLOCK;
        const uint64_t g_max = (uint64_t)ps->n_cu * 8;
        if (g > g_max) g = g_max;
        if (g < 1) g = 1;
        hipLaunchKernelGGL(pt_gather_kernel, dim3((uint32_t)g), dim3(PT_BLOCK), 0, s, p);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ps->h_res, p.res, PT_R_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    ps->parsed = true;
    ps->fasta = false;
    return KAAMER_OK;
}

int kaamer_text_parser_finish(kaamer_text_parser *ps, void *stream, kaamer_text_parse_result *out)
{
    if (!ps || !out) return kaamer_fail(KAAMER_E_ARG, "text_parser_finish: bad argument");
    memset(out, 0, sizeof *out);
    if (!ps->parsed) return kaamer_fail(KAAMER_E_ARG, "text_parser_finish: nothing was parsed");
    HIPCHK(hipSetDevice(ps->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    const unsigned long long st = ps->h_res[PT_R_STATUS];
    const char *who = ps->fasta ? "parse_fasta_device" : "parse_fastq_device";
    if (st & PT_ST_LINES)
        return kaamer_fail(KAAMER_E_CAPACITY, "%s: %llu lines, the parser holds %u (max_records %u): create it for more records%s", who,
                           ps->h_res[PT_R_NL], ps->line_cap, ps->rec_cap, ps->fasta ? " or more lines (kaamer_text_parser_create_lines)" : "");
    if (st & PT_ST_RECORDS)
        return kaamer_fail(KAAMER_E_CAPACITY, "%s: %llu records, the parser holds %u", who, ps->h_res[PT_R_RECORDS], ps->rec_cap);
    out->n_records = (uint32_t)ps->h_res[PT_R_RECORDS];
    out->n_lines = ps->h_res[PT_R_LINES];
    out->seq_bytes = ps->h_res[PT_R_SEQ_BYTES];
    out->d_seqs = ps->d_seqs;
    out->d_offsets = ps->p.offsets;
    out->d_spans = ps->d_spans;
    return KAAMER_OK;
}

}  // extern "C"
