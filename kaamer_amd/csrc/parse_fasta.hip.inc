// parse_fasta.hip.inc — GetQueriesFasta (search.go:222-322) on the device: raw FASTA text in HBM -> the packed batch
// kaamer_search_device takes, plus one span per record (included by search.hip after parse_text.hip.inc, whose parser
// object, tiling, count / tile-scan kernels, scans and result words it shares).
//
// The rules, stated per line (the header repeats them next to kaamer_parse_fasta_device; RecordParser in host_search.cpp
// is the host's statement of the same reader):
//   lines    as for FASTQ: split at '\n', a last piece without '\n' is a line, one trailing '\r' is dropped
//   trim     leading and trailing bytes out of ' ' \t \n \v \f \r leave a non-header line (the host's is_space: ASCII only)
//   class    H  non-empty after the '\r' drop and the first byte is '>' (tested before any trim)
//            S  any other line with a byte left after the trim
//            X  empty and whitespace-only lines (ignored)
//   records  a maximal run of S lines with no H line between them: the concatenation of their trimmed bytes; the name is
//            what follows the '>' of the nearest preceding H line (only the '\r' dropped), empty when there is none
//   case     a-z -> A-Z in every record that an H line closes (search.go:295); the record still pending at the text's end
//            is copied as it is (:313-320) -- "every record but the last", except that a last record with a header line
//            behind it is upper-cased like the others; with upper_last the pending one is upper-cased too
//
// Seven launches on one stream, as for FASTQ (the first two ARE the FASTQ kernels):
//   pt_count_kernel, pt_tile_scan_kernel
//   pf_lines_kernel      per tile: where every line starts, and BY POSITION the first and the last non-space byte of every
//                        line: a lane looks at its own 16 bytes, the run of lanes that lie in one line is reduced in the
//                        wave (a segmented shuffle scan), and one lane per wave and line issues the atomic min / max
//   pf_records_kernel<0> per PT_LINES lines: class and kept bytes of every line, the record starts decided inside the block,
//                        the block's summary (last non-X class, last H line, kept bytes, "the first non-X line is an S")
//   pf_block_scan_kernel one workgroup: the class before every block, record and byte bases, totals
//   pf_records_kernel<1> per PT_LINES lines again: the destination offset of EVERY line, offsets[] and spans[] at record
//                        starts, the record's end through one atomic max per record and block
//   pf_gather_kernel     BY DESTINATION: every lane fills 16 bytes of the packed buffer, finding its source line by binary
//                        search in the per-line destination offsets, crossing as many lines as the piece needs
enum { PF_NONE = 0xFFFFFFFFu };

struct PfParams {
    PtParams pt;             // bad[] holds line_end (below); blk_first: the block's last non-X class; blk_next: the class before
                             // the block; blk_tail: the block's first non-X line is an S
    uint32_t *line_first;    // position of line i's first non-space byte (PF_NONE: none); line_cap + 2
    uint32_t *line_end;      // one past its last non-space byte (0: none)
    uint32_t *line_dst;      // where line i's kept bytes go in the packed buffer (lines that keep nothing: their successor's)
    uint32_t *rec_end;       // one past the last kept byte of record r, as a text position; rec_cap + 1
    uint32_t *last_cls;      // one word: the class of the text's last non-X line (PT_S: its last record is still pending)
    uint32_t upper_last;
};

__device__ __forceinline__ bool pf_is_space(uint32_t c) { return c == ' ' || (c - 9u) <= 4u; }   // ' ' \t \n \v \f \r

// a-z -> A-Z in the four bytes of w (bytes >= 0x80 stay)
__device__ __forceinline__ uint32_t pf_upper4(uint32_t w)
{
    const uint32_t l = w & 0x7F7F7F7Fu;
    const uint32_t ge_a = l + 0x1F1F1F1Fu, gt_z = l + 0x05050505u;   // bit 7 of a byte: >= 'a' / > 'z' (no carry leaves a byte)
    return w - ((ge_a & ~gt_z & ~w & 0x80808080u) >> 2);
}

__global__ __launch_bounds__(PT_BLOCK) void pf_lines_kernel(PfParams f)
{
    __shared__ uint32_t wsum[PT_BLOCK / 64];
    const PtParams &p = f.pt;
    if (p.res[PT_R_STATUS]) return;
    const uint32_t tile = blockIdx.x;
    const int lane = threadIdx.x & 63;
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
        uint32_t mn = PF_NONE, mx = 0;        // non-space bytes of the line the lane is in: first, last + 1
#pragma unroll
        for (int b = 0; b < PT_PIECE; b++) {
            const uint32_t c = pt_piece_byte(v, b);
            if ((uint32_t)b >= nv) {
                // (beyond the text)
            } else if (c == '\n') {
                // the line ends in this piece: at most one lane of the text closes it
                if (mx && line <= p.line_cap) { atomicMin(&f.line_first[line], mn); atomicMax(&f.line_end[line], mx); }
                mn = PF_NONE; mx = 0;
                line++;
                if (line <= p.line_cap) p.line_start[line] = pos + (uint32_t)b + 1u;
            } else if (!pf_is_space(c)) {
                if (mn == PF_NONE) mn = pos + (uint32_t)b;
                mx = pos + (uint32_t)b + 1u;
            }
        }
        // what is left belongs to the line that goes on in the next lane: lines only grow along the wave, so the lanes of one
        // line are a run, reduced by a segmented scan; the run's last lane holds its min / max and issues the two atomics
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ol = __shfl_up(line, d, 64), on = __shfl_up(mn, d, 64), ox = __shfl_up(mx, d, 64);
            if (lane >= d && ol == line) { mn = on < mn ? on : mn; mx = ox > mx ? ox : mx; }
        }
        const uint32_t next_line = __shfl_down(line, 1, 64);
        if ((lane == 63 || next_line != line) && mx && line <= p.line_cap) {
            atomicMin(&f.line_first[line], mn);
            atomicMax(&f.line_end[line], mx);
        }
    }
}

struct PfLast { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return b ? b : a; } };   // the later non-X class

template <bool EMIT> __global__ __launch_bounds__(PT_LINES) void pf_records_kernel(PfParams f)
{
    __shared__ uint32_t lds[PT_LINES];
    const PtParams &p = f.pt;
    if (p.res[PT_R_STATUS]) return;
    const unsigned long long nl = p.res[PT_R_NL];
    const uint32_t blk = blockIdx.x;
    if ((unsigned long long)blk * PT_LINES >= nl) return;
    const int t = threadIdx.x;
    const unsigned long long i64 = (unsigned long long)blk * PT_LINES + t;
    const uint32_t i = (uint32_t)i64;
    uint32_t cls = PT_X, first = 0, end = 0, kept = 0;
    if (i64 < nl) {
        uint32_t start;
        const uint32_t len = pt_line_len(p, i, start);
        if (len && p.text[start] == '>') cls = PT_H;
        else {
            first = f.line_first[i]; end = f.line_end[i];
            if (end) { cls = PT_S; kept = end - first; }
        }
    }
    // the class of the previous non-X line: inside the block, else what precedes the block (known on the second pass)
    (void)pt_scan<false>(cls, lds, PfLast());
    uint32_t prev = t ? lds[t - 1] : 0u;
    const uint32_t last_in_block = lds[PT_LINES - 1];
    const bool undecided = cls == PT_S && prev == 0;   // at most the block's first non-X line
    if (EMIT && prev == 0) prev = p.blk_next[blk];
    const bool rec = cls == PT_S && (EMIT ? prev != PT_S : prev == PT_H);
    uint32_t h = pt_scan<false>(cls == PT_H ? i + 1u : 0u, lds, PtMax32());
    const uint32_t last_h_in_block = lds[PT_LINES - 1];
    const uint32_t cnt_incl = pt_scan<false>(rec ? 1u : 0u, lds, PtAdd32());
    const uint32_t cnt_total = lds[PT_LINES - 1];
    // (a text has fewer than 2^32 bytes, so every byte sum fits 32 bits)
    const uint32_t bytes_incl = pt_scan<false>(kept, lds, PtAdd32());
    const uint32_t bytes_total = lds[PT_LINES - 1];
    if (!EMIT) {
        if (t == 0) {
            p.blk_first[blk] = last_in_block;
            p.blk_last_h[blk] = last_h_in_block;
            p.blk_cnt[blk] = cnt_total;
            p.blk_bytes[blk] = bytes_total;
            p.blk_tail[blk] = 0;
        }
        __syncthreads();
        if (undecided) p.blk_tail[blk] = 1;
        return;
    }
    // the class of the next non-X line inside the block (0: none): the last S line of a record or of the block reports the
    // record's end -- one atomic per record and block, however many lines the record has
    (void)pt_scan<true>(cls, lds, PtFirst());
    const uint32_t next = t + 1 < PT_LINES ? lds[t + 1] : 0u;
    const uint32_t dst = (uint32_t)p.blk_byte_base[blk] + bytes_incl - kept;
    if (i64 < nl) f.line_dst[i] = dst;
    if (cls != PT_S) return;
    const unsigned long long r = (unsigned long long)p.blk_rec_base[blk] + cnt_incl - 1u;   // (an S line that starts no record follows one)
    if (r >= p.rec_cap) return;   // (the status word is set: pf_block_scan_kernel)
    if (next != PT_S) atomicMax(&f.rec_end[r], end);
    if (!rec) return;
    if (h == 0) h = p.blk_h_before[blk];
    kaamer_text_span sp;
    sp.name_off = 0; sp.name_len = 0; sp.seq_off = first; sp.seq_len = 0;   // seq_len: pf_gather_kernel, from rec_end
    if (h) {
        uint32_t hs;
        const uint32_t hl = pt_line_len(p, h - 1u, hs);   // (an H line has at least its '>')
        sp.name_off = hs + 1u; sp.name_len = hl - 1u;
    }
    p.spans[r] = sp;
    p.offsets[r] = dst;
}

__global__ __launch_bounds__(PT_LINES) void pf_block_scan_kernel(PfParams f)
{
    __shared__ uint32_t lds[PT_LINES];
    __shared__ uint32_t carry_cls_s, carry_cnt_s, carry_h_s, carry_bytes_s;
    const PtParams &p = f.pt;
    if (p.res[PT_R_STATUS]) return;
    const unsigned long long nl = p.res[PT_R_NL];
    const uint32_t nb = (uint32_t)((nl + PT_LINES - 1) / PT_LINES);
    const int t = threadIdx.x;
    if (t == 0) { carry_cls_s = 0; carry_cnt_s = 0; carry_h_s = 0; carry_bytes_s = 0; }
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += PT_LINES) {
        const uint32_t b = base + t;
        uint32_t last = 0, cnt = 0, lh = 0, bytes = 0, head_s = 0;
        if (b < nb) {
            last = p.blk_first[b]; cnt = p.blk_cnt[b]; lh = p.blk_last_h[b];
            bytes = (uint32_t)p.blk_bytes[b]; head_s = (uint32_t)p.blk_tail[b];
        }
        // the class of the last non-X line before every block
        const uint32_t cls_incl = pt_scan<false>(last, lds, PfLast());
        uint32_t prev = t ? lds[t - 1] : 0u;
        const uint32_t cls0 = carry_cls_s;
        if (!prev) prev = cls0;
        if (head_s && prev != PT_S) cnt++;   // the block's first non-X line starts a record after all
        const uint32_t cnt_incl = pt_scan<false>(cnt, lds, PtAdd32());
        const uint32_t c0 = carry_cnt_s;
        const uint32_t h_incl = pt_scan<false>(lh, lds, PtMax32());
        const uint32_t h_excl = t ? lds[t - 1] : 0u;
        const uint32_t h0 = carry_h_s;
        const uint32_t bytes_incl = pt_scan<false>(bytes, lds, PtAdd32());
        const uint32_t b0 = carry_bytes_s;
        if (b < nb) {
            p.blk_next[b] = prev;
            p.blk_rec_base[b] = c0 + cnt_incl - cnt;
            p.blk_byte_base[b] = b0 + bytes_incl - bytes;
            p.blk_h_before[b] = h_excl > h0 ? h_excl : h0;
        }
        __syncthreads();
        if (t == PT_LINES - 1) {
            carry_cls_s = cls_incl ? cls_incl : cls0; carry_cnt_s = c0 + cnt_incl;
            carry_h_s = h_incl > h0 ? h_incl : h0; carry_bytes_s = b0 + bytes_incl;
        }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t n_rec = carry_cnt_s;   // < 2^31: a record takes two bytes of text
        p.res[PT_R_RECORDS] = n_rec;
        p.res[PT_R_SEQ_BYTES] = carry_bytes_s;
        if (n_rec > p.rec_cap) p.res[PT_R_STATUS] = PT_ST_RECORDS;
        else {
            p.offsets[n_rec] = carry_bytes_s;
            f.line_dst[(uint32_t)nl] = carry_bytes_s;   // (nl <= line_cap: pt_tile_scan_kernel)
            *f.last_cls = carry_cls_s;
        }
    }
}

// 16 bytes of the packed buffer per lane.  The buffer holds 16 bytes more than the text, so the last piece is stored whole.
__global__ __launch_bounds__(PT_BLOCK) void pf_gather_kernel(PfParams f)
{
    const PtParams &p = f.pt;
    if (p.res[PT_R_STATUS]) return;
    const uint32_t n_rec = (uint32_t)p.res[PT_R_RECORDS];
    if (!n_rec) return;
    const uint32_t nl = (uint32_t)p.res[PT_R_NL];
    const uint32_t total = (uint32_t)p.res[PT_R_SEQ_BYTES];
    const uint64_t stride = (uint64_t)gridDim.x * PT_BLOCK, tid = (uint64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    for (uint64_t r = tid; r < n_rec; r += stride) p.spans[r].seq_len = f.rec_end[r] - p.spans[r].seq_off;
    // the packed bytes from here on keep their case: the last record, when no header line closes it and no input follows
    const uint32_t as_is_from = (f.upper_last || *f.last_cls != PT_S) ? PF_NONE : (uint32_t)p.offsets[n_rec - 1];
    const uint64_t n_pieces = ((uint64_t)total + PT_PIECE - 1) / PT_PIECE;
    for (uint64_t k = tid; k < n_pieces; k += stride) {
        const uint32_t d = (uint32_t)(k * PT_PIECE);
        // the line that holds byte d: the last i with line_dst[i] <= d.  Lines that keep nothing share their successor's
        // offset, so it is never one of them (line_dst[nl] = total > d)
        uint32_t lo = 0, hi = nl - 1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (f.line_dst[mid] <= d) lo = mid; else hi = mid - 1;
        }
        uint32_t i = lo;
        uint32_t l_end = f.line_dst[i + 1];
        uint32_t src = f.line_first[i] + (d - f.line_dst[i]);
        uint32_t w[4] = {0, 0, 0, 0};
        const uint32_t a = src & ~3u;
        if (l_end - d >= (uint32_t)PT_PIECE && (uint64_t)a + 20 <= p.n) {
            // the whole piece lies in one line (the common case at 60-80 columns): five aligned words, shifted into place
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p.text + a);
            const uint32_t x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3], x4 = q[4];
            const uint32_t sh = (src & 3u) * 8u;
            w[0] = __funnelshift_r(x0, x1, sh); w[1] = __funnelshift_r(x1, x2, sh);
            w[2] = __funnelshift_r(x2, x3, sh); w[3] = __funnelshift_r(x3, x4, sh);
        } else {
#pragma unroll 1
            for (int b = 0; b < PT_PIECE; b++) {
                const uint32_t at = d + (uint32_t)b;
                if (at >= total) break;
                while (at >= l_end) {   // the next line that keeps a byte (at < total: there is one)
                    i++;
                    l_end = f.line_dst[i + 1];
                    src = f.line_first[i];
                }
                w[b >> 2] |= (uint32_t)p.text[src] << (8 * (b & 3));
                src++;
            }
        }
        if ((uint64_t)d + PT_PIECE <= as_is_from) {
#pragma unroll
            for (int q = 0; q < 4; q++) w[q] = pf_upper4(w[q]);
        } else if (d < as_is_from) {   // the piece straddles the start of the last record
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t at = d + 4u * q;
                const uint32_t m = at + 4u <= as_is_from ? 0xFFFFFFFFu : at >= as_is_from ? 0u : (1u << (8u * (as_is_from - at))) - 1u;
                w[q] = (pf_upper4(w[q]) & m) | (w[q] & ~m);
            }
        }
        *reinterpret_cast<uint4 *>(p.seqs + d) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ------------------------------------------------------------------------------------------------------------------
extern "C" {

int kaamer_text_parser_create_lines(int device, uint64_t max_text_bytes, uint32_t max_records, uint64_t max_lines, kaamer_text_parser **out)
{
    const uint64_t dflt = pt_default_line_cap(max_text_bytes, max_records);
    return text_parser_create_lines(device, max_text_bytes, max_records, max_lines > dflt ? max_lines : dflt, out);
}

int kaamer_parse_fasta_device(kaamer_text_parser *ps, const uint8_t *d_text, uint64_t n_bytes, int32_t upper_last, void *stream)
{
    if (!ps || (!d_text && n_bytes)) return kaamer_fail(KAAMER_E_ARG, "parse_fasta_device: bad argument");
    if (n_bytes > ps->max_text) return kaamer_fail(KAAMER_E_ARG, "parse_fasta_device: %llu bytes of text, the parser was created for %llu",
                                                   (unsigned long long)n_bytes, (unsigned long long)ps->max_text);
    if ((uintptr_t)d_text & (PT_PIECE - 1)) return kaamer_fail(KAAMER_E_ARG, "parse_fasta_device: the text must start at a 16-byte boundary (any hipMalloc'd buffer does)");
    HIPCHK(hipSetDevice(ps->device));
    const size_t lc = ps->line_cap;
    hipStream_t s = (hipStream_t)stream;
    {   // the words only FASTA needs, at the parser's first FASTA text
        const int rc = reserve(ps->d_fa, 2 * (lc + 2) + (size_t)ps->rec_cap + 1 + 1, GROW_EXACT, s);
        if (rc) return rc;
    }
    PfParams f;
    f.pt = ps->p;
    PtParams &p = f.pt;
    p.text = d_text;
    p.n = (uint32_t)n_bytes;
    p.n_tiles = (uint32_t)((n_bytes + PT_TILE - 1) / PT_TILE);
    f.line_first = ps->d_fa;
    f.line_dst = ps->d_fa + (lc + 2);
    f.rec_end = ps->d_fa + 2 * (lc + 2);
    f.last_cls = f.rec_end + (size_t)ps->rec_cap + 1;
    f.line_end = p.bad;   // (line_cap + 1 words, zeroed below as FASTQ's flags are)
    f.upper_last = upper_last ? 1u : 0u;
    const uint64_t line_bound = n_bytes + 1 < ps->line_cap ? n_bytes + 1 : ps->line_cap;
    const uint32_t n_blk = (uint32_t)((line_bound + PT_LINES - 1) / PT_LINES);
    const uint64_t rec_bound = n_bytes / 2 + 1 < ps->rec_cap ? n_bytes / 2 + 1 : ps->rec_cap;
    HIPCHK(hipMemsetAsync(p.res, 0, PT_R_N * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(f.line_end, 0, (size_t)(line_bound + 1) * sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(f.line_first, 0xFF, (size_t)(line_bound + 1) * sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(f.rec_end, 0, (size_t)(rec_bound + 1) * sizeof(uint32_t), s));
    if (p.n_tiles) hipLaunchKernelGGL(pt_count_kernel, dim3(p.n_tiles), dim3(PT_BLOCK), 0, s, p);
    hipLaunchKernelGGL(pt_tile_scan_kernel, dim3(1), dim3(PT_LINES), 0, s, p);
    if (p.n_tiles) hipLaunchKernelGGL(pf_lines_kernel, dim3(p.n_tiles), dim3(PT_BLOCK), 0, s, f);
    hipLaunchKernelGGL(pf_records_kernel<false>, dim3(n_blk), dim3(PT_LINES), 0, s, f);
    hipLaunchKernelGGL(pf_block_scan_kernel, dim3(1), dim3(PT_LINES), 0, s, f);
    hipLaunchKernelGGL(pf_records_kernel<true>, dim3(n_blk), dim3(PT_LINES), 0, s, f);
    if (n_bytes) {
        uint64_t g = (n_bytes / PT_PIECE + PT_BLOCK - 1) / PT_BLOCK;
        const uint64_t g_max = (uint64_t)ps->n_cu * 8;
        if (g > g_max) g = g_max;
        if (g < 1) g = 1;
        hipLaunchKernelGGL(pf_gather_kernel, dim3((uint32_t)g), dim3(PT_BLOCK), 0, s, f);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ps->h_res, p.res, PT_R_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    ps->parsed = true;
    ps->fasta = true;
    return KAAMER_OK;
}

}  // extern "C"
