// makedb_fasta.hip.inc — runFASTA + processProteinInputFASTA (pkg/makedb/inputFASTA.go:64-125, 195-250) on the device:
// the text of a database FASTA file in, the protein table out, the packed sequences left in HBM in the layout
// bd_windows_kernel reads (included by search.hip after parse_fasta.hip.inc: the tiling, the count / tile-scan kernels,
// the workgroup scans, pt_line_len and pf_upper4 are the parser's).  kaamer_makedb_fasta (makedb.cpp) is the host's
// statement of the same rules; they are NOT the query reader's:
//   lines    split at '\n', a last piece without '\n' is a line, one trailing '\r' is dropped, an empty line is skipped
//   class    H  the first byte is '>';  S  every other non-empty line.  Nothing is trimmed
//   entries  an H line and the S lines up to the next H line; S lines in front of the first H line are entry 0
//   ids      the entry the k-th H line opens is queued by the next H line under k + 1, the last one at the text's end under
//            N (with `more`: under N + 1), all of them on top of nb_before
//   header   EntryId: after '>' up to the line's first ' '; ProteinName: what follows that space
//   drops    ", partial" in the ProteinName; fewer than 7 sequence bytes.  A dropped entry takes no room anywhere
//
// Launches, all on the null stream, ordered by the end of each grid:
//   pt_count_kernel, pt_tile_scan_kernel   with a line bound of 0: they only count, every per-line buffer is sized from it
//   mf_lines_kernel      per tile, BY POSITION: where every line starts, the first ' ' of every line (runs of lanes inside
//                        one line are reduced in the wave), and the last ", partial" that starts in it (a lane that holds
//                        the ',' compares the eight bytes behind it wherever they lie: next piece, wave step or tile)
//   mf_entries_kernel<0> per PT_LINES lines: every H line whose next H line lies in the block decides its entry; the block's
//                        summary (H lines, bytes before the first and behind the last H line, what the decided entries keep)
//   mf_block_scan_kernel one workgroup: the bytes that follow every block up to the next H line, the decision of every
//                        block's last entry and of entry 0, then N and the record, byte, EntryId and name bases
//   mf_entries_kernel<1> per PT_LINES lines again: the destination of EVERY line, and ids / offsets / EntryId and name spans
//                        of the accepted entries
//   mf_gather_seq_kernel BY DESTINATION: 16 upper-cased bytes of the packed sequences per lane, the source line by binary
//                        search in the per-line destinations
//   mf_gather_bytes_kernel  twice, BY DESTINATION: the EntryId bytes and the name bytes, the record by binary search
enum { MF_R_HEADERS = 0, MF_R_RECORDS, MF_R_SEQ_BYTES, MF_R_ID_BYTES, MF_R_NAME_BYTES, MF_R_PRE, MF_R_N };
enum { MF_REJECTED = 1, MF_ACCEPTED = 2 };   // the decision of an entry, as the "last one wins" scans carry it (0: no H line)

struct MfParams {
    PtParams pt;             // text, n, n_tiles, tile_nl, line_start, line_cap (= the text's lines), res
    unsigned long long *res; // MF_R_*
    uint32_t *line_sp;       // position of line i's first ' ' (PF_NONE: none); lines + 1
    uint32_t *line_pm;       // one past the start of the last ", partial" that starts in line i (0: none)
    uint32_t *line_dst;      // where line i's bytes go in the packed sequences (lines that keep nothing: their successor's)
    // per block of PT_LINES lines, from mf_entries_kernel<0>
    uint32_t *blk_nh, *blk_head, *blk_tail, *blk_last_h;
    unsigned long long *blk_acc;     // bytes | records << 32 of the entries decided inside the block
    unsigned long long *blk_idname;  // EntryId bytes | name bytes << 32 of the same
    // ... and from mf_block_scan_kernel
    uint32_t *blk_follow, *blk_open, *blk_hord, *blk_rec_base, *blk_e, *blk_id_base, *blk_name_base;
    // the accepted entries
    uint32_t *ids, *id_src, *name_src;
    uint64_t *offsets, *id_off, *name_off;
    uint8_t *seqs;
    uint64_t nb_before;
    uint32_t more;
};

// what the H line i = [start, start + len) says: EntryId = [start + 1, +id_len), ProteinName = [name_src, +name_len)
__device__ __forceinline__ void mf_header(const MfParams &f, uint32_t i, uint32_t start, uint32_t len, uint32_t &id_len, uint32_t &name_src,
                                          uint32_t &name_len, bool &partial)
{
    const uint32_t end = start + len, sp = f.line_sp[i];   // (a ' ' of the line lies before the dropped '\r')
    if (sp == PF_NONE) { id_len = len - 1u; name_src = end; name_len = 0; partial = false; return; }
    id_len = sp - start - 1u;
    name_src = sp + 1u;
    name_len = end - sp - 1u;
    partial = f.line_pm[i] > sp + 1u;   // a match holds neither '\r' nor '\n': one that starts behind the space ends inside the name
}

__global__ __launch_bounds__(PT_BLOCK) void mf_lines_kernel(MfParams f)
{
    __shared__ uint32_t wsum[PT_BLOCK / 64];
    const PtParams &p = f.pt;
    const uint32_t tile = blockIdx.x;
    const int lane = threadIdx.x & 63;
    if (tile == 0 && threadIdx.x == 0) { p.line_start[0] = 0; p.line_start[p.line_cap] = p.n + 1u; }   // (the text's end as one more '\n')
    uint32_t carry = p.tile_nl[tile < p.n_tiles ? tile : p.n_tiles];
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
        uint32_t mn = PF_NONE;                // the first ' ' of the line the lane is in
#pragma unroll
        for (int b = 0; b < PT_PIECE; b++) {
            const uint32_t c = pt_piece_byte(v, b);
            if ((uint32_t)b >= nv) {
                // (beyond the text)
            } else if (c == '\n') {
                if (mn != PF_NONE && line < p.line_cap) atomicMin(&f.line_sp[line], mn);
                mn = PF_NONE;
                line++;
                if (line < p.line_cap) p.line_start[line] = pos + (uint32_t)b + 1u;
            } else if (c == ' ') {
                if (mn == PF_NONE) mn = pos + (uint32_t)b;
            } else if (c == ',') {
                const uint32_t q = pos + (uint32_t)b;
                if ((uint64_t)q + 9u <= p.n && line < p.line_cap) {
                    const uint8_t *s = p.text + q;
                    if (s[1] == ' ' && s[2] == 'p' && s[3] == 'a' && s[4] == 'r' && s[5] == 't' && s[6] == 'i' && s[7] == 'a' && s[8] == 'l')
                        atomicMax(&f.line_pm[line], q + 1u);
                }
            }
        }
        // what is left belongs to the line that goes on in the next lane: the lanes of one line are a run of the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ol = __shfl_up(line, d, 64), on = __shfl_up(mn, d, 64);
            if (lane >= d && ol == line) mn = on < mn ? on : mn;
        }
        const uint32_t next_line = __shfl_down(line, 1, 64);
        if ((lane == 63 || next_line != line) && mn != PF_NONE && line < p.line_cap) atomicMin(&f.line_sp[line], mn);
    }
}

struct MfAdd64 { __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; } };
// (an H line was seen) << 32 | bytes before the first H line, of a stretch of blocks: a (earlier) before b (later)
struct MfHead {
    __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const
    {
        return (a >> 32) ? a : ((b >> 32) << 32) | (uint32_t)((uint32_t)a + (uint32_t)b);
    }
};

template <bool EMIT> __global__ __launch_bounds__(PT_LINES) void mf_entries_kernel(MfParams f)
{
    __shared__ unsigned long long lds64[PT_LINES];
    uint32_t *lds = reinterpret_cast<uint32_t *>(lds64);
    const PtParams &p = f.pt;
    const unsigned long long nl = p.line_cap;
    const uint32_t blk = blockIdx.x;
    if ((unsigned long long)blk * PT_LINES >= nl) return;
    const int t = threadIdx.x;
    const unsigned long long i64 = (unsigned long long)blk * PT_LINES + t;
    const uint32_t i = (uint32_t)i64;
    uint32_t cls = PT_X, start = 0, len = 0;
    if (i64 < nl) {
        len = pt_line_len(p, i, start);
        if (len) cls = p.text[start] == '>' ? PT_H : PT_S;
    }
    const bool is_h = cls == PT_H;
    // the next H line inside the block, as thread + 1 (0: none)
    (void)pt_scan<true>(is_h ? (uint32_t)t + 1u : 0u, lds, PtFirst());
    const uint32_t first_h = lds[0];
    const uint32_t next_h = t + 1 < PT_LINES ? lds[t + 1] : 0u;
    // (a text has fewer than 2^32 bytes, so every byte sum fits 32 bits)
    const uint32_t b_incl = pt_scan<false>(cls == PT_S ? len : 0u, lds, PtAdd32());
    const uint32_t b_total = lds[PT_LINES - 1];
    const uint32_t head = first_h ? lds[first_h - 1u] : b_total;             // bytes before the block's first H line
    const uint32_t seg = is_h ? (next_h ? lds[next_h - 1u] : b_total) - b_incl : 0u;   // bytes from this H line to the next
    const bool last_h = is_h && !next_h;
    uint32_t id_len = 0, name_src = 0, name_len = 0;
    bool partial = false;
    if (is_h) mf_header(f, i, start, len, id_len, name_src, name_len, partial);
    // an entry is decided where its H line is: inside the block when the next H line is there too, else once the bytes that
    // follow the block are known (second pass)
    const uint32_t all = seg + (EMIT && last_h ? f.blk_follow[blk] : 0u);
    const bool acc = is_h && (EMIT || !last_h) && !partial && all >= (uint32_t)KAAMER_KMER_SIZE;
    if (!EMIT) {
        (void)pt_scan<false>((acc ? (unsigned long long)seg | (1ull << 32) : 0ull) + (is_h ? 1ull << 48 : 0ull), lds64, MfAdd64());
        const unsigned long long a_total = lds64[PT_LINES - 1];
        (void)pt_scan<false>(acc ? (unsigned long long)id_len | ((unsigned long long)name_len << 32) : 0ull, lds64, MfAdd64());
        const unsigned long long n_total = lds64[PT_LINES - 1];
        if (t == 0) {
            f.blk_nh[blk] = (uint32_t)(a_total >> 48);
            f.blk_head[blk] = head;
            f.blk_acc[blk] = a_total & 0xFFFFFFFFFFFFull;
            f.blk_idname[blk] = n_total;
            f.blk_tail[blk] = b_total;   // (no H line: all of the block, before and behind)
            f.blk_last_h[blk] = 0;
        }
        __syncthreads();
        if (last_h) { f.blk_tail[blk] = seg; f.blk_last_h[blk] = i + 1u; }
        return;
    }
    // the decision of the entry every line belongs to: the nearest H line's at or before it, else what is open at the block's start
    uint32_t code = pt_scan<false>(is_h ? (acc ? (uint32_t)MF_ACCEPTED : (uint32_t)MF_REJECTED) : 0u, lds, PfLast());
    if (!code) code = f.blk_open[blk];
    const uint32_t kept = (cls == PT_S && code == MF_ACCEPTED) ? len : 0u;
    const unsigned long long a_incl = pt_scan<false>((unsigned long long)kept + (acc ? 1ull << 32 : 0ull) + (is_h ? 1ull << 48 : 0ull), lds64, MfAdd64());
    const unsigned long long n_incl = pt_scan<false>(acc ? (unsigned long long)id_len | ((unsigned long long)name_len << 32) : 0ull, lds64, MfAdd64());
    const uint32_t dst = f.blk_e[blk] + (uint32_t)a_incl - kept;
    if (i64 < nl) f.line_dst[i] = dst;
    const unsigned long long n_hdr = f.res[MF_R_HEADERS];
    if (blk == 0 && t == 0) {
        const unsigned long long n_rec = f.res[MF_R_RECORDS];
        if (f.res[MF_R_PRE]) {   // entry 0: no header, so no EntryId and no name; queued by the first H line or by the text's end
            f.offsets[0] = 0; f.id_off[0] = 0; f.name_off[0] = 0; f.id_src[0] = 0; f.name_src[0] = 0;
            f.ids[0] = (uint32_t)(f.nb_before + ((f.more || n_hdr) ? 1ull : 0ull));
        }
        f.offsets[n_rec] = f.res[MF_R_SEQ_BYTES];
        f.id_off[n_rec] = f.res[MF_R_ID_BYTES];
        f.name_off[n_rec] = f.res[MF_R_NAME_BYTES];
        f.line_dst[(uint32_t)nl] = (uint32_t)f.res[MF_R_SEQ_BYTES];
    }
    if (!acc) return;
    const unsigned long long r = (unsigned long long)f.blk_rec_base[blk] + ((a_incl >> 32) & 0xFFFFu) - 1u;
    if (r >= f.res[MF_R_RECORDS]) return;   // (both passes decide alike, so this never holds: the buffers are sized from the first)
    const unsigned long long k = (unsigned long long)f.blk_hord[blk] + (a_incl >> 48);   // this H line is the k-th of the text
    f.ids[r] = (uint32_t)(f.nb_before + ((f.more || k < n_hdr) ? k + 1u : n_hdr));
    f.offsets[r] = dst;
    f.id_off[r] = (unsigned long long)f.blk_id_base[blk] + (uint32_t)n_incl - id_len;
    f.name_off[r] = (unsigned long long)f.blk_name_base[blk] + (uint32_t)(n_incl >> 32) - name_len;
    f.id_src[r] = start + 1u;
    f.name_src[r] = name_src;
}

__global__ __launch_bounds__(PT_LINES) void mf_block_scan_kernel(MfParams f)
{
    __shared__ unsigned long long lds64[PT_LINES];
    __shared__ unsigned long long carry64_s, carry_n_s;
    __shared__ uint32_t carry_open_s, carry_h_s;
    uint32_t *lds = reinterpret_cast<uint32_t *>(lds64);
    const PtParams &p = f.pt;
    const unsigned long long nl = p.line_cap;
    const uint32_t nb = (uint32_t)((nl + PT_LINES - 1) / PT_LINES);
    const int t = threadIdx.x;
    // the bytes that follow every block up to the next H line: a suffix scan, chunk by chunk from the end
    if (t == 0) carry64_s = 0;
    __syncthreads();
    for (uint32_t base = (nb - 1) / PT_LINES * PT_LINES;; base -= PT_LINES) {
        const uint32_t b = base + t;
        const unsigned long long v = b < nb ? ((unsigned long long)(f.blk_nh[b] ? 1u : 0u) << 32) | f.blk_head[b] : 0ull;
        (void)pt_scan<true>(v, lds64, MfHead());
        const unsigned long long carry = carry64_s;
        const unsigned long long behind = MfHead()(t + 1 < PT_LINES ? lds64[t + 1] : 0ull, carry);
        if (b < nb) f.blk_follow[b] = (uint32_t)behind;
        const unsigned long long whole = MfHead()(lds64[0], carry);
        __syncthreads();
        if (t == 0) carry64_s = whole;
        __syncthreads();
        if (base == 0) break;
    }
    // entry 0: the S lines in front of the first H line
    const uint32_t pre_bytes = (uint32_t)carry64_s;
    const bool pre = pre_bytes >= (uint32_t)KAAMER_KMER_SIZE;
    __syncthreads();
    if (t == 0) {
        carry64_s = pre ? 1ull << 32 : 0ull;   // accepted bytes in front of the block | records << 32
        carry_n_s = 0;                         // EntryId bytes | name bytes << 32
        carry_open_s = pre ? MF_ACCEPTED : MF_REJECTED;
        carry_h_s = 0;
    }
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += PT_LINES) {
        const uint32_t b = base + t;
        uint32_t nh = 0, head = 0, tail = 0, code = 0;
        unsigned long long a = 0, idname = 0;
        bool last_acc = false;
        if (b < nb) {
            nh = f.blk_nh[b]; head = f.blk_head[b]; tail = f.blk_tail[b];
            a = f.blk_acc[b]; idname = f.blk_idname[b];
            if (nh) {   // the block's last entry, now that the bytes behind the block are known
                const uint32_t h = f.blk_last_h[b] - 1u;
                uint32_t start, id_len, name_src, name_len;
                bool partial;
                const uint32_t len = pt_line_len(p, h, start);
                mf_header(f, h, start, len, id_len, name_src, name_len, partial);
                last_acc = !partial && tail + f.blk_follow[b] >= (uint32_t)KAAMER_KMER_SIZE;
                if (last_acc) { a += 1ull << 32; idname += (unsigned long long)id_len | ((unsigned long long)name_len << 32); }
                code = last_acc ? MF_ACCEPTED : MF_REJECTED;
            }
        }
        // the decision of the entry that is open where every block starts
        const uint32_t code_incl = pt_scan<false>(code, lds, PfLast());
        uint32_t open = t ? lds[t - 1] : 0u;
        const uint32_t open0 = carry_open_s;
        if (!open) open = open0;
        // the bytes the block's LINES keep: of its decided entries, of the entry open at its start, of its last entry
        if (open == MF_ACCEPTED) a += head;
        if (nh && last_acc) a += tail;
        const unsigned long long a_incl = pt_scan<false>(a, lds64, MfAdd64());
        const unsigned long long a0 = carry64_s;
        const unsigned long long n_incl = pt_scan<false>(idname, lds64, MfAdd64());
        const unsigned long long n0 = carry_n_s;
        const uint32_t h_incl = pt_scan<false>(nh, lds, PtAdd32());
        const uint32_t h0 = carry_h_s;
        if (b < nb) {
            f.blk_open[b] = open;
            f.blk_e[b] = (uint32_t)(a0 + a_incl - a);
            f.blk_rec_base[b] = (uint32_t)((a0 + a_incl - a) >> 32);
            f.blk_id_base[b] = (uint32_t)(n0 + n_incl - idname);
            f.blk_name_base[b] = (uint32_t)((n0 + n_incl - idname) >> 32);
            f.blk_hord[b] = h0 + h_incl - nh;
        }
        __syncthreads();
        if (t == PT_LINES - 1) {
            carry64_s = a0 + a_incl; carry_n_s = n0 + n_incl; carry_h_s = h0 + h_incl;
            carry_open_s = code_incl ? code_incl : open0;
        }
        __syncthreads();
    }
    if (t == 0) {
        f.res[MF_R_HEADERS] = carry_h_s;
        f.res[MF_R_RECORDS] = carry64_s >> 32;   // < 2^29: an accepted entry takes eight bytes of text
        f.res[MF_R_SEQ_BYTES] = (uint32_t)carry64_s;
        f.res[MF_R_ID_BYTES] = (uint32_t)carry_n_s;
        f.res[MF_R_NAME_BYTES] = carry_n_s >> 32;
        f.res[MF_R_PRE] = pre ? 1u : 0u;
    }
}

// 16 bytes of the packed sequences per lane, upper-cased.  The buffer holds 16 bytes more than it needs, so the last piece is
// stored whole.
__global__ __launch_bounds__(PT_BLOCK) void mf_gather_seq_kernel(MfParams f)
{
    const PtParams &p = f.pt;
    const uint32_t nl = p.line_cap;
    const uint32_t total = (uint32_t)f.res[MF_R_SEQ_BYTES];
    const uint64_t stride = (uint64_t)gridDim.x * PT_BLOCK, tid = (uint64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
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
        uint32_t src = p.line_start[i] + (d - f.line_dst[i]);
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
                while (at >= l_end && i + 1 < nl) {   // the next line that keeps a byte (at < total: there is one)
                    i++;
                    l_end = f.line_dst[i + 1];
                    src = p.line_start[i];
                }
                if (src < p.n) w[b >> 2] |= (uint32_t)p.text[src] << (8 * (b & 3));
                src++;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = pf_upper4(w[q]);
        *reinterpret_cast<uint4 *>(f.seqs + d) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// 16 bytes of a packed byte buffer per lane: record r's bytes are text[src[r] .. + off[r + 1] - off[r]) of the n-byte text
// (records may be empty).
// The buffer holds 16 bytes more than `total`.
__global__ __launch_bounds__(PT_BLOCK) void mf_gather_bytes_kernel(const uint8_t *__restrict__ text, uint32_t n, const uint64_t *__restrict__ off,
                                                                   const uint32_t *__restrict__ src_of, uint32_t n_rec, uint32_t total,
                                                                   uint8_t *__restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * PT_BLOCK, tid = (uint64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    const uint64_t n_pieces = ((uint64_t)total + PT_PIECE - 1) / PT_PIECE;
    for (uint64_t k = tid; k < n_pieces; k += stride) {
        const uint32_t d = (uint32_t)(k * PT_PIECE);
        // the record that holds byte d: the last r with off[r] <= d, which is never an empty one (off[n_rec] = total > d)
        uint32_t lo = 0, hi = n_rec - 1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (off[mid] <= d) lo = mid; else hi = mid - 1;
        }
        uint32_t r = lo;
        uint32_t r_end = (uint32_t)off[r + 1];
        uint32_t src = src_of[r] + (d - (uint32_t)off[r]);
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int b = 0; b < PT_PIECE; b++) {
            const uint32_t at = d + (uint32_t)b;
            if (at >= total) break;
            while (at >= r_end && r + 1 < n_rec) {   // the next record that holds a byte (at < total: there is one)
                r++;
                r_end = (uint32_t)off[r + 1];
                src = src_of[r];
            }
            if (src < n) w[b >> 2] |= (uint32_t)text[src] << (8 * (b & 3));
            src++;
        }
        *reinterpret_cast<uint4 *>(out + d) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// One text's reader: its buffers live for the call.  After mf_read the accepted entries lie on the device: d_seqs (32 bytes
// of slack behind the last residue, as bd_windows_kernel wants), offsets, ids, and the EntryId / name bytes with their offsets.
struct MfReader {
    int device = 0;
    DevBuf<uint8_t> d_text, d_seqs, d_idb, d_nameb;
    DevBuf<uint32_t> d_cnt32, d_line32, d_rec32;
    DevBuf<unsigned long long> d_res, d_blk64, d_rec64;
    MfParams f{};
    uint64_t n_headers = 0, n_rec = 0, seq_bytes = 0, id_bytes = 0, name_bytes = 0;
    ~MfReader() { (void)hipSetDevice(device); }   // (before the buffers go)
};

// KAAMER_MAKEDB_TRACE: a reader's stages by HIP events, on stderr
struct MfTrace {
    bool on = getenv("KAAMER_MAKEDB_TRACE") != nullptr;
    const char *format = "fasta";   // (makedb_tsv.hip.inc: "tsv")
    uint64_t bytes = 0;
    hipEvent_t a = nullptr, b = nullptr;
    ~MfTrace() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void begin() { if (on && !a) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); } if (on) (void)hipEventRecord(a, 0); }
    void lap(const char *what)
    {
        if (!on) return;
        float ms = 0;
        (void)hipEventRecord(b, 0);
        (void)hipEventSynchronize(b);
        (void)hipEventElapsedTime(&ms, a, b);
        fprintf(stderr, "[kaamer makedb %s] %-16s %9.3f ms  %8.2f GB/s of text\n", format, what, ms, ms > 0 ? (double)bytes / ms * 1e-6 : 0.0);
        (void)hipEventRecord(a, 0);
    }
};

static unsigned mf_grid(uint64_t bytes, int n_cu)
{
    uint64_t g = (bytes / PT_PIECE + PT_BLOCK - 1) / PT_BLOCK;
    const uint64_t g_max = (uint64_t)n_cu * 8;
    if (g > g_max) g = g_max;
    return (unsigned)(g < 1 ? 1 : g);
}

static int mf_read(MfReader &m, const char *text, uint64_t len, uint64_t nb_before, int32_t more, int device)
{
    HIPCHK(hipSetDevice(device));
    m.device = device;
    hipDeviceProp_t prop;
    const int n_cu = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
    MfTrace tr;
    tr.bytes = len;
    tr.begin();
    const uint32_t n_tiles = (uint32_t)((len + PT_TILE - 1) / PT_TILE);
    int rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_text, (size_t)len + 2 * PT_PIECE), want(m.d_cnt32, (size_t)n_tiles + 1 + 2),
                                                  want(m.d_res, (size_t)PT_R_N + MF_R_N) });
    if (rc) return rc;
    if (len) HIPCHK(hipMemcpy(m.d_text, text, (size_t)len, hipMemcpyHostToDevice));
    tr.lap("upload");
    MfParams &f = m.f;
    PtParams &p = f.pt;
    p.text = m.d_text;
    p.n = (uint32_t)len;
    p.n_tiles = n_tiles;
    p.tile_nl = m.d_cnt32;
    p.line_start = m.d_cnt32 + n_tiles + 1;   // two words: with a line bound of 0 the tile scan only counts
    p.line_cap = 0;
    p.res = m.d_res;
    f.res = m.d_res + PT_R_N;
    f.nb_before = nb_before;
    f.more = more ? 1u : 0u;
    HIPCHK(hipMemset(m.d_res, 0, (PT_R_N + MF_R_N) * sizeof(unsigned long long)));
    if (n_tiles) hipLaunchKernelGGL(pt_count_kernel, dim3(n_tiles), dim3(PT_BLOCK), 0, 0, p);
    hipLaunchKernelGGL(pt_tile_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, p);
    HIPCHK(hipGetLastError());
    unsigned long long h_res[PT_R_N + MF_R_N];
    HIPCHK(hipMemcpy(h_res, m.d_res, sizeof h_res, hipMemcpyDeviceToHost));
    tr.lap("count lines");
    const unsigned long long nl = h_res[PT_R_NL];
    if (nl < 1 || nl > 0xFFFFFFF0ull) return kaamer_fail(KAAMER_E_CAPACITY, "makedb_fasta_device: %llu lines in one text: cut it (kaamer_text_cut_fasta)", nl);
    const size_t nb = (size_t)((nl + PT_LINES - 1) / PT_LINES) + 1;
    rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_line32, 4 * ((size_t)nl + 2) + 11 * nb), want(m.d_blk64, 2 * nb) });
    if (rc) return rc;
    {
        uint32_t *a = m.d_line32;
        p.line_start = a; a += nl + 2;
        f.line_sp = a; a += nl + 2;
        f.line_pm = a; a += nl + 2;
        f.line_dst = a; a += nl + 2;
        f.blk_nh = a; a += nb; f.blk_head = a; a += nb; f.blk_tail = a; a += nb; f.blk_last_h = a; a += nb;
        f.blk_follow = a; a += nb; f.blk_open = a; a += nb; f.blk_hord = a; a += nb; f.blk_rec_base = a; a += nb;
        f.blk_e = a; a += nb; f.blk_id_base = a; a += nb; f.blk_name_base = a; a += nb;
        f.blk_acc = m.d_blk64;
        f.blk_idname = m.d_blk64 + nb;
    }
    p.line_cap = (uint32_t)nl;
    HIPCHK(hipMemset(f.line_sp, 0xFF, ((size_t)nl + 2) * sizeof(uint32_t)));
    HIPCHK(hipMemset(f.line_pm, 0, ((size_t)nl + 2) * sizeof(uint32_t)));
    const uint32_t n_blk = (uint32_t)(nb - 1);
    hipLaunchKernelGGL(mf_lines_kernel, dim3(n_tiles ? n_tiles : 1u), dim3(PT_BLOCK), 0, 0, f);
    tr.lap("lines");
    hipLaunchKernelGGL(mf_entries_kernel<false>, dim3(n_blk), dim3(PT_LINES), 0, 0, f);
    hipLaunchKernelGGL(mf_block_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, f);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(h_res, m.d_res, sizeof h_res, hipMemcpyDeviceToHost));
    tr.lap("entries");
    const unsigned long long *r = h_res + PT_R_N;
    m.n_headers = r[MF_R_HEADERS]; m.n_rec = r[MF_R_RECORDS]; m.seq_bytes = r[MF_R_SEQ_BYTES];
    m.id_bytes = r[MF_R_ID_BYTES]; m.name_bytes = r[MF_R_NAME_BYTES];
    const size_t n = (size_t)m.n_rec;
    rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_rec32, 3 * (n + 1)), want(m.d_rec64, 3 * (n + 1)),
                                              want(m.d_seqs, (size_t)m.seq_bytes + 3 * PT_PIECE), want(m.d_idb, (size_t)m.id_bytes + 2 * PT_PIECE),
                                              want(m.d_nameb, (size_t)m.name_bytes + 2 * PT_PIECE) });
    if (rc) return rc;
    f.ids = m.d_rec32; f.id_src = m.d_rec32 + (n + 1); f.name_src = m.d_rec32 + 2 * (n + 1);
    f.offsets = reinterpret_cast<uint64_t *>(m.d_rec64.get());
    f.id_off = f.offsets + (n + 1); f.name_off = f.offsets + 2 * (n + 1);
    f.seqs = m.d_seqs;
    {   // (the builder's window kernel reads up to 17 bytes behind the last residue: they are zero, not left-over)
        const size_t whole = (size_t)(m.seq_bytes / PT_PIECE) * PT_PIECE;
        HIPCHK(hipMemset(m.d_seqs + whole, 0, (size_t)m.seq_bytes - whole + 3 * PT_PIECE));
    }
    hipLaunchKernelGGL(mf_entries_kernel<true>, dim3(n_blk), dim3(PT_LINES), 0, 0, f);
    tr.lap("entries, emit");
    if (m.seq_bytes) hipLaunchKernelGGL(mf_gather_seq_kernel, dim3(mf_grid(m.seq_bytes, n_cu)), dim3(PT_BLOCK), 0, 0, f);
    tr.lap("gather sequences");
    if (m.id_bytes) hipLaunchKernelGGL(mf_gather_bytes_kernel, dim3(mf_grid(m.id_bytes, n_cu)), dim3(PT_BLOCK), 0, 0, p.text, p.n, f.id_off, f.id_src,
                                       (uint32_t)n, (uint32_t)m.id_bytes, m.d_idb.get());
    if (m.name_bytes) hipLaunchKernelGGL(mf_gather_bytes_kernel, dim3(mf_grid(m.name_bytes, n_cu)), dim3(PT_BLOCK), 0, 0, p.text, p.n, f.name_off, f.name_src,
                                         (uint32_t)n, (uint32_t)m.name_bytes, m.d_nameb.get());
    HIPCHK(hipGetLastError());
    tr.lap("gather headers");
    return KAAMER_OK;
}

// the host's table of what mf_read left on the device: bulk copies into the table's arrays, then makedb.cpp's by_id and KStats
static int mf_table(MfReader &m, kaamer_proteins **out)
{
    MfTrace tr;
    tr.bytes = m.f.pt.n;
    tr.begin();
    kaamer_table_arrays a;
    kaamer_proteins *t = kaamer_proteins_table_new({ "ProteinName" }, (uint32_t)m.n_rec, m.seq_bytes, m.id_bytes, m.name_bytes, &a);   // FASTA_DEF_FTS, inputFASTA.go:41
    if (!t) return kaamer_fail(KAAMER_E_NOMEM, "makedb_fasta_device: the table");
    const size_t n = (size_t)m.n_rec;
    hipError_t e = hipSuccess;
    auto get = [&](void *dst, const void *src, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); };
    get(a.ids, m.f.ids, n * 4);
    get(a.offsets, m.f.offsets, (n + 1) * 8);
    get(a.seqs, m.d_seqs, (size_t)m.seq_bytes);
    get(a.entry_off, m.f.id_off, (n + 1) * 8);
    get(a.entry_ids, m.d_idb, (size_t)m.id_bytes);
    get(a.feature_off, m.f.name_off, (n + 1) * 8);
    get(a.features, m.d_nameb, (size_t)m.name_bytes);
    if (e != hipSuccess) { kaamer_proteins_free(t); return kaamer_fail(KAAMER_E_HIP, "makedb_fasta_device: download: %s", hipGetErrorString(e)); }
    tr.lap("download");
    kaamer_proteins_table_seal(t);
    *out = t;
    return KAAMER_OK;
}

// the index over a table that was built on its device (kaamer_index_build_proteins, kaamer_index_build_fasta); on failure
// di's two allocations are freed
static int index_of_device_image(const kaamer_device_image &di, int device, kaamer_index **out)
{
    kaamer_index *ix = new (std::nothrow) kaamer_index();
    if (!ix) { (void)hipFree(di.d_buckets); (void)hipFree(di.d_arena); return kaamer_fail(KAAMER_E_NOMEM, "index alloc"); }
    ix->device = device;
    ix->n_top = read_knobs().host_slots;
    ix->hdr = di.hdr;
    ix->d_buckets = di.d_buckets;
    ix->d_arena = di.d_arena;   // its first 16 bytes are zero (builder_device.hip), as kaamer_index_open_image leaves them
    *out = ix;
    return KAAMER_OK;
}

extern "C" {

int kaamer_makedb_fasta_device(const char *text, uint64_t len, uint64_t nb_before, int32_t more, int device, kaamer_proteins **out)
{
    if (len > 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_ARG, "makedb_fasta_device: a text holds at most 2^32 - 1 bytes: cut it (kaamer_text_cut_fasta)");
    if (!out || (!text && len)) return kaamer_fail(KAAMER_E_ARG, "makedb_fasta_device: bad argument");
    *out = nullptr;
    MfReader m;
    const int rc = mf_read(m, text, len, nb_before, more, device);
    if (rc) return rc;
    return mf_table(m, out);
}

// the arguments of the calls that build from a text (`cut`: where such a text may be cut)
static int mf_build_args(const char *who, const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, const void *proteins, const void *out,
                         const char *cut = "(kaamer_text_cut_fasta)")
{
    if (len > 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_ARG, "%s: a text holds at most 2^32 - 1 bytes: cut it %s", who, cut);
    if (!proteins || !out || (!text && len) || n_shards == 0 || shard >= n_shards) return kaamer_fail(KAAMER_E_ARG, "%s: bad argument", who);
    return KAAMER_OK;
}

// text -> the reader's buffers -> the build that takes device buffers -> the table's host copy
static int mf_build(MfReader &m, const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                    kaamer_proteins **proteins, kaamer_device_image *di)
{
    int rc = mf_read(m, text, len, 0, 0, device);
    if (rc) return rc;
    m.d_text.reset(); m.d_cnt32.reset(); m.d_line32.reset(); m.d_blk64.reset();   // (the build wants the room; hipFree waits for the gathers)
    rc = kaamer_build_resident(m.d_seqs, m.f.offsets, m.f.ids, (uint32_t)m.n_rec, m.seq_bytes, shard, n_shards, load_factor, device, di);
    if (rc) return rc;
    rc = mf_table(m, proteins);
    if (rc) { (void)hipFree(di->d_buckets); (void)hipFree(di->d_arena); }
    return rc;
}

int kaamer_image_build_fasta_device(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                                    kaamer_proteins **proteins, kaamer_image **image)
{
    int rc = mf_build_args("image_build_fasta_device", text, len, shard, n_shards, proteins, image);
    if (rc) return rc;
    *proteins = nullptr; *image = nullptr;
    MfReader m;
    kaamer_device_image di;
    rc = mf_build(m, text, len, shard, n_shards, load_factor, device, proteins, &di);
    if (rc) return rc;
    rc = kaamer_device_image_download(&di, image);
    if (rc) { kaamer_proteins_free(*proteins); *proteins = nullptr; }
    return rc;
}

int kaamer_index_build_fasta(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                             kaamer_proteins **proteins, kaamer_index **out)
{
    int rc = mf_build_args("index_build_fasta", text, len, shard, n_shards, proteins, out);
    if (rc) return rc;
    *proteins = nullptr; *out = nullptr;
    MfReader m;
    kaamer_device_image di;
    rc = mf_build(m, text, len, shard, n_shards, load_factor, device, proteins, &di);
    if (rc) return rc;
    rc = index_of_device_image(di, device, out);
    if (rc) { kaamer_proteins_free(*proteins); *proteins = nullptr; }
    return rc;
}

}  // extern "C"
