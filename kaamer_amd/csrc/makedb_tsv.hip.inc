// makedb_tsv.hip.inc — runTSV (pkg/makedb/inputTSV.go:92-142) on the device: the rows of a database TSV in, the protein
// table with its feature columns out, the packed sequences left in HBM in the layout bd_windows_kernel reads (included by
// search.hip after makedb_fasta.hip.inc: the tiling, pt_tile_scan_kernel, the workgroup scans and pt_line_len are the
// parser's, mf_gather_bytes_kernel, the trace, the grids and the builds are the FASTA reader's).  kaamer_makedb_tsv
// (makedb.cpp) is the host's statement of the same rules.  The header row is read on the host, by the routine that reader
// uses (kaamer_tsv_header): the device sees rows only, and of the header the number of columns H, which columns are
// EntryID and Sequence columns, and which column every feature is.
//   lines    split at '\n', a last piece without '\n' is a line, one trailing '\r' is dropped
//   rows     every line is a row, an empty one too; its cells are the pieces between tabs; the first H count, missing ones
//            are empty
//   columns  EntryId / Sequence: the LAST such column among the cells the row has; every other cell of the first H is the
//            feature of its column
//   accept   Sequence of 7 bytes or more and a non-empty EntryId; the k-th accepted row gets id id_base + k.  No byte is
//            changed.  A rejected row takes no room anywhere
//
// A cell is never looked for: tabs are ranked in text order like lines, so cell c of a line is what lies between two
// consecutive entries of tab_pos[], and the bytes of the feature cells in front of column c are the distance from the
// line's start less the tabs and the EntryID / Sequence cells in between.  No pass walks a line or a cell.
//
// Launches, all on the null stream, ordered by the end of each grid:
//   mt_count_kernel      per tile: the '\n's and the '\t's (the text is read once for both)
//   pt_tile_scan_kernel  twice, with a line bound of 0: the tiles' line bases, the tiles' tab bases, the totals
//   mt_lines_kernel      per tile, BY POSITION: where every line starts and the rank of its first tab; where every tab is
//   mt_rows_kernel<0>    per PT_LINES lines: which rows are accepted, and what the block's accepted rows keep
//   mt_block_scan_kernel one workgroup: N and the record, sequence, EntryId and feature bases of every block
//   mt_rows_kernel<1>    per PT_LINES lines again: id, offsets, entry_off, line and feature base of every accepted row
//   mt_cells_kernel      per (accepted row, feature): its feature_off entry and where the cell lies in the text
//   mf_gather_bytes_kernel  three times, BY DESTINATION: sequences, EntryIds, feature cells (there record = cell)
enum { MT_R_RECORDS = 0, MT_R_SEQ_BYTES, MT_R_ID_BYTES, MT_R_FEAT_BYTES, MT_R_N };

struct MtParams {
    PtParams pt;               // text, n, n_tiles, tile_nl, line_start, line_cap (= the text's lines), res
    unsigned long long *res;   // MT_R_*
    uint32_t *tile_tab;        // n_tiles + 1: counts, then (in place) exclusive bases
    uint32_t n_tabs;
    uint32_t *tab_pos;         // where the k-th tab of the text is
    uint32_t *line_tab;        // the tabs in front of line i; lines + 1
    // the header: columns in ascending order
    uint32_t n_cols, n_feat, n_idc, n_seqc;
    const uint32_t *id_cols, *seq_cols;   // the EntryID columns, the Sequence columns
    const uint32_t *key_cols;             // both (n_idc + n_seqc): the columns that are no feature
    const uint32_t *feat_col;             // the column of feature j
    // per block of PT_LINES lines: what mt_rows_kernel<0> counted, and in front of it (mt_block_scan_kernel)
    unsigned long long *blk_seq, *blk_idf;             // sequence bytes | records << 32;  EntryId bytes | feature bytes << 32
    unsigned long long *blk_seq_base, *blk_idf_base;
    // the accepted rows
    uint32_t *ids, *seq_src, *id_src, *rec_line;
    uint64_t *offsets, *id_off, *rec_feat;             // rec_feat: where the row's feature bytes start; n + 1 each
    // the feature cells, row-major
    uint64_t *feat_off;        // n * n_feat + 1
    uint32_t *feat_src;
    uint64_t id_base;
};

// line i as a row: its bytes and its tabs
struct MtLine {
    uint32_t start, end;   // the '\r' drop applied
    uint32_t t0, nt;       // its tabs are tab_pos[t0 .. t0 + nt)
    uint32_t m;            // the cells that count: min(nt + 1, H)
};
__device__ __forceinline__ MtLine mt_line(const MtParams &f, uint32_t i)
{
    MtLine l;
    const uint32_t len = pt_line_len(f.pt, i, l.start);
    l.end = l.start + len;
    l.t0 = f.line_tab[i];
    l.nt = f.line_tab[i + 1] - l.t0;
    l.m = (l.nt < f.n_cols - 1u ? l.nt : f.n_cols - 1u) + 1u;
    return l;
}
// cell c <= nt of the line.  (The dropped '\r' lies behind the last tab, so the last cell ends at the line's end.)
__device__ __forceinline__ uint32_t mt_cell_start(const MtParams &f, const MtLine &l, uint32_t c) { return c ? f.tab_pos[l.t0 + c - 1u] + 1u : l.start; }
__device__ __forceinline__ uint32_t mt_cell_end(const MtParams &f, const MtLine &l, uint32_t c) { return c < l.nt ? f.tab_pos[l.t0 + c] : l.end; }
// the last of the ascending cols[0 .. n) below m, as index + 1 (0: none)
__device__ __forceinline__ uint32_t mt_last_below(const uint32_t *cols, uint32_t n, uint32_t m)
{
    uint32_t lo = 0, hi = n;   // cols[.. lo) < m <= cols[hi ..)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cols[mid] < m) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the bytes of the EntryID and Sequence cells in columns below c (c <= m)
__device__ __forceinline__ uint32_t mt_key_bytes(const MtParams &f, const MtLine &l, uint32_t c)
{
    uint32_t sum = 0;
    for (uint32_t k = 0; k < f.n_idc + f.n_seqc; k++) {
        const uint32_t col = f.key_cols[k];
        if (col >= c) break;
        sum += mt_cell_end(f, l, col) - mt_cell_start(f, l, col);
    }
    return sum;
}

struct MtRow {
    bool acc;
    uint32_t seq_src, seq_len, id_src, id_len, feat_len;
};
__device__ __forceinline__ MtRow mt_row(const MtParams &f, uint32_t i)
{
    MtRow r = { false, 0, 0, 0, 0, 0 };
    const MtLine l = mt_line(f, i);
    const uint32_t ki = mt_last_below(f.id_cols, f.n_idc, l.m), ks = mt_last_below(f.seq_cols, f.n_seqc, l.m);
    if (!ki || !ks) return r;   // (a missing cell is empty)
    const uint32_t ci = f.id_cols[ki - 1u], cs = f.seq_cols[ks - 1u];
    r.id_src = mt_cell_start(f, l, ci);
    r.id_len = mt_cell_end(f, l, ci) - r.id_src;
    r.seq_src = mt_cell_start(f, l, cs);
    r.seq_len = mt_cell_end(f, l, cs) - r.seq_src;
    r.acc = r.seq_len >= (uint32_t)KAAMER_KMER_SIZE && r.id_len >= 1u;
    if (r.acc) r.feat_len = mt_cell_end(f, l, l.m - 1u) - l.start - (l.m - 1u) - mt_key_bytes(f, l, l.m);
    return r;
}

__device__ __forceinline__ uint32_t mt_count(const uint4 &v, uint32_t nv)   // '\n's | '\t's << 16
{
    uint32_t c = 0;
#pragma unroll
    for (int b = 0; b < PT_PIECE; b++) {
        const uint32_t x = pt_piece_byte(v, b);
        c += ((uint32_t)b < nv && x == '\n') ? 1u : 0u;
        c += ((uint32_t)b < nv && x == '\t') ? 1u << 16 : 0u;
    }
    return c;
}

__global__ __launch_bounds__(PT_BLOCK) void mt_count_kernel(MtParams f)
{
    __shared__ uint32_t wsum[PT_BLOCK / 64];
    const PtParams &p = f.pt;
    const uint32_t tile = blockIdx.x;
    uint32_t cnt = 0;   // (a tile holds 2^14 bytes: neither half overflows)
#pragma unroll
    for (int j = 0; j < PT_PIECES; j++) {
        const uint64_t pos = (uint64_t)tile * PT_TILE + (uint64_t)(j * PT_BLOCK + threadIdx.x) * PT_PIECE;
        if (pos >= p.n) continue;
        uint32_t nv;
        const uint4 v = pt_load_piece(p.text, p.n, (uint32_t)pos, nv);
        cnt += mt_count(v, nv);
    }
    uint32_t total;
    (void)pt_block_incl_sum(cnt, wsum, total);
    if (threadIdx.x == 0) { p.tile_nl[tile] = total & 0xFFFFu; f.tile_tab[tile] = total >> 16; }
}

__global__ __launch_bounds__(PT_BLOCK) void mt_lines_kernel(MtParams f)
{
    __shared__ uint32_t wsum[PT_BLOCK / 64];
    const PtParams &p = f.pt;
    const uint32_t tile = blockIdx.x;
    if (tile == 0 && threadIdx.x == 0) {
        p.line_start[0] = 0; f.line_tab[0] = 0;
        p.line_start[p.line_cap] = p.n + 1u; f.line_tab[p.line_cap] = f.n_tabs;   // (the text's end as one more '\n')
    }
    const uint32_t t_at = tile < p.n_tiles ? tile : p.n_tiles;
    uint32_t carry_nl = p.tile_nl[t_at], carry_tab = f.tile_tab[t_at];
#pragma unroll 1
    for (int j = 0; j < PT_PIECES; j++) {
        const uint64_t pos64 = (uint64_t)tile * PT_TILE + (uint64_t)(j * PT_BLOCK + threadIdx.x) * PT_PIECE;
        uint32_t nv = 0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (pos64 < p.n) v = pt_load_piece(p.text, p.n, (uint32_t)pos64, nv);
        const uint32_t pos = (uint32_t)pos64;
        const uint32_t cnt = mt_count(v, nv);
        uint32_t total;
        const uint32_t before = pt_block_incl_sum(cnt, wsum, total) - cnt;   // (a piece of the tile: both halves stay below 2^13)
        uint32_t line = carry_nl + (before & 0xFFFFu);   // the line this piece's first byte belongs to
        uint32_t tab = carry_tab + (before >> 16);       // the tabs in front of that byte
        carry_nl += total & 0xFFFFu;
        carry_tab += total >> 16;
        if ((cnt & 0xFFFFu) == 0 && (cnt >> 16) == 0) continue;
#pragma unroll
        for (int b = 0; b < PT_PIECE; b++) {
            const uint32_t c = pt_piece_byte(v, b);
            if ((uint32_t)b >= nv) {
                // (beyond the text)
            } else if (c == '\n') {
                line++;
                if (line < p.line_cap) { p.line_start[line] = pos + (uint32_t)b + 1u; f.line_tab[line] = tab; }
            } else if (c == '\t') {
                if (tab < f.n_tabs) f.tab_pos[tab] = pos + (uint32_t)b;
                tab++;
            }
        }
    }
}

template <bool EMIT> __global__ __launch_bounds__(PT_LINES) void mt_rows_kernel(MtParams f)
{
    __shared__ unsigned long long lds64[PT_LINES];
    const unsigned long long nl = f.pt.line_cap;
    const uint32_t blk = blockIdx.x;
    if ((unsigned long long)blk * PT_LINES >= nl) return;
    const int t = threadIdx.x;
    const unsigned long long i64 = (unsigned long long)blk * PT_LINES + t;
    const uint32_t i = (uint32_t)i64;
    MtRow r = { false, 0, 0, 0, 0, 0 };
    if (i64 < nl) r = mt_row(f, i);
    // (a text has fewer than 2^32 bytes, so every byte sum fits 32 bits; an accepted row takes 9 of them)
    const unsigned long long s_incl = pt_scan<false>(r.acc ? (unsigned long long)r.seq_len | (1ull << 32) : 0ull, lds64, MfAdd64());
    const unsigned long long s_total = lds64[PT_LINES - 1];
    const unsigned long long f_incl = pt_scan<false>(r.acc ? (unsigned long long)r.id_len | ((unsigned long long)r.feat_len << 32) : 0ull, lds64, MfAdd64());
    const unsigned long long f_total = lds64[PT_LINES - 1];
    if (!EMIT) {
        if (t == 0) { f.blk_seq[blk] = s_total; f.blk_idf[blk] = f_total; }
        return;
    }
    const unsigned long long n_rec = f.res[MT_R_RECORDS];
    if (blk == 0 && t == 0) {
        f.offsets[n_rec] = f.res[MT_R_SEQ_BYTES];
        f.id_off[n_rec] = f.res[MT_R_ID_BYTES];
        f.rec_feat[n_rec] = f.res[MT_R_FEAT_BYTES];
    }
    if (!r.acc) return;
    const unsigned long long s_at = f.blk_seq_base[blk] + s_incl, f_at = f.blk_idf_base[blk] + f_incl;
    const unsigned long long k = (s_at >> 32) - 1u;
    if (k >= n_rec) return;   // (both passes decide alike, so this never holds: the buffers are sized from the first)
    f.ids[k] = (uint32_t)(f.id_base + k);
    f.offsets[k] = (uint32_t)s_at - r.seq_len;
    f.id_off[k] = (uint32_t)f_at - r.id_len;
    f.rec_feat[k] = (f_at >> 32) - r.feat_len;
    f.seq_src[k] = r.seq_src;
    f.id_src[k] = r.id_src;
    f.rec_line[k] = i;
}

__global__ __launch_bounds__(PT_LINES) void mt_block_scan_kernel(MtParams f)
{
    __shared__ unsigned long long lds64[PT_LINES];
    __shared__ unsigned long long carry_s, carry_f;
    const unsigned long long nl = f.pt.line_cap;
    const uint32_t nb = (uint32_t)((nl + PT_LINES - 1) / PT_LINES);
    const int t = threadIdx.x;
    if (t == 0) { carry_s = 0; carry_f = 0; }
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += PT_LINES) {
        const uint32_t b = base + t;
        const unsigned long long s = b < nb ? f.blk_seq[b] : 0ull, x = b < nb ? f.blk_idf[b] : 0ull;
        const unsigned long long s_incl = pt_scan<false>(s, lds64, MfAdd64());
        const unsigned long long f_incl = pt_scan<false>(x, lds64, MfAdd64());
        const unsigned long long s0 = carry_s, f0 = carry_f;
        if (b < nb) { f.blk_seq_base[b] = s0 + s_incl - s; f.blk_idf_base[b] = f0 + f_incl - x; }
        __syncthreads();
        if (t == PT_LINES - 1) { carry_s = s0 + s_incl; carry_f = f0 + f_incl; }
        __syncthreads();
    }
    if (t == 0) {
        f.res[MT_R_RECORDS] = carry_s >> 32;   // < 2^29
        f.res[MT_R_SEQ_BYTES] = (uint32_t)carry_s;
        f.res[MT_R_ID_BYTES] = (uint32_t)carry_f;
        f.res[MT_R_FEAT_BYTES] = carry_f >> 32;
    }
}

// entry k = row * n_feat + j of feature_off, and where that cell lies.  A cell the row does not have is empty, behind the
// cells it has.
__global__ __launch_bounds__(PT_BLOCK) void mt_cells_kernel(MtParams f)
{
    const uint64_t n_cells = f.res[MT_R_RECORDS] * f.n_feat;   // < 2^32 (mt_read)
    const uint64_t stride = (uint64_t)gridDim.x * PT_BLOCK, tid = (uint64_t)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (tid == 0) f.feat_off[n_cells] = f.res[MT_R_FEAT_BYTES];
    for (uint64_t k = tid; k < n_cells; k += stride) {
        const uint32_t r = (uint32_t)k / f.n_feat, j = (uint32_t)k - r * f.n_feat;
        const MtLine l = mt_line(f, f.rec_line[r]);
        const uint32_t col = f.feat_col[j];
        if (col < l.m) {
            const uint32_t at = mt_cell_start(f, l, col);
            f.feat_off[k] = f.rec_feat[r] + (at - l.start - col - mt_key_bytes(f, l, col));
            f.feat_src[k] = at;
        } else {
            f.feat_off[k] = f.rec_feat[r + 1];
            f.feat_src[k] = l.end;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// One text's reader, as MfReader is: after mt_read the accepted rows lie on the device: d_seqs (32 bytes of slack behind
// the last residue), offsets, ids, the EntryId bytes and the feature bytes with their offsets.
struct MtReader {
    int device = 0;
    DevBuf<uint8_t> d_text, d_seqs, d_idb, d_featb;
    DevBuf<uint32_t> d_cnt32, d_line32, d_tab32, d_hdr32, d_rec32, d_cell32;
    DevBuf<unsigned long long> d_res, d_blk64, d_rec64, d_cell64;
    MtParams f{};
    uint64_t n_rec = 0, seq_bytes = 0, id_bytes = 0, feat_bytes = 0;
    ~MtReader() { (void)hipSetDevice(device); }   // (before the buffers go)
};

// the rows [text, text + len) under the header `cols`
static int mt_read(MtReader &m, const char *text, uint64_t len, const kaamer_tsv_columns &cols, uint64_t id_base, int device)
{
    HIPCHK(hipSetDevice(device));
    m.device = device;
    hipDeviceProp_t prop;
    const int n_cu = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
    MfTrace tr;
    tr.format = "tsv";
    tr.bytes = len;
    tr.begin();
    // the header's columns, each list ascending: EntryID columns, Sequence columns, both, the features' columns
    std::vector<uint32_t> h_idc, h_seqc, h_key, h_feat;
    for (size_t c = 0; c < cols.slot.size(); c++) {
        if (cols.slot[c] == KAAMER_TSV_ENTRY_ID) h_idc.push_back((uint32_t)c);
        else if (cols.slot[c] == KAAMER_TSV_SEQUENCE) h_seqc.push_back((uint32_t)c);
        else h_feat.push_back((uint32_t)c);
        if (cols.slot[c] < 0) h_key.push_back((uint32_t)c);
    }
    std::vector<uint32_t> h_hdr(h_idc);
    h_hdr.insert(h_hdr.end(), h_seqc.begin(), h_seqc.end());
    h_hdr.insert(h_hdr.end(), h_key.begin(), h_key.end());
    h_hdr.insert(h_hdr.end(), h_feat.begin(), h_feat.end());
    const uint32_t n_tiles = (uint32_t)((len + PT_TILE - 1) / PT_TILE);
    int rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_text, (size_t)len + 2 * PT_PIECE), want(m.d_cnt32, 2 * ((size_t)n_tiles + 1) + 2),
                                                  want(m.d_res, (size_t)2 * PT_R_N + MT_R_N), want(m.d_hdr32, h_hdr.size()) });
    if (rc) return rc;
    if (len) HIPCHK(hipMemcpy(m.d_text, text, (size_t)len, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.d_hdr32, h_hdr.data(), h_hdr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    tr.lap("upload");
    MtParams &f = m.f;
    PtParams &p = f.pt;
    p.text = m.d_text;
    p.n = (uint32_t)len;
    p.n_tiles = n_tiles;
    p.tile_nl = m.d_cnt32;
    f.tile_tab = m.d_cnt32 + n_tiles + 1;
    p.line_start = m.d_cnt32 + 2 * ((size_t)n_tiles + 1);   // two words: with a line bound of 0 the tile scan only counts
    p.line_cap = 0;
    p.res = m.d_res;
    f.res = m.d_res + 2 * PT_R_N;
    f.id_base = id_base;
    f.n_cols = (uint32_t)cols.slot.size();
    f.n_feat = (uint32_t)h_feat.size();
    f.n_idc = (uint32_t)h_idc.size();
    f.n_seqc = (uint32_t)h_seqc.size();
    f.id_cols = m.d_hdr32;
    f.seq_cols = f.id_cols + h_idc.size();
    f.key_cols = f.seq_cols + h_seqc.size();
    f.feat_col = f.key_cols + h_key.size();
    HIPCHK(hipMemset(m.d_res, 0, (2 * PT_R_N + MT_R_N) * sizeof(unsigned long long)));
    if (n_tiles) hipLaunchKernelGGL(mt_count_kernel, dim3(n_tiles), dim3(PT_BLOCK), 0, 0, f);
    hipLaunchKernelGGL(pt_tile_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, p);
    {   // the same scan over the tab counts: its "lines" are the tabs + 1
        PtParams q = p;
        q.tile_nl = f.tile_tab;
        q.res = m.d_res + PT_R_N;
        hipLaunchKernelGGL(pt_tile_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, q);
    }
    HIPCHK(hipGetLastError());
    unsigned long long h_res[2 * PT_R_N + MT_R_N];
    HIPCHK(hipMemcpy(h_res, m.d_res, sizeof h_res, hipMemcpyDeviceToHost));
    tr.lap("count");
    const unsigned long long nl = h_res[PT_R_NL], n_tabs = h_res[PT_R_N + PT_R_NL] - 1u;
    if (nl < 1 || nl > 0xFFFFFFF0ull) return kaamer_fail(KAAMER_E_CAPACITY, "makedb_tsv_device: %llu lines in one text: cut it at a line end", nl);
    const size_t nb = (size_t)((nl + PT_LINES - 1) / PT_LINES) + 1;
    rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_line32, 2 * ((size_t)nl + 2)), want(m.d_tab32, (size_t)n_tabs + 1), want(m.d_blk64, 4 * nb) });
    if (rc) return rc;
    p.line_start = m.d_line32;
    f.line_tab = m.d_line32 + (nl + 2);
    f.tab_pos = m.d_tab32;
    f.n_tabs = (uint32_t)n_tabs;
    f.blk_seq = m.d_blk64; f.blk_idf = m.d_blk64 + nb; f.blk_seq_base = m.d_blk64 + 2 * nb; f.blk_idf_base = m.d_blk64 + 3 * nb;
    p.line_cap = (uint32_t)nl;
    const uint32_t n_blk = (uint32_t)(nb - 1);
    hipLaunchKernelGGL(mt_lines_kernel, dim3(n_tiles ? n_tiles : 1u), dim3(PT_BLOCK), 0, 0, f);
    tr.lap("lines and tabs");
    hipLaunchKernelGGL(mt_rows_kernel<false>, dim3(n_blk), dim3(PT_LINES), 0, 0, f);
    hipLaunchKernelGGL(mt_block_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, f);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(h_res, m.d_res, sizeof h_res, hipMemcpyDeviceToHost));
    tr.lap("rows");
    const unsigned long long *r = h_res + 2 * PT_R_N;
    m.n_rec = r[MT_R_RECORDS]; m.seq_bytes = r[MT_R_SEQ_BYTES]; m.id_bytes = r[MT_R_ID_BYTES]; m.feat_bytes = r[MT_R_FEAT_BYTES];
    const size_t n = (size_t)m.n_rec;
    const unsigned long long n_cells = (unsigned long long)m.n_rec * f.n_feat;
    if (n_cells > 0xFFFFFFF0ull)
        return kaamer_fail(KAAMER_E_CAPACITY, "makedb_tsv_device: %llu rows of %u features in one text: cut it at a line end", (unsigned long long)m.n_rec, f.n_feat);
    rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_rec32, 4 * (n + 1)), want(m.d_rec64, 3 * (n + 1)), want(m.d_cell32, (size_t)n_cells + 1),
                                              want(m.d_cell64, (size_t)n_cells + 1), want(m.d_seqs, (size_t)m.seq_bytes + 3 * PT_PIECE),
                                              want(m.d_idb, (size_t)m.id_bytes + 2 * PT_PIECE), want(m.d_featb, (size_t)m.feat_bytes + 2 * PT_PIECE) });
    if (rc) return rc;
    f.ids = m.d_rec32; f.seq_src = m.d_rec32 + (n + 1); f.id_src = m.d_rec32 + 2 * (n + 1); f.rec_line = m.d_rec32 + 3 * (n + 1);
    f.offsets = reinterpret_cast<uint64_t *>(m.d_rec64.get());
    f.id_off = f.offsets + (n + 1); f.rec_feat = f.offsets + 2 * (n + 1);
    f.feat_off = reinterpret_cast<uint64_t *>(m.d_cell64.get());
    f.feat_src = m.d_cell32;
    {   // (the builder's window kernel reads up to 17 bytes behind the last residue: they are zero, not left-over)
        const size_t whole = (size_t)(m.seq_bytes / PT_PIECE) * PT_PIECE;
        HIPCHK(hipMemset(m.d_seqs + whole, 0, (size_t)m.seq_bytes - whole + 3 * PT_PIECE));
    }
    hipLaunchKernelGGL(mt_rows_kernel<true>, dim3(n_blk), dim3(PT_LINES), 0, 0, f);
    hipLaunchKernelGGL(mt_cells_kernel, dim3(mf_grid(n_cells * PT_PIECE, n_cu)), dim3(PT_BLOCK), 0, 0, f);
    tr.lap("rows, emit");
    if (m.seq_bytes) hipLaunchKernelGGL(mf_gather_bytes_kernel, dim3(mf_grid(m.seq_bytes, n_cu)), dim3(PT_BLOCK), 0, 0, p.text, p.n, f.offsets, f.seq_src,
                                        (uint32_t)n, (uint32_t)m.seq_bytes, m.d_seqs.get());
    tr.lap("gather sequences");
    if (m.id_bytes) hipLaunchKernelGGL(mf_gather_bytes_kernel, dim3(mf_grid(m.id_bytes, n_cu)), dim3(PT_BLOCK), 0, 0, p.text, p.n, f.id_off, f.id_src,
                                       (uint32_t)n, (uint32_t)m.id_bytes, m.d_idb.get());
    if (m.feat_bytes) hipLaunchKernelGGL(mf_gather_bytes_kernel, dim3(mf_grid(m.feat_bytes, n_cu)), dim3(PT_BLOCK), 0, 0, p.text, p.n, f.feat_off, f.feat_src,
                                         (uint32_t)n_cells, (uint32_t)m.feat_bytes, m.d_featb.get());
    HIPCHK(hipGetLastError());
    tr.lap("gather cells");
    return KAAMER_OK;
}

// the host's table of what mt_read left on the device: bulk copies into the table's arrays, then makedb.cpp's by_id and KStats
static int mt_table(MtReader &m, const kaamer_tsv_columns &cols, kaamer_proteins **out)
{
    MfTrace tr;
    tr.format = "tsv";
    tr.bytes = m.f.pt.n;
    tr.begin();
    kaamer_table_arrays a;
    kaamer_proteins *t = kaamer_proteins_table_new(cols.feature_names, (uint32_t)m.n_rec, m.seq_bytes, m.id_bytes, m.feat_bytes, &a);
    if (!t) return kaamer_fail(KAAMER_E_NOMEM, "makedb_tsv_device: the table");
    tr.lap("host table");   // (its arrays, sized and zero-filled: the first touch of their pages)
    const size_t n = (size_t)m.n_rec;
    hipError_t e = hipSuccess;
    auto get = [&](void *dst, const void *src, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); };
    get(a.ids, m.f.ids, n * 4);
    get(a.offsets, m.f.offsets, (n + 1) * 8);
    get(a.seqs, m.d_seqs, (size_t)m.seq_bytes);
    get(a.entry_off, m.f.id_off, (n + 1) * 8);
    get(a.entry_ids, m.d_idb, (size_t)m.id_bytes);
    get(a.feature_off, m.f.feat_off, (n * m.f.n_feat + 1) * 8);
    get(a.features, m.d_featb, (size_t)m.feat_bytes);
    if (e != hipSuccess) { kaamer_proteins_free(t); return kaamer_fail(KAAMER_E_HIP, "makedb_tsv_device: download: %s", hipGetErrorString(e)); }
    tr.lap("download");
    kaamer_proteins_table_seal(t);
    *out = t;
    return KAAMER_OK;
}

// header == NULL: the text's first line is the header and the rows follow it; else `header` is that line and the text is rows
static int mt_header(const char *who, const char *&text, uint64_t &len, const char *header, uint64_t header_len, kaamer_tsv_columns *cols)
{
    if (header) {
        if (memchr(header, '\n', (size_t)header_len)) return kaamer_fail(KAAMER_E_ARG, "%s: the header is one line without its line end", who);
        return kaamer_tsv_header(header, header + header_len, cols);
    }
    uint64_t rows_at = 0;
    const int rc = kaamer_tsv_header_of_text(text, len, cols, &rows_at);
    text += rows_at; len -= rows_at;
    return rc;
}

extern "C" {

int kaamer_makedb_tsv_device(const char *text, uint64_t len, const char *header, uint64_t header_len, uint64_t id_base, int device, kaamer_proteins **out)
{
    if (len > 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_ARG, "makedb_tsv_device: a text holds at most 2^32 - 1 bytes: cut it at a line end");
    if (!out || (!text && len)) return kaamer_fail(KAAMER_E_ARG, "makedb_tsv_device: bad argument");
    *out = nullptr;
    kaamer_tsv_columns cols;
    int rc = mt_header("makedb_tsv_device", text, len, header, header_len, &cols);
    if (rc) return rc;
    MtReader m;
    rc = mt_read(m, text, len, cols, id_base, device);
    if (rc) return rc;
    return mt_table(m, cols, out);
}

// text -> the reader's buffers -> the build that takes device buffers -> the table's host copy
static int mt_build(MtReader &m, const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                    kaamer_proteins **proteins, kaamer_device_image *di)
{
    kaamer_tsv_columns cols;
    int rc = mt_header("makedb_tsv_device", text, len, nullptr, 0, &cols);
    if (rc) return rc;
    rc = mt_read(m, text, len, cols, 0, device);
    if (rc) return rc;
    m.d_text.reset(); m.d_cnt32.reset(); m.d_line32.reset(); m.d_tab32.reset(); m.d_blk64.reset();   // (the build wants the room; hipFree waits for the gathers)
    rc = kaamer_build_resident(m.d_seqs, m.f.offsets, m.f.ids, (uint32_t)m.n_rec, m.seq_bytes, shard, n_shards, load_factor, device, di);
    if (rc) return rc;
    rc = mt_table(m, cols, proteins);
    if (rc) { (void)hipFree(di->d_buckets); (void)hipFree(di->d_arena); }
    return rc;
}

int kaamer_image_build_tsv_device(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                                  kaamer_proteins **proteins, kaamer_image **image)
{
    int rc = mf_build_args("image_build_tsv_device", text, len, shard, n_shards, proteins, image, "at a line end");
    if (rc) return rc;
    *proteins = nullptr; *image = nullptr;
    MtReader m;
    kaamer_device_image di;
    rc = mt_build(m, text, len, shard, n_shards, load_factor, device, proteins, &di);
    if (rc) return rc;
    rc = kaamer_device_image_download(&di, image);
    if (rc) { kaamer_proteins_free(*proteins); *proteins = nullptr; }
    return rc;
}

int kaamer_index_build_tsv(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                           kaamer_proteins **proteins, kaamer_index **out)
{
    int rc = mf_build_args("index_build_tsv", text, len, shard, n_shards, proteins, out, "at a line end");
    if (rc) return rc;
    *proteins = nullptr; *out = nullptr;
    MtReader m;
    kaamer_device_image di;
    rc = mt_build(m, text, len, shard, n_shards, load_factor, device, proteins, &di);
    if (rc) return rc;
    rc = index_of_device_image(di, device, out);
    if (rc) { kaamer_proteins_free(*proteins); *proteins = nullptr; }
    return rc;
}

}  // extern "C"
