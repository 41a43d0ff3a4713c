// makedb_embl.hip.inc — runEMBL + processProteinInputEMBL (pkg/makedb/inputEMBL.go:66-119, 189-314) on the device: the
// text of a UniProt flat file in, the protein table with its ten feature columns out, the packed sequences left in HBM in
// the layout bd_windows_kernel reads (included by search.hip after makedb_tsv.hip.inc: the tiling, pt_count_kernel,
// pt_tile_scan_kernel, the workgroup scans and pt_line_len are the parser's, the trace, the grids and the build hand-over
// are the FASTA reader's).  kaamer_makedb_embl (makedb.cpp, process_embl_entry + makedb_flat) is the host's statement of
// the same rules, and where the words below and that code differ, the code holds.
//   lines    split at '\n', a last piece without '\n' is a line, one trailing '\r' is dropped.  A line that is then exactly
//            "//" ends an entry and takes a number, even when the entry is empty: "// ", "///" and "//\r\r" are ordinary
//            lines.  Lines shorter than 2 bytes are ignored.  What lies behind the text's last "//" belongs to no entry
//   tag      the first two bytes.  Only ID GN DE OX OS OC DR SQ and two spaces matter, every other line is skipped without
//            being read further
//   Skip     (the whole entry is dropped; where the reference would panic)
//            a line of ID DE OX OS OC DR SQ or two spaces with fewer than 5 bytes (a two-space line of 2 to 4 bytes too;
//            a GN line that short cannot hold "Name=" and is not read);  ID / OX / DR with no field behind column 5;  an OX
//            first field under 12 bytes;  a matched DR (first field exactly KEGG; GO; BioCyc; HAMAP;) without a second field;
//            SQ with fewer than two fields;  a DE line under 19 bytes that is RecName or SubName, or under 17 bytes that is
//            EC;  a declared length above the residues held
//   drops    a DE line whose [5:] contains none of "RecName", "SubName", "EC=" (looked for in that order) but contains
//            "Flags: Fragment;";  a declared length below 7: the last SQ line wins, and a number Atoi refuses ("+", "12x",
//            20 digits) is 0, a negative one is below 7.  Skip and drop have the same effect, so their order does not matter
//   GN       looked at only while GeneName is still empty: among the GN lines that contain "Name=" anywhere, the first
//            that is malformed (no field behind column 5, or a first field under 5 bytes) or yields a non-empty value
//            decides: Skip, or the value.  A malformed GN line behind the deciding one is harmless
//   ProteinName  the last RecName line resets it; each later SubName appends ";;" + v if the value so far is non-empty,
//            else becomes the value; without a RecName the same from the first SubName
//   EC, TaxId, EntryId   the last line wins
//   separators   Organism (" ") and the four DR columns (";") put theirs in front of every contribution but the first, even
//            when earlier ones were empty; FullTaxonomy puts " " only when what is gathered so far is non-empty
//   values   RecName / SubName: [19:], EC: [17:], each with " {.*};" removed greedily -- from the first " {" to the last
//            "};" behind it -- and then ALL trailing ';' of the result cut, which may reach into the part in front of the
//            removed span.  OS: [5:] less all trailing '.'.  OC: [5:].  GN: field 0 [5:], OX: field 0 [12:], DR: field 1,
//            each less its trailing ';'.  EntryId: field 0 of ID.  Fields split at ' ' and '\t'..'\r' (an interior '\r' too)
//   sequence every two-space line's bytes behind column 5 with ' ' removed, wherever in the entry the line stands.  Nothing
//            is upper-cased, bytes >= 0x80 stay as they are.  Indexed (seqs[]) is Sequence[:declared]; an entry that holds
//            more than it declares keeps its whole string beside (kaamer_proteins_table_full_seqs)
//   ids      record k of the text (1-based ordinal of its "//") gets id (uint32_t)(nb_before + k)
//
// The shape: a line record per line, then a wave per entry.  It differs from a piece list gathered by destination in one
// point: the wave that folds an entry copies that entry's bytes itself, 64 a step, so there is no piece buffer and no second
// ranking of pieces.  No pass is serial over the text, no lane walks a line or an entry: a long line is read 64 bytes a step
// by a wave with ballots, a long entry 64 line records a step, and the lines of an entry that contribute a value are taken
// in order by the whole wave (the order rules are then plain: state carried from one contribution to the next).  No atomic
// decides a byte: the one atomic add hands out worklist slots, whose order nothing reads.
//
// Launches, all on the null stream, ordered by the end of each grid:
//   pt_count_kernel, pt_tile_scan_kernel   with a line bound of 0: they only count, every per-line buffer is sized from it
//   me_lines_kernel      per tile, BY POSITION: where every line starts
//   me_classify_kernel   per PT_LINES lines: two bytes and the length of every line: terminators, lines that drop their
//                        entry by length alone, the lines of a read tag onto the worklist; the block's terminator count
//   me_term_scan_kernel  one workgroup: the terminators in front of every block, T
//   me_terms_kernel      per PT_LINES lines: the line of the k-th terminator
//   me_read_kernel       a wave per worklist line: kind, Skip / non-empty flags, up to two source spans trimmed, the declared
//                        length of an SQ line, the non-space count of a sequence line
//   me_fold_kernel<0>    a wave per entry: decides it and sizes what it keeps (which ID / GN / EC / OX / RecName line counts,
//                        the ten cell lengths, declared and held residues)
//   me_ent_kernel<0>, me_ent_scan_kernel, me_ent_kernel<1>   per PT_LINES entries, one workgroup, per PT_LINES entries: N and
//                        every kept entry's record, sequence, EntryId, cell and whole-string bases
//   me_fold_kernel<1>    a wave per kept entry: id, offsets, the 10 feature offsets, and the bytes: EntryId, cells with their
//                        separators, the sequence lines squeezed (ballot, prefix popcount, store) and clipped at the declared
//                        length for seqs[], unclipped into the whole strings of the held > declared records
enum { ME_R_WORK = 0, ME_R_TERMS, ME_R_RECORDS, ME_R_SEQ_BYTES, ME_R_ID_BYTES, ME_R_FEAT_BYTES, ME_R_FULL, ME_R_FULL_BYTES, ME_R_N };
// kinds of a line record; kinds 1 .. 11 contribute to cell (kind == ME_SUB ? 0 : kind - 1) of EMBL_DEF_FTS
enum { ME_NONE_K = 0, ME_REC, ME_GN, ME_EC, ME_GO, ME_KEGG, ME_BIOCYC, ME_HAMAP, ME_OS, ME_OX, ME_OC, ME_SUB, ME_ID, ME_SQ, ME_SEQ, ME_DROP, ME_TERM };
enum { ME_F_SKIP = 0x100u, ME_F_VALUE = 0x200u, ME_KIND = 0xFFu };
enum { ME_FEATURES = 10 };
#define ME_NONE 0xFFFFFFFFu

// what me_fold_kernel<0> leaves of an entry
struct MeEnt {
    uint32_t keep, declared, held, id_len;
    uint32_t id_line, gn_line, ec_line, ox_line, rec_line;   // the line that counts (ME_NONE: none)
    uint32_t feat_len[ME_FEATURES];
    uint32_t pad;
};

struct MeParams {
    PtParams pt;               // text, n, n_tiles, tile_nl, line_start, line_cap (= the text's lines), res
    unsigned long long *res;   // ME_R_*
    uint32_t *kf;              // kind | flags of line i
    uint4 *span;               // line i: src0, len0, src1, len1 (SQ: len0 = declared; sequence line: len0 = non-space bytes, len1 = bytes)
    uint32_t *work;            // the lines me_read_kernel reads
    uint32_t *blk_term, *blk_term_base;
    uint32_t n_terms;
    uint32_t *term_line;       // n_terms
    MeEnt *ent;                // n_terms
    unsigned long long *ent_a, *ent_b, *ent_c;   // per entry, exclusive: sequence bytes | records << 32;  EntryId bytes | cell bytes << 32;  whole-string bytes | such records << 32
    unsigned long long *eb_a, *eb_b, *eb_c;      // per block of PT_LINES entries: totals, then (in place) bases
    // the kept entries
    uint32_t *ids, *full_rec;
    uint64_t *offsets, *id_off, *feat_off, *full_off;
    uint8_t *seqs, *idb, *featb, *fullb;
    uint64_t nb_before;
    uint32_t n_feat;           // feature columns of a record: ME_FEATURES here (makedb_gbk.hip.inc: 3)
};

__global__ __launch_bounds__(PT_BLOCK) void me_lines_kernel(MeParams f)
{
    __shared__ uint32_t wsum[PT_BLOCK / 64];
    const PtParams &p = f.pt;
    const uint32_t tile = blockIdx.x;
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
        if (!cnt) continue;
#pragma unroll
        for (int b = 0; b < PT_PIECE; b++) {
            if ((uint32_t)b < nv && pt_piece_byte(v, b) == '\n') {
                line++;
                if (line < p.line_cap) p.line_start[line] = pos + (uint32_t)b + 1u;
            }
        }
    }
}

__global__ __launch_bounds__(PT_LINES) void me_classify_kernel(MeParams f)
{
    __shared__ uint32_t lds[PT_LINES];
    __shared__ unsigned long long base_s;
    const PtParams &p = f.pt;
    const unsigned long long nl = p.line_cap;
    const uint32_t blk = blockIdx.x;
    if ((unsigned long long)blk * PT_LINES >= nl) return;
    const int t = threadIdx.x;
    const unsigned long long i64 = (unsigned long long)blk * PT_LINES + t;
    const uint32_t i = (uint32_t)i64;
    uint32_t kind = ME_NONE_K;
    bool todo = false;
    if (i64 < nl) {
        uint32_t start;
        const uint32_t len = pt_line_len(p, i, start);
        if (len >= 2u) {
            const uint32_t tag = (uint32_t)p.text[start] << 8 | p.text[start + 1u];
            const bool gn = tag == ('G' << 8 | 'N');
            const bool read = gn || tag == ('I' << 8 | 'D') || tag == ('D' << 8 | 'E') || tag == ('O' << 8 | 'X') || tag == ('O' << 8 | 'S') ||
                              tag == ('O' << 8 | 'C') || tag == ('D' << 8 | 'R') || tag == ('S' << 8 | 'Q') || tag == (' ' << 8 | ' ');
            if (len == 2u && tag == ('/' << 8 | '/')) kind = ME_TERM;
            else if (read && len >= 5u) todo = true;
            else if (read && !gn) kind = ME_DROP;
        }
        f.kf[i] = kind;   // (a worklist line's word is me_read_kernel's to write; until then it is no terminator)
    }
    const uint32_t w_incl = pt_scan<false>(todo ? 1u : 0u, lds, PtAdd32());
    const uint32_t w_total = lds[PT_LINES - 1];
    (void)pt_scan<false>(kind == ME_TERM ? 1u : 0u, lds, PtAdd32());
    if (t == 0) {
        f.blk_term[blk] = lds[PT_LINES - 1];
        base_s = w_total ? atomicAdd(&f.res[ME_R_WORK], (unsigned long long)w_total) : 0ull;   // (slots: their order is read by nobody)
    }
    __syncthreads();
    if (todo) f.work[(uint32_t)base_s + w_incl - 1u] = i;
}

__global__ __launch_bounds__(PT_LINES) void me_term_scan_kernel(MeParams f)
{
    __shared__ uint32_t lds[PT_LINES];
    __shared__ uint32_t carry_s;
    const unsigned long long nl = f.pt.line_cap;
    const uint32_t nb = (uint32_t)((nl + PT_LINES - 1) / PT_LINES);
    const int t = threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += PT_LINES) {
        const uint32_t b = base + t;
        const uint32_t v = b < nb ? f.blk_term[b] : 0u;
        const uint32_t incl = pt_scan<false>(v, lds, PtAdd32());
        const uint32_t c = carry_s;
        if (b < nb) f.blk_term_base[b] = c + incl - v;
        __syncthreads();
        if (t == PT_LINES - 1) carry_s = c + incl;
        __syncthreads();
    }
    if (t == 0) f.res[ME_R_TERMS] = carry_s;
}

__global__ __launch_bounds__(PT_LINES) void me_terms_kernel(MeParams f)
{
    __shared__ uint32_t lds[PT_LINES];
    const unsigned long long nl = f.pt.line_cap;
    const uint32_t blk = blockIdx.x;
    if ((unsigned long long)blk * PT_LINES >= nl) return;
    const int t = threadIdx.x;
    const unsigned long long i64 = (unsigned long long)blk * PT_LINES + t;
    const bool term = i64 < nl && f.kf[(uint32_t)i64] == ME_TERM;
    const uint32_t incl = pt_scan<false>(term ? 1u : 0u, lds, PtAdd32());
    if (!term) return;
    const uint32_t k = f.blk_term_base[blk] + incl - 1u;
    if (k < f.n_terms) f.term_line[k] = (uint32_t)i64;
}

// ---- a wave over the bytes [lo, hi) of the text, 64 a step ----
// the first / the last position where pred holds (ME_NONE: nowhere), and how many there are
template <class P> __device__ __forceinline__ uint32_t me_first(uint32_t lo, uint32_t hi, P pred)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t at = lo; at < hi; at += 64) {
        const uint64_t q = at + lane;
        const unsigned long long m = __ballot(q < hi && pred((uint32_t)q));
        if (m) return (uint32_t)at + (uint32_t)__builtin_ctzll(m);
    }
    return ME_NONE;
}
template <class P> __device__ __forceinline__ uint32_t me_last(uint32_t lo, uint32_t hi, P pred)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t top = hi;
    while (top > lo) {
        const uint32_t base = top - lo >= 64u ? top - 64u : lo;
        const uint32_t q = base + lane;
        const unsigned long long m = __ballot(q < top && pred(q));
        if (m) return base + 63u - (uint32_t)__builtin_clzll(m);
        top = base;
    }
    return ME_NONE;
}
template <class P> __device__ __forceinline__ uint32_t me_count(uint32_t lo, uint32_t hi, P pred)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n = 0;
    for (uint64_t at = lo; at < hi; at += 64) {
        const uint64_t q = at + lane;
        n += (uint32_t)__popcll(__ballot(q < hi && pred((uint32_t)q)));
    }
    return n;
}
__device__ __forceinline__ bool me_white(uint32_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
// does the L-byte word w start at q and end inside [.., hi)?
template <int L> __device__ __forceinline__ bool me_is(const uint8_t *text, uint32_t q, uint32_t hi, const char (&w)[L])
{
    if ((uint64_t)q + (L - 1) > hi) return false;
    bool same = true;
#pragma unroll
    for (int k = 0; k < L - 1; k++) same = same && text[q + k] == (uint8_t)w[k];
    return same;
}
// [lo, hi) less its trailing bytes c: the new end
__device__ __forceinline__ uint32_t me_trim(const uint8_t *text, uint32_t lo, uint32_t hi, uint32_t c)
{
    const uint32_t q = me_last(lo, hi, [&](uint32_t x) { return text[x] != c; });
    return q == ME_NONE ? lo : q + 1u;
}
// the field that starts at or behind `from`: [a, b) (false: none)
__device__ __forceinline__ bool me_field(const uint8_t *text, uint32_t from, uint32_t hi, uint32_t &a, uint32_t &b)
{
    a = me_first(from, hi, [&](uint32_t x) { return !me_white(text[x]); });
    if (a == ME_NONE) return false;
    b = me_first(a, hi, [&](uint32_t x) { return me_white(text[x]); });
    if (b == ME_NONE) b = hi;
    return true;
}

// line [s, e), e - s >= 5, of a read tag: its record
__device__ __forceinline__ void me_read_line(const uint8_t *text, uint32_t s, uint32_t e, uint32_t &kf, uint4 &sp)
{
    const uint32_t t0 = text[s], t1 = text[s + 1u], v = s + 5u;
    uint32_t a, b, a1, b1;
    kf = ME_NONE_K;
    sp = make_uint4(0, 0, 0, 0);
    if (t0 == 'I') {   // ID
        kf = ME_ID;
        if (!me_field(text, v, e, a, b)) { kf |= ME_F_SKIP; return; }
        sp.x = a; sp.y = b - a;
    } else if (t0 == 'G') {   // GN
        if (me_first(s, e, [&](uint32_t x) { return me_is(text, x, e, "Name="); }) == ME_NONE) return;
        kf = ME_GN;
        if (!me_field(text, v, e, a, b) || b - a < 5u) { kf |= ME_F_SKIP; return; }
        sp.x = a + 5u; sp.y = me_trim(text, a + 5u, b, ';') - sp.x;
        if (sp.y) kf |= ME_F_VALUE;
    } else if (t0 == 'D' && t1 == 'E') {
        uint32_t at;
        if (me_first(v, e, [&](uint32_t x) { return me_is(text, x, e, "RecName"); }) != ME_NONE) { kf = ME_REC; at = 19u; }
        else if (me_first(v, e, [&](uint32_t x) { return me_is(text, x, e, "SubName"); }) != ME_NONE) { kf = ME_SUB; at = 19u; }
        else if (me_first(v, e, [&](uint32_t x) { return me_is(text, x, e, "EC="); }) != ME_NONE) { kf = ME_EC; at = 17u; }
        else {
            if (me_first(v, e, [&](uint32_t x) { return me_is(text, x, e, "Flags: Fragment;"); }) != ME_NONE) kf = ME_DROP;
            return;
        }
        if (e - s < at) { kf |= ME_F_SKIP; return; }
        const uint32_t lo = s + at;
        const uint32_t open = me_first(lo, e, [&](uint32_t x) { return me_is(text, x, e, " {"); });
        const uint32_t close = open == ME_NONE ? ME_NONE : me_last(open + 2u, e, [&](uint32_t x) { return me_is(text, x, e, "};"); });
        sp.x = lo;
        if (close == ME_NONE) { sp.y = me_trim(text, lo, e, ';') - lo; return; }
        const uint32_t tail_end = me_trim(text, close + 2u, e, ';');
        if (tail_end > close + 2u) { sp.y = open - lo; sp.z = close + 2u; sp.w = tail_end - sp.z; }
        else sp.y = me_trim(text, lo, open, ';') - lo;   // (the cut reaches into the part in front of the removed span)
    } else if (t0 == 'O' && t1 == 'X') {
        kf = ME_OX;
        if (!me_field(text, v, e, a, b) || b - a < 12u) { kf |= ME_F_SKIP; return; }
        sp.x = a + 12u; sp.y = me_trim(text, a + 12u, b, ';') - sp.x;
    } else if (t0 == 'O' && t1 == 'S') {
        kf = ME_OS;
        sp.x = v; sp.y = me_trim(text, v, e, '.') - v;
    } else if (t0 == 'O') {   // OC
        kf = ME_OC;
        sp.x = v; sp.y = e - v;
    } else if (t0 == 'D') {   // DR
        if (!me_field(text, v, e, a, b)) { kf = ME_DROP; return; }
        const uint32_t n = b - a;
        if (n == 3u && me_is(text, a, b, "GO;")) kf = ME_GO;
        else if (n == 5u && me_is(text, a, b, "KEGG;")) kf = ME_KEGG;
        else if (n == 7u && me_is(text, a, b, "BioCyc;")) kf = ME_BIOCYC;
        else if (n == 6u && me_is(text, a, b, "HAMAP;")) kf = ME_HAMAP;
        else return;
        if (!me_field(text, b, e, a1, b1)) { kf |= ME_F_SKIP; return; }
        sp.x = a1; sp.y = me_trim(text, a1, b1, ';') - a1;
    } else if (t0 == 'S') {   // SQ: strconv.Atoi of field 1, its error ignored
        kf = ME_SQ;
        if (!me_field(text, v, e, a, b) || !me_field(text, b, e, a1, b1)) { kf |= ME_F_SKIP; return; }
        const bool neg = text[a1] == '-';
        if (neg || text[a1] == '+') a1++;
        if (a1 >= b1 || neg) return;   // (a negative length is below 7 like 0)
        if (me_first(a1, b1, [&](uint32_t x) { return text[x] < '0' || text[x] > '9'; }) != ME_NONE) return;
        const uint32_t z = me_first(a1, b1, [&](uint32_t x) { return text[x] != '0'; });
        if (z == ME_NONE) return;
        unsigned long long val = 0xFFFFFFFFull;   // 11 digits and more: above what any text holds (or refused: dropped alike)
        if (b1 - z <= 10u) {
            val = 0;
            for (uint32_t q = z; q < b1; q++) val = val * 10u + (text[q] - '0');
            if (val > 0xFFFFFFFFull) val = 0xFFFFFFFFull;
        }
        sp.y = (uint32_t)val;
    } else {   // two spaces: a sequence line
        kf = ME_SEQ;
        sp.x = v; sp.w = e - v;
        sp.y = me_count(v, e, [&](uint32_t x) { return text[x] != ' '; });
    }
}

__global__ __launch_bounds__(PT_BLOCK) void me_read_kernel(MeParams f)
{
    const PtParams &p = f.pt;
    const uint32_t n_work = (uint32_t)f.res[ME_R_WORK];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * (PT_BLOCK / 64);
    for (uint64_t w = (uint64_t)blockIdx.x * (PT_BLOCK / 64) + (threadIdx.x >> 6); w < n_work; w += stride) {
        const uint32_t i = f.work[w];
        uint32_t s;
        const uint32_t len = pt_line_len(p, i, s);
        uint32_t kf;
        uint4 sp;
        me_read_line(p.text, s, s + len, kf, sp);
        if (lane == 0) { f.kf[i] = kf; f.span[i] = sp; }
    }
}

// 64 bytes a step
__device__ __forceinline__ void me_copy(uint8_t *dst, const uint8_t *src, uint32_t n)
{
    for (uint32_t o = threadIdx.x & 63u; o < n; o += 64u) dst[o] = src[o];
}
// the non-space bytes of src[0, n) to out[done ..), what lies at `clip` and beyond left out; returns how many there were
// (UPPER: 'a'..'z' upper-cased on the way, the GBK reader's rule)
template <bool UPPER = false> __device__ __forceinline__ uint32_t me_squeeze(uint8_t *out, uint32_t done, uint32_t clip, const uint8_t *src, uint32_t n)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t at = 0; at < n; at += 64u) {
        const uint32_t q = at + lane;
        uint32_t c = q < n ? src[q] : ' ';
        if (UPPER && c >= 'a' && c <= 'z') c -= 32u;
        const unsigned long long m = __ballot(c != ' ');
        const uint32_t to = done + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (c != ' ' && to < clip) out[to] = (uint8_t)c;
        done += (uint32_t)__popcll(m);
    }
    return done;
}

// EMIT = false: entry k is decided and sized.  EMIT = true: the kept entries are written.  Both take the contributing lines
// of the entry in order, the state wave-uniform: lane c < 10 of `w` holds the bytes cell c has so far, bit c of `had` says
// that cell c has had a contribution (Organism, the DR cells) or a non-empty one (ProteinName, FullTaxonomy).
template <bool EMIT> __global__ __launch_bounds__(PT_BLOCK) void me_fold_kernel(MeParams f)
{
    const PtParams &p = f.pt;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * (PT_BLOCK / 64);
    for (uint64_t k64 = (uint64_t)blockIdx.x * (PT_BLOCK / 64) + (threadIdx.x >> 6); k64 < f.n_terms; k64 += stride) {
        const uint32_t k = (uint32_t)k64;
        const uint32_t first = k ? f.term_line[k - 1u] + 1u : 0u, end = f.term_line[k];
        MeEnt en;
        uint32_t r = 0, cell_at = 0;   // EMIT: the record; lane c: where cell c starts in featb
        uint64_t seq_at = 0, id_at = 0, full_at = 0;
        bool full = false;
        if (EMIT) {
            en = f.ent[k];
            if (!en.keep) continue;
            const unsigned long long a = f.ent_a[k], b = f.ent_b[k], c = f.ent_c[k];
            r = (uint32_t)(a >> 32);
            if (r >= f.res[ME_R_RECORDS]) continue;   // (both passes decide alike, so this never holds: the buffers are sized from the first)
            seq_at = (uint32_t)a; id_at = (uint32_t)b;
            full = en.held > en.declared;
            full_at = (uint32_t)c;
            uint32_t before = 0;
            for (uint32_t j = 0; j < (uint32_t)ME_FEATURES; j++) { if (j == lane) cell_at = (uint32_t)(b >> 32) + before; before += en.feat_len[j]; }
            if (lane < (uint32_t)ME_FEATURES) f.feat_off[(uint64_t)r * ME_FEATURES + lane] = cell_at;
            if (lane == 0) {
                f.ids[r] = (uint32_t)(f.nb_before + k64 + 1u);
                f.offsets[r] = seq_at;
                f.id_off[r] = id_at;
                if (full) { f.full_rec[(uint32_t)(c >> 32)] = r; f.full_off[(uint32_t)(c >> 32)] = full_at; }
            }
        } else {
            en.keep = 0; en.declared = 0; en.held = 0; en.id_len = 0;
            en.id_line = en.gn_line = en.ec_line = en.ox_line = en.rec_line = ME_NONE;
        }
        uint32_t w = 0, had = 0, held = 0, declared = 0;
        bool drop = false, gn_done = false;
        for (uint64_t base = first; base < end && !drop; base += 64) {
            const uint64_t i64 = base + lane;
            const uint32_t my_kf = i64 < end ? f.kf[(uint32_t)i64] : 0u;
            const uint32_t my_kind = my_kf & ME_KIND;
            uint4 my_sp = make_uint4(0, 0, 0, 0);
            if (my_kind != ME_NONE_K && my_kind != ME_DROP && !(my_kf & ME_F_SKIP)) my_sp = f.span[(uint32_t)i64];
            unsigned long long todo = __ballot(my_kind != ME_NONE_K);
            // (a line that drops the entry: the reference stops there; nothing is kept of the entry either way)
            if (!EMIT && __ballot(my_kind == ME_DROP || ((my_kf & ME_F_SKIP) && my_kind != ME_GN))) { drop = true; break; }
            while (todo) {
                const int b = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const uint32_t kf = __shfl(my_kf, b, 64), kind = kf & ME_KIND, line = (uint32_t)base + (uint32_t)b;
                const uint32_t src0 = __shfl(my_sp.x, b, 64), len0 = __shfl(my_sp.y, b, 64), src1 = __shfl(my_sp.z, b, 64), len1 = __shfl(my_sp.w, b, 64);
                if (kind == ME_ID) {
                    if (!EMIT) { en.id_line = line; en.id_len = len0; }
                    else if (line == en.id_line) me_copy(f.idb + id_at, p.text + src0, len0);
                } else if (kind == ME_SQ) {
                    declared = len0;
                } else if (kind == ME_SEQ) {
                    if (EMIT) {
                        (void)me_squeeze(f.seqs + seq_at, held, en.declared, p.text + src0, len1);
                        if (full) (void)me_squeeze(f.fullb + full_at, held, ME_NONE, p.text + src0, len1);
                    }
                    held += len0;
                } else if (kind == ME_GN) {
                    if (!EMIT) {
                        if (!gn_done && (kf & (ME_F_SKIP | ME_F_VALUE))) {
                            gn_done = true;
                            if (kf & ME_F_SKIP) { drop = true; break; }
                            en.gn_line = line;
                            if (lane == ME_GN - 1) w = len0;
                        }
                    } else if (line == en.gn_line) me_copy(f.featb + __shfl(cell_at, ME_GN - 1, 64), p.text + src0, len0);
                } else {   // a cell
                    const uint32_t c = kind == ME_SUB ? 0u : kind - 1u, n = len0 + len1;
                    const bool last_wins = kind == ME_REC || kind == ME_EC || kind == ME_OX;
                    uint32_t sep = 0;     // bytes of separator in front: ";;" ";" " "
                    bool counts = true;   // EMIT: lines that a later one replaced are passed over
                    if (last_wins) {
                        if (!EMIT) {
                            if (kind == ME_REC) en.rec_line = line; else if (kind == ME_EC) en.ec_line = line; else en.ox_line = line;
                            if (lane == c) w = 0;
                            had &= ~(1u << c);
                        } else counts = line == (kind == ME_REC ? en.rec_line : kind == ME_EC ? en.ec_line : en.ox_line);
                    } else if (kind == ME_SUB) {
                        if (EMIT && en.rec_line != ME_NONE && line < en.rec_line) counts = false;
                        sep = (had & 1u) ? 2u : 0u;
                    } else sep = (had >> c) & 1u;
                    if (!counts) continue;
                    if (EMIT) {
                        uint8_t *to = f.featb + __shfl(cell_at, (int)c, 64) + __shfl(w, (int)c, 64);
                        if (lane < sep) to[lane] = (kind == ME_OS || kind == ME_OC) ? ' ' : ';';
                        me_copy(to + sep, p.text + src0, len0);
                        me_copy(to + sep + len0, p.text + src1, len1);
                    }
                    if (lane == c) w += sep + n;
                    if (kind == ME_REC || kind == ME_SUB || kind == ME_OC) { if (n) had |= 1u << c; }
                    else had |= 1u << c;
                }
            }
        }
        if (EMIT) continue;
        if (!drop && declared >= (uint32_t)KAAMER_KMER_SIZE && declared <= held) { en.keep = 1; en.declared = declared; en.held = held; }
        for (uint32_t j = 0; j < (uint32_t)ME_FEATURES; j++) en.feat_len[j] = __shfl(w, (int)j, 64);
        en.pad = 0;
        if (lane == 0) f.ent[k] = en;
    }
}

// what entry k adds to the three running sums
__device__ __forceinline__ void me_ent_sums(const MeParams &f, uint32_t k, unsigned long long &a, unsigned long long &b, unsigned long long &c)
{
    a = b = c = 0;
    const MeEnt &en = f.ent[k];
    if (!en.keep) return;
    uint32_t cells = 0;
    for (int j = 0; j < ME_FEATURES; j++) cells += en.feat_len[j];
    a = (unsigned long long)en.declared | (1ull << 32);
    b = (unsigned long long)en.id_len | ((unsigned long long)cells << 32);
    if (en.held > en.declared) c = (unsigned long long)en.held | (1ull << 32);
}

template <bool EMIT> __global__ __launch_bounds__(PT_LINES) void me_ent_kernel(MeParams f)
{
    __shared__ unsigned long long lds64[PT_LINES];
    const uint32_t blk = blockIdx.x;
    const int t = threadIdx.x;
    const uint64_t k64 = (uint64_t)blk * PT_LINES + t;
    unsigned long long a = 0, b = 0, c = 0;
    if (k64 < f.n_terms) me_ent_sums(f, (uint32_t)k64, a, b, c);
    // (a text has fewer than 2^32 bytes, and no cell byte but a separator is not one of the text's: every half fits 32 bits)
    const unsigned long long a_incl = pt_scan<false>(a, lds64, MfAdd64());
    const unsigned long long a_total = lds64[PT_LINES - 1];
    const unsigned long long b_incl = pt_scan<false>(b, lds64, MfAdd64());
    const unsigned long long b_total = lds64[PT_LINES - 1];
    const unsigned long long c_incl = pt_scan<false>(c, lds64, MfAdd64());
    const unsigned long long c_total = lds64[PT_LINES - 1];
    if (!EMIT) {
        if (t == 0) { f.eb_a[blk] = a_total; f.eb_b[blk] = b_total; f.eb_c[blk] = c_total; }
        return;
    }
    if (blk == 0 && t == 0) {
        const unsigned long long n_rec = f.res[ME_R_RECORDS], n_full = f.res[ME_R_FULL];
        f.offsets[n_rec] = f.res[ME_R_SEQ_BYTES];
        f.id_off[n_rec] = f.res[ME_R_ID_BYTES];
        f.feat_off[n_rec * f.n_feat] = f.res[ME_R_FEAT_BYTES];
        f.full_off[n_full] = f.res[ME_R_FULL_BYTES];
    }
    if (k64 < f.n_terms) {
        f.ent_a[k64] = f.eb_a[blk] + a_incl - a;
        f.ent_b[k64] = f.eb_b[blk] + b_incl - b;
        f.ent_c[k64] = f.eb_c[blk] + c_incl - c;
    }
}

__global__ __launch_bounds__(PT_LINES) void me_ent_scan_kernel(MeParams f)
{
    __shared__ unsigned long long lds64[PT_LINES];
    __shared__ unsigned long long carry_a, carry_b, carry_c;
    const uint32_t nb = (uint32_t)(((uint64_t)f.n_terms + PT_LINES - 1) / PT_LINES);
    const int t = threadIdx.x;
    if (t == 0) { carry_a = 0; carry_b = 0; carry_c = 0; }
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += PT_LINES) {
        const uint32_t b = base + t;
        const unsigned long long va = b < nb ? f.eb_a[b] : 0ull, vb = b < nb ? f.eb_b[b] : 0ull, vc = b < nb ? f.eb_c[b] : 0ull;
        const unsigned long long ia = pt_scan<false>(va, lds64, MfAdd64());
        const unsigned long long ib = pt_scan<false>(vb, lds64, MfAdd64());
        const unsigned long long ic = pt_scan<false>(vc, lds64, MfAdd64());
        const unsigned long long a0 = carry_a, b0 = carry_b, c0 = carry_c;
        if (b < nb) { f.eb_a[b] = a0 + ia - va; f.eb_b[b] = b0 + ib - vb; f.eb_c[b] = c0 + ic - vc; }
        __syncthreads();
        if (t == PT_LINES - 1) { carry_a = a0 + ia; carry_b = b0 + ib; carry_c = c0 + ic; }
        __syncthreads();
    }
    if (t == 0) {
        f.res[ME_R_RECORDS] = carry_a >> 32;
        f.res[ME_R_SEQ_BYTES] = (uint32_t)carry_a;
        f.res[ME_R_ID_BYTES] = (uint32_t)carry_b;
        f.res[ME_R_FEAT_BYTES] = carry_b >> 32;
        f.res[ME_R_FULL] = carry_c >> 32;
        f.res[ME_R_FULL_BYTES] = (uint32_t)carry_c;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// One text's reader, as MfReader is: after me_read the kept entries lie on the device: d_seqs (32 bytes of slack behind the
// last residue), offsets, ids, the EntryId bytes, the cells with their offsets, and the whole strings of the records that
// hold more than they declare.
struct MeReader {
    int device = 0;
    DevBuf<uint8_t> d_text, d_seqs, d_idb, d_featb, d_fullb;
    DevBuf<uint32_t> d_cnt32, d_line32, d_ent32, d_rec32;
    DevBuf<uint4> d_span;
    DevBuf<unsigned long long> d_res, d_ent64, d_rec64;
    MeParams f{};
    uint64_t n_rec = 0, seq_bytes = 0, id_bytes = 0, feat_bytes = 0, n_full = 0, full_bytes = 0;
    const char *format = "embl";             // the format that was read, for messages and the trace
    std::vector<std::string> feature_names;   // its columns
    ~MeReader() { (void)hipSetDevice(device); }   // (before the buffers go)
};

static unsigned me_wave_grid(uint64_t waves, int n_cu)
{
    uint64_t g = (waves + PT_BLOCK / 64 - 1) / (PT_BLOCK / 64);
    const uint64_t g_max = (uint64_t)n_cu * 8;
    if (g > g_max) g = g_max;
    return (unsigned)(g < 1 ? 1 : g);
}

// What a flat-file format puts into me_read: its name and columns, and the launches between the shared steps (the line
// starts, the terminators, the entry scans).  classify leaves kf (ME_TERM on every terminator line), the block's terminator
// count and a worklist; read_lines finishes every line's record; fold<0> leaves MeEnt, fold<1> writes the kept entries.
struct MeEmbl {
    typedef MeReader Reader;
    static const char *name() { return "embl"; }
    static std::vector<std::string> feature_names()   // EMBL_DEF_FTS, inputEMBL.go:43
    {
        return { "ProteinName", "GeneName", "EC", "GO", "KEGG_ID", "BioCyc_ID", "HAMAP", "Organism", "TaxId", "FullTaxonomy" };
    }
    static int lines_ready(MeReader &, size_t, size_t) { return KAAMER_OK; }
    static void classify(MeReader &m, uint32_t n_blk) { hipLaunchKernelGGL(me_classify_kernel, dim3(n_blk), dim3(PT_LINES), 0, 0, m.f); }
    static int entries_ready(MeReader &, size_t) { return KAAMER_OK; }
    static void read_lines(MeReader &m, size_t n_work, uint32_t, int n_cu)
    {
        if (n_work) hipLaunchKernelGGL(me_read_kernel, dim3(me_wave_grid(n_work, n_cu)), dim3(PT_BLOCK), 0, 0, m.f);
    }
    static void fold(MeReader &m, bool emit, unsigned grid)
    {
        if (emit) hipLaunchKernelGGL(me_fold_kernel<true>, dim3(grid), dim3(PT_BLOCK), 0, 0, m.f);
        else hipLaunchKernelGGL(me_fold_kernel<false>, dim3(grid), dim3(PT_BLOCK), 0, 0, m.f);
    }
    static void release(MeReader &) {}
};

template <class F> static int me_read(typename F::Reader &m, const char *text, uint64_t len, uint64_t nb_before, int device)
{
    m.format = F::name();
    m.feature_names = F::feature_names();
    int n_dev = 0;
    if (device < 0 || hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) {
        (void)hipGetLastError();
        return kaamer_fail(KAAMER_E_ARG, "makedb_%s_device: there is no device %d", m.format, device);
    }
    HIPCHK(hipSetDevice(device));
    m.device = device;
    hipDeviceProp_t prop;
    const int n_cu = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
    MfTrace tr;
    tr.format = m.format;
    tr.bytes = len;
    tr.begin();
    const uint32_t n_tiles = (uint32_t)((len + PT_TILE - 1) / PT_TILE);
    int rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_text, (size_t)len + 2 * PT_PIECE), want(m.d_cnt32, (size_t)n_tiles + 1 + 2),
                                                  want(m.d_res, (size_t)PT_R_N + ME_R_N) });
    if (rc) return rc;
    if (len) HIPCHK(hipMemcpy(m.d_text, text, (size_t)len, hipMemcpyHostToDevice));
    tr.lap("upload");
    MeParams &f = m.f;
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
    f.n_feat = (uint32_t)m.feature_names.size();
    HIPCHK(hipMemset(m.d_res, 0, (PT_R_N + ME_R_N) * sizeof(unsigned long long)));
    if (n_tiles) hipLaunchKernelGGL(pt_count_kernel, dim3(n_tiles), dim3(PT_BLOCK), 0, 0, p);
    hipLaunchKernelGGL(pt_tile_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, p);
    HIPCHK(hipGetLastError());
    unsigned long long h_res[PT_R_N + ME_R_N];
    HIPCHK(hipMemcpy(h_res, m.d_res, sizeof h_res, hipMemcpyDeviceToHost));
    tr.lap("count lines");
    const unsigned long long nl = h_res[PT_R_NL];
    if (nl < 1 || nl > 0xFFFFFFF0ull) return kaamer_fail(KAAMER_E_CAPACITY, "makedb_%s_device: %llu lines in one text: cut it (kaamer_text_cut_embl)", m.format, nl);
    const size_t nb = (size_t)((nl + PT_LINES - 1) / PT_LINES) + 1;
    rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_line32, 3 * ((size_t)nl + 2) + 2 * nb), want(m.d_span, (size_t)nl + 1) });
    if (rc) return rc;
    {
        uint32_t *a = m.d_line32;
        p.line_start = a; a += nl + 2;
        f.kf = a; a += nl + 2;
        f.work = a; a += nl + 2;
        f.blk_term = a; a += nb; f.blk_term_base = a;
        f.span = m.d_span;
    }
    p.line_cap = (uint32_t)nl;
    const uint32_t n_blk = (uint32_t)(nb - 1);
    rc = F::lines_ready(m, (size_t)nl, nb);
    if (rc) return rc;
    hipLaunchKernelGGL(me_lines_kernel, dim3(n_tiles ? n_tiles : 1u), dim3(PT_BLOCK), 0, 0, f);
    tr.lap("lines");
    F::classify(m, n_blk);
    hipLaunchKernelGGL(me_term_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, f);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(h_res, m.d_res, sizeof h_res, hipMemcpyDeviceToHost));
    tr.lap("classify");
    const unsigned long long *r = h_res + PT_R_N;
    const size_t n_terms = (size_t)r[ME_R_TERMS], n_work = (size_t)r[ME_R_WORK];
    const size_t neb = (n_terms + PT_LINES - 1) / PT_LINES + 1;
    static_assert(sizeof(MeEnt) % sizeof(uint32_t) == 0, "MeEnt is words");
    rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_ent32, (n_terms + 1) * (1 + sizeof(MeEnt) / sizeof(uint32_t))), want(m.d_ent64, 3 * (n_terms + 1) + 3 * neb) });
    if (rc) return rc;
    f.n_terms = (uint32_t)n_terms;
    f.ent = reinterpret_cast<MeEnt *>(m.d_ent32.get());
    f.term_line = m.d_ent32 + (n_terms + 1) * (sizeof(MeEnt) / sizeof(uint32_t));
    f.ent_a = m.d_ent64; f.ent_b = f.ent_a + (n_terms + 1); f.ent_c = f.ent_b + (n_terms + 1);
    f.eb_a = f.ent_c + (n_terms + 1); f.eb_b = f.eb_a + neb; f.eb_c = f.eb_b + neb;
    const uint32_t n_eblk = (uint32_t)(neb - 1);
    rc = F::entries_ready(m, n_terms);
    if (rc) return rc;
    if (n_terms) hipLaunchKernelGGL(me_terms_kernel, dim3(n_blk), dim3(PT_LINES), 0, 0, f);
    F::read_lines(m, n_work, n_blk, n_cu);
    tr.lap("read lines");
    if (n_terms) {
        F::fold(m, false, me_wave_grid(n_terms, n_cu));
        hipLaunchKernelGGL(me_ent_kernel<false>, dim3(n_eblk), dim3(PT_LINES), 0, 0, f);
    }
    hipLaunchKernelGGL(me_ent_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, f);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(h_res, m.d_res, sizeof h_res, hipMemcpyDeviceToHost));
    tr.lap("entries");
    m.n_rec = r[ME_R_RECORDS]; m.seq_bytes = r[ME_R_SEQ_BYTES]; m.id_bytes = r[ME_R_ID_BYTES]; m.feat_bytes = r[ME_R_FEAT_BYTES];
    m.n_full = r[ME_R_FULL]; m.full_bytes = r[ME_R_FULL_BYTES];
    const size_t n = (size_t)m.n_rec, nf = (size_t)m.n_full;
    if ((unsigned long long)n * f.n_feat > 0xFFFFFFF0ull)
        return kaamer_fail(KAAMER_E_CAPACITY, "makedb_%s_device: %llu records in one text: cut it (kaamer_text_cut_embl)", m.format, (unsigned long long)m.n_rec);
    rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_rec32, (n + 1) + (nf + 1)), want(m.d_rec64, 2 * (n + 1) + (n * f.n_feat + 1) + (nf + 1)),
                                              want(m.d_seqs, (size_t)m.seq_bytes + 3 * PT_PIECE), want(m.d_idb, (size_t)m.id_bytes + 2 * PT_PIECE),
                                              want(m.d_featb, (size_t)m.feat_bytes + 2 * PT_PIECE), want(m.d_fullb, (size_t)m.full_bytes + 2 * PT_PIECE) });
    if (rc) return rc;
    f.ids = m.d_rec32; f.full_rec = m.d_rec32 + (n + 1);
    f.offsets = reinterpret_cast<uint64_t *>(m.d_rec64.get());
    f.id_off = f.offsets + (n + 1); f.feat_off = f.id_off + (n + 1); f.full_off = f.feat_off + (n * f.n_feat + 1);
    f.seqs = m.d_seqs; f.idb = m.d_idb; f.featb = m.d_featb; f.fullb = m.d_fullb;
    {   // (the builder's window kernel reads up to 17 bytes behind the last residue: they are zero, not left-over)
        const size_t whole = (size_t)(m.seq_bytes / PT_PIECE) * PT_PIECE;
        HIPCHK(hipMemset(m.d_seqs + whole, 0, (size_t)m.seq_bytes - whole + 3 * PT_PIECE));
    }
    hipLaunchKernelGGL(me_ent_kernel<true>, dim3(n_eblk ? n_eblk : 1u), dim3(PT_LINES), 0, 0, f);
    if (n_terms) F::fold(m, true, me_wave_grid(n_terms, n_cu));
    HIPCHK(hipGetLastError());
    tr.lap("entries, emit");
    return KAAMER_OK;
}

// the host's table of what me_read left on the device: bulk copies into the table's arrays, then makedb.cpp's by_id and KStats
static int me_table(MeReader &m, kaamer_proteins **out)
{
    MfTrace tr;
    tr.format = m.format;
    tr.bytes = m.f.pt.n;
    tr.begin();
    kaamer_table_arrays a;
    kaamer_proteins *t = kaamer_proteins_table_new(m.feature_names, (uint32_t)m.n_rec, m.seq_bytes, m.id_bytes, m.feat_bytes, &a);
    if (!t) return kaamer_fail(KAAMER_E_NOMEM, "makedb_%s_device: the table", m.format);
    tr.lap("host table");
    const size_t n = (size_t)m.n_rec, nf = (size_t)m.n_full;
    hipError_t e = hipSuccess;
    auto get = [&](void *dst, const void *src, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); };
    get(a.ids, m.f.ids, n * 4);
    get(a.offsets, m.f.offsets, (n + 1) * 8);
    get(a.seqs, m.d_seqs, (size_t)m.seq_bytes);
    get(a.entry_off, m.f.id_off, (n + 1) * 8);
    get(a.entry_ids, m.d_idb, (size_t)m.id_bytes);
    get(a.feature_off, m.f.feat_off, (n * m.f.n_feat + 1) * 8);
    get(a.features, m.d_featb, (size_t)m.feat_bytes);
    std::vector<uint32_t> full_rec;
    std::vector<uint64_t> full_off;
    std::vector<char> full_bytes;
    try { full_rec.resize(nf); full_off.resize(nf + 1); full_bytes.resize((size_t)m.full_bytes); }
    catch (const std::bad_alloc &) { kaamer_proteins_free(t); return kaamer_fail(KAAMER_E_NOMEM, "makedb_%s_device: the whole sequences", m.format); }
    if (nf) {
        get(full_rec.data(), m.f.full_rec, nf * 4);
        get(full_off.data(), m.f.full_off, (nf + 1) * 8);
        get(full_bytes.data(), m.d_fullb, (size_t)m.full_bytes);
    }
    if (e != hipSuccess) { kaamer_proteins_free(t); return kaamer_fail(KAAMER_E_HIP, "makedb_%s_device: download: %s", m.format, hipGetErrorString(e)); }
    tr.lap("download");
    kaamer_proteins_table_seal(t);
    if (nf && kaamer_proteins_table_full_seqs(t, full_rec.data(), full_off.data(), full_bytes.data(), (uint32_t)nf)) {
        kaamer_proteins_free(t);
        return kaamer_fail(KAAMER_E_NOMEM, "makedb_%s_device: the whole sequences", m.format);
    }
    *out = t;
    return KAAMER_OK;
}

// the text the host reader would read: inflated when it starts with the gzip signature (inputEMBL.go:76-84)
static int me_plain(const char *who, const char *&text, uint64_t &len, std::string &inflated)
{
    if (!kaamer_is_gzip(text, len)) return KAAMER_OK;
    const int rc = kaamer_gunzip(text, len, &inflated);
    if (rc) return rc;
    if (inflated.size() > 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_ARG, "%s: the inflated text holds more than 2^32 - 1 bytes: inflate it and cut it (kaamer_text_cut_embl)", who);
    text = inflated.data(); len = inflated.size();
    return KAAMER_OK;
}

// text -> the reader's buffers -> the build that takes device buffers (it sees the indexed prefixes) -> the table's host copy
template <class F> static int me_build(typename F::Reader &m, const char *who, const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                    kaamer_proteins **proteins, kaamer_device_image *di)
{
    std::string inflated;
    int rc = me_plain(who, text, len, inflated);
    if (rc) return rc;
    rc = me_read<F>(m, text, len, 0, device);
    if (rc) return rc;
    F::release(m);
    m.d_text.reset(); m.d_cnt32.reset(); m.d_line32.reset(); m.d_span.reset(); m.d_ent32.reset(); m.d_ent64.reset();   // (the build wants the room; hipFree waits for the fold)
    rc = kaamer_build_resident(m.d_seqs, m.f.offsets, m.f.ids, (uint32_t)m.n_rec, m.seq_bytes, shard, n_shards, load_factor, device, di);
    if (rc) return rc;
    rc = me_table(m, proteins);
    if (rc) { (void)hipFree(di->d_buckets); (void)hipFree(di->d_arena); }
    return rc;
}

extern "C" {

int kaamer_makedb_embl_device(const char *text, uint64_t len, uint64_t nb_before, int device, kaamer_proteins **out)
{
    if (len > 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_ARG, "makedb_embl_device: a text holds at most 2^32 - 1 bytes: cut it (kaamer_text_cut_embl)");
    if (!out || (!text && len)) return kaamer_fail(KAAMER_E_ARG, "makedb_embl_device: bad argument");
    *out = nullptr;
    std::string inflated;
    int rc = me_plain("makedb_embl_device", text, len, inflated);
    if (rc) return rc;
    MeReader m;
    rc = me_read<MeEmbl>(m, text, len, nb_before, device);
    if (rc) return rc;
    return me_table(m, out);
}

int kaamer_image_build_embl_device(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                                   kaamer_proteins **proteins, kaamer_image **image)
{
    int rc = mf_build_args("image_build_embl_device", text, len, shard, n_shards, proteins, image, "(kaamer_text_cut_embl)");
    if (rc) return rc;
    *proteins = nullptr; *image = nullptr;
    MeReader m;
    kaamer_device_image di;
    rc = me_build<MeEmbl>(m, "image_build_embl_device", text, len, shard, n_shards, load_factor, device, proteins, &di);
    if (rc) return rc;
    rc = kaamer_device_image_download(&di, image);
    if (rc) { kaamer_proteins_free(*proteins); *proteins = nullptr; }
    return rc;
}

int kaamer_index_build_embl(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                            kaamer_proteins **proteins, kaamer_index **out)
{
    int rc = mf_build_args("index_build_embl", text, len, shard, n_shards, proteins, out, "(kaamer_text_cut_embl)");
    if (rc) return rc;
    *proteins = nullptr; *out = nullptr;
    MeReader m;
    kaamer_device_image di;
    rc = me_build<MeEmbl>(m, "index_build_embl", text, len, shard, n_shards, load_factor, device, proteins, &di);
    if (rc) return rc;
    rc = index_of_device_image(di, device, out);
    if (rc) { kaamer_proteins_free(*proteins); *proteins = nullptr; }
    return rc;
}

}  // extern "C"
