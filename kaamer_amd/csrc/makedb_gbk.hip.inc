// makedb_gbk.hip.inc — runGBK + processProteinInputGBK (pkg/makedb/inputGBK.go:65-118, 186-301) on the device: the text of
// a GenBank / GenPept flat file in, the protein table with its three feature columns out, the packed sequences left in HBM
// in the layout bd_windows_kernel reads (included by search.hip after makedb_embl.hip.inc: the tiling, pt_count_kernel,
// pt_tile_scan_kernel, the workgroup scans and pt_line_len are the parser's; the line starts, the terminators, the entry
// scans, the wave steps me_first / me_last / me_count / me_field / me_copy / me_squeeze and the driver me_read are the EMBL
// reader's; the trace, the grids and the build hand-over are the FASTA reader's).  kaamer_makedb_gbk (makedb.cpp,
// process_gbk_entry + makedb_flat) is the host's statement of the same rules, and where the words below and that code
// differ, the code holds.
//   lines    split at '\n', a last piece without '\n' is a line, one trailing '\r' is dropped.  A line that is then exactly
//            "//" ends an entry and takes a number, even when the entry is empty.  Lines shorter than 2 bytes change nothing
//            and contribute nothing.  What lies behind the text's last "//" belongs to no entry
//   token    the line with leading and trailing ' ' removed (spaces only, a tab is a byte of the token), up to its first ' ';
//            an all-space line has the empty token.  Compared case-sensitively, it sets the section state:
//              0  LOCUS ACCESSION KEYWORDS SOURCE COMMENT REFERENCE DBLINK DBSOURCE      1  DEFINITION     2  VERSION
//              3  ORGANISM     4  FEATURES     5  ORIGIN     6  "//" (" //" and "// x" are such lines inside an entry)
//            any other token leaves the state as it is; every entry starts in state 0.  A continuation line whose first
//            word happens to be a keyword switches the state: the quirk is kept
//   contribution   taken under the state AFTER the line's own token:
//              1  [12:] is appended to ProteinName, " " in front when what is gathered so far is non-empty (an all-space
//                 line of 12 bytes or more so adds a trailing space)
//              2  EntryId is the first field of [12:] (fields split at ' ' and '\t'..'\r'); the last such line wins
//              3  while Organism is empty, [12:] becomes Organism (an empty [12:] leaves it empty: the next line tries
//                 again); otherwise [12:] is appended to FullTaxonomy, " " in front when that is non-empty
//              5  [10:] with every ' ' removed and 'a'..'z' upper-cased, other bytes (those >= 0x80 too) as they are; the
//                 ORIGIN line itself contributes this way
//              0, 4, 6  nothing
//   Skip     (the whole entry is dropped; where the reference would panic) a line of 2 to 11 bytes in state 1, 2 or 3;  a
//            line of 2 to 9 bytes in state 5, a bare ORIGIN among them;  a state-2 line with no field behind column 12
//   drops    the joined ProteinName contains ", partial" -- the match may span a join: one line ends in ',' and the next
//            one's [12:] starts with "partial";  fewer than 7 residues
//   ProteinName, last step   from the first " [" to the last "]." behind it is removed, on the joined string (the " [" may
//            be a join's space in front of a line that starts with '['); without a "]." at or behind the byte after the
//            " [" nothing is removed (drop_greedy)
//   table    feature_names = GBK_DEF_FTS (ProteinName Organism FullTaxonomy); no record holds more than it indexes
//   ids      record k of the text (1-based ordinal of its "//") gets id (uint32_t)(nb_before + k)
//
// The shape: what a line is depends on the last keyword line in front of it, so the reader first gives every line the
// state its own token sets (or none), then carries the state along the lines by a segmented scan, and only then knows
// which lines to read.  A terminator acts in that scan as a keyword of state 0: the carry of a block of PT_LINES lines is
// the state its last keyword or terminator sets, or none.  No lane or wave walks an entry's lines to find a state, no lane
// walks a line of unbounded length: a lane looks at the first MG_LEAD bytes of its line, a line that is all spaces that far
// is read 64 bytes a step by a wave with ballots.  The spans of state 1 and 3 lines follow from their length alone; state 2
// and state 5 lines are read by a wave each (first field, non-space count).  Then a wave per entry, as in the EMBL reader:
// it folds the line records 64 a step and copies the entry's bytes itself.  The joined ProteinName is written in the first
// fold, into a scratch of the text's size at the offset of the entry's first DEFINITION byte -- every joined byte lies at or
// in front of the text byte it came from, so entries never overlap -- and ", partial", " [" and "]." are looked for there
// 64 bytes a step, across step edges and across joins alike, since the join's space is an ordinary byte of the scratch.  No
// atomic decides a byte: the atomic adds hand out worklist slots, whose order nothing reads.
//
// Launches, all on the null stream, ordered by the end of each grid (me_read<MgGbk>):
//   pt_count_kernel, pt_tile_scan_kernel   with a line bound of 0: they only count
//   me_lines_kernel      per tile: where every line starts
//   mg_classify_kernel   per PT_LINES lines: terminators; the state the line's token sets when the token starts within
//                        MG_LEAD bytes; the lines that are all spaces that far onto the worklist; the block's terminators
//   me_term_scan_kernel  one workgroup: the terminators in front of every block, T
//   me_terms_kernel      per PT_LINES lines: the line of the k-th terminator
//   mg_lead_kernel       a wave per worklist line: the first non-space byte, 64 bytes a step, and the token's state
//   mg_state_kernel<0>   per PT_LINES lines: the block's carry
//   mg_state_scan_kernel one workgroup: the state every block starts in
//   mg_state_kernel<1>   per PT_LINES lines: every line's state, so its kind; the spans of state 1 and 3 lines, the lines
//                        that drop their entry by length, state 2 and 5 lines onto the (second) worklist
//   mg_read_kernel       a wave per worklist line: the first field of a state-2 line, the non-space count of a state-5 line
//   mg_fold_kernel<0>    a wave per entry: decides it and sizes what it keeps; joins ProteinName and searches it
//   me_ent_kernel<0>, me_ent_scan_kernel, me_ent_kernel<1>   N and every kept entry's bases
//   mg_fold_kernel<1>    a wave per kept entry: id, offsets, the 3 feature offsets, and the bytes: EntryId, ProteinName less
//                        its removed span, Organism, FullTaxonomy with its separators, the sequence squeezed and upper-cased
enum { MG_FEATURES = 3, MG_LEAD = 32 };
enum { MG_ST_NONE = 7u, MG_ST_MASK = 7u };   // 0 .. 6: the state a token sets
#define MG_KW 0x1000u   // kf of a line between mg_classify_kernel and mg_state_kernel<1>: MG_KW | state (ME_TERM: a terminator)
// kinds of a line record behind mg_state_kernel<1> (ME_DROP, ME_TERM and ME_F_SKIP as in the EMBL reader)
enum { MG_NONE_K = 0, MG_DEF, MG_ORG, MG_VER, MG_SEQ };

struct MgParams {
    MeParams me;
    unsigned long long *n_work2;           // the second worklist's length
    uint32_t *blk_state, *blk_state_base;  // per block of PT_LINES lines: its carry, the state it starts in
    uint8_t *join;                         // the joined ProteinNames: entry k's at the text offset of its first DEFINITION byte
    uint4 *pn;                             // entry k: ProteinName = join[x, x + y) + join[z, z + w)
};

// the token that starts at a (text[a] != ' ', a < e) of a line that ends at e: the state it sets (MG_ST_NONE: none)
__device__ __forceinline__ uint32_t mg_keyword(const uint8_t *text, uint32_t a, uint32_t e)
{
    uint32_t n = 0;   // the token's bytes; 11: more than any keyword has
    while (n < 11u && n < e - a && text[a + n] != ' ') n++;
    switch (n) {
    case 2: return me_is(text, a, e, "//") ? 6u : MG_ST_NONE;
    case 5: return me_is(text, a, e, "LOCUS") ? 0u : MG_ST_NONE;
    case 6: return me_is(text, a, e, "ORIGIN") ? 5u : (me_is(text, a, e, "SOURCE") || me_is(text, a, e, "DBLINK")) ? 0u : MG_ST_NONE;
    case 7: return me_is(text, a, e, "VERSION") ? 2u : me_is(text, a, e, "COMMENT") ? 0u : MG_ST_NONE;
    case 8: return me_is(text, a, e, "ORGANISM") ? 3u : me_is(text, a, e, "FEATURES") ? 4u
                 : (me_is(text, a, e, "KEYWORDS") || me_is(text, a, e, "DBSOURCE")) ? 0u : MG_ST_NONE;
    case 9: return (me_is(text, a, e, "ACCESSION") || me_is(text, a, e, "REFERENCE")) ? 0u : MG_ST_NONE;
    case 10: return me_is(text, a, e, "DEFINITION") ? 1u : MG_ST_NONE;
    default: return MG_ST_NONE;
    }
}

__global__ __launch_bounds__(PT_LINES) void mg_classify_kernel(MgParams g)
{
    __shared__ uint32_t lds[PT_LINES];
    __shared__ unsigned long long base_s;
    const MeParams &f = g.me;
    const PtParams &p = f.pt;
    const unsigned long long nl = p.line_cap;
    const uint32_t blk = blockIdx.x;
    if ((unsigned long long)blk * PT_LINES >= nl) return;
    const int t = threadIdx.x;
    const unsigned long long i64 = (unsigned long long)blk * PT_LINES + t;
    const uint32_t i = (uint32_t)i64;
    bool term = false, todo = false;
    if (i64 < nl) {
        uint32_t start, st = MG_ST_NONE;
        const uint32_t len = pt_line_len(p, i, start);
        if (len == 2u && p.text[start] == '/' && p.text[start + 1u] == '/') term = true;
        else if (len >= 2u) {
            const uint32_t lim = len < (uint32_t)MG_LEAD ? len : (uint32_t)MG_LEAD;
            uint32_t a = 0;
            while (a < lim && p.text[start + a] == ' ') a++;
            if (a < lim) st = mg_keyword(p.text, start + a, start + len);
            else todo = len > (uint32_t)MG_LEAD;   // (a shorter line is all spaces: the empty token)
        }
        f.kf[i] = term ? (uint32_t)ME_TERM : MG_KW | st;   // (a worklist line's state is mg_lead_kernel's to write)
    }
    const uint32_t w_incl = pt_scan<false>(todo ? 1u : 0u, lds, PtAdd32());
    const uint32_t w_total = lds[PT_LINES - 1];
    (void)pt_scan<false>(term ? 1u : 0u, lds, PtAdd32());
    if (t == 0) {
        f.blk_term[blk] = lds[PT_LINES - 1];
        base_s = w_total ? atomicAdd(&f.res[ME_R_WORK], (unsigned long long)w_total) : 0ull;   // (slots: their order is read by nobody)
    }
    __syncthreads();
    if (todo) f.work[(uint32_t)base_s + w_incl - 1u] = i;
}

__global__ __launch_bounds__(PT_BLOCK) void mg_lead_kernel(MgParams g)
{
    const MeParams &f = g.me;
    const PtParams &p = f.pt;
    const uint32_t n_work = (uint32_t)f.res[ME_R_WORK];
    const uint64_t stride = (uint64_t)gridDim.x * (PT_BLOCK / 64);
    for (uint64_t w = (uint64_t)blockIdx.x * (PT_BLOCK / 64) + (threadIdx.x >> 6); w < n_work; w += stride) {
        const uint32_t i = f.work[w];
        uint32_t s;
        const uint32_t len = pt_line_len(p, i, s);   // (> MG_LEAD, and all spaces that far)
        const uint32_t a = me_first(s + (uint32_t)MG_LEAD, s + len, [&](uint32_t x) { return p.text[x] != ' '; });
        const uint32_t st = a == ME_NONE ? (uint32_t)MG_ST_NONE : mg_keyword(p.text, a, s + len);
        if ((threadIdx.x & 63u) == 0) f.kf[i] = MG_KW | st;
    }
}

// the later of two lines decides, unless it sets nothing
struct MgLast { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return b != MG_ST_NONE ? b : a; } };

// EMIT = false: the carry of the block.  EMIT = true: with the state the block starts in, every line's record
template <bool EMIT> __global__ __launch_bounds__(PT_LINES) void mg_state_kernel(MgParams g)
{
    __shared__ uint32_t lds[PT_LINES];
    __shared__ unsigned long long base_s;
    const MeParams &f = g.me;
    const PtParams &p = f.pt;
    const unsigned long long nl = p.line_cap;
    const uint32_t blk = blockIdx.x;
    if ((unsigned long long)blk * PT_LINES >= nl) return;
    const int t = threadIdx.x;
    const unsigned long long i64 = (unsigned long long)blk * PT_LINES + t;
    const uint32_t i = (uint32_t)i64;
    uint32_t x = MG_ST_NONE;
    bool term = false;
    if (i64 < nl) {
        const uint32_t kf = f.kf[i];
        term = kf == (uint32_t)ME_TERM;
        x = term ? 0u : kf & MG_ST_MASK;   // (behind a terminator an entry starts in state 0)
    }
    const uint32_t incl = pt_scan<false>(x, lds, MgLast());
    if (!EMIT) {
        if (t == PT_LINES - 1) g.blk_state[blk] = incl;
        return;
    }
    const uint32_t st = incl != MG_ST_NONE ? incl : g.blk_state_base[blk];
    bool todo = false;
    if (i64 < nl && !term) {
        uint32_t start, kind = MG_NONE_K;
        const uint32_t len = pt_line_len(p, i, start);
        uint4 sp = make_uint4(0, 0, 0, 0);
        if (len >= 2u) {
            if (st == 1u || st == 2u || st == 3u) {
                if (len < 12u) kind = ME_DROP;
                else if (st == 2u) { kind = MG_VER; todo = true; }
                else { kind = st == 1u ? MG_DEF : MG_ORG; sp.x = start + 12u; sp.y = len - 12u; }
            } else if (st == 5u) {
                if (len < 10u) kind = ME_DROP;
                else { kind = MG_SEQ; todo = true; }
            }
        }
        f.kf[i] = kind;   // (of a worklist line: which of the two it is; mg_read_kernel may add ME_F_SKIP)
        if (kind == MG_DEF || kind == MG_ORG) f.span[i] = sp;
    }
    const uint32_t w_incl = pt_scan<false>(todo ? 1u : 0u, lds, PtAdd32());
    const uint32_t w_total = lds[PT_LINES - 1];
    if (t == 0) base_s = w_total ? atomicAdd(g.n_work2, (unsigned long long)w_total) : 0ull;   // (slots: their order is read by nobody)
    __syncthreads();
    if (todo) f.work[(uint32_t)base_s + w_incl - 1u] = i;
}

__global__ __launch_bounds__(PT_LINES) void mg_state_scan_kernel(MgParams g)
{
    __shared__ uint32_t lds[PT_LINES];
    __shared__ uint32_t carry_s;
    const unsigned long long nl = g.me.pt.line_cap;
    const uint32_t nb = (uint32_t)((nl + PT_LINES - 1) / PT_LINES);
    const int t = threadIdx.x;
    if (t == 0) carry_s = 0;   // the text starts in state 0
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += PT_LINES) {
        const uint32_t b = base + t;
        const uint32_t v = b < nb ? g.blk_state[b] : (uint32_t)MG_ST_NONE;
        const uint32_t incl = pt_scan<false>(v, lds, MgLast());
        const uint32_t c = carry_s;
        const uint32_t before = t ? lds[t - 1] : (uint32_t)MG_ST_NONE;
        if (b < nb) g.blk_state_base[b] = before != MG_ST_NONE ? before : c;
        __syncthreads();
        if (t == PT_LINES - 1) carry_s = incl != MG_ST_NONE ? incl : c;
        __syncthreads();
    }
}

__global__ __launch_bounds__(PT_BLOCK) void mg_read_kernel(MgParams g)
{
    const MeParams &f = g.me;
    const PtParams &p = f.pt;
    const uint32_t n_work = (uint32_t)*g.n_work2;
    const uint64_t stride = (uint64_t)gridDim.x * (PT_BLOCK / 64);
    for (uint64_t w = (uint64_t)blockIdx.x * (PT_BLOCK / 64) + (threadIdx.x >> 6); w < n_work; w += stride) {
        const uint32_t i = f.work[w];
        uint32_t s;
        const uint32_t len = pt_line_len(p, i, s), e = s + len;
        uint32_t kf = f.kf[i];
        uint4 sp = make_uint4(0, 0, 0, 0);
        if (kf == MG_VER) {   // len >= 12
            uint32_t a, b;
            if (me_field(p.text, s + 12u, e, a, b)) { sp.x = a; sp.y = b - a; }
            else kf |= ME_F_SKIP;
        } else {   // MG_SEQ, len >= 10
            sp.x = s + 10u; sp.w = e - sp.x;
            sp.y = me_count(sp.x, e, [&](uint32_t x) { return p.text[x] != ' '; });
        }
        if ((threadIdx.x & 63u) == 0) { f.kf[i] = kf; f.span[i] = sp; }
    }
}

// EMIT = false: entry k is decided and sized, its ProteinName joined and searched.  EMIT = true: the kept entries are
// written.  Both take the lines of the entry that contribute in order, the state wave-uniform.
template <bool EMIT> __global__ __launch_bounds__(PT_BLOCK) void mg_fold_kernel(MgParams g)
{
    const MeParams &f = g.me;
    const PtParams &p = f.pt;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * (PT_BLOCK / 64);
    for (uint64_t k64 = (uint64_t)blockIdx.x * (PT_BLOCK / 64) + (threadIdx.x >> 6); k64 < f.n_terms; k64 += stride) {
        const uint32_t k = (uint32_t)k64;
        const uint32_t first = k ? f.term_line[k - 1u] + 1u : 0u, end = f.term_line[k];
        MeEnt en;
        uint64_t seq_at = 0, id_at = 0, org_at = 0, tax_at = 0;
        if (EMIT) {
            en = f.ent[k];
            if (!en.keep) continue;
            const unsigned long long a = f.ent_a[k], b = f.ent_b[k];
            const uint32_t r = (uint32_t)(a >> 32);
            if (r >= f.res[ME_R_RECORDS]) continue;   // (both passes decide alike, so this never holds: the buffers are sized from the first)
            seq_at = (uint32_t)a; id_at = (uint32_t)b;
            const uint64_t pn_at = b >> 32;
            org_at = pn_at + en.feat_len[0]; tax_at = org_at + en.feat_len[1];
            if (lane < (uint32_t)MG_FEATURES) f.feat_off[(uint64_t)r * MG_FEATURES + lane] = lane == 0 ? pn_at : lane == 1 ? org_at : tax_at;
            if (lane == 0) {
                f.ids[r] = (uint32_t)(f.nb_before + k64 + 1u);
                f.offsets[r] = seq_at;
                f.id_off[r] = id_at;
            }
            const uint4 pn = g.pn[k];
            me_copy(f.featb + pn_at, g.join + pn.x, pn.y);
            me_copy(f.featb + pn_at + pn.y, g.join + pn.z, pn.w);
        } else {
            en.keep = 0; en.declared = 0; en.held = 0; en.id_len = 0;
            en.id_line = en.gn_line = en.ec_line = en.ox_line = en.rec_line = ME_NONE;
        }
        uint32_t pn_len = 0, org_len = 0, tax_len = 0, held = 0, join_at = 0;
        bool drop = false;
        for (uint64_t base = first; base < end; base += 64) {
            const uint64_t i64 = base + lane;
            const uint32_t my_kf = i64 < end ? f.kf[(uint32_t)i64] : 0u;
            const uint32_t my_kind = my_kf & ME_KIND;
            // (a line that drops the entry: the reference stops there; nothing is kept of the entry either way)
            if (!EMIT && __ballot(my_kind == ME_DROP || (my_kf & ME_F_SKIP))) { drop = true; break; }
            const bool mine = my_kind >= (uint32_t)MG_DEF && my_kind <= (uint32_t)MG_SEQ;
            uint4 my_sp = make_uint4(0, 0, 0, 0);
            if (mine) my_sp = f.span[(uint32_t)i64];
            unsigned long long todo;
            if (EMIT) todo = __ballot(mine && my_kind != MG_DEF);   // (ProteinName lies joined in the scratch)
            else {
                todo = __ballot(mine && my_kind != MG_SEQ);         // (residues only add up)
                uint32_t s = my_kind == MG_SEQ ? my_sp.y : 0u;
#pragma unroll
                for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d, 64);
                held += s;
            }
            while (todo) {
                const int b = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const uint32_t kind = __shfl(my_kind, b, 64), line = (uint32_t)base + (uint32_t)b;
                const uint32_t src0 = __shfl(my_sp.x, b, 64), len0 = __shfl(my_sp.y, b, 64), len1 = __shfl(my_sp.w, b, 64);
                if (kind == MG_VER) {
                    if (!EMIT) { en.id_line = line; en.id_len = len0; }
                    else if (line == en.id_line) me_copy(f.idb + id_at, p.text + src0, len0);
                } else if (kind == MG_SEQ) {   // EMIT
                    (void)me_squeeze<true>(f.seqs + seq_at, held, en.declared, p.text + src0, len1);
                    held += len0;
                } else if (kind == MG_DEF) {   // !EMIT
                    if (!pn_len) join_at = src0;
                    const uint32_t sep = pn_len ? 1u : 0u;
                    uint8_t *to = g.join + join_at + pn_len;
                    if (lane < sep) to[lane] = ' ';
                    me_copy(to + sep, p.text + src0, len0);
                    pn_len += sep + len0;
                } else if (!org_len) {         // MG_ORG
                    if (EMIT) me_copy(f.featb + org_at, p.text + src0, len0);
                    org_len = len0;
                } else {
                    const uint32_t sep = tax_len ? 1u : 0u;
                    if (EMIT) {
                        uint8_t *to = f.featb + tax_at + tax_len;
                        if (lane < sep) to[lane] = ' ';
                        me_copy(to + sep, p.text + src0, len0);
                    }
                    tax_len += sep + len0;
                }
            }
        }
        if (EMIT) continue;
        uint4 pn = make_uint4(join_at, pn_len, 0, 0);
        if (!drop && pn_len) {
            __threadfence_block();   // (the wave reads what its other lanes wrote)
            const uint32_t lo = join_at, hi = join_at + pn_len;
            if (me_first(lo, hi, [&](uint32_t x) { return me_is(g.join, x, hi, ", partial"); }) != ME_NONE) drop = true;
            else {
                const uint32_t open = me_first(lo, hi, [&](uint32_t x) { return me_is(g.join, x, hi, " ["); });
                const uint32_t close = open == ME_NONE ? ME_NONE : me_last(open + 2u, hi, [&](uint32_t x) { return me_is(g.join, x, hi, "]."); });
                if (close != ME_NONE) { pn.y = open - lo; pn.z = close + 2u; pn.w = hi - pn.z; }
            }
        }
        if (!drop && held >= (uint32_t)KAAMER_KMER_SIZE) { en.keep = 1; en.declared = held; en.held = held; }
        for (int j = 0; j < ME_FEATURES; j++) en.feat_len[j] = 0;
        en.feat_len[0] = pn.y + pn.w; en.feat_len[1] = org_len; en.feat_len[2] = tax_len;
        en.pad = 0;
        if (lane == 0) { f.ent[k] = en; g.pn[k] = pn; }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// One text's reader: the EMBL reader's buffers, and what the state scan and the joined ProteinNames take.
struct MgReader : MeReader {
    DevBuf<uint32_t> d_state;
    DevBuf<uint8_t> d_join;
    DevBuf<uint4> d_pn;
    DevBuf<unsigned long long> d_work2;
    MgParams g{};
    MgParams params() { g.me = f; return g; }
    ~MgReader() { (void)hipSetDevice(device); }   // (before the buffers go)
};

struct MgGbk {
    typedef MgReader Reader;
    static const char *name() { return "gbk"; }
    static std::vector<std::string> feature_names() { return { "ProteinName", "Organism", "FullTaxonomy" }; }   // GBK_DEF_FTS, inputGBK.go:41
    static int lines_ready(MgReader &m, size_t, size_t nb)
    {
        const int rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_state, 2 * nb), want(m.d_join, (size_t)m.f.pt.n + 2 * PT_PIECE), want(m.d_work2, (size_t)1) });
        if (rc) return rc;
        m.g.blk_state = m.d_state; m.g.blk_state_base = m.d_state + nb;
        m.g.join = m.d_join;
        m.g.n_work2 = m.d_work2;
        HIPCHK(hipMemset(m.d_work2, 0, sizeof(unsigned long long)));
        return KAAMER_OK;
    }
    static void classify(MgReader &m, uint32_t n_blk) { hipLaunchKernelGGL(mg_classify_kernel, dim3(n_blk), dim3(PT_LINES), 0, 0, m.params()); }
    static int entries_ready(MgReader &m, size_t n_terms)
    {
        const int rc = reserve_group(nullptr, GROW_EXACT, { want(m.d_pn, n_terms + 1) });
        if (rc) return rc;
        m.g.pn = m.d_pn;
        return KAAMER_OK;
    }
    static void read_lines(MgReader &m, size_t n_work, uint32_t n_blk, int n_cu)
    {
        const MgParams g = m.params();
        if (n_work) hipLaunchKernelGGL(mg_lead_kernel, dim3(me_wave_grid(n_work, n_cu)), dim3(PT_BLOCK), 0, 0, g);
        hipLaunchKernelGGL(mg_state_kernel<false>, dim3(n_blk), dim3(PT_LINES), 0, 0, g);
        hipLaunchKernelGGL(mg_state_scan_kernel, dim3(1), dim3(PT_LINES), 0, 0, g);
        hipLaunchKernelGGL(mg_state_kernel<true>, dim3(n_blk), dim3(PT_LINES), 0, 0, g);
        // (the second worklist's length stays on the device: the grid is sized for every line, the waves stride)
        hipLaunchKernelGGL(mg_read_kernel, dim3(me_wave_grid(g.me.pt.line_cap, n_cu)), dim3(PT_BLOCK), 0, 0, g);
    }
    static void fold(MgReader &m, bool emit, unsigned grid)
    {
        if (emit) hipLaunchKernelGGL(mg_fold_kernel<true>, dim3(grid), dim3(PT_BLOCK), 0, 0, m.params());
        else hipLaunchKernelGGL(mg_fold_kernel<false>, dim3(grid), dim3(PT_BLOCK), 0, 0, m.params());
    }
    static void release(MgReader &m) { m.d_state.reset(); m.d_join.reset(); m.d_pn.reset(); }
};

extern "C" {

int kaamer_makedb_gbk_device(const char *text, uint64_t len, uint64_t nb_before, int device, kaamer_proteins **out)
{
    if (len > 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_ARG, "makedb_gbk_device: a text holds at most 2^32 - 1 bytes: cut it (kaamer_text_cut_embl)");
    if (!out || (!text && len)) return kaamer_fail(KAAMER_E_ARG, "makedb_gbk_device: bad argument");
    *out = nullptr;
    std::string inflated;
    int rc = me_plain("makedb_gbk_device", text, len, inflated);
    if (rc) return rc;
    MgReader m;
    rc = me_read<MgGbk>(m, text, len, nb_before, device);
    if (rc) return rc;
    return me_table(m, out);
}

int kaamer_image_build_gbk_device(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                                  kaamer_proteins **proteins, kaamer_image **image)
{
    int rc = mf_build_args("image_build_gbk_device", text, len, shard, n_shards, proteins, image, "(kaamer_text_cut_embl)");
    if (rc) return rc;
    *proteins = nullptr; *image = nullptr;
    MgReader m;
    kaamer_device_image di;
    rc = me_build<MgGbk>(m, "image_build_gbk_device", text, len, shard, n_shards, load_factor, device, proteins, &di);
    if (rc) return rc;
    rc = kaamer_device_image_download(&di, image);
    if (rc) { kaamer_proteins_free(*proteins); *proteins = nullptr; }
    return rc;
}

int kaamer_index_build_gbk(const char *text, uint64_t len, uint32_t shard, uint32_t n_shards, double load_factor, int device,
                           kaamer_proteins **proteins, kaamer_index **out)
{
    int rc = mf_build_args("index_build_gbk", text, len, shard, n_shards, proteins, out, "(kaamer_text_cut_embl)");
    if (rc) return rc;
    *proteins = nullptr; *out = nullptr;
    MgReader m;
    kaamer_device_image di;
    rc = me_build<MgGbk>(m, "index_build_gbk", text, len, shard, n_shards, load_factor, device, proteins, &di);
    if (rc) return rc;
    rc = index_of_device_image(di, device, out);
    if (rc) { kaamer_proteins_free(*proteins); *proteins = nullptr; }
    return rc;
}

}  // extern "C"
