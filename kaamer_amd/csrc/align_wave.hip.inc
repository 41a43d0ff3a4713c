// align_wave.hip.inc — the one statement of the alignment's recurrence, tie rules and tallies (included by align.hip
// and, through top_align.hip.inc, by search.hip).
//
//   align_wave_pair   one WAVE aligns one pair, the anti-diagonal wavefront align.hip describes: 64 lanes hold 64
//                     consecutive query rows, the cell above comes from the neighbouring lane (one DPP wave shift per
//                     layer), one byte per cell goes to the pair's direction slab, lane 0 walks it backwards.
//                     Both launch forms call it: align_wave_kernel (a workgroup per pair, launched by the host in
//                     budgeted rounds: kaamer_align_pairs) and the resident waves of top_align.hip.inc that take the
//                     reported hits of a top-N call by ticket.  LONG = true keeps the strip boundary row and the subject
//                     in HBM instead of LDS: subjects beyond ALN_WAVE_NS, same cells, same ties, same numbers.
//   AlnTally          align.go:87-133 over the columns of an alignment, in either direction: identical / similar /
//                     mismatch columns on the RAW letters after [uU] -> '*' (the similarity mark through the exact-letter
//                     map, in which lower case is a map miss that reads index 0), the feature pairs (maximal runs of one
//                     operation), a run a gap when its score equals -GapOpen, its extensions charged afterwards.  The host
//                     (kaamer_align_pairs, from the operations) and the device (inside the traceback) step the same code.
#pragma once

#define ALN_NL 26
#define ALN_WAVE_NS 2048u   /* longest subject the LDS row buffer holds (3 layers x 4 bytes x (ALN_WAVE_NS + 1)) */

// exact letters (the map of matrixScores.go:117, "-ABCDEFGHIJKLMNPQRSTVWXYZ*"); -1: a map miss
__host__ __device__ inline int aln_letter_index(int c)
{
    if (c == '-') return 0;
    if (c == '*') return 25;
    if (c >= 'A' && c <= 'Z' && c != 'O' && c != 'U') {
        int i = c - 'A' + 1;          // A=1 .. N=14
        if (c > 'O') i--;             // P=15 .. T=19
        if (c > 'U') i--;             // V=20 .. Z=24
        return i;
    }
    return -1;
}
// [uU] -> '*' (align.go:54-55): the letter the reference's strings hold
__host__ __device__ inline int aln_star(int c) { return (c == 'u' || c == 'U') ? '*' : c; }
// the aligner's index of a raw letter (not case sensitive); -1: outside the alphabet, the pair fails
__host__ __device__ inline int aln_code(int c)
{
    c = aln_star(c);
    return aln_letter_index((c >= 'a' && c <= 'z') ? c - 32 : c);
}

struct PairOut {
    int32_t max_s, end_i, end_j, start_i, start_j, n_ops;
};

struct AlnTally {
    int identical, similar, mismatches, gap_openings, raw;
    int run_op, run_len, run_score;
    __host__ __device__ void init() { identical = similar = mismatches = gap_openings = raw = 0; run_op = 0; run_len = 0; run_score = 0; }
    // the run that just ended (align.go:105-133)
    __host__ __device__ void close_run(int dp_open, int gap_open, int gap_extend)
    {
        if (!run_len) return;
        int score = run_score;
        if (run_op != 'M') score += dp_open;
        raw += score;
        if (score == -gap_open) {                                    // align.go:127
            gap_openings += 1;
            raw -= (run_len - 1) * gap_extend;                        // align.go:129-130
        }
        run_len = 0; run_score = 0;
    }
    // one column: op 'M' both letters, 'U' the query letter against a gap, 'L' a gap against the subject letter; qa / sb the
    // raw letters (ignored where the column holds a gap).  Returns the column's character of the match row.
    __host__ __device__ char step(int op, int qa, int sb, const int *matrix, int dp_open, int gap_open, int gap_extend)
    {
        const int ca = op == 'L' ? '-' : aln_star(qa), cb = op == 'U' ? '-' : aln_star(sb);
        char mark;
        if (cb == ca) { identical += 1; similar += 1; mark = (char)cb; }                 // align.go:87-90
        else {
            if (cb != '-' && ca != '-') mismatches += 1;                                  // align.go:92-94
            const int ib = aln_letter_index(cb), ia = aln_letter_index(ca);
            if (matrix[(ib < 0 ? 0 : ib) * ALN_NL + (ia < 0 ? 0 : ia)] > 0) { similar += 1; mark = '+'; }   // GetAlnScoreAA > 0
            else mark = ' ';
        }
        if (run_len && op != run_op) close_run(dp_open, gap_open, gap_extend);
        const int kq = op == 'L' ? 0 : aln_code(qa), ks = op == 'U' ? 0 : aln_code(sb);
        run_op = op; run_len += 1;
        run_score += matrix[(kq < 0 ? 0 : kq) * ALN_NL + (ks < 0 ? 0 : ks)];             // (row / column 0: the gap column)
        return mark;
    }
};

#if defined(__HIPCC__)
// first maximum of (a, b, c): its value and its index + 1
__device__ __forceinline__ void arg3(int a, int b, int c, int &v, unsigned &k)
{
    v = a; k = 1u;
    if (b > v) { v = b; k = 2u; }
    if (c > v) { v = c; k = 3u; }
}

// value of the next lower lane (lane 0: `first`): DPP wave_shr:1
__device__ __forceinline__ int from_lower_lane(int v, int first)
{
    return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false);
}

// the LDS of one aligning wave
struct AlnWaveLds {
    int m[ALN_NL * ALN_NL];
    int bnd[3][ALN_WAVE_NS + 1];   // the last row of the previous strip, per layer, by column (0 = zeros)
    uint8_t sub[ALN_WAVE_NS];
};

// One pair by one wave (a workgroup of 64 threads: the barriers below are the workgroup's).  L.m holds the matrix.
// qc / sc: letter indices of the query (nq) and the subject (ns); dir: the pair's direction slab,
// ceil(nq / 64) x (ns + 63) x 64 bytes; ops: nq + ns bytes, the operations in reverse; g_bnd (LONG): 3 x (ns + 1) ints.
// TALLY: lane 0 steps `tally` through the columns of the traceback (qraw / sraw: the raw letters).  The result is valid
// in lane 0; every lane returns (the caller may go on to the next pair after a barrier).
template <bool LONG, bool TALLY>
__device__ __forceinline__ void align_wave_pair(AlnWaveLds &L, const uint8_t *qc, uint32_t nq, const uint8_t *sc, uint32_t ns, int gap_open,
                                                uint8_t *dirs, uint8_t *ops, int *g_bnd, const uint8_t *qraw, const uint8_t *sraw,
                                                int opt_gap_open, int opt_gap_extend, PairOut &o, AlnTally &tally)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t W = ns + 1;
    if (LONG) {
        for (uint32_t j = lane; j < 3 * W; j += 64) g_bnd[j] = 0;
        __threadfence_block();
    } else {
        for (uint32_t j = lane; j < ns; j += 64) L.sub[j] = sc[j];
        for (uint32_t j = lane; j <= ns; j += 64) { L.bnd[0][j] = 0; L.bnd[1][j] = 0; L.bnd[2][j] = 0; }
    }
    __syncthreads();
    const uint32_t steps = ns + 63u;
    uint8_t *const dir = dirs + lane;
    int best = 0, best_i = 0, best_j = 0, best_l = 0;
    uint32_t strip = 0;
    for (uint32_t i0 = 0; i0 < nq; i0 += 64, strip++) {
        const uint32_t i = i0 + lane + 1;                 // this lane's row (1-based)
        const bool row_live = i <= nq;
        const int rv = row_live ? (int)qc[i - 1] : 0;
        const int gr = L.m[rv * ALN_NL];                  // the gap-column score of the query letter
        int cm = 0, cu = 0, cl = 0;                       // this lane's last cell (zeros: column 0 / not a cell)
        int pu_m = 0, pu_u = 0, pu_l = 0;                 // the cell above last step's cell = this step's diagonal
        uint8_t *const sdir = dir + (uint64_t)strip * steps * 64;
        for (uint32_t st = 0; st < steps; st++) {
            const int j = (int)st - (int)lane + 1;        // this step's column (1-based)
            const bool cell = row_live && j >= 1 && j <= (int)ns;
            // the cell above: the lower lane's last results (its row is i - 1, its last column was j); lane 0 reads the
            // previous strip's last row
            const int jc = j < 0 ? 0 : (j > (int)ns ? (int)ns : j);
            int b_m, b_u, b_l;
            if (LONG) { b_m = g_bnd[jc]; b_u = g_bnd[W + jc]; b_l = g_bnd[2 * W + jc]; }
            else { b_m = L.bnd[0][jc]; b_u = L.bnd[1][jc]; b_l = L.bnd[2][jc]; }
            const int up_m = from_lower_lane(cm, b_m), up_u = from_lower_lane(cu, b_u), up_l = from_lower_lane(cl, b_l);
            const int qv = cell ? (int)(LONG ? sc[j - 1] : L.sub[j - 1]) : 0;
            int v, nm = 0, nu = 0, nl = 0;
            unsigned k, f = 0;
            arg3(pu_m, pu_u, pu_l, v, k);                 // diag: the best layer of (i-1, j-1) + the substitution score
            const int pm = v;
            v += L.m[rv * ALN_NL + qv];
            if (v > 0) { nm = v; f |= pm > 0 ? k : 0u; }
            arg3(up_m + gap_open + gr, up_u + gr, up_l + gap_open + gr, v, k);       // up: consumes the query letter
            if (v > 0) { nu = v; f |= k << 2; }
            const int gq = L.m[qv];
            arg3(cm + gap_open + gq, cu + gap_open + gq, cl + gq, v, k);             // left: consumes the subject letter
            if (v > 0) { nl = v; f |= k << 4; }
            if (!cell) { nm = nu = nl = 0; f = 0; }
            sdir[(uint64_t)st * 64] = (uint8_t)f;
            // the first best cell in row-major order: within a row columns ascend, a lane's rows ascend with the strips
            if (nm > best) { best = nm; best_i = (int)i; best_j = j; best_l = 0; }
            if (nu > best) { best = nu; best_i = (int)i; best_j = j; best_l = 1; }
            if (nl > best) { best = nl; best_i = (int)i; best_j = j; best_l = 2; }
            pu_m = up_m; pu_u = up_u; pu_l = up_l;
            cm = nm; cu = nu; cl = nl;
            // the strip's last row feeds the next strip (column j was read by lane 0 sixty-three steps ago)
            if (lane == 63 && cell) {
                if (LONG) { g_bnd[j] = nm; g_bnd[W + j] = nu; g_bnd[2 * W + j] = nl; }
                else { L.bnd[0][j] = nm; L.bnd[1][j] = nu; L.bnd[2][j] = nl; }
            }
        }
        if (LONG) __threadfence_block();
        __syncthreads();   // (one wave: orders the boundary row between strips)
    }
    // the best cell over the lanes: highest score, then the smallest row
    unsigned long long key = ((unsigned long long)(uint32_t)best << 32) | (uint32_t)(0x7FFFFFFF - best_i);
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
        const unsigned long long other = __shfl_xor(key, x, 64);
        key = other > key ? other : key;
    }
    const int w_best = (int)(key >> 32), w_i = 0x7FFFFFFF - (int)(uint32_t)key;
    const unsigned long long mine = __ballot(best == w_best && best_i == w_i && w_best > 0);
    int max_j = 0, max_l = 0;
    if (mine) {
        const int src = __ffsll((long long)mine) - 1;
        max_j = __shfl(best_j, src, 64);
        max_l = __shfl(best_l, src, 64);
    }
    __threadfence_block();
    __syncthreads();
    if (lane != 0) return;
    // traceback (lane 0): cell (i, j) lives in strip (i-1)/64 at step (j-1) + (i-1)%64, lane (i-1)%64
    int i = w_best > 0 ? w_i : 0, j = max_j, l = max_l, n_ops = 0;
    const int end_i = i, end_j = j;
    if (TALLY) tally.init();
    while (i > 0 && j > 0) {
        const uint32_t ln = (uint32_t)(i - 1) & 63u, sp = (uint32_t)(i - 1) >> 6;
        const unsigned f = dirs[((uint64_t)sp * steps + (uint32_t)(j - 1) + ln) * 64 + ln];
        const unsigned pred = (f >> (2 * l)) & 3u;
        const int op = l == 0 ? 'M' : l == 1 ? 'U' : 'L';
        ops[n_ops++] = (uint8_t)op;
        if (TALLY) (void)tally.step(op, qraw[i - 1], sraw[j - 1], L.m, gap_open, opt_gap_open, opt_gap_extend);
        if (l == 0) { i--; j--; } else if (l == 1) i--; else j--;
        if (pred == 0) break;
        l = (int)pred - 1;
    }
    if (TALLY) tally.close_run(gap_open, opt_gap_open, opt_gap_extend);
    o.max_s = w_best; o.end_i = end_i; o.end_j = end_j; o.start_i = i; o.start_j = j; o.n_ops = n_ops;
}
#endif
