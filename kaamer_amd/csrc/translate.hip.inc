// translate.hip.inc — 6-frame translation and ORF segmentation on the device
// (included by search.hip).
//
// Replaces GetORFs / GetFrame / ReverseComplement (pkg/search/dna.go:55-196).  By default with the
// bacterial table gcodeBacteria (gcode.go:36-101; the geneticCode argument is ignored by
// the reference, dna.go:106); a request that names another of search.GCodes' tables gets that
// table (a deliberate divergence: the codon classes are all that changes, see GENERIC below).
// One wave walks one input sequence: six frames, 64 codons
// at a time; codon classes are ballots (known / start / stop) and the reference's
// per-codon state machine runs on those 64-bit masks:
//
//   insideORF starts true (dna.go:98): the first ORF of a frame opens at the frame start;
//   after a stop the next ORF opens at the next start codon (dna.go:108-116);
//   a codon with a byte other than a/c/g/t translates to "" (map miss): it adds nothing to
//   the cds but still advances currentAAPos (dna.go:123-125,152);
//   an ORF is emitted iff len(cds) >= 21, the '*' of its stop included (dna.go:127-137);
//   the open ORF at the frame end is emitted under the same rule (dna.go:155-163).
//
// Reads (<= TS_MAX nt) take translate_reads_kernel: one lane per read, one kernel for the whole of
// GetORFs, output offsets from a chain of chunk totals.  Longer sequences take translate_kernel
// (a wave per piece of a frame) in two passes of the same code: COUNT (sizes per piece, scanned
// and summed per (sequence, frame)), then WRITE, then orf_order_long_kernel puts their ORFs in
// the order of the reference's final sort (dna.go:167-177; key = EndPosition on the plus strand,
// StartPosition on the minus strand; ties in emission order) by merging the six per-frame lists,
// which are already monotonic.

// the thirteen tables of search.GCodes (gcodes.h), tcag order; row KT_SLOT_DEFAULT is table 11
#define KT_AA_(code_, aa_, start_) aa_,
#define KT_START_(code_, aa_, start_) start_,
__constant__ char kt_aa[KT_N_GCODES][65] = { KT_GCODES(KT_AA_) };
__constant__ char kt_start[KT_N_GCODES][65] = { KT_GCODES(KT_START_) };
#undef KT_AA_
#undef KT_START_
// Every translation kernel exists twice.  GENERIC = false is the reference's behaviour (code 0 or 11): table 11 and its
// class masks are compile-time constants, and the kernels are instruction for instruction what they were before a
// request could name a code (translate_reads_kernel<192> sits one register under the 4-waves-per-SIMD cliff).
// GENERIC = true reads the table slot and the two class masks the host put into TranslateParams for this call.
#define KT_START_BITS_DEFAULT 0x0008000F00080008ull  /* kt_start[KT_SLOT_DEFAULT] == 'M', bit = codon index */
#define KT_STOP_BITS_DEFAULT 0x0000000000004C00ull   /* kt_aa[KT_SLOT_DEFAULT] == '*' */

#define MIN_LEN_CDS 21  /* dna.go:26 */
// Sequences up to TranslateParams::ts_max nucleotides (reads) take translate_reads_kernel<MAXNT>, which exists twice:
// MAXNT = 192 (64 codons per frame: one 64-bit mask, 3 ORFs per frame, 4 waves per SIMD) for batches of short reads, and
// MAXNT = 384 (128 codons, 6 ORFs per frame, 199 registers: 2 waves per SIMD) for batches whose MEAN length says that reads
// of 193 .. 384 nt are common (2 x 250, 2 x 300): those went a wave per (read, frame) through translate_kernel before
// round 4 (Q-mix: 21.1-21.5 -> 20.3 ms per 1 M reads with one batch in flight, 18.0-18.4 -> 17.7 with three), while a batch
// of 150-nt reads is 4 % slower through the wide kernel.  The host picks per batch (search.hip).
#define TS_MAX 192      /* the short kernel's limit: what the long-sequence lists are sized for */
#define TS_MAX_WIDE 384
template <uint32_t MAXNT> struct TsCfg;
template <> struct TsCfg<192> {
    static constexpr int HALVES = 2;        // a lane stages nucleotides 2 lane, 2 lane + 1 of every 128-nucleotide part of a read
    static constexpr uint32_t PITCH = 100;  // bytes per staged read, two 4-bit codes per byte: 25 dwords (odd), so lanes reading the same offset hit different banks
    static constexpr int TRQ = 3;           // ORFs one frame of <= 64 codons can close (3 x 21 codons)
    static constexpr int MIN_WAVES = 4;     // 128 VGPRs + 2 spilled (12 bytes of scratch per lane).  With 3 waves per SIMD (134 VGPRs, nothing spilled) the
                                            // kernel alone takes 1.21 instead of 1.11 ms per 1 M reads (profiles/r04_experiments.md): the spill stays
};
template <> struct TsCfg<384> {
    static constexpr int HALVES = 3;
    static constexpr uint32_t PITCH = 196;  // 49 dwords
    static constexpr int TRQ = 6;           // 128 codons
    static constexpr int MIN_WAVES = 2;     // 199 VGPRs, nothing spilled (the queue of up to 36 ORFs of a read lives in registers)
};
#define TS_WAVES 2
#define TP_PIECE 4096    /* codons per piece of a long sequence's frame (translate_kernel) */

struct TranslateParams {
    const uint8_t *seqs;
    const uint64_t *offsets;
    uint32_t n_seqs;
    uint64_t seq_bound;  // bytes of the batch as the caller gave them: device offsets beyond it are an error, not an access
    uint32_t *piece_li;          // [piece] -> index of its long sequence (the item -> sequence map of translate_kernel)
    uint32_t ts_max;             // sequences up to this many nucleotides are reads (translate_reads_kernel<192> or <384>: the host picks per batch)
    uint32_t max_long;           // capacity of long_seq / long_np
    uint64_t max_piece_items;    // capacity of the per-piece arrays
    // COUNT pass output / WRITE pass input, indexed [seq * 6 + frame]
    uint32_t *cnt_orf, *cnt_aa, *cnt_sa;
    uint32_t *d_n6;  // device scalar 6 * n_seqs for the scans
    const uint64_t *off_orf, *off_aa, *off_sa;
    // WRITE pass output
    kaamer_query_meta *tmp_meta;  // emission order (frame-major per sequence)
    uint8_t *orf_aa;
    int32_t *starts_alt;
    uint64_t q_cap, aa_cap, sa_cap;
    uint32_t *status;
    uint32_t *n_long;  // sequences longer than TS_MAX (listed by translate_short_kernel<COUNT>, zeroed by the finalize step)
    // the long sequences and their pieces (translate_kernel)
    uint32_t *long_seq, *long_np;          // [n_long] sequence index, pieces per frame
    const uint64_t *piece_base;            // [n_long + 1] exclusive scan of long_np
    uint32_t *pcnt_orf, *pcnt_aa, *pcnt_sa;              // per piece item
    const uint64_t *poff_orf, *poff_aa, *poff_sa;        // their exclusive scans
    uint32_t *d_n_piece_items;             // device scalar 6 * piece_base[n_long]
    // translate_reads_kernel: chunk tickets, the chain of chunk totals, final ORF descriptors and batch totals
    uint32_t *ticket;                      // zeroed by the finalize step
    unsigned long long *chain;             // 3 words per 64-sequence chunk, tagged with the batch epoch
    uint32_t epoch;
    kaamer_query_meta *out_meta;
    uint32_t *d_nq;
    unsigned long long *d_n_pos;
    uint64_t *w_off_orf, *w_off_aa, *w_off_sa;  // off_* again, writable: the entries of the long sequences
    // the call's genetic code (GENERIC kernels only; never kept in the workspace): row of kt_aa / kt_start, and its start /
    // stop classes as masks over the codon index (wave-uniform: pass 1 of the lane-per-read kernels needs no table lookup)
    uint32_t gc_slot;
    unsigned long long gc_start_bits, gc_stop_bits;
};

__device__ __forceinline__ uint32_t nt_code(uint8_t c)
{
    // strings.ToLower (dna.go:68) then the map key: t c a g -> 0..3, anything else -> 4
    if (c >= 'A' && c <= 'Z') c = (uint8_t)(c + 32);
    return c == 't' ? 0u : c == 'c' ? 1u : c == 'a' ? 2u : c == 'g' ? 3u : 4u;
}

__device__ __forceinline__ unsigned long long bits_from(uint32_t lo)  // bits lo..63
{
    return lo >= 64 ? 0ull : (~0ull << lo);
}
__device__ __forceinline__ unsigned long long bits_upto(uint32_t hi)  // bits 0..hi
{
    return hi >= 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull);
}

// raw nucleotide bytes of codon j of frame f (minus frames read the reverse complement
// in place: dna.go:55-63), 0xFF beyond the frame
__device__ __forceinline__ void load_codon(const uint8_t *dna, int64_t len, int f, int64_t ncod, int64_t j, uint32_t &a,
                                           uint32_t &b, uint32_t &c)
{
    a = b = c = 0xFFu;
    if (j < ncod) {
        const int64_t pnt = (f % 3) + 3 * j;
        if (f < 3) { a = dna[pnt]; b = dna[pnt + 1]; c = dna[pnt + 2]; }
        else { a = dna[len - 1 - pnt]; b = dna[len - 2 - pnt]; c = dna[len - 3 - pnt]; }
    }
}

// Long sequences (contigs, long reads): one wave per PIECE of a frame, TP_PIECE codons.  The ORF state
// machine is sequential along a frame, but a stop codon resets it: a piece first looks BACKWARD from
// its first codon for the previous stop (or the frame start), runs the state machine forward from
// there, and emits exactly the ORFs that CLOSE inside the piece (on their stop, or at the frame end
// in the last piece) -- so the pieces of a frame are independent work items and a 5 Mb contig is
// 2 400 of them instead of 6.  The (sequence, frame, piece) items of all long sequences are numbered
// t = 6 * piece_base[li] + frame * np(li) + piece; their ORF / residue / start counts are scanned
// (poff_*) and summed into the per-(sequence, frame) counts the rest of the pipeline uses.
template <bool WRITE, bool GENERIC>
__global__ __launch_bounds__(256) void translate_kernel(TranslateParams p)
{
    __shared__ uint8_t s_pend_aa_all[4][32];
    __shared__ int32_t s_pend_sa_all[4][32];
    __shared__ uint8_t s_aa_tab[64];
    __shared__ uint8_t s_nt[2][256];  // byte -> nucleotide code (nt_code), as it is and complemented: one LDS read per base
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint8_t *s_pend_aa = s_pend_aa_all[wv];
    int32_t *s_pend_sa = s_pend_sa_all[wv];
    const uint32_t n_long = *p.n_long;
    uint64_t n_items = n_long ? 6ull * p.piece_base[n_long] : 0ull;
    if (n_items > p.max_piece_items) {  // (overlapping offsets again: reported by list_long_kernel's twin check below)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(p.status, (uint32_t)ST_AA_CAP);
        n_items = 0;
    }
    if (!WRITE && blockIdx.x == 0 && threadIdx.x == 0) *p.d_n_piece_items = (uint32_t)n_items;
    if (n_long == 0 || n_items == 0) return;  // a reads-only batch: translate_reads_kernel does everything
    {
        const uint32_t c0_ = nt_code((uint8_t)threadIdx.x);
        s_nt[0][threadIdx.x] = (uint8_t)c0_;
        s_nt[1][threadIdx.x] = (uint8_t)(c0_ < 4 ? c0_ ^ 2u : c0_);  // t<->a, c<->g
    }
    if (threadIdx.x < 64) {
        const uint32_t slot = GENERIC ? p.gc_slot : (uint32_t)KT_SLOT_DEFAULT;
        s_aa_tab[threadIdx.x] = (uint8_t)((uint8_t)kt_aa[slot][threadIdx.x] | (kt_start[slot][threadIdx.x] == 'M' ? 0x80u : 0u));
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;

    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + wv; t < n_items; t += stride) {
        // item -> (long sequence, frame, piece): items 6 * piece_base[li] .. 6 * piece_base[li + 1] - 1 are sequence li's,
        // so piece t / 6 is one of its pieces (one load: a binary search over piece_base was 18 dependent loads per item,
        // 2 ms per pass on a batch with 200 000 medium-length reads)
        const uint32_t li = p.piece_li[t / 6];
        const uint32_t np = p.long_np[li];
        const uint64_t t_first = 6ull * p.piece_base[li];
        const uint32_t r = (uint32_t)(t - t_first);
        const int f = (int)(r / np);
        const uint32_t pc = r % np;
        const uint32_t seq = p.long_seq[li];
        const uint64_t sb = p.offsets[seq];
        const int64_t len = (int64_t)(p.offsets[seq + 1] - sb);
        const uint8_t *dna = p.seqs + sb;
        const uint64_t item = (uint64_t)seq * 6 + (uint64_t)f;
        const int s = f % 3;          // frameStartPosition (dna.go:25)
        const bool plus = f < 3;      // dna.go:81
        const int64_t ncod = (len - s) >= 3 ? (int64_t)((uint32_t)(len - s) / 3u) : 0;  // GetFrame (dna.go:183-196)
        const int64_t c_lo = (int64_t)pc * TP_PIECE;
        const int64_t c_hi = c_lo + TP_PIECE < ncod ? c_lo + TP_PIECE : ncod;
        uint32_t n_orf = 0, n_aa = 0, n_sa = 0;
        if (c_lo < ncod) {
            // codon j of the frame -> amino acid and classes (raw bytes: minus frames read the reverse
            // complement in place, dna.go:55-63)
            auto classify = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t &aa, bool &is_start, bool &is_stop) {
                const uint8_t *lut = s_nt[plus ? 0 : 1];
                a = lut[a & 255u]; b = lut[b & 255u]; c = lut[c & 255u];
                // (codes 0..3, 4 = not a/c/g/t: one of them at 4 or more sets bit 2 of the OR)
                const uint32_t t_ = ((a | b | c) & 4u) ? 0u : (uint32_t)s_aa_tab[(a << 4) | (b << 2) | c];  // amino acid | 0x80: start codon
                aa = t_ & 0x7Fu;
                is_start = (t_ & 0x80u) != 0u;
                is_stop = aa == (uint32_t)'*';   // (in all thirteen tables Stop <=> amino acid '*')
            };
            // ---- where the state machine starts: after the last stop before the piece
            bool inside = true;             // dna.go:98 (no stop before: the first ORF of the frame)
            int64_t c_start = 0;
            for (int64_t hi = c_lo; hi > 0;) {
                const int64_t lo = hi > 64 ? hi - 64 : 0;
                uint32_t a, b, c, aa;
                bool st, sp;
                load_codon(dna, len, f, hi, lo + lane, a, b, c);
                classify(a, b, c, aa, st, sp);
                const unsigned long long T = __ballot(sp && lo + (int64_t)lane < hi);
                if (T) { c_start = lo + (63 - __clzll((long long)T)) + 1; inside = false; break; }
                hi = lo;
            }
            uint64_t aa_cur = 0, sa_cur = 0, orf_cur = 0;
            if (WRITE) {
                const uint64_t t0 = t_first + (uint64_t)f * np;  // first piece of this frame
                aa_cur = p.off_aa[item] + (p.poff_aa[t] - p.poff_aa[t0]);
                sa_cur = p.off_sa[item] + (p.poff_sa[t] - p.poff_sa[t0]);
                orf_cur = p.off_orf[item] + (p.poff_orf[t] - p.poff_orf[t0]);
            }
            int64_t orf_begin = 0;          // codon index where the ORF opened
            uint32_t cds_len = 0, n_starts = 0;
            uint32_t ra, rb, rc;
            load_codon(dna, len, f, c_hi, c_start + lane, ra, rb, rc);
            for (int64_t c0 = c_start; c0 < c_hi; c0 += 64) {
                uint32_t na, nb, nc;   // the next chunk's codons are in flight while this one is walked
                load_codon(dna, len, f, c_hi, c0 + 64 + lane, na, nb, nc);
                uint32_t aa;
                bool is_start, is_stop;
                classify(ra, rb, rc, aa, is_start, is_stop);
                const unsigned long long K = __ballot(aa != 0);
                const unsigned long long S = __ballot(is_start);
                const unsigned long long T = __ballot(is_stop);
                const uint32_t n_here = (uint32_t)((c_hi - c0) < 64 ? (c_hi - c0) : 64);

                // ---- the chunk's ORF segments, all at once.  A stop codon ends a segment; the frame's last codon ends
                // one too (dna.go:155-163).  Every lane works out the segment it lies in from the three ballots -- the stop
                // before it, the closing codon at or after it, the first start codon in between (dna.go:108-116: after a
                // stop the next ORF opens at the next start codon), the known codons and start codons of the ORF -- so
                // the ORFs that close in this chunk are found, counted and written without walking them one by one.
                const unsigned long long Tv = T, Sv = S, Kv = K;
                const bool frame_end_here = c0 + (int64_t)n_here >= ncod;
                const unsigned long long C = Tv | (frame_end_here ? (1ull << (n_here - 1u)) : 0ull);  // closing codons
                const unsigned long long prevT = Tv & below;                 // stops before this lane
                const uint32_t lo = prevT ? 64u - (uint32_t)__clzll((long long)prevT) : 0u;   // the codon after the previous stop
                const unsigned long long cm = C & bits_from(lane);
                const bool closed = cm != 0;                                 // my segment closes in this chunk
                const uint32_t cl = closed ? (uint32_t)__ffsll((long long)cm) - 1u : 63u;
                const bool cont = prevT == 0 && inside;                      // my segment continues the ORF that was open
                const unsigned long long seg = bits_from(lo) & bits_upto(cl);
                const unsigned long long sm = Sv & seg;
                const bool has = cont || sm != 0;
                const uint32_t b_rel = (cont || !sm) ? lo : (uint32_t)__ffsll((long long)sm) - 1u;   // where the ORF begins
                const unsigned long long R = bits_from(b_rel) & bits_upto(cl);
                const uint32_t seg_cds = (cont ? cds_len : 0u) + (uint32_t)__popcll(Kv & R);
                const uint32_t seg_ns = (cont ? n_starts : 0u) + (uint32_t)__popcll(Sv & R);
                const bool seg_emit = closed && has && seg_cds >= MIN_LEN_CDS;             // dna.go:127-137
                const bool closer = closed && cl == lane;
                const unsigned long long E = __ballot(closer && seg_emit);    // the codons that close an emitted ORF
                // the open tail behind the last stop (or the whole chunk when it holds no stop)
                const uint32_t t_lo = Tv ? 64u - (uint32_t)__clzll((long long)Tv) : 0u;
                const bool t_cont = Tv == 0 && inside;
                const unsigned long long t_sm = Sv & bits_from(t_lo);
                const bool t_has = !frame_end_here && (t_cont || t_sm != 0);
                const uint32_t t_b = (t_cont || !t_sm) ? t_lo : (uint32_t)__ffsll((long long)t_sm) - 1u;
                const unsigned long long t_R = bits_from(t_b);
                uint32_t e_orf = 0, e_aa = 0, e_sa = 0;   // emitted in this chunk
                if (E) {  // wave-uniform
                    const uint32_t my_aa = (closer && seg_emit) ? seg_cds : 0u, my_sa = (closer && seg_emit) ? seg_ns : 0u;
                    const uint32_t inc_aa = wave_inclusive_scan_dpp(my_aa), inc_sa = wave_inclusive_scan_dpp(my_sa);
                    e_orf = (uint32_t)__popcll(E);
                    e_aa = (uint32_t)__builtin_amdgcn_readlane((int)inc_aa, 63);
                    e_sa = (uint32_t)__builtin_amdgcn_readlane((int)inc_sa, 63);
                    if (WRITE) {
                        // where my segment's ORF goes: the emitted ORFs before it in the chunk
                        const uint32_t ex_aa_c = (uint32_t)__shfl((int)(inc_aa - my_aa), (int)cl, 64);
                        const uint32_t ex_sa_c = (uint32_t)__shfl((int)(inc_sa - my_sa), (int)cl, 64);
                        const uint64_t o_aa = aa_cur + ex_aa_c, o_sa = sa_cur + ex_sa_c;
                        const uint64_t o_orf = orf_cur + (uint32_t)__popcll(E & bits_upto(cl)) - 1u;
                        const bool fits = seg_emit && o_orf < p.q_cap && o_aa + seg_cds <= p.aa_cap && o_sa + seg_ns <= p.sa_cap;
                        if (seg_emit && !fits && closer) atomicOr(p.status, (uint32_t)(ST_QUERY_CAP | ST_AA_CAP));
                        const int64_t begin_abs = cont ? orf_begin : c0 + (int64_t)b_rel;
                        if (fits && lane >= b_rel) {
                            if ((Kv >> lane) & 1ull)
                                p.orf_aa[o_aa + (cont ? cds_len : 0u) + (uint32_t)__popcll(Kv & bits_from(b_rel) & below)] = (uint8_t)aa;
                            if ((Sv >> lane) & 1ull)
                                p.starts_alt[o_sa + (cont ? n_starts : 0u) + (uint32_t)__popcll(Sv & bits_from(b_rel) & below)] =
                                    (int32_t)(c0 + (int64_t)lane - begin_abs);     // currentAAPos (dna.go:116-119,152)
                        }
                        // the ORF that was open: what earlier chunks kept back (its first residues and starts)
                        const unsigned long long firstC = C & (0ull - C);  // lowest closing codon
                        const bool cont_emitted = inside && firstC && (E & firstC) && (Tv & (firstC - 1ull)) == 0ull;
                        if (cont_emitted) {
                            const bool f0 = orf_cur < p.q_cap;  // (the same test its lanes made above, for lane-independent use)
                            const uint32_t pa = cds_len < MIN_LEN_CDS ? cds_len : MIN_LEN_CDS, ps = n_starts < MIN_LEN_CDS ? n_starts : MIN_LEN_CDS;
                            if (f0 && lane < pa && aa_cur + lane < p.aa_cap) p.orf_aa[aa_cur + lane] = s_pend_aa[lane];
                            if (f0 && lane < ps && sa_cur + lane < p.sa_cap) p.starts_alt[sa_cur + lane] = s_pend_sa[lane];
                        }
                        if (closer && fits) {
                            kaamer_query_meta m;
                            const bool has_stop = (Tv >> lane) & 1ull;
                            int32_t start_position, end_position;
                            if (plus) {
                                start_position = (int32_t)(f + 3 * begin_abs + 1);                      // dna.go:89,112
                                end_position = (int32_t)(3 * (c0 + (int64_t)lane) + 3 + f);            // dna.go:129,156
                            } else {
                                start_position = (int32_t)(len - s - 3 * begin_abs);                    // dna.go:84,89,114
                                end_position = start_position - (int32_t)(seg_cds * 3) + 1;             // dna.go:131,158
                            }
                            m.src_seq = seq;
                            m.size_in_kmer = (int32_t)seg_cds - KAAMER_KMER_SIZE + 1 - (has_stop ? 1 : 0);  // search_fastq.go:81-92
                            m.start_position = start_position;
                            m.end_position = end_position;
                            m.plus_strand = plus ? 1 : 0;
                            m.aa_len = seg_cds;
                            m.aa_off = o_aa;
                            m.sa_off = (uint32_t)o_sa;
                            m.sa_len = seg_ns;
                            p.tmp_meta[o_orf] = m;
                        }
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();  // the kept-back residues are read before the tail keeps new ones back
                    }
                }
                n_orf += e_orf; n_aa += e_aa; n_sa += e_sa;
                aa_cur += e_aa; sa_cur += e_sa; orf_cur += e_orf;
                if (WRITE && t_has && lane >= t_b) {
                    // the ORF still open at the end of the chunk: its first MIN_LEN_CDS residues and starts are kept back until it
                    // is known to be long enough; the rest goes straight to where it will be (it is the next ORF to be emitted)
                    const int64_t begin_abs = t_cont ? orf_begin : c0 + (int64_t)t_b;
                    if ((Kv >> lane) & 1ull) {
                        const uint32_t idx = (t_cont ? cds_len : 0u) + (uint32_t)__popcll(Kv & t_R & below);
                        if (idx < MIN_LEN_CDS) s_pend_aa[idx] = (uint8_t)aa;
                        else if (aa_cur + idx < p.aa_cap) p.orf_aa[aa_cur + idx] = (uint8_t)aa;
                    }
                    if ((Sv >> lane) & 1ull) {
                        const uint32_t idx = (t_cont ? n_starts : 0u) + (uint32_t)__popcll(Sv & t_R & below);
                        const int32_t v = (int32_t)(c0 + (int64_t)lane - begin_abs);
                        if (idx < MIN_LEN_CDS) s_pend_sa[idx] = v;
                        else if (sa_cur + idx < p.sa_cap) p.starts_alt[sa_cur + idx] = v;
                    }
                }
                // the state the next chunk starts from
                if (t_has) {
                    if (!t_cont) { orf_begin = c0 + (int64_t)t_b; cds_len = 0; n_starts = 0; }
                    cds_len += (uint32_t)__popcll(Kv & t_R);
                    n_starts += (uint32_t)__popcll(Sv & t_R);
                    inside = true;
                } else {
                    inside = false; cds_len = 0; n_starts = 0;
                }
                if (WRITE) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                ra = na; rb = nb; rc = nc;
            }
        }
        if (!WRITE && lane == 0) {
            p.pcnt_orf[t] = n_orf;
            p.pcnt_aa[t] = n_aa;
            p.pcnt_sa[t] = n_sa;
        }
    }
}

// piece -> its long sequence
__global__ void piece_li_kernel(TranslateParams p)
{
    const uint32_t n_long = *p.n_long;
    const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n_long || 6ull * p.piece_base[n_long] > p.max_piece_items) return;
    for (uint64_t g = p.piece_base[li]; g < p.piece_base[li + 1]; g++) p.piece_li[g] = li;
}

// per-(sequence, frame) counts of the long sequences = sums over their pieces
__global__ void long_totals_kernel(TranslateParams p)
{
    const uint32_t n_long = *p.n_long;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n_long * 6 || 6ull * p.piece_base[n_long] > p.max_piece_items) return;
    const uint32_t li = (uint32_t)(i / 6), f = (uint32_t)(i % 6);
    const uint32_t np = p.long_np[li];
    const uint64_t t0 = 6ull * p.piece_base[li] + (uint64_t)f * np, t1 = t0 + np;
    const uint64_t item = (uint64_t)p.long_seq[li] * 6 + f;
    p.cnt_orf[item] = (uint32_t)(p.poff_orf[t1] - p.poff_orf[t0]);
    p.cnt_aa[item] = (uint32_t)(p.poff_aa[t1] - p.poff_aa[t0]);
    p.cnt_sa[item] = (uint32_t)(p.poff_sa[t1] - p.poff_sa[t0]);
}

// The sequences longer than TS_MAX, listed for translate_kernel (any order), and the scan sizes.  One atomic per
// 1024-thread block: in a batch of mixed read lengths every wave has long reads to list, and one atomic per wave on the
// one counter serialised at ~90 per microsecond (180 us per 1 M reads).
#define LL_BLOCK 1024
__global__ __launch_bounds__(LL_BLOCK) void list_long_kernel(TranslateParams p)
{
    __shared__ uint32_t s_cnt[LL_BLOCK / 64];
    __shared__ uint32_t s_base;
    const uint64_t seq = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (seq == 0) *p.d_n6 = p.n_seqs * 6u;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t l = 0;
    if (seq < p.n_seqs) {
        const uint64_t b = p.offsets[seq], e = p.offsets[seq + 1];
        l = (e >= b && e <= p.seq_bound) ? e - b : 0;  // (translate_reads_kernel reports the inconsistent ones)
    }
    const bool is_long = l > p.ts_max;
    const unsigned long long lm = __ballot(is_long);
    if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(lm);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int i = 0; i < LL_BLOCK / 64; i++) { const uint32_t c = s_cnt[i]; s_cnt[i] = tot; tot += c; }
        s_base = tot ? atomicAdd(p.n_long, tot) : 0u;
        // the counter never stays above the list's capacity (what does not fit is reported below and taken back here,
        // so every later kernel can trust it)
        const uint64_t end = (uint64_t)s_base + tot;
        if (end > p.max_long) {
            const uint32_t stored = s_base < p.max_long ? p.max_long - s_base : 0u;
            atomicSub(p.n_long, tot - stored);
        }
    }
    __syncthreads();
    if (is_long) {
        const uint32_t k = s_base + s_cnt[wv] + (uint32_t)__popcll(lm & ((1ull << lane) - 1ull));
        if (k < p.max_long) {
            p.long_seq[k] = (uint32_t)seq;
            p.long_np[k] = (uint32_t)((l / 3) / TP_PIECE) + 1u;  // covers the codons of every frame
        } else {
            atomicOr(p.status, (uint32_t)ST_AA_CAP);  // only offsets that overlap one another list more than fit the batch
        }
    }
}

// Reads (<= TS_MAX nucleotides): one LANE per read, the whole of GetORFs in ONE kernel.  A 150-nt read has 50 codons
// per frame, so a wave per (read, frame) spends ~300 wave instructions on 50 busy lanes and is bound by instruction
// issue; here the per-codon state machine (dna.go:104-153, restated literally) runs in scalar form in every lane,
// 64 reads per wave.  The reads of a wave are staged into LDS once (coalesced loads, two 4-bit codes per byte) and:
//   pass 1  walks the six frames and QUEUES the ORFs it closes in registers (codon range, lengths: <= 3 per frame);
//   chain   the wave's ORF / residue / start-codon totals go on a chain of chunk totals (decoupled look-back, chunks
//           handed out by ticket so a chunk only ever waits for chunks that are already running); what comes back
//           is where the chunk's output starts -- no counting pass, no scans over 6 x n_seqs counters;
//   pass 2  decodes the queued ORFs' codons once more and writes residues, StartsAlternative and the descriptor,
//           the descriptor straight at its place in the reference's final order (dna.go:167-177: ascending key =
//           EndPosition on the plus strand, StartPosition on the minus strand; equal keys in frame order), which the
//           lane works out among its own <= 6 x TR_Q ORFs.
// Longer sequences of the same batch have been counted by translate_kernel<false> before this kernel runs: their lane
// puts those counts on the chain and leaves the offsets of their six frames for translate_kernel<true>.
template <uint32_t MAXNT, bool GENERIC>
__global__ __launch_bounds__(64 * TS_WAVES, TsCfg<MAXNT>::MIN_WAVES) void translate_reads_kernel(TranslateParams p)
{
    constexpr int TS_HALVES = TsCfg<MAXNT>::HALVES;
    constexpr uint32_t TS_PITCH = TsCfg<MAXNT>::PITCH;
    constexpr int TR_Q = TsCfg<MAXNT>::TRQ;
    constexpr bool WIDE = MAXNT > 192;   // codon masks of two words
    static_assert(MAXNT / 3 <= (WIDE ? 128 : 64) && TR_Q * MIN_LEN_CDS <= MAXNT / 3 && (TR_Q + 1) * MIN_LEN_CDS > MAXNT / 3, "codon masks, TR_Q ORFs per frame");
    static_assert(TS_PITCH >= MAXNT / 2 + 2 && (TS_PITCH / 4) % 2 == 1 && TS_PITCH % 4 == 0 && TS_HALVES * 128 >= MAXNT, "staged read: two codes per byte, an odd number of dwords");
    __shared__ uint8_t s_read[TS_WAVES][64 * TS_PITCH];
    __shared__ uint8_t s_aa_tab[64];  // amino acid of the codon (t c a g order) | 0x80 when it is a start codon
    __shared__ uint8_t s_ntc[256];    // byte -> nucleotide code (nt_code): one LDS read per base when the reads are staged
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (threadIdx.x < 64) {
        const uint32_t slot = GENERIC ? p.gc_slot : (uint32_t)KT_SLOT_DEFAULT;
        s_aa_tab[threadIdx.x] = (uint8_t)((uint8_t)kt_aa[slot][threadIdx.x] | (kt_start[slot][threadIdx.x] == 'M' ? 0x80u : 0u));
    }
    for (uint32_t i = threadIdx.x; i < 256; i += 64 * TS_WAVES) s_ntc[i] = (uint8_t)nt_code((uint8_t)i);
    __syncthreads();
    uint8_t *rd = s_read[wv];
    const uint32_t n_chunks = p.n_seqs ? (uint32_t)(((uint64_t)p.n_seqs + 63) / 64) : 1u;  // an empty batch still reports its totals
    const uint64_t seq_total = p.offsets[p.n_seqs] < p.seq_bound ? p.offsets[p.n_seqs] : p.seq_bound;  // bytes of the batch

    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(p.ticket, 1u);
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        if (c >= n_chunks) break;
        const uint64_t seq = (uint64_t)c * 64 + lane;
        uint64_t sb = 0;
        uint32_t len = 0;
        bool mine = false, is_long = false;
        if (seq < p.n_seqs) {
            sb = p.offsets[seq];
            const uint64_t se = p.offsets[seq + 1];
            uint64_t l = se - sb;
            if (se < sb || se > p.seq_bound) {  // offsets that do not agree with the batch size: an error, nothing is read
                atomicOr(p.status, (uint32_t)ST_AA_CAP);
                sb = 0; l = 0;
            }
            mine = l <= p.ts_max;
            is_long = !mine;
            len = mine ? (uint32_t)l : 0u;
        }
        // stage the wave's reads as codes t c a g -> 0..3, anything else -> 4 (nt_code), two per byte.  Eight reads at a
        // time: a lane loads nucleotides 2 lane, 2 lane + 1 and
        // 128 + 2 lane, 128 + 2 lane + 1 of each, and all 32 byte loads are in flight before the first is used -- one
        // read per round trip left the wave waiting on memory 64 times per chunk
        // (the loads are unconditional, at clamped addresses: a load under a branch makes the compiler wait for all of them)
        for (uint32_t r0 = 0; r0 < 64 && seq_total; r0 += 8) {
            uint32_t raw[8][2 * TS_HALVES];
            uint32_t rlen[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                // read r0 + u is lane r0 + u's: its offset and length come from that lane's registers (v_readlane)
                const int src = (int)(r0 + (uint32_t)u);
                const uint64_t rs = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(sb >> 32), src) << 32) |
                                    (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)sb, src);
                rlen[u] = (uint32_t)__builtin_amdgcn_readlane((int)len, src);
#pragma unroll
                for (int h = 0; h < TS_HALVES; h++) {
                    const uint64_t i = rs + 2 * (lane + 64u * (uint32_t)h);
                    raw[u][2 * h] = p.seqs[i < seq_total ? i : seq_total - 1];
                    raw[u][2 * h + 1] = p.seqs[i + 1 < seq_total ? i + 1 : seq_total - 1];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
#pragma unroll
                for (int h = 0; h < TS_HALVES; h++) {
                    const uint32_t k = lane + 64u * (uint32_t)h;
                    if (2 * k < rlen[u]) {
                        const uint32_t lo = s_ntc[raw[u][2 * h] & 255u];
                        const uint32_t hi = 2 * k + 1 < rlen[u] ? (uint32_t)s_ntc[raw[u][2 * h + 1] & 255u] : 4u;
                        rd[(r0 + (uint32_t)u) * TS_PITCH + k] = (uint8_t)(lo | (hi << 4));
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint8_t *my = rd + lane * TS_PITCH;
        // index (t c a g order, 0..63) of codon j of frame f, or 64 and above when one of its bytes is not a/c/g/t
        auto codon = [&](uint32_t f, uint32_t j) -> uint32_t {
            const uint32_t pnt = (f % 3) + 3 * j;
            const uint32_t lo = f < 3 ? pnt : len - 3 - pnt;  // lowest of the three positions
            const uint32_t k = lo >> 1;
            const uint32_t c = (((uint32_t)my[k] | ((uint32_t)my[k + 1] << 8)) >> ((lo & 1u) * 4u)) & 0xFFFu;
            uint32_t idx;
            if (f < 3) idx = ((c & 3u) << 4) | ((c >> 2) & 12u) | ((c >> 8) & 3u);
            else idx = ((((c >> 8) & 3u) << 4) | ((c >> 2) & 12u) | (c & 3u)) ^ 42u;
            return idx | ((c & 0x444u) << 4);
        };
        // the classes pass 1 needs, without a table lookup: start / stop codons of the table as bit masks over the index
        // (kt_start == 'M' and kt_aa == '*'; constants for table 11, the call's otherwise), known = all three bytes are a/c/g/t
        const unsigned long long START_BITS = GENERIC ? p.gc_start_bits : KT_START_BITS_DEFAULT;
        const unsigned long long STOP_BITS = GENERIC ? p.gc_stop_bits : KT_STOP_BITS_DEFAULT;
        auto classify = [&](uint32_t f, uint32_t j, bool &known, bool &is_start, bool &is_stop) {
            const uint32_t ci = codon(f, j);
            known = ci < 64u;
            is_start = known && ((START_BITS >> (ci & 63u)) & 1ull);
            is_stop = known && ((STOP_BITS >> (ci & 63u)) & 1ull);
        };
        // pass 2: the amino acid ('\0': a codon with a byte other than a/c/g/t is a map miss: "") and the start class
        auto decode = [&](uint32_t f, uint32_t j, bool &is_start) -> uint32_t {
            const uint32_t ci = codon(f, j);
            const uint32_t t = ci < 64u ? (uint32_t)s_aa_tab[ci & 63u] : 0u;
            is_start = (t & 0x80u) != 0u;
            return t & 0x7Fu;
        };

        // ---- pass 1: the state machine; closed ORFs queued as cds_len | n_starts << 8 | first codon << 16 |
        // last codon << 23 | closed-on-a-stop << 30 (0: no ORF)
        uint32_t q[6 * TR_Q];
#pragma unroll
        for (int i = 0; i < 6 * TR_Q; i++) q[i] = 0u;
        uint32_t t_orf = 0, t_aa = 0, t_sa = 0;
        if (mine) {
#pragma unroll
            for (int f = 0; f < 6; f++) {
                const uint32_t s = (uint32_t)f % 3u;   // frameStartPosition (dna.go:25)
                const uint32_t ncod = len >= s + 3 ? (len - s) / 3 : 0;  // GetFrame (dna.go:183-196)
                bool inside = true;           // dna.go:98
                uint32_t orf_begin = 0, cds_len = 0, n_starts = 0, n_orf = 0;
                for (uint32_t j = 0; j < ncod; j++) {
                    bool known, is_start, is_stop;
                    classify((uint32_t)f, j, known, is_start, is_stop);
                    if (is_start) {           // dna.go:108-121
                        if (!inside) { inside = true; orf_begin = j; cds_len = 0; n_starts = 0; }
                        n_starts++;
                    }
                    if (inside && known) cds_len++;  // dna.go:123-125
                    const bool frame_end = j + 1 == ncod;
                    if (is_stop || frame_end) {   // dna.go:127-150, 155-163
                        if (inside && cds_len >= MIN_LEN_CDS) {
                            const uint32_t w = cds_len | (n_starts << 8) | (orf_begin << 16) | (j << 23) | ((is_stop ? 1u : 0u) << 30);
#pragma unroll
                            for (int k = 0; k < TR_Q; k++) q[f * TR_Q + k] = n_orf == (uint32_t)k ? w : q[f * TR_Q + k];
                            n_orf++; t_aa += cds_len; t_sa += n_starts;
                        }
                        if (is_stop) { inside = false; cds_len = 0; n_starts = 0; }   // dna.go:138-149
                    }
                }
                t_orf += n_orf;
            }
        }
        uint32_t l_orf[6], l_aa[6], l_sa[6];  // a long sequence: its frames' counts (translate_kernel<false>, long_totals_kernel)
        if (is_long) {
#pragma unroll
            for (int f = 0; f < 6; f++) {
                l_orf[f] = p.cnt_orf[seq * 6 + f]; l_aa[f] = p.cnt_aa[seq * 6 + f]; l_sa[f] = p.cnt_sa[seq * 6 + f];
                t_orf += l_orf[f]; t_aa += l_aa[f]; t_sa += l_sa[f];
            }
        }
        // ---- where the lane's output starts: scan over the wave, then the chain over the chunks
        unsigned long long i_orf = t_orf, i_aa = t_aa, i_sa = t_sa;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long a = __shfl_up(i_orf, o, 64), b = __shfl_up(i_aa, o, 64), d = __shfl_up(i_sa, o, 64);
            if ((int)lane >= o) { i_orf += a; i_aa += b; i_sa += d; }
        }
        const unsigned long long w_orf = __shfl(i_orf, 63, 64), w_aa = __shfl(i_aa, 63, 64), w_sa = __shfl(i_sa, 63, 64);
        unsigned long long pre_orf = 0, pre_aa = 0, pre_sa = 0;
        unsigned long long *const ch = p.chain;
        if (c > 0) {
            if (lane < 3) __hip_atomic_store(&ch[3ull * c + lane], chain_pack(p.epoch, 1u, lane == 0 ? w_orf : lane == 1 ? w_aa : w_sa),
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            long long j = (long long)c - 1;  // nearest predecessor still to be added
            uint32_t spins = 0;
            bool done = false;
            while (!done) {
                const long long idx = j - (long long)lane;
                unsigned long long v0 = chain_pack(p.epoch, 2u, 0ull), v1 = v0, v2 = v0;  // before chunk 0: inclusive prefix 0
                if (idx >= 0) {
                    v0 = __hip_atomic_load(&ch[3ull * idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    v1 = __hip_atomic_load(&ch[3ull * idx + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    v2 = __hip_atomic_load(&ch[3ull * idx + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                // the three words of a chunk are published one by one: they count once they agree
                const unsigned long long tag = v0 >> CHAIN_VAL_BITS;
                const bool agree = tag == (v1 >> CHAIN_VAL_BITS) && tag == (v2 >> CHAIN_VAL_BITS) && (uint32_t)(tag >> 2) == p.epoch;
                const uint32_t flag = agree ? (uint32_t)tag & 3u : 0u;
                const unsigned long long m_inc = __ballot(flag == 2u), m_inv = __ballot(flag == 0u);
                const uint32_t first_inc = m_inc ? (uint32_t)__ffsll((long long)m_inc) - 1u : 64u;
                const unsigned long long need = first_inc >= 63u ? ~0ull : ((2ull << first_inc) - 1ull);
                if (m_inv & need) {  // a predecessor has not published yet
                    if (++spins > (1u << 22)) { if (lane == 0) atomicOr(p.status, (uint32_t)ST_CHAIN_TIMEOUT); break; }
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                const bool use = lane <= first_inc;
                unsigned long long a = use ? (v0 & CHAIN_VAL_MASK) : 0ull, b = use ? (v1 & CHAIN_VAL_MASK) : 0ull, d = use ? (v2 & CHAIN_VAL_MASK) : 0ull;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); d += __shfl_xor(d, o, 64); }
                pre_orf += a; pre_aa += b; pre_sa += d;
                done = first_inc < 64u;
                j -= 64;
            }
        }
        if (lane < 3) __hip_atomic_store(&ch[3ull * c + lane], chain_pack(p.epoch, 2u, lane == 0 ? pre_orf + w_orf : lane == 1 ? pre_aa + w_aa : pre_sa + w_sa),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == n_chunks - 1 && lane == 0) {  // the batch totals
            const unsigned long long total = pre_orf + w_orf;
            if (total > p.q_cap || pre_aa + w_aa > p.aa_cap || pre_sa + w_sa > p.sa_cap) {  // nothing of the batch is searched
                atomicOr(p.status, (uint32_t)(total > p.q_cap ? ST_QUERY_CAP : ST_AA_CAP));
                *p.d_nq = 0; *p.d_n_pos = 0;
            } else { *p.d_nq = (uint32_t)total; *p.d_n_pos = pre_aa + w_aa; }
            const uint64_t n6 = (uint64_t)p.n_seqs * 6;  // the totals, where the scans used to leave them
            p.w_off_orf[n6] = total; p.w_off_aa[n6] = pre_aa + w_aa; p.w_off_sa[n6] = pre_sa + w_sa;
        }
        unsigned long long orf_cur = pre_orf + i_orf - t_orf, aa_cur = pre_aa + i_aa - t_aa, sa_cur = pre_sa + i_sa - t_sa;
        if (is_long) {
            // the six frames' offsets (and the end of the last one), as translate_kernel<true> and orf_order_long_kernel read them
#pragma unroll
            for (int f = 0; f < 6; f++) {
                p.w_off_orf[seq * 6 + f] = orf_cur; p.w_off_aa[seq * 6 + f] = aa_cur; p.w_off_sa[seq * 6 + f] = sa_cur;
                orf_cur += l_orf[f]; aa_cur += l_aa[f]; sa_cur += l_sa[f];
            }
            p.w_off_orf[seq * 6 + 6] = orf_cur;
        }
        // ---- pass 2: write
        if (mine && t_orf) {
            if (orf_cur + t_orf > p.q_cap || aa_cur + t_aa > p.aa_cap || sa_cur + t_sa > p.sa_cap) {
                atomicOr(p.status, (uint32_t)(ST_QUERY_CAP | ST_AA_CAP));
            } else {
                // sort keys (dna.go:167-177); a slot without an ORF never counts as smaller
                int32_t key[6 * TR_Q];
                uint32_t nf[6];
#pragma unroll
                for (int f = 0; f < 6; f++) {
                    nf[f] = 0;
#pragma unroll
                    for (int k = 0; k < TR_Q; k++) {
                        const uint32_t w = q[f * TR_Q + k];
                        const uint32_t ob = (w >> 16) & 127u, je = (w >> 23) & 127u;
                        const int32_t kk = f < 3 ? (int32_t)(3 * je + 3 + (uint32_t)f)            // EndPosition, dna.go:129,156
                                                 : (int32_t)(len - (uint32_t)(f % 3) - 3 * ob);  // StartPosition, dna.go:84,89,114
                        key[f * TR_Q + k] = w ? kk : 0x7FFFFFFF;
                        nf[f] += w ? 1u : 0u;
                    }
                }
                // residues go out as a byte stream of the whole read, whole dwords where the stream covers them
                uint32_t acc = 0, nacc = (uint32_t)(aa_cur & 3ull), lead = nacc;
                uint8_t *const aa_out = p.orf_aa;
                unsigned long long wptr = aa_cur & ~3ull;
                auto put = [&](uint32_t aa) {
                    acc |= aa << (8u * nacc);
                    nacc++;
                    if (nacc == 4u) {
                        if (lead == 0u) *reinterpret_cast<uint32_t *>(aa_out + wptr) = acc;
                        else for (uint32_t b = lead; b < 4u; b++) aa_out[wptr + b] = (uint8_t)(acc >> (8u * b));
                        lead = 0u; acc = 0u; nacc = 0u; wptr += 4;
                    }
                };
                unsigned long long a_cur = aa_cur, s_cur = sa_cur, s_ptr = sa_cur;
#pragma unroll
                for (int f = 0; f < 6; f++) {
                    // the frame's ORFs as codon masks (128 codons: two words each): inside an ORF / first codon of an ORF
                    unsigned long long inm0 = 0, inm1 = 0, begm0 = 0, begm1 = 0;
                    uint32_t jlo = 128u, jhi = 0u;
                    // bits [a, b] of a 128-bit mask, as its two words
                    auto range_lo = [](uint32_t a, uint32_t b) -> unsigned long long {
                        if (a > 63u) return 0ull;
                        const unsigned long long upto = b >= 63u ? ~0ull : ((2ull << b) - 1ull);
                        return upto & ~((1ull << a) - 1ull);
                    };
                    auto range_hi = [](uint32_t a, uint32_t b) -> unsigned long long {
                        if (b < 64u) return 0ull;
                        const uint32_t a1 = a > 64u ? a - 64u : 0u, b1 = b - 64u;
                        const unsigned long long upto = b1 >= 63u ? ~0ull : ((2ull << b1) - 1ull);
                        return upto & ~((1ull << a1) - 1ull);
                    };
#pragma unroll
                    for (int k = 0; k < TR_Q; k++) {
                        const uint32_t w = q[f * TR_Q + k];
                        if (!__ballot(w != 0u)) continue;  // no lane of the wave has this slot
                        if (w == 0u) continue;
                        const uint32_t cl = w & 255u, ns = (w >> 8) & 255u, ob = (w >> 16) & 127u, je = (w >> 23) & 127u, stop = (w >> 30) & 1u;
                        inm0 |= range_lo(ob, je);
                        if (WIDE) inm1 |= range_hi(ob, je);
                        if (!WIDE || ob < 64u) begm0 |= 1ull << ob; else begm1 |= 1ull << (ob - 64u);
                        jlo = k == 0 ? ob : jlo;
                        jhi = je;
                        // rank in the final order: ORFs of the read with a smaller key, or the same key in an earlier frame
                        const int32_t kx = key[f * TR_Q + k];
                        uint32_t rank = f < 3 ? (uint32_t)k : nf[f] - 1u - (uint32_t)k;  // own frame: plus keys ascend, minus keys descend
#pragma unroll
                        for (int g = 0; g < 6; g++) {
                            if (g == f) continue;
#pragma unroll
                            for (int kk = 0; kk < TR_Q; kk++) {
                                const int32_t ky = key[g * TR_Q + kk];
                                rank += (g < f ? ky <= kx : ky < kx) ? 1u : 0u;
                            }
                        }
                        kaamer_query_meta m;
                        int32_t start_position, end_position;
                        if (f < 3) {
                            start_position = (int32_t)((uint32_t)f + 3 * ob + 1);                       // dna.go:89,112
                            end_position = (int32_t)(3 * je + 3 + (uint32_t)f);                         // dna.go:129,156
                        } else {
                            start_position = (int32_t)(len - (uint32_t)(f % 3) - 3 * ob);               // dna.go:84,89,114
                            end_position = start_position - (int32_t)(cl * 3) + 1;                      // dna.go:131,158
                        }
                        m.src_seq = (uint32_t)seq;
                        m.size_in_kmer = (int32_t)cl - KAAMER_KMER_SIZE + 1 - (int32_t)stop;            // search_fastq.go:81-92
                        m.start_position = start_position;
                        m.end_position = end_position;
                        m.plus_strand = f < 3 ? 1 : 0;
                        m.aa_len = cl;
                        m.aa_off = a_cur;
                        m.sa_off = (uint32_t)s_cur;
                        m.sa_len = ns;
                        p.out_meta[orf_cur + rank] = m;
                        a_cur += cl; s_cur += ns;
                    }
                    // ONE walk over the frame's codons from its first ORF to its last: every codon inside an ORF gives
                    // its residue (if it is a known codon) and, if it is a start codon, its position in the ORF
                    // (currentAAPos = codons since the ORF's first).  ORFs of a frame are disjoint and in order, so
                    // residues and starts come out in emission order.
                    uint32_t rel = 0;
                    for (uint32_t j = jlo; j <= jhi; j++) {
                        bool st;
                        const uint32_t aa = decode((uint32_t)f, j, st);
                        const bool in = (((!WIDE || j < 64u) ? inm0 >> j : inm1 >> (j - 64u)) & 1ull) != 0ull;
                        rel = (((!WIDE || j < 64u) ? begm0 >> j : begm1 >> (j - 64u)) & 1ull) ? 0u : rel + 1u;
                        if (in && aa != 0) put(aa);
                        if (in && st) p.starts_alt[s_ptr++] = (int32_t)rel;
                    }
                }
                for (uint32_t b = lead; b < nacc; b++) aa_out[wptr + b] = (uint8_t)(acc >> (8u * b));  // the stream's last bytes
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the next chunk overwrites the staging area
    }
}

// ORFs of one LONG sequence in the reference's final order (dna.go:167-177): a stable merge of the six per-frame
// lists translate_kernel<true> wrote in emission order (plus frames: EndPosition ascending; minus frames:
// StartPosition descending).  One thread per ORF computes its rank by binary search; a wave per long sequence.
__device__ __forceinline__ int32_t orf_key(const kaamer_query_meta &m) { return m.plus_strand ? m.end_position : m.start_position; }

__global__ void orf_order_long_kernel(const kaamer_query_meta *tmp, const uint64_t *off_orf, const uint32_t *long_seq, const uint32_t *d_n_long,
                                      kaamer_query_meta *out, const uint32_t *d_nq)
{
    const uint32_t n_long = *d_n_long;
    const uint64_t total = *d_nq;  // 0 when the batch overflowed the query capacity: nothing to order
    const uint32_t wpb = blockDim.x >> 6;  // a wave per sequence: a read of a few hundred nucleotides has a dozen ORFs
    for (uint32_t li = blockIdx.x * wpb + (threadIdx.x >> 6); li < n_long; li += gridDim.x * wpb) {
        const uint64_t sb = (uint64_t)long_seq[li] * 6;
        const uint64_t t0 = off_orf[sb], t1 = off_orf[sb + 6];
        if (t1 > total) continue;
        for (uint64_t t = t0 + (threadIdx.x & 63u); t < t1; t += 64) {
            const kaamer_query_meta m = tmp[t];
            // own frame: the list that contains t
            int f = 0;
#pragma unroll
            for (int g = 1; g < 6; g++) if (t >= off_orf[sb + g]) f = g;
            const int32_t k = orf_key(m);
            uint64_t rank = 0;
            for (int g = 0; g < 6; g++) {
                const uint64_t b = off_orf[sb + g], e = off_orf[sb + g + 1];
                if (g == f) {
                    rank += (g < 3) ? (t - b) : (e - 1 - t);  // plus: keys ascend; minus: keys descend
                    continue;
                }
                // count entries of list g with key < k (g after f) or key <= k (g before f)
                const bool inclusive = g < f;
                uint64_t lo = b, hi = e;  // first index whose key fails the predicate, in list order
                if (g < 3) {              // ascending keys
                    while (lo < hi) {
                        const uint64_t mid = lo + (hi - lo) / 2;
                        const int32_t km = orf_key(tmp[mid]);
                        if (inclusive ? (km <= k) : (km < k)) lo = mid + 1; else hi = mid;
                    }
                    rank += lo - b;
                } else {                  // descending keys: the qualifying entries are a suffix
                    while (lo < hi) {
                        const uint64_t mid = lo + (hi - lo) / 2;
                        const int32_t km = orf_key(tmp[mid]);
                        if (inclusive ? (km <= k) : (km < k)) hi = mid; else lo = mid + 1;
                    }
                    rank += e - lo;
                }
            }
            out[t0 + rank] = m;
        }
    }
}

// ORF batch -> not-a-k-mer-start bitmap + per-query table capacities (the ORF twin of prep_protein_kernel)
__global__ void prep_orf_kernel(const kaamer_query_meta *q, const uint32_t *d_nq, unsigned long long *invalid,
                                const unsigned long long *d_n_pos, QInfo *qinfo, uint32_t *slots, uint64_t *hit_off,
                                uint32_t *q_cnt, const uint32_t *slot_scale_p, unsigned long long room_slots)
{
    const uint32_t nq = *d_nq;
    // table capacity scale left by the previous batch, as far as this batch's ORFs leave room for it (count_group.hip.inc)
    const uint32_t slot_scale = fit_table_scale(*slot_scale_p, *d_n_pos, nq, room_slots);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq || i == 0; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i == 0) {
            const unsigned long long n_pos = *d_n_pos;
            mark_invalid_range(invalid, n_pos, (n_pos + 63) & ~63ull);
            if (nq == 0) break;
        }
        const kaamer_query_meta m = q[i];
        q_cnt[i] = 0;
        hit_off[i] = 0;
        QInfo qi;
        qi.size = m.size_in_kmer;
        qi.aa_off = m.aa_off;
        qi.slots = table_slots_for(m.size_in_kmer, slot_scale);
        const uint64_t b = m.aa_off, e = m.aa_off + m.aa_len;
        if (m.size_in_kmer > 0) mark_invalid_range(invalid, b + (uint64_t)m.size_in_kmer, e);
        else mark_invalid_range(invalid, b, e);
        qinfo[i] = qi;
        slots[i] = qi.slots;
    }
}
