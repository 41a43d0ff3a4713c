// inflate.hip.inc — RFC 1951 inflate of BGZF blocks on the device (included by search.hip next to parse_text.hip.inc):
// compressed bytes + a block table in HBM -> the text in HBM, one status word per block.
//
// A BGZF file is a run of independent gzip members of at most 64 KiB of text each; kaamer_bgzf_scan (host_search.cpp)
// finds them without inflating: one kaamer_bgzf_block {comp_off, comp_len, isize, crc} each, comp_off / comp_len being the
// deflate payload between the member's header and its 8-byte trailer.  Blocks share no window, so every block is one
// wave's job.
//
// The first half of this file is the decoder itself, written once as host + device code over one state struct (InfState):
// the kernel runs it with 64 lanes, tools/inflate_check compiles the same text with one "lane" for the CPU (g++, ASan +
// UBSan, against zlib).  Every value that steers control flow is the same in all lanes of a wave: the lanes walk the
// Huffman symbols together (one decodes as fast as 64 do), and split up only where there is data-parallel work -- table
// construction, the input window, stored-block copies, match copies, the CRC.
//
// Bounds, none of them left to a fault:
//   input    the reader sees the payload through a window of INF_WIN_WORDS words that is filled with bytes of
//            [in, in + in_len) only (inf_window_load); what lies beyond reads as zero bits and sets status 4 as soon as a
//            symbol has used one of them
//   output   every store is preceded by out_pos + n <= isize (status 5); a distance above out_pos is status 3
//   loops    every iteration of every loop consumes at least one bit, produces a byte or ends the block
//   status   1 bad block type, stored LEN/NLEN mismatch, payload bytes left behind the final block
//            2 over-subscribed or incomplete code (also: no end-of-block code, more than 286 / 30 symbols)
//            3 invalid symbol or distance   4 input exhausted   5 more output than ISIZE   6 less output than ISIZE
//            7 CRC-32 mismatch
//
// Per-wave tables (InfTables, 3 968 bytes of LDS):
//   lit_fast[1024] u16   the next 10 bits -> symbol << 4 | code length (0: a longer code, or none: the canonical walk)
//   dist_fast[256] u16   the same over 8 bits (also the code-length code while a dynamic header is read)
//   lit_sym[288], dist_sym[32] u16   symbols in canonical order; lit_cnt/off/first[16], dist_...[16] u16 per code length
//   lens[320] u8         the code lengths of the current block          win[64] u32   the input window / the CRC partials
// A workgroup is INF_WAVES = 4 waves plus the CRC byte table (1 KiB) and the segment-shift matrix (128 B): 17 024 bytes,
// so nine workgroups = 36 waves fit the CU's 160 KiB -- more than the 32 waves (8 per SIMD) a CU can hold.
#if defined(__HIPCC__)
#define INF_HD __host__ __device__ __forceinline__
#else
#define INF_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define INF_NLANES 64
#define INF_LANE() ((int)(threadIdx.x & 63u))
// Orders what the wave's lanes stored before it against what they load after it -- LDS and HBM alike.  The fence keeps the
// compiler from moving memory accesses across it; at wavefront scope it costs no instruction, because the hardware
// already issues one wave's LDS operations, and one wave's vector memory operations to the CU's L1, in program order
// (LLVM's AMDGPU backend guide, "Memory Model" for gfx90a / gfx942, which gfx950 follows: the memory operations of one
// wavefront are performed in program order, which is why its code sequences for wavefront-scope fences and atomics hold
// no s_waitcnt and no cache action; the L1 is write-through and shared by the CU).
#define INF_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#else
#define INF_NLANES 1
#define INF_LANE() 0
#define INF_SYNC() ((void)0)
#endif

enum {
    INF_LIT_BITS = 10, INF_DIST_BITS = 8,
    INF_WIN_WORDS = 64,           // the input window: one word per lane
    INF_CRC_SEG = 1024,           // bytes of output per lane of the CRC (64 lanes x 1 KiB = the largest BGZF block)
    INF_WAVES = 4,                // waves (= BGZF blocks) per workgroup
    INF_MAX_ISIZE = 65536,
    INF_CUT_TILE = 4096,          // bytes of text per workgroup of the cut kernel
};
enum { INF_OK = 0, INF_E_BLOCK = 1, INF_E_CODE = 2, INF_E_SYMBOL = 3, INF_E_INPUT = 4, INF_E_OVER = 5, INF_E_UNDER = 6, INF_E_CRC = 7 };

struct InfTables {
    uint16_t lit_fast[1 << INF_LIT_BITS];
    uint16_t dist_fast[1 << INF_DIST_BITS];
    uint16_t lit_sym[288], dist_sym[32];
    uint16_t lit_cnt[16], lit_off[16], lit_first[16];
    uint16_t dist_cnt[16], dist_off[16], dist_first[16];
    uint8_t lens[320];
    uint32_t win[INF_WIN_WORDS];
};

struct InfState {
    // the bit reader, bounded by the payload [in, in + in_len)
    const uint8_t *in;
    uint32_t in_len;
    uint32_t skew;        // (address of in) & 3: word k of the payload starts at in - skew + 4 k
    uint32_t win_base;    // the window holds words [win_base, win_base + INF_WIN_WORDS)
    uint32_t next_word;   // the next word that goes into bitbuf
    uint64_t bitbuf;
    uint32_t bitcnt;
    // the output cursor, bounded by the block's stated size
    uint8_t *out;
    uint32_t isize, out_pos;
    InfTables *t;
};

// words [base, base + 64) of the payload into the window; a byte outside [in, in + in_len) is never read and counts as 0
INF_HD void inf_window_load(InfState &s, uint32_t base)
{
    INF_SYNC();   // (the lanes are done with the old window)
    for (int i = INF_LANE(); i < INF_WIN_WORDS; i += INF_NLANES) {
        const int64_t at = (int64_t)(base + (uint32_t)i) * 4 - (int64_t)s.skew;   // offset of the word's first byte in the payload
        uint32_t w = 0;
        if (at >= 0 && at + 4 <= (int64_t)s.in_len) {
#if defined(__HIP_DEVICE_COMPILE__)
            w = *reinterpret_cast<const uint32_t *>(s.in + at);   // (in + at is a multiple of 4)
#else
            memcpy(&w, s.in + at, 4);
#endif
        } else {
            for (int b = 0; b < 4; b++)
                if (at + b >= 0 && at + b < (int64_t)s.in_len) w |= (uint32_t)s.in[at + b] << (8 * b);
        }
        s.t->win[i] = w;
    }
    s.win_base = base;
    INF_SYNC();
}

INF_HD uint32_t inf_word(InfState &s, uint32_t k)
{
    if (k - s.win_base >= (uint32_t)INF_WIN_WORDS) inf_window_load(s, k);
    return s.t->win[k - s.win_base];
}

// the reader at byte `pos` of the payload
INF_HD void inf_seek(InfState &s, uint32_t pos)
{
    const uint32_t k = (s.skew + pos) >> 2, sub = (s.skew + pos) & 3u;
    s.bitbuf = (uint64_t)(inf_word(s, k) >> (8 * sub));
    s.bitcnt = 32 - 8 * sub;
    s.next_word = k + 1;
}

// bits of the payload handed out so far; above 8 in_len: zero bits from beyond the payload were used
INF_HD uint64_t inf_bits_used(const InfState &s) { return (uint64_t)s.next_word * 32 - 8 * s.skew - s.bitcnt; }
INF_HD bool inf_overrun(const InfState &s) { return inf_bits_used(s) > (uint64_t)s.in_len * 8; }

// at least 33 bits in bitbuf
INF_HD void inf_refill(InfState &s)
{
    if (s.bitcnt <= 32) {
        s.bitbuf |= (uint64_t)inf_word(s, s.next_word) << s.bitcnt;
        s.bitcnt += 32;
        s.next_word++;
    }
}

INF_HD uint32_t inf_take(InfState &s, uint32_t n)   // n <= 16, after inf_refill
{
    const uint32_t v = (uint32_t)s.bitbuf & ((1u << n) - 1u);
    s.bitbuf >>= n;
    s.bitcnt -= n;
    return v;
}

INF_HD uint32_t inf_bits(InfState &s, uint32_t n)
{
    inf_refill(s);
    return inf_take(s, n);
}

// One Huffman symbol (after inf_refill: a code has at most 15 bits); -1: the bits are no code of this table
INF_HD int inf_symbol(InfState &s, const uint16_t *fast, int fast_bits, const uint16_t *cnt, const uint16_t *sym)
{
    const uint32_t e = fast[(uint32_t)s.bitbuf & ((1u << fast_bits) - 1u)];
    if (e & 15u) {
        s.bitbuf >>= (e & 15u);
        s.bitcnt -= (e & 15u);
        return (int)(e >> 4);
    }
    // the canonical walk, one bit per length (codes longer than the fast table, and bits that are no code at all)
    int code = 0, first = 0, index = 0;
    uint64_t b = s.bitbuf;
    for (int len = 1; len <= 15; len++) {
        code |= (int)(b & 1u);
        b >>= 1;
        const int c = cnt[len];
        if (code - c < first) {
            s.bitbuf = b;
            s.bitcnt -= (uint32_t)len;
            return sym[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// The tables of one code from its n lengths (n <= 288).  All lanes: lane l counts and places the symbols of length l, then
// every lane fills the fast-table entries of its share of the symbols.  single_ok: a code whose only lengths are 1 may be
// incomplete (zlib's rule for the literal/length and distance codes; the code-length code must be complete).
INF_HD int inf_build(const uint8_t *lens, int n, uint16_t *fast, int fast_bits, uint16_t *sym, uint16_t *cnt, uint16_t *off,
                     uint16_t *first, bool single_ok)
{
    INF_SYNC();   // (lens[] is written, the old tables are no longer read)
    for (int l = INF_LANE(); l < 16; l += INF_NLANES) {
        int c = 0;
#pragma unroll 4
        for (int i = 0; i < n; i++) c += lens[i] == l ? 1 : 0;
        cnt[l] = (uint16_t)c;
    }
    for (int j = INF_LANE(); j < (1 << fast_bits); j += INF_NLANES) fast[j] = 0;
    INF_SYNC();
    int left = 1, max_len = 0;
    for (int l = 1; l <= 15; l++) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return INF_E_CODE;   // over-subscribed
        if (cnt[l]) max_len = l;
    }
    if (left > 0 && max_len != 0 && !(single_ok && max_len == 1)) return INF_E_CODE;   // incomplete (no code at all: every symbol is invalid)
    for (int l = 1 + INF_LANE(); l < 16; l += INF_NLANES) {
        int o = 0, code = 0;
        for (int b = 1; b < l; b++) { o += cnt[b]; code = (code + cnt[b]) << 1; }
        off[l] = (uint16_t)o;
        first[l] = (uint16_t)code;
#pragma unroll 4
        for (int i = 0; i < n; i++)
            if (lens[i] == l) sym[o++] = (uint16_t)i;
    }
    INF_SYNC();
    const int total = n - (int)cnt[0];
    for (int i = INF_LANE(); i < total; i += INF_NLANES) {
        const int sy = sym[i], l = lens[sy];
        if (l > fast_bits) continue;
        uint32_t code = (uint32_t)first[l] + (uint32_t)(i - (int)off[l]), rev = 0;
        for (int b = 0; b < l; b++) { rev = (rev << 1) | (code & 1u); code >>= 1; }
        for (uint32_t j = rev; j < (1u << fast_bits); j += 1u << l) fast[j] = (uint16_t)((sy << 4) | l);
    }
    INF_SYNC();
    return INF_OK;
}

INF_HD int inf_build_lit(InfState &s, int n)
{
    InfTables *t = s.t;
    return inf_build(t->lens, n, t->lit_fast, INF_LIT_BITS, t->lit_sym, t->lit_cnt, t->lit_off, t->lit_first, true);
}
INF_HD int inf_build_dist(InfState &s, const uint8_t *lens, int n, bool single_ok)
{
    InfTables *t = s.t;
    return inf_build(lens, n, t->dist_fast, INF_DIST_BITS, t->dist_sym, t->dist_cnt, t->dist_off, t->dist_first, single_ok);
}

// the header of a dynamic block -> the two tables
INF_HD int inf_dynamic_tables(InfState &s)
{
    InfTables *t = s.t;
    const int nlen = (int)inf_bits(s, 5) + 257, ndist = (int)inf_bits(s, 5) + 1, ncode = (int)inf_bits(s, 4) + 4;
    if (nlen > 286 || ndist > 30) return INF_E_CODE;
    // the code-length code: its 19 lengths at the far end of lens[] (dead once its tables are built, before the distance
    // lengths land there), its tables where the distance code's will be
    uint8_t *cl = t->lens + 300;
    INF_SYNC();
    for (int i = INF_LANE(); i < 19; i += INF_NLANES) cl[i] = 0;
    INF_SYNC();
    constexpr uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };   // RFC 1951 3.2.7
    for (int i = 0; i < ncode; i++) {
        const uint32_t v = inf_bits(s, 3);
        if (INF_LANE() == 0) cl[order[i]] = (uint8_t)v;
    }
    if (inf_overrun(s)) return INF_E_INPUT;
    int rc = inf_build_dist(s, cl, 19, false);
    if (rc) return rc;
    int i = 0, prev = 0;
    while (i < nlen + ndist) {
        inf_refill(s);
        const int sy = inf_symbol(s, t->dist_fast, INF_DIST_BITS, t->dist_cnt, t->dist_sym);
        if (sy < 0) return INF_E_SYMBOL;
        int rep = 1, v = sy;
        if (sy == 16) {
            if (i == 0) return INF_E_SYMBOL;   // nothing to repeat
            v = prev; rep = 3 + (int)inf_take(s, 2);
        } else if (sy == 17) { v = 0; rep = 3 + (int)inf_take(s, 3); }
        else if (sy == 18) { v = 0; rep = 11 + (int)inf_take(s, 7); }
        if (inf_overrun(s)) return INF_E_INPUT;
        if (i + rep > nlen + ndist) return INF_E_SYMBOL;
        // lens[0, nlen) the literal/length code, lens[288, 288 + ndist) the distance code
        for (int j = INF_LANE(); j < rep; j += INF_NLANES) {
            const int at = i + j;
            t->lens[at < nlen ? at : 288 + (at - nlen)] = (uint8_t)v;
        }
        i += rep;
        prev = v;
    }
    INF_SYNC();
    if (t->lens[256] == 0) return INF_E_CODE;   // no end-of-block code
    rc = inf_build_lit(s, nlen);
    if (!rc) rc = inf_build_dist(s, t->lens + 288, ndist, true);
    return rc;
}

INF_HD int inf_fixed_tables(InfState &s)
{
    InfTables *t = s.t;
    INF_SYNC();
    for (int i = INF_LANE(); i < 288; i += INF_NLANES) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = INF_LANE(); i < 32; i += INF_NLANES) t->lens[288 + i] = 5;   // (30 and 31 are refused where they are used)
    const int rc = inf_build_lit(s, 288);
    return rc ? rc : inf_build_dist(s, t->lens + 288, 32, true);
}

// the symbols of one fixed or dynamic block, up to its end-of-block code
INF_HD int inf_codes(InfState &s)
{
    InfTables *t = s.t;
    for (;;) {
        inf_refill(s);
        const int sy = inf_symbol(s, t->lit_fast, INF_LIT_BITS, t->lit_cnt, t->lit_sym);
        if (sy < 0) return INF_E_SYMBOL;
        if (sy < 256) {
            if (inf_overrun(s)) return INF_E_INPUT;
            if (s.out_pos >= s.isize) return INF_E_OVER;
            if (INF_LANE() == 0) s.out[s.out_pos] = (uint8_t)sy;
            s.out_pos++;
            continue;
        }
        if (sy == 256) return inf_overrun(s) ? INF_E_INPUT : INF_OK;
        const uint32_t ls = (uint32_t)sy - 257u;
        if (ls >= 29) return INF_E_SYMBOL;   // 286, 287
        // RFC 1951 3.2.5: lengths 3-10 one per code, then four codes per extra bit, 258 on its own
        uint32_t len = 3 + ls;
        if (ls == 28) len = 258;
        else if (ls >= 8) { const uint32_t e = (ls >> 2) - 1; len = 3 + ((4 + (ls & 3u)) << e) + inf_take(s, e); }
        inf_refill(s);
        const int ds = inf_symbol(s, t->dist_fast, INF_DIST_BITS, t->dist_cnt, t->dist_sym);
        if (ds < 0 || ds >= 30) return INF_E_SYMBOL;
        uint32_t dist = 1 + (uint32_t)ds;   // ... distances 1-4 one per code, then two codes per extra bit
        if (ds >= 4) { const uint32_t e = ((uint32_t)ds >> 1) - 1; dist = 1 + ((2 + ((uint32_t)ds & 1u)) << e) + inf_take(s, e); }
        if (inf_overrun(s)) return INF_E_INPUT;
        if (dist > s.out_pos) return INF_E_SYMBOL;   // before the block's first byte: BGZF blocks share no window
        if (len > s.isize - s.out_pos) return INF_E_OVER;
        // The match copy, all lanes: byte i of the match is byte (i mod dist) of the `dist` bytes before out_pos, so every
        // source byte lies before out_pos -- written by EARLIER instructions of this wave (other lanes' literal and match
        // stores, possibly the one just before this), never by this copy.  INF_SYNC is what orders these loads after
        // those stores (see its definition): no lane can read a byte of the window before it is there.
        INF_SYNC();
        const uint8_t *src = s.out + s.out_pos - dist;
        for (uint32_t i = (uint32_t)INF_LANE(); i < len; i += INF_NLANES) s.out[s.out_pos + i] = src[dist < len ? i % dist : i];
        s.out_pos += len;
    }
}

INF_HD int inf_stored(InfState &s)
{
    inf_refill(s);
    (void)inf_take(s, s.bitcnt & 7u);   // to the byte boundary
    const uint32_t len = inf_bits(s, 16), nlen = inf_bits(s, 16);
    if (inf_overrun(s)) return INF_E_INPUT;
    if ((len ^ nlen) != 0xFFFFu) return INF_E_BLOCK;
    const uint32_t pos = (uint32_t)(inf_bits_used(s) >> 3);
    if (len > s.in_len - pos) return INF_E_INPUT;
    if (len > s.isize - s.out_pos) return INF_E_OVER;
    for (uint32_t i = (uint32_t)INF_LANE(); i < len; i += INF_NLANES) s.out[s.out_pos + i] = s.in[pos + i];
    s.out_pos += len;
    inf_seek(s, pos + len);
    return INF_OK;
}

// raw CRC-32 register steps (reflected polynomial 0xEDB88320), table-driven; crc_tab: 256 words
INF_HD uint32_t inf_crc_bytes(const uint32_t *crc_tab, uint32_t c, const uint8_t *p, uint32_t n)
{
#pragma unroll 4
    for (uint32_t i = 0; i < n; i++) c = crc_tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c;
}

// CRC-32 of out[0, n): one segment of INF_CRC_SEG bytes per lane, the FIRST one short, so that every later segment is
// appended with the same operator: reg(A || B) = shift(reg(A)) ^ reg0(B), where shift is the register run over INF_CRC_SEG
// zero bytes -- a 32 x 32 matrix over GF(2) (column j = the image of bit j) -- and reg0 starts from a zero register.
INF_HD uint32_t inf_crc(InfState &s, const uint32_t *crc_tab, const uint32_t *shift_mat)
{
    const uint32_t n = s.out_pos;
    const uint32_t n_seg = n ? (n + INF_CRC_SEG - 1) / INF_CRC_SEG : 1u;   // <= 64
    const uint32_t head = n - (n_seg - 1) * INF_CRC_SEG;                    // bytes of segment 0
    INF_SYNC();   // (the output is stored; the window is free)
    for (uint32_t i = (uint32_t)INF_LANE(); i < n_seg; i += INF_NLANES)
        s.t->win[i] = i == 0 ? inf_crc_bytes(crc_tab, 0xFFFFFFFFu, s.out, head)
                             : inf_crc_bytes(crc_tab, 0u, s.out + head + (size_t)(i - 1) * INF_CRC_SEG, INF_CRC_SEG);
    INF_SYNC();
    uint32_t acc = s.t->win[0];
    for (uint32_t i = 1; i < n_seg; i++) {
        uint32_t m = 0;
        for (int j = 0; j < 32; j++) m ^= ((acc >> j) & 1u) ? shift_mat[j] : 0u;
        acc = m ^ s.t->win[i];
    }
    return acc ^ 0xFFFFFFFFu;
}

// One BGZF block: payload in[0, in_len) -> out[0, isize), checked against the trailer's crc.  Returns the status.
INF_HD int inf_block(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t isize, uint32_t crc, InfTables *t,
                     const uint32_t *crc_tab, const uint32_t *shift_mat)
{
    InfState s;
    s.in = in; s.in_len = in_len; s.skew = (uint32_t)((uintptr_t)in & 3u);
    s.win_base = 0xFFFFFFFFu - INF_WIN_WORDS;   // (no word is in the window)
    s.out = out; s.isize = isize; s.out_pos = 0; s.t = t;
    s.bitbuf = 0; s.bitcnt = 0; s.next_word = 0;
    inf_seek(s, 0);
    for (;;) {
        const uint32_t last = inf_bits(s, 1), type = inf_bits(s, 2);
        if (inf_overrun(s)) return INF_E_INPUT;
        int rc;
        if (type == 0) rc = inf_stored(s);
        else if (type == 3) rc = INF_E_BLOCK;
        else {
            rc = type == 1 ? inf_fixed_tables(s) : inf_dynamic_tables(s);
            if (!rc) rc = inf_codes(s);
        }
        if (rc) return rc;
        if (last) break;
    }
    if (((inf_bits_used(s) + 7) >> 3) != s.in_len) return INF_E_BLOCK;   // the trailer does not follow the final block
    if (s.out_pos != s.isize) return INF_E_UNDER;
    return inf_crc(s, crc_tab, shift_mat) == crc ? INF_OK : INF_E_CRC;
}

// the CRC byte table and the segment-shift matrix (host, at create time)
static void inf_crc_tables(uint32_t *crc_tab /* 256 */, uint32_t *shift_mat /* 32 */)
{
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        crc_tab[i] = c;
    }
    for (int j = 0; j < 32; j++) {
        uint32_t c = 1u << j;
        for (int i = 0; i < INF_CRC_SEG; i++) c = crc_tab[c & 0xFFu] ^ (c >> 8);
        shift_mat[j] = c;
    }
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------------------
struct InfParams {
    const uint8_t *comp;
    uint64_t comp_cap;                 // bytes behind comp that may be read
    const kaamer_bgzf_block *blocks;
    uint32_t n_blocks;
    uint8_t *out;
    uint64_t out_cap;
    unsigned long long *out_off;       // n_blocks + 1: where every block's output starts (prefix sum of isize)
    uint32_t *status;                  // n_blocks
    const uint32_t *crc_tab, *shift_mat;
    unsigned long long *res;           // INF_R_*
};
enum { INF_R_BAD = 0, INF_R_FIRST, INF_R_OUT_BYTES, INF_R_CUT, INF_R_FIRST_STATUS, INF_R_N };
enum { INF_SCAN_THREADS = 1024 };

// out_off[] = exclusive prefix sum of isize (one workgroup: a stretch of blocks per thread, then a scan of the 1024 sums)
__global__ __launch_bounds__(INF_SCAN_THREADS) void inf_offsets_kernel(InfParams p)
{
    __shared__ unsigned long long lds[INF_SCAN_THREADS];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (p.n_blocks + INF_SCAN_THREADS - 1) / INF_SCAN_THREADS;
    const uint64_t b0 = (uint64_t)t * per, b1 = b0 + per < p.n_blocks ? b0 + per : p.n_blocks;
    unsigned long long sum = 0;
    for (uint64_t b = b0; b < b1; b++) sum += p.blocks[b].isize;
    lds[t] = sum;
    __syncthreads();
    unsigned long long v = sum;
    for (uint32_t d = 1; d < INF_SCAN_THREADS; d <<= 1) {
        const unsigned long long o = t >= d ? lds[t - d] : 0ull;
        __syncthreads();
        v += o;
        lds[t] = v;
        __syncthreads();
    }
    unsigned long long at = v - sum;
    for (uint64_t b = b0; b < b1; b++) { p.out_off[b] = at; at += p.blocks[b].isize; }
    if (t == INF_SCAN_THREADS - 1) {
        p.out_off[p.n_blocks] = v;
        p.res[INF_R_OUT_BYTES] = v;
        p.res[INF_R_BAD] = 0;
        p.res[INF_R_FIRST] = 0xFFFFFFFFull;
        p.res[INF_R_CUT] = 0;
        p.res[INF_R_FIRST_STATUS] = 0;
    }
}

__global__ __launch_bounds__(INF_WAVES * 64) __attribute__((amdgpu_waves_per_eu(8))) void inf_blocks_kernel(InfParams p)
{
    __shared__ InfTables tabs[INF_WAVES];
    __shared__ uint32_t crc_tab[256];
    __shared__ uint32_t shift_mat[32];
    for (uint32_t i = threadIdx.x; i < 256; i += INF_WAVES * 64) crc_tab[i] = p.crc_tab[i];
    if (threadIdx.x < 32) shift_mat[threadIdx.x] = p.shift_mat[threadIdx.x];
    __syncthreads();   // the only workgroup barrier: from here on every wave is on its own
    // the wave's number as a scalar: everything the decoder branches on is then uniform to the compiler as well
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t b = blockIdx.x * INF_WAVES + wave;
    if (b >= p.n_blocks) return;
    const kaamer_bgzf_block blk = p.blocks[b];
    const unsigned long long off = p.out_off[b];
    uint32_t st;
    if (blk.isize > (uint32_t)INF_MAX_ISIZE || off + blk.isize > p.out_cap) st = INF_E_OVER;
    else if (blk.comp_off > p.comp_cap || blk.comp_len > p.comp_cap - blk.comp_off) st = INF_E_INPUT;
    else st = (uint32_t)inf_block(p.comp + blk.comp_off, blk.comp_len, p.out + off, blk.isize, blk.crc, &tabs[wave], crc_tab, shift_mat);
    if ((threadIdx.x & 63u) == 0) p.status[b] = st;
}

// (number of bad blocks, index of the first)
__global__ __launch_bounds__(256) void inf_status_kernel(InfParams p)
{
    for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < p.n_blocks; b += (uint64_t)gridDim.x * 256)
        if (p.status[b]) {
            atomicAdd(&p.res[INF_R_BAD], 1ull);
            atomicMin(&p.res[INF_R_FIRST], (unsigned long long)b);
        }
}

// ... and the first bad block's status word next to them (one thread, after inf_status_kernel)
__global__ void inf_first_status_kernel(InfParams p)
{
    if (p.res[INF_R_BAD]) p.res[INF_R_FIRST_STATUS] = p.status[p.res[INF_R_FIRST]];
}

// kaamer_text_cut_fastq on the device: *cut = max(*cut, the greatest p in this tile with text[p-1] == '\n', text[p] == '@')
__global__ __launch_bounds__(256) void inf_cut_kernel(const uint8_t *text, uint64_t n, unsigned long long *cut)
{
    const uint64_t p0 = (uint64_t)blockIdx.x * INF_CUT_TILE + (uint64_t)threadIdx.x * (INF_CUT_TILE / 256);
    unsigned long long best = 0;
    for (uint64_t p = p0 ? p0 : 1; p < p0 + INF_CUT_TILE / 256 && p < n; p++)
        if (text[p] == '@' && text[p - 1] == '\n') best = p;
    for (int d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63u) == 0 && best) atomicMax(cut, best);
}

struct kaamer_inflater {
    int device = 0;
    uint64_t max_comp = 0;
    uint32_t max_blocks = 0;
    DevBuf<unsigned long long> d_out_off;      // max_blocks + 1, then INF_R_N result words
    DevBuf<uint32_t> d_status;                 // max_blocks, then the CRC table (256) and the shift matrix (32)
    PinnedBuf<unsigned long long> h_res;
    bool queued = false;
    ~kaamer_inflater() { (void)hipSetDevice(device); }   // (before the buffers go)
};

static void inf_launch_cut(const uint8_t *d_text, uint64_t n, unsigned long long *d_cut, hipStream_t s)
{
    const uint64_t tiles = (n + INF_CUT_TILE - 1) / INF_CUT_TILE;
    if (tiles) hipLaunchKernelGGL(inf_cut_kernel, dim3((uint32_t)tiles), dim3(256), 0, s, d_text, n, d_cut);
}

extern "C" {

void kaamer_inflater_free(kaamer_inflater *inf) { delete inf; }

int kaamer_inflater_create(int device, uint64_t max_comp_bytes, uint32_t max_blocks, kaamer_inflater **out)
{
    if (!out) return kaamer_fail(KAAMER_E_ARG, "inflater_create: bad argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(device));
    kaamer_inflater *inf = new (std::nothrow) kaamer_inflater();
    if (!inf) return kaamer_fail(KAAMER_E_NOMEM, "inflater");
    inf->device = device; inf->max_comp = max_comp_bytes; inf->max_blocks = max_blocks;
    int rc = reserve_group(nullptr, GROW_EXACT, { want(inf->d_out_off, (size_t)max_blocks + 1 + INF_R_N), want(inf->d_status, (size_t)max_blocks + 256 + 32),
                                                  want(inf->h_res, (size_t)INF_R_N) });
    if (!rc) {
        uint32_t tabs[256 + 32];
        inf_crc_tables(tabs, tabs + 256);
        const hipError_t e = hipMemcpy(inf->d_status + max_blocks, tabs, sizeof tabs, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "inflater: H2D: %s", hipGetErrorString(e));
    }
    if (rc) { delete inf; return rc; }
    *out = inf;
    return KAAMER_OK;
}

void kaamer_inflater_geometry(uint32_t out[4])
{
    if (!out) return;
    out[0] = INF_CRC_SEG; out[1] = INF_WAVES; out[2] = INF_CUT_TILE; out[3] = INF_SCAN_THREADS;
}

// the inflate, and behind it on the same stream -- when cut_len is not 0 -- the cut of cut_text[0, cut_len) (a text that
// ends with the inflated bytes: the file form's tail + blocks): one wait brings the status words' summary and the cut
static int inf_enqueue(kaamer_inflater *inf, const uint8_t *d_comp, uint64_t comp_bytes, const kaamer_bgzf_block *d_blocks, uint32_t n_blocks,
                       uint8_t *d_out, uint64_t out_cap, const uint8_t *cut_text, uint64_t cut_len, void *stream)
{
    if (!inf || (n_blocks && (!d_comp || !d_blocks)) || (!d_out && out_cap)) return kaamer_fail(KAAMER_E_ARG, "inflate_bgzf_device: bad argument");
    if (n_blocks > inf->max_blocks)
        return kaamer_fail(KAAMER_E_ARG, "inflate_bgzf_device: %u blocks, the inflater was created for %u", n_blocks, inf->max_blocks);
    if ((uintptr_t)d_blocks & 7u) return kaamer_fail(KAAMER_E_ARG, "inflate_bgzf_device: the block table must start at an 8-byte boundary");
    HIPCHK(hipSetDevice(inf->device));
    hipStream_t s = (hipStream_t)stream;
    InfParams p;
    p.comp = d_comp; p.comp_cap = comp_bytes; p.blocks = d_blocks; p.n_blocks = n_blocks;
    p.out = d_out; p.out_cap = out_cap;
    p.out_off = inf->d_out_off; p.res = inf->d_out_off + (size_t)inf->max_blocks + 1;
    p.status = inf->d_status; p.crc_tab = inf->d_status + inf->max_blocks; p.shift_mat = p.crc_tab + 256;
    hipLaunchKernelGGL(inf_offsets_kernel, dim3(1), dim3(INF_SCAN_THREADS), 0, s, p);
    if (n_blocks) {
        hipLaunchKernelGGL(inf_blocks_kernel, dim3((n_blocks + INF_WAVES - 1) / INF_WAVES), dim3(INF_WAVES * 64), 0, s, p);
        uint32_t g = (n_blocks + 255) / 256;
        if (g > 1024) g = 1024;
        hipLaunchKernelGGL(inf_status_kernel, dim3(g), dim3(256), 0, s, p);
        hipLaunchKernelGGL(inf_first_status_kernel, dim3(1), dim3(1), 0, s, p);
    }
    if (cut_len) inf_launch_cut(cut_text, cut_len, p.res + INF_R_CUT, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(inf->h_res, p.res, INF_R_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    inf->queued = true;
    return KAAMER_OK;
}

int kaamer_inflate_bgzf_device(kaamer_inflater *inf, const uint8_t *d_comp, uint64_t comp_bytes, const kaamer_bgzf_block *d_blocks,
                               uint32_t n_blocks, uint8_t *d_out, uint64_t out_cap, void *stream)
{
    if (inf && comp_bytes > inf->max_comp)
        return kaamer_fail(KAAMER_E_ARG, "inflate_bgzf_device: %llu compressed bytes, the inflater was created for %llu",
                           (unsigned long long)comp_bytes, (unsigned long long)inf->max_comp);
    return inf_enqueue(inf, d_comp, comp_bytes, d_blocks, n_blocks, d_out, out_cap, nullptr, 0, stream);
}

int kaamer_inflater_finish(kaamer_inflater *inf, void *stream, kaamer_inflate_result *out)
{
    if (!inf || !out) return kaamer_fail(KAAMER_E_ARG, "inflater_finish: bad argument");
    memset(out, 0, sizeof *out);
    if (!inf->queued) return kaamer_fail(KAAMER_E_ARG, "inflater_finish: nothing was inflated");
    HIPCHK(hipSetDevice(inf->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    out->n_bad = (uint32_t)inf->h_res[INF_R_BAD];
    out->first_bad = (uint32_t)inf->h_res[INF_R_FIRST];
    out->first_bad_status = (uint32_t)inf->h_res[INF_R_FIRST_STATUS];
    out->out_bytes = inf->h_res[INF_R_OUT_BYTES];
    out->d_status = inf->d_status;
    return KAAMER_OK;
}

int kaamer_text_cut_fastq_device(int device, const uint8_t *d_text, uint64_t n_bytes, void *stream, uint64_t *cut)
{
    if (!cut || (!d_text && n_bytes)) return kaamer_fail(KAAMER_E_ARG, "text_cut_fastq_device: bad argument");
    *cut = 0;
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf<unsigned long long> d_cut;   // the call's scratch: goes when the call returns (the stream is waited for below)
    const int rc = reserve(d_cut, 1, GROW_EXACT, s);
    if (rc) return rc;
    unsigned long long h = 0;
    hipError_t e = hipMemsetAsync(d_cut, 0, sizeof h, s);
    if (e == hipSuccess) { inf_launch_cut(d_text, n_bytes, d_cut, s); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_cut, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return kaamer_fail(KAAMER_E_HIP, "text_cut_fastq_device: %s", hipGetErrorString(e));
    *cut = h;
    return KAAMER_OK;
}

}  // extern "C"
#endif  // __HIPCC__
