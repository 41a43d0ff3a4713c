// fmt_double.h — "%e" and "%.2f" of a float64 as Go's fmt (strconv.FormatFloat with precision 6 / 2) prints them: the
// double's EXACT value rounded half-even at the last printed digit, for every finite double, subnormals included; NaN,
// +Inf and -Inf as Go spells them.  One statement for the host formatter (tsv_format.cpp) and the device stage
// (tsv_aln_rows.hip.inc): the functions are templates over a byte sink (put(char)) and a limb store (get(i) / set(i, v),
// KFMT_LIMBS 32-bit words), so that the device keeps the limbs in LDS, where a runtime index costs nothing, and the host
// in an array.
//
// A finite double is m * 2^e with m < 2^53.  What both formats need of its decimal expansion is a HEAD -- the first
// significant digits, at least eight of them -- where the head starts (the decimal exponent of its first digit) and whether
// any nonzero digit follows it (sticky): rounding half-even at any digit of the head is then exact.
//   e >= 0   an integer.  Up to 2^64 in a register; beyond, m << e in limbs, divided by 10^9 until nothing is left: the
//            remainders are its base-10^9 digits, least significant first, kept at the top of the same store (a division
//            frees 29.9 bits, a digit takes 32: with 36 limbs for the 32 of 2^1024 digit i never meets the quotient).
//   e <  0   integer part m >> -e (below 2^53) and a fraction over 2^-e, shifted so that the binary point lies on a limb
//            boundary: every multiplication by 10^9 carries the next nine decimals out of the top limb.  At most 36 zero
//            groups precede the first nonzero one (2^-1074 = 4.9e-324).
#ifndef KAAMER_FMT_DOUBLE_H
#define KAAMER_FMT_DOUBLE_H
#include <stdint.h>
#include <string.h>

#if defined(__HIP__)
#define KFMT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KFMT_HD inline
#endif
#define KFMT_LIMBS 36
#define KFMT_E9 1000000000u

// the limb store of the host
struct KfmtArray {
    uint32_t x[KFMT_LIMBS];
    KFMT_HD uint32_t get(uint32_t i) const { return x[i]; }
    KFMT_HD void set(uint32_t i, uint32_t v) { x[i] = v; }
};

struct KfmtHead {
    uint64_t head;    // the first ndig significant digits (the first one is not 0)
    int32_t ndig;     // 8 to 20
    int32_t exp10;    // the value is d.ddd... * 10^exp10
    bool sticky;      // a nonzero digit follows the head
};

KFMT_HD uint64_t kfmt_bits(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

// v = m * 2^e (finite v): false for zero
KFMT_HD bool kfmt_split(uint64_t bits, uint64_t *m, int32_t *e)
{
    const uint64_t frac = bits & 0xFFFFFFFFFFFFFull;
    const int32_t ex = (int32_t)((bits >> 52) & 0x7FFu);
    *m = ex ? (frac | (1ull << 52)) : frac;
    *e = (ex ? ex : 1) - 1075;
    return *m != 0;
}

KFMT_HD int32_t kfmt_digits(uint64_t v)
{
    int32_t n = 1;
    while (v >= 10ull) { v /= 10ull; n++; }
    return n;
}

KFMT_HD uint64_t kfmt_pow10(int32_t n)
{
    uint64_t d = 1;
    for (int32_t k = 0; k < n; k++) d *= 10ull;
    return d;
}

template <class Sink> KFMT_HD void kfmt_put_u64(Sink &o, uint64_t v)
{
    for (uint64_t div = kfmt_pow10(kfmt_digits(v) - 1); div; div /= 10ull) { o.put((char)('0' + (uint32_t)(v / div))); v %= div; }
}

// nine digits, zeros in front
template <class Sink> KFMT_HD void kfmt_put_group(Sink &o, uint32_t v)
{
    for (uint32_t div = 100000000u; div; div /= 10u) { o.put((char)('0' + v / div)); v %= div; }
}

// limbs [first, first + 3) = m << sh (sh < 32, m < 2^53)
template <class Limbs> KFMT_HD void kfmt_set3(Limbs &X, uint32_t first, uint64_t m, uint32_t sh)
{
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    X.set(first, lo << sh);
    X.set(first + 1, (hi << sh) | (sh ? lo >> (32u - sh) : 0u));
    X.set(first + 2, sh ? hi >> (32u - sh) : 0u);
}

// m * 2^e with e >= 12 as base-10^9 digits: digit i (the least significant is 0) is left in limb KFMT_LIMBS - 1 - i;
// -> their number (at least 3: the value is 2^64 or more)
template <class Limbs> KFMT_HD uint32_t kfmt_int_groups(Limbs &X, uint64_t m, int32_t e)
{
    const uint32_t ws = (uint32_t)e >> 5, sh = (uint32_t)e & 31u;
    for (uint32_t i = 0; i < ws; i++) X.set(i, 0u);
    kfmt_set3(X, ws, m, sh);                         // e <= 971: ws + 3 <= 33
    uint32_t n = ws + 3u, groups = 0;
    while (n && X.get(n - 1u) == 0u) n--;
    while (n) {
        uint64_t rem = 0;
        for (uint32_t i = n; i-- > 0u;) {
            const uint64_t cur = (rem << 32) | X.get(i);
            X.set(i, (uint32_t)(cur / KFMT_E9));
            rem = cur % KFMT_E9;
        }
        while (n && X.get(n - 1u) == 0u) n--;
        X.set(KFMT_LIMBS - 1u - groups, (uint32_t)rem);
        groups++;
    }
    return groups;
}

// the fraction in limbs [0, *top) times 10^9: -> the nine decimals that leave it (L limbs make the whole fraction)
template <class Limbs> KFMT_HD uint32_t kfmt_frac_step(Limbs &X, uint32_t *top, uint32_t L)
{
    uint64_t carry = 0;
    for (uint32_t i = 0; i < *top; i++) {
        const uint64_t t = (uint64_t)X.get(i) * KFMT_E9 + carry;
        X.set(i, (uint32_t)t);
        carry = t >> 32;
    }
    if (*top < L) { X.set(*top, (uint32_t)carry); (*top)++; return 0u; }
    return (uint32_t)carry;
}

// the head of m * 2^e (m != 0)
template <class Limbs> KFMT_HD KfmtHead kfmt_head(Limbs &X, uint64_t m, int32_t e)
{
    KfmtHead h;
    if (e >= 0 && e <= 11) {
        h.head = m << e;
        h.ndig = kfmt_digits(h.head);
        h.exp10 = h.ndig - 1;
        h.sticky = false;
        return h;
    }
    if (e > 11) {
        const uint32_t groups = kfmt_int_groups(X, m, e);
        const uint32_t c0 = X.get(KFMT_LIMBS - groups), c1 = X.get(KFMT_LIMBS - groups + 1u);
        h.head = (uint64_t)c0 * KFMT_E9 + c1;
        h.ndig = kfmt_digits(c0) + 9;
        h.exp10 = kfmt_digits(c0) + 9 * (int32_t)(groups - 1u) - 1;
        h.sticky = false;
        for (uint32_t i = KFMT_LIMBS - groups + 2u; i < KFMT_LIMBS; i++) h.sticky = h.sticky || X.get(i) != 0u;
        return h;
    }
    const uint32_t s = (uint32_t)(-e);               // 1 .. 1074
    const uint64_t ip = s <= 52u ? m >> s : 0ull;
    const uint64_t fm = s <= 52u ? m & ((1ull << s) - 1ull) : m;
    if (ip >= 10000000ull) {
        h.head = ip;
        h.ndig = kfmt_digits(ip);
        h.exp10 = h.ndig - 1;
        h.sticky = fm != 0ull;
        return h;
    }
    const uint32_t L = (s + 31u) >> 5;               // 1 .. 34
    kfmt_set3(X, 0u, fm, 32u * L - s);               // fm < 2^min(s, 53): the shifted fraction is below 2^(32 L)
    uint32_t top = L < 3u ? L : 3u;
    uint32_t c0 = kfmt_frac_step(X, &top, L);
    if (ip) {
        h.head = ip * KFMT_E9 + c0;
        h.ndig = kfmt_digits(ip) + 9;
        h.exp10 = kfmt_digits(ip) - 1;
    } else {
        int32_t zeros = 0;
        for (; c0 == 0u && zeros < 40; zeros++) c0 = kfmt_frac_step(X, &top, L);
        const uint32_t c1 = kfmt_frac_step(X, &top, L);
        h.head = (uint64_t)c0 * KFMT_E9 + c1;
        h.ndig = kfmt_digits(c0) + 9;
        h.exp10 = -(9 * zeros + (9 - kfmt_digits(c0)) + 1);
    }
    h.sticky = false;
    for (uint32_t i = 0; i < top; i++) h.sticky = h.sticky || X.get(i) != 0u;
    return h;
}

// NaN, +Inf, -Inf: true when v is one of them (and printed)
template <class Sink> KFMT_HD bool kfmt_special(Sink &o, uint64_t bits)
{
    if (((bits >> 52) & 0x7FFu) != 0x7FFu) return false;
    if (bits & 0xFFFFFFFFFFFFFull) { o.put('N'); o.put('a'); o.put('N'); return true; }
    o.put((bits >> 63) ? '-' : '+'); o.put('I'); o.put('n'); o.put('f');
    return true;
}

// fmt.Sprintf("%e", v): d.dddddde+XX, the exponent with at least two digits
template <class Sink, class Limbs> KFMT_HD void kfmt_exp6(Sink &o, double v, Limbs &X)
{
    const uint64_t bits = kfmt_bits(v);
    if (kfmt_special(o, bits)) return;
    if (bits >> 63) o.put('-');
    uint64_t m;
    int32_t e;
    uint64_t q = 0;
    int32_t exp10 = 0;
    if (kfmt_split(bits, &m, &e)) {
        const KfmtHead h = kfmt_head(X, m, e);
        const uint64_t div = kfmt_pow10(h.ndig - 7), rem = h.head % div, half = div / 2ull;
        q = h.head / div;
        exp10 = h.exp10;
        if (rem > half || (rem == half && (h.sticky || (q & 1ull)))) q++;
        if (q == 10000000ull) { q = 1000000ull; exp10++; }
    }
    o.put((char)('0' + (uint32_t)(q / 1000000ull)));
    o.put('.');
    uint32_t f = (uint32_t)(q % 1000000ull);
    for (uint32_t div = 100000u; div; div /= 10u) { o.put((char)('0' + f / div)); f %= div; }
    o.put('e');
    o.put(exp10 < 0 ? '-' : '+');
    const uint32_t a = (uint32_t)(exp10 < 0 ? -exp10 : exp10);
    if (a >= 100u) o.put((char)('0' + a / 100u));
    o.put((char)('0' + a / 10u % 10u));
    o.put((char)('0' + a % 10u));
}

// fmt.Sprintf("%.2f", v) of a value below 2^64 in 64-bit integers: false (nothing printed but the sign) for a larger one
template <class Sink> KFMT_HD bool kfmt_fixed2_small(Sink &o, double v)
{
    const uint64_t bits = kfmt_bits(v);
    if (kfmt_special(o, bits)) return true;
    if (bits >> 63) o.put('-');
    uint64_t m, cents = 0;
    int32_t e;
    if (kfmt_split(bits, &m, &e)) {
        if (e > 11) return false;
        if (e >= 0) {
            kfmt_put_u64(o, m << e);
            o.put('.'); o.put('0'); o.put('0');
            return true;
        }
        const uint32_t s = (uint32_t)(-e);
        // s >= 61: m * 100 < 2^60 <= 2^(s - 1), less than half a hundredth
        if (s < 61u) {
            const uint64_t ip = s <= 52u ? m >> s : 0ull, fm = s <= 52u ? m & ((1ull << s) - 1ull) : m;
            const uint64_t p = fm * 100ull, rem = p & ((1ull << s) - 1ull), half = 1ull << (s - 1u);
            cents = ip * 100ull + (p >> s);
            if (rem > half || (rem == half && (cents & 1ull))) cents++;
        }
    }
    kfmt_put_u64(o, cents / 100ull);
    const uint32_t c = (uint32_t)(cents % 100ull);
    o.put('.');
    o.put((char)('0' + c / 10u));
    o.put((char)('0' + c % 10u));
    return true;
}

// ... of any double
template <class Sink, class Limbs> KFMT_HD void kfmt_fixed2(Sink &o, double v, Limbs &X)
{
    if (kfmt_fixed2_small(o, v)) return;
    uint64_t m;
    int32_t e;
    (void)kfmt_split(kfmt_bits(v), &m, &e);
    const uint32_t groups = kfmt_int_groups(X, m, e);
    kfmt_put_u64(o, X.get(KFMT_LIMBS - groups));
    for (uint32_t i = KFMT_LIMBS - groups + 1u; i < KFMT_LIMBS; i++) kfmt_put_group(o, X.get(i));
    o.put('.'); o.put('0'); o.put('0');
}

#endif /* KAAMER_FMT_DOUBLE_H */
