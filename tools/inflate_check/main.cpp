// inflate_check — the BGZF decoder of the device inflate (kaamer_amd/csrc/inflate.hip.inc: the very text the kernel is
// compiled from, here with one "lane") and kaamer_bgzf_scan under AddressSanitizer + UBSan, against zlib:
//   1. a built-in corpus (stored, fixed, dynamic, many deflate blocks per BGZF block, Huffman-only, RLE, empty, 1 byte,
//      65 280 and 65 536 bytes, every period 1-70, a hand-made match at distance 32 768, incompressible bytes) must inflate
//      to what zlib gives, with status 0;
//   2. seeded mutations of valid blocks (byte flips, truncations, header / trailer / BSIZE edits) must each end with a
//      status -- or a refusal by the scan -- or with output equal to zlib's.  Payload and output live in exact-size heap
//      blocks, so a byte read or written outside them is the sanitizer's to find.
// CPU only.    make -C tools/inflate_check test
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <zlib.h>

#include "../../kaamer_amd/csrc/kaamer_internal.h"
#include "../../kaamer_amd/csrc/inflate.hip.inc"

// the two symbols host_search.cpp takes from search.hip
static char g_err[512] = "";
int kaamer_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *kaamer_last_error(void) { return g_err; }

static int g_failed = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            if (g_failed < 20) {                                \
                fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__);                   \
                fprintf(stderr, "\n");                          \
            }                                                   \
            g_failed++;                                         \
        }                                                       \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static uint32_t g_crc_tab[256], g_shift[32];

static uint64_t g_state = 20261019ull;
static uint64_t rnd(uint64_t n) { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (g_state >> 33) % n; }

static Bytes deflate_raw(const Bytes &text, int level, int mem_level, int strategy)
{
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, -15, mem_level, strategy) != Z_OK) abort();
    Bytes buf(deflateBound(&z, text.size()) + 64);
    z.next_in = (Bytef *)text.data(); z.avail_in = (uInt)text.size();
    z.next_out = buf.data(); z.avail_out = (uInt)buf.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    buf.resize(buf.size() - z.avail_out);
    deflateEnd(&z);
    return buf;
}

// one BGZF member around a deflate payload; pre_extra: a subfield in front of BC
static Bytes bgzf_member(const Bytes &payload, const Bytes &text, bool pre_extra = false)
{
    Bytes m = { 0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF };
    const uint32_t xlen = pre_extra ? 6 + 7 : 6;
    m.push_back(xlen & 0xFF); m.push_back(xlen >> 8);
    if (pre_extra) { const uint8_t x[7] = { 'X', 'Y', 3, 0, 1, 2, 3 }; m.insert(m.end(), x, x + 7); }
    const uint32_t bsize = 12 + xlen + (uint32_t)payload.size() + 8 - 1;
    const uint8_t bc[6] = { 'B', 'C', 2, 0, (uint8_t)(bsize & 0xFF), (uint8_t)(bsize >> 8) };
    m.insert(m.end(), bc, bc + 6);
    m.insert(m.end(), payload.begin(), payload.end());
    const uint32_t crc = (uint32_t)crc32(crc32(0, nullptr, 0), text.data(), (uInt)text.size()), isize = (uint32_t)text.size();
    for (int i = 0; i < 4; i++) m.push_back((crc >> (8 * i)) & 0xFF);
    for (int i = 0; i < 4; i++) m.push_back((isize >> (8 * i)) & 0xFF);
    return m;
}

struct BitWriter {
    Bytes out;
    uint32_t acc = 0, n = 0;
    void bits(uint32_t v, uint32_t k) { for (uint32_t i = 0; i < k; i++) { acc |= ((v >> i) & 1u) << n; if (++n == 8) { out.push_back((uint8_t)acc); acc = 0; n = 0; } } }
    void code(uint32_t v, uint32_t k) { for (uint32_t i = k; i-- > 0;) bits((v >> i) & 1u, 1); }   // Huffman codes go most significant bit first
    void align() { if (n) { out.push_back((uint8_t)acc); acc = 0; n = 0; } }
};

// zlib on one member: true and the text when it is a whole valid gzip member
static bool zlib_member(const uint8_t *m, size_t len, Bytes *text)
{
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) abort();
    text->assign(65536 + 1024, 0);
    z.next_in = (Bytef *)m; z.avail_in = (uInt)len;
    z.next_out = text->data(); z.avail_out = (uInt)text->size();
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.avail_in == 0;
    text->resize(text->size() - z.avail_out);
    inflateEnd(&z);
    return ok;
}

// The first block of `buf` through the scan and the decoder.  -1: the scan refuses it; else the status, and the text.
static int decode_first(const Bytes &buf, Bytes *text, uint64_t *member_len)
{
    kaamer_bgzf_block b;
    uint64_t n = 0, consumed = 0;
    std::vector<uint8_t> exact(buf.begin(), buf.end());   // (exact size: the scan's reads are checked too)
    const int rc = kaamer_bgzf_scan(exact.data(), exact.size(), &b, 1, &n, &consumed);
    CHECK(rc == KAAMER_OK, "scan: %d", rc);
    if (rc || n == 0) return -1;
    CHECK(b.comp_off + b.comp_len + 8 <= exact.size() && b.isize <= 65536, "the scan's block leaves the buffer");
    *member_len = b.comp_off + b.comp_len + 8;
    const uint32_t skew = (uint32_t)rnd(4);
    // malloc aligns to 16: the payload at every offset within a word, its end at the end of the allocation
    uint8_t *in = (uint8_t *)malloc(skew + b.comp_len + (skew + b.comp_len == 0 ? 1 : 0));
    uint8_t *out = (uint8_t *)malloc(b.isize ? b.isize : 1);
    if (b.comp_len) memcpy(in + skew, exact.data() + b.comp_off, b.comp_len);
    InfTables *t = (InfTables *)malloc(sizeof(InfTables));
    memset(t, 0xA5, sizeof *t);
    const int st = inf_block(in + skew, b.comp_len, out, b.isize, b.crc, t, g_crc_tab, g_shift);
    text->assign(out, out + (st == 0 ? b.isize : 0));
    free(t); free(out); free(in);
    return st;
}

static void expect_good(const char *what, const Bytes &member, const Bytes &text)
{
    Bytes got, ztext;
    uint64_t mlen = 0;
    const int st = decode_first(member, &got, &mlen);
    CHECK(st == 0, "%s: status %d", what, st);
    CHECK(zlib_member(member.data(), member.size(), &ztext) && ztext == text, "%s: zlib does not give the text back", what);
    if (st == 0) CHECK(got == text && mlen == member.size(), "%s: %zu bytes out, %zu expected", what, got.size(), text.size());
}

// where BSIZE sits: BC is the last subfield of the members made here
static size_t bsize_at(const Bytes &m) { return 12 + ((size_t)m[10] | (size_t)m[11] << 8) - 2; }
static void set_bsize(Bytes &m, uint32_t bs) { const size_t at = bsize_at(m); m[at] = bs & 0xFF; m[at + 1] = (bs >> 8) & 0xFF; }

static Bytes fastq_text(size_t n)
{
    Bytes t;
    uint64_t r = 0;
    while (t.size() < n) {
        char head[64];
        const int len = 40 + (int)rnd(110);
        snprintf(head, sizeof head, "@read%llu len=%d\n", (unsigned long long)r++, len);
        t.insert(t.end(), head, head + strlen(head));
        for (int i = 0; i < len; i++) t.push_back("ACGTN"[rnd(100) < 99 ? rnd(4) : 4]);
        t.push_back('\n'); t.push_back('+'); t.push_back('\n');
        for (int i = 0; i < len; i++) t.push_back((uint8_t)('!' + 20 + rnd(20)));
        t.push_back('\n');
    }
    t.resize(n);
    return t;
}

int main(int argc, char **argv)
{
    const long n_mut = argc > 1 ? atol(argv[1]) : 120000;
    inf_crc_tables(g_crc_tab, g_shift);
    struct Mode { const char *name; int level, mem, strategy; };
    const Mode modes[] = { { "stored", 0, 8, Z_DEFAULT_STRATEGY }, { "level 1", 1, 8, Z_DEFAULT_STRATEGY }, { "fixed", 6, 8, Z_FIXED },
                           { "level 9 memLevel 1", 9, 1, Z_DEFAULT_STRATEGY }, { "huffman only", 6, 8, Z_HUFFMAN_ONLY },
                           { "rle", 6, 8, Z_RLE }, { "level 6", 6, 8, Z_DEFAULT_STRATEGY } };
    std::vector<std::pair<std::string, Bytes>> texts;
    texts.push_back({ "empty", Bytes() });
    texts.push_back({ "one byte", Bytes(1, 'x') });
    texts.push_back({ "fastq 65280", fastq_text(65280) });
    texts.push_back({ "fastq 3000", fastq_text(3000) });
    texts.push_back({ "65536 A", Bytes(65536, 'A') });
    for (uint32_t seg : { (uint32_t)INF_CRC_SEG - 1, (uint32_t)INF_CRC_SEG, (uint32_t)INF_CRC_SEG + 1, 2u * INF_CRC_SEG + 1 }) texts.push_back({ "fastq at the CRC segment", fastq_text(seg) });
    { Bytes r(65280); for (auto &c : r) c = (uint8_t)rnd(256); texts.push_back({ "incompressible", r }); }
    for (int k = 1; k <= 70; k++) {
        Bytes unit(k), t;
        for (auto &c : unit) c = (uint8_t)('a' + rnd(26));
        while (t.size() < 700) t.insert(t.end(), unit.begin(), unit.end());
        texts.push_back({ "period " + std::to_string(k), t });
    }
    std::vector<std::pair<Bytes, Bytes>> valid_small;   // (member, text) for the mutations
    std::vector<std::pair<Bytes, Bytes>> valid_large;
    for (auto &tx : texts)
        for (const Mode &m : modes) {
            const Bytes member = bgzf_member(deflate_raw(tx.second, m.level, m.mem, m.strategy), tx.second, tx.second.size() == 3000);
            if (member.size() > 65536) continue;   // (no BGZF block: bgzip would have cut the text)
            expect_good((tx.first + ", " + m.name).c_str(), member, tx.second);
            if (tx.second.size() <= 3000 && (tx.first[0] != 'p' || m.level != 0)) valid_small.push_back({ member, tx.second });
            else if (tx.second.size() > 3000) valid_large.push_back({ member, tx.second });
        }
    {   // a match at distance 32 768 (zlib's deflate stops 262 short of it): 32 768 stored bytes, then a fixed block
        Bytes head(32768);
        for (auto &c : head) c = (uint8_t)rnd(256);
        BitWriter w;
        w.bits(0, 1); w.bits(0, 2); w.align();
        w.bits(32768, 16); w.bits(32768 ^ 0xFFFF, 16);
        w.out.insert(w.out.end(), head.begin(), head.end());
        w.bits(1, 1); w.bits(1, 2);
        w.code(0xC0 + 5, 8);                    // length symbol 285: 258 bytes
        w.code(29, 5); w.bits(32768 - 24577, 13);
        w.code(0, 7);                            // end of block
        w.align();
        Bytes text = head;
        text.insert(text.end(), head.begin(), head.begin() + 258);
        const Bytes member = bgzf_member(w.out, text);
        expect_good("distance 32768", member, text);
        valid_large.push_back({ member, text });
    }
    // the malformed cases the GPU test uses: each has its status here first
    {
        const Bytes text = fastq_text(2000);
        const Bytes member = bgzf_member(deflate_raw(text, 6, 8, Z_DEFAULT_STRATEGY), text);
        Bytes got;
        uint64_t mlen;
        Bytes m = member; m[m.size() - 8] ^= 1;
        CHECK(decode_first(m, &got, &mlen) == INF_E_CRC, "flipped CRC");
        m = member; m[m.size() - 4] += 1;
        CHECK(decode_first(m, &got, &mlen) == INF_E_UNDER, "ISIZE + 1");
        m = member; m[m.size() - 4] -= 1;
        CHECK(decode_first(m, &got, &mlen) == INF_E_OVER, "ISIZE - 1");
        // the payload cut short by 5 bytes (BSIZE follows, so the scan still takes the block)
        m = member; m.erase(m.end() - 13, m.end() - 8);
        set_bsize(m, (uint32_t)m.size() - 1);
        CHECK(decode_first(m, &got, &mlen) == INF_E_INPUT, "payload cut short");
        BitWriter w;   // a dynamic block whose 19 code-length codes all have length 1
        w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4);
        for (int i = 0; i < 19; i++) w.bits(1, 3);
        w.align();
        CHECK(decode_first(bgzf_member(w.out, Bytes(4, 'A')), &got, &mlen) == INF_E_CODE, "over-subscribed code");
        BitWriter d;   // fixed block: 'A', then length 3 at distance 2
        d.bits(1, 1); d.bits(1, 2); d.code(0x30 + 'A', 8); d.code(1, 7); d.code(1, 5); d.code(0, 7); d.align();
        CHECK(decode_first(bgzf_member(d.out, Bytes(4, 'A')), &got, &mlen) == INF_E_SYMBOL, "distance before the block's start");
        BitWriter b3;
        b3.bits(1, 1); b3.bits(3, 2); b3.align();
        CHECK(decode_first(bgzf_member(b3.out, Bytes()), &got, &mlen) == INF_E_BLOCK, "block type 3");
    }
    // the scan by hand
    {
        const Bytes text = fastq_text(500);
        const Bytes a = bgzf_member(deflate_raw(text, 6, 8, Z_DEFAULT_STRATEGY), text), eof = bgzf_member(deflate_raw(Bytes(), 6, 8, Z_DEFAULT_STRATEGY), Bytes());
        CHECK(eof.size() == 28, "the empty block has %zu bytes", eof.size());
        Bytes file = a; file.insert(file.end(), a.begin(), a.end()); file.insert(file.end(), eof.begin(), eof.end());
        kaamer_bgzf_block blk[4];
        uint64_t n = 0, used = 0;
        CHECK(kaamer_bgzf_scan(file.data(), file.size(), blk, 4, &n, &used) == KAAMER_OK && n == 3 && used == file.size() && blk[2].isize == 0 && blk[1].comp_off == a.size() + 18, "three blocks");
        CHECK(kaamer_bgzf_scan(file.data(), file.size() - 1, blk, 4, &n, &used) == KAAMER_OK && n == 2 && used == 2 * a.size(), "a last block cut short");
        CHECK(kaamer_bgzf_scan(file.data(), file.size(), nullptr, 0, &n, &used) == KAAMER_OK && n == 3, "counting only");
        CHECK(kaamer_bgzf_scan(nullptr, 0, nullptr, 0, &n, &used) == KAAMER_OK && n == 0 && used == 0, "no bytes");
    }
    // seeded mutations
    long refused = 0, status[8] = { 0 }, same = 0;
    for (long it = 0; it < n_mut; it++) {
        const bool large = it % 64 == 0;
        const auto &pick = large ? valid_large[rnd(valid_large.size())] : valid_small[rnd(valid_small.size())];
        Bytes m = pick.first;
        const Bytes &next = valid_small[rnd(valid_small.size())].first;   // what follows the member in the buffer
        const uint64_t kind = rnd(8);
        if (kind <= 2 && m.size() > 26) m[18 + rnd(m.size() - 26)] ^= (uint8_t)(1u << rnd(8));       // a bit of the payload
        else if (kind == 3) m[rnd(m.size())] = (uint8_t)rnd(256);                                    // a byte anywhere
        else if (kind == 4) m.resize(rnd(m.size()));                                                 // truncation of the member
        else if (kind == 5) {                                                                        // payload cut short, BSIZE follows
            const size_t cut = 1 + rnd(m.size() > 40 ? 12 : 1);
            if (m.size() >= 26 + cut) { m.erase(m.end() - 8 - cut, m.end() - 8); set_bsize(m, (uint32_t)m.size() - 1); }
        } else if (kind == 6) m[m.size() - 1 - rnd(8)] ^= (uint8_t)(1u << rnd(8));                   // the trailer
        else set_bsize(m, (uint32_t)m.size() - 1 + (uint32_t)rnd(9) - 4);   // BSIZE
        if (rnd(4) == 0 && m.size() >= 18) m[rnd(18)] ^= (uint8_t)(1u << rnd(8));                    // ... and the header
        Bytes buf = m;
        buf.insert(buf.end(), next.begin(), next.end());
        Bytes got, ztext;
        uint64_t mlen = 0;
        const int st = decode_first(buf, &got, &mlen);
        if (st < 0) { refused++; continue; }
        CHECK(st >= 0 && st <= 7, "status %d", st);
        if (st < 0 || st > 7) continue;
        status[st]++;
        if (st == 0) {
            const bool zok = zlib_member(buf.data(), (size_t)mlen, &ztext);
            CHECK(zok && ztext == got, "mutation %ld (kind %llu): status 0 with %zu bytes, zlib %s with %zu", it, (unsigned long long)kind, got.size(), zok ? "agrees" : "refuses", ztext.size());
            if (zok && ztext == got) same++;
        }
    }
    printf("inflate_check: %ld mutations: %ld refused by the scan, status 0 (output == zlib's) %ld, 1:%ld 2:%ld 3:%ld 4:%ld 5:%ld 6:%ld 7:%ld\n",
           n_mut, refused, same, status[1], status[2], status[3], status[4], status[5], status[6], status[7]);
    if (g_failed) { fprintf(stderr, "%d check(s) failed\n", g_failed); return 1; }
    printf("inflate_check: ok\n");
    return 0;
}
