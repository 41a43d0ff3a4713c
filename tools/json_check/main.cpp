// json_check — the host formatter of the JSON response (json_format.cpp: kaamer_json_escape, kaamer_json_protein_value,
// kaamer_format_json_header / _trailer, kaamer_format_json_arrays) under AddressSanitizer + UBSan, as a stand-alone program.
// The escaper is held against a decoder written the other way round (it computes the code point and tests its value, where
// the library tests byte ranges) over every byte, every pair with a lead byte, crafted sequences and 100 000 random byte
// strings, into exact and short buffers.  The objects of a hand-built result are formatted into exact and short buffers, with
// and without bitmaps, and checked for their framing.  CPU only.    make -C tools/json_check test
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kaamer_amd/csrc/kaamer_internal.h"

// the two symbols the host sources take from search.hip
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
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
            g_failed++;                                         \
        }                                                       \
    } while (0)

// encoding/json's string escaping, by code point
static std::string ref_escape(const std::string &s)
{
    std::string o;
    char tmp[8];
    for (size_t i = 0; i < s.size();) {
        const unsigned b = (unsigned char)s[i];
        if (b < 0x80) {
            if (b == '"' || b == '\\') { o += '\\'; o += (char)b; }
            else if (b == '\n') o += "\\n";
            else if (b == '\r') o += "\\r";
            else if (b == '\t') o += "\\t";
            else if (b < 0x20 || b == '<' || b == '>' || b == '&') { snprintf(tmp, sizeof tmp, "\\u%04x", b); o += tmp; }
            else o += (char)b;
            i++;
            continue;
        }
        const int size = b >= 0xF0 ? 4 : b >= 0xE0 ? 3 : b >= 0xC0 ? 2 : 0;
        bool ok = size && i + (size_t)size <= s.size() && b < 0xF8;
        unsigned long cp = ok ? b & (0xFFu >> (size + 1)) : 0;
        for (int k = 1; ok && k < size; k++) {
            const unsigned c = (unsigned char)s[i + (size_t)k];
            ok = (c & 0xC0u) == 0x80u;
            cp = (cp << 6) | (c & 0x3Fu);
        }
        static const unsigned long least[5] = { 0, 0, 0x80, 0x800, 0x10000 };
        ok = ok && cp >= least[size] && cp <= 0x10FFFF && !(cp >= 0xD800 && cp <= 0xDFFF);
        if (!ok) { o += "\\ufffd"; i++; continue; }
        if (cp == 0x2028 || cp == 0x2029) { snprintf(tmp, sizeof tmp, "\\u%04lx", cp); o += tmp; }
        else o.append(s, i, (size_t)size);
        i += (size_t)size;
    }
    return o;
}

static uint64_t g_strings = 0;
static void check_escape(const std::string &s)
{
    const std::string want = ref_escape(s);
    // (a copy of exactly s.size() bytes: a read beyond the string is the sanitizer's to see)
    std::vector<uint8_t> in(s.begin(), s.end());
    const uint64_t need = kaamer_json_escape(in.data(), in.size(), nullptr, 0);
    CHECK(need == want.size(), "escape of %zu bytes needs %llu, expected %zu", s.size(), (unsigned long long)need, want.size());
    for (uint64_t cap : { (uint64_t)1, need / 2 + 1, need, need + 1 }) {
        if (!cap) continue;   // (the empty string: covered by need + 1)
        std::vector<char> buf((size_t)cap);
        const uint64_t got = kaamer_json_escape(in.data(), in.size(), buf.data(), cap);
        const size_t n = (size_t)(cap - 1 < need ? cap - 1 : need);
        CHECK(got == need && std::string(buf.data(), n) == want.substr(0, n) && buf[n] == '\0', "escape into %llu bytes", (unsigned long long)cap);
    }
    g_strings++;
}

static void strings()
{
    for (int b = 0; b < 256; b++) check_escape(std::string(1, (char)b));
    for (int a = 0xC0; a < 256; a++)
        for (int b = 0; b < 256; b++) check_escape(std::string(1, (char)a) + (char)b);
    const char *crafted[] = { "\xc3\xa9", "\xe2\x82\xac", "\xf0\x9f\x98\x80", "\xf4\x8f\xbf\xbf", "\xe2\x80\xa8", "\xe2\x80\xa9", "\xc0\x80", "\xe0\x80\x80",
                              "\xe0\x9f\xbf", "\xed\xa0\x80", "\xed\x9f\xbf", "\xf0\x8f\xbf\xbf", "\xf4\x90\x80\x80", "\xf8\x88\x80\x80\x80", "\xe2", "\xe2\x82",
                              "\xe2z", "\xe2\x82z", "\xf0\x9f\x98", "\xf0\x9f\x98z", "\xef\xbf\xbd", "" };
    for (const char *c : crafted) {
        check_escape(c);
        check_escape(std::string("x") + c + "y");
    }
    uint64_t x = 20261020;
    for (int i = 0; i < 100000; i++) {
        std::string s;
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const int len = (int)((x >> 33) % 24);
        for (int k = 0; k < len; k++) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const unsigned r = (unsigned)(x >> 40);
            // lead and continuation bytes are drawn often, so that valid and nearly valid sequences occur
            const unsigned kind = r & 7u;
            s += (char)(kind < 2 ? 0x80 + ((r >> 3) & 0x3F) : kind < 4 ? 0xC0 + ((r >> 3) & 0x3F) : kind == 4 ? (r >> 3) & 0x7F : (r >> 3) & 0xFF);
        }
        check_escape(s);
    }
}

static void objects()
{
    const std::string db = "EntryID\tSequence\tOrganism\tEC\nA1\tMKTAYIAKQR\tE. coli\t1.1.1.1\nB\"2\tACDEFGHIKLMN\t\tnone\nC3\tMKTAYIAKQRACD\t<yeast>\t\n";
    kaamer_proteins *table = nullptr;
    CHECK(kaamer_makedb_tsv(db.data(), db.size(), &table) == KAAMER_OK, "makedb: %s", g_err);
    if (!table) return;
    const std::string names = "@read/1 first\n@tab\tname \"here\"\n@\xe2\x82\n";
    const kaamer_text_span spans[3] = { { 1, 12, 0, 0 }, { 15, 15, 0, 0 }, { 32, 2, 0, 0 } };
    const std::string seqs = "MKTAYIAKQRACDEFGHIKLMN<&>";
    const uint64_t offsets[4] = { 0, 10, 22, 25 };
    const uint32_t hits[3][3] = { { 0, 2, 0 }, { 1, 1000, 2 }, { 2, 0, 0 } };
    const uint32_t n_hits[3] = { 2, 3, 1 };
    const int32_t bits_len[3] = { 10, 0, 200 }, trims[3] = { 3, 0, 70 };
    const std::string orf = "MKTAYIA##ACDEFGHIKLMNPQ#" + std::string(130, 'W');
    std::vector<kaamer_query_meta> q(3);
    memset(q.data(), 0, sizeof(kaamer_query_meta) * 3);
    std::vector<uint64_t> top_off(4, 0), pos_off, pos_bits;
    std::vector<uint32_t> pid, km;
    const uint64_t aa_off[3] = { 0, 9, 24 };
    const uint32_t aa_len[3] = { 7, 14, 130 };
    for (uint32_t i = 0; i < 3; i++) {
        q[i].src_seq = i == 2 ? 7 : i;   // (a record beyond the names and the sequences)
        q[i].size_in_kmer = (int32_t)aa_len[i] - 6; q[i].start_position = i == 1 ? -7 : 4; q[i].end_position = 2147483647; q[i].plus_strand = (int32_t)(i & 1);
        q[i].aa_off = aa_off[i]; q[i].aa_len = aa_len[i];
        for (uint32_t r = 0; r < n_hits[i]; r++) {
            pid.push_back(hits[i][r]);
            km.push_back(100 - r);
            pos_off.push_back(pos_bits.size());
            for (int w = 0; w < (bits_len[i] + 63) / 64; w++) pos_bits.push_back(w == 1 ? 0x8000000000000337ull : 0xF0F0F0F0F0F0F0F1ull);
        }
        top_off[i + 1] = pid.size();
    }
    pos_off.push_back(pos_bits.size());
    kaamer_batch_top top;
    memset(&top, 0, sizeof top);
    top.n_queries = 5; top.n_reported = 3; top.max_results = 3;
    top.q = q.data(); top.top_off = top_off.data(); top.top_pid = pid.data(); top.top_kmatch = km.data(); top.trim = trims;
    std::vector<uint8_t> orf_bytes(orf.begin(), orf.end());   // exactly: the last window ends at the buffer's end
    top.orf_aa = orf_bytes.data();
    CHECK(orf_bytes.size() == aa_off[2] + aa_len[2], "the ORF buffer is %zu bytes", orf_bytes.size());
    for (int protein = 0; protein < 2; protein++)
        for (int positions = 0; positions < 2; positions++)
            for (int fmt = 0; fmt < 2; fmt++) {
                const int32_t seq_type = protein ? KAAMER_PROTEIN : (KAAMER_READS | (4 << 8));
                const bool bitmaps = !protein || positions;
                auto call = [&](char *buf, uint64_t cap, uint64_t *off) {
                    return kaamer_format_json_arrays(&top, nullptr, bitmaps ? bits_len : nullptr, bitmaps ? pos_off.data() : nullptr,
                                                     bitmaps ? pos_bits.data() : nullptr, protein ? reinterpret_cast<const uint8_t *>(seqs.data()) : nullptr,
                                                     protein ? offsets : nullptr, protein ? 3 : 0, names.data(), names.size(), spans, 3, table, seq_type, fmt, positions,
                                                     buf, cap, off);
                };
                std::vector<uint64_t> off(4, 99);
                const int64_t need = call(nullptr, 0, off.data());
                CHECK(need > 0 && off[0] == 0 && off[3] == (uint64_t)need, "needed %lld (%s)", (long long)need, g_err);
                if (need <= 0) continue;
                std::vector<char> whole((size_t)need + 1);
                CHECK(call(whole.data(), (uint64_t)need + 1, nullptr) == need && whole[(size_t)need] == '\0', "the whole body");
                for (int i = 0; i < 3; i++) {
                    CHECK(whole[(size_t)off[(size_t)i]] == '{' && whole[(size_t)off[(size_t)i + 1] - (i < 2 ? 2 : 1)] == '}', "object %d is not framed", i);
                    if (i) CHECK(whole[(size_t)off[(size_t)i] - 1] == ',', "no comma before object %d", i);
                }
                const std::string body(whole.data(), (size_t)need);
                CHECK((body.find("\"PositionHits\":{}") != std::string::npos) == !bitmaps, "PositionHits");
                CHECK(body.find(protein ? "\"Type\":\"Protein Query\"" : "\"Type\":\"DNA Query\"") != std::string::npos, "Type");
                CHECK(body.find("\"B\\\"2\"") != std::string::npos && body.find("\\u003cyeast\\u003e") != std::string::npos, "entries");
                for (uint64_t cap : { (uint64_t)1, (uint64_t)17, (uint64_t)need / 2, (uint64_t)need }) {
                    std::vector<char> buf((size_t)cap);
                    const int64_t got = call(buf.data(), cap, nullptr);
                    const size_t n = (size_t)(cap - 1);
                    CHECK(got == need && std::string(buf.data(), n) == body.substr(0, n) && buf[n] == '\0', "objects into %llu bytes", (unsigned long long)cap);
                }
            }
    // refusals: a result with alignments; bitmaps required and absent; no result
    kaamer_alignment a;
    memset(&a, 0, sizeof a);
    CHECK(kaamer_format_json_arrays(&top, &a, nullptr, nullptr, nullptr, nullptr, nullptr, 0, names.data(), names.size(), spans, 3, table, KAAMER_PROTEIN, 0, 0, nullptr, 0,
                                    nullptr) == KAAMER_E_ARG, "alignments");
    CHECK(kaamer_format_json_arrays(&top, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, names.data(), names.size(), spans, 3, table, KAAMER_READS, 1, 0, nullptr,
                                    0, nullptr) == KAAMER_E_ARG, "no bitmaps");
    top.n_reported = 0;
    uint64_t one = 99;
    CHECK(kaamer_format_json_arrays(&top, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, KAAMER_PROTEIN, 0, 0, nullptr, 0, &one) == 0 &&
          one == 0, "nothing reported");
    // the entries on their own, hand-built: every field empty; features without names
    kaamer_protein_entry e;
    memset(&e, 0, sizeof e);
    char buf[64];
    CHECK(kaamer_json_protein_value(&e, nullptr, buf, sizeof buf) == 2 && !strcmp(buf, "{}"), "the empty entry: %s", buf);
    const uint64_t foff[3] = { 0, 0, 1 };
    const char *fnames[2] = { "b", "a" };
    e.n_features = 2; e.features = "x"; e.feature_off = foff; e.length = 7;
    CHECK(kaamer_json_protein_value(&e, fnames, buf, sizeof buf) == strlen(buf) && !strcmp(buf, "{\"Length\":7,\"Features\":{\"a\":\"x\",\"b\":\"\"}}"), "features: %s", buf);
    char hdr[128];
    CHECK(kaamer_format_json_header(1, table, hdr, sizeof hdr) == strlen(hdr) && !strcmp(hdr, "{\"dbProteinFeatures\":[\"Organism\",\"EC\"],\"results\":["), "header: %s", hdr);
    CHECK(kaamer_format_json_header(0, table, hdr, sizeof hdr) == strlen(hdr) && !strcmp(hdr, "{\"dbProteinFeatures\":[],\"results\":["), "header: %s", hdr);
    CHECK(kaamer_format_json_trailer(hdr, 2) == 2 && !strcmp(hdr, "]"), "trailer into 2 bytes");
    kaamer_proteins_free(table);
}

int main()
{
    strings();
    objects();
    if (g_failed) {
        fprintf(stderr, "%d checks FAILED\n", g_failed);
        return 1;
    }
    printf("json_check: %llu strings agree with the code-point decoder; the objects of 8 requests fit their buffers\n", (unsigned long long)g_strings);
    return 0;
}
