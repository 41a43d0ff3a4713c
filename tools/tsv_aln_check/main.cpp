// tsv_aln_check — the host formatter of the -aln TSV rows (tsv_format.cpp: kaamer_format_tsv_aln_header,
// kaamer_format_tsv_aln_arrays, kaamer_format_double over fmt_double.h) under AddressSanitizer + UBSan, as a stand-alone
// program.  The two number formats are held against the C library's "%e" / "%.2f" (correctly rounded on the double's exact
// value, as strconv is) over the vectors the device test uses: zeros, the smallest subnormal and the largest double, every
// power of two, the doubles around every power of ten, carries into the exponent, exact ties, the specials and random bit
// patterns.  The rows are held against a restatement of search.go:556-604 that prints its numbers with the C library, into
// exact and short buffers.  CPU only.    make -C tools/tsv_aln_check test
#include <cmath>
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

static double from_bits(uint64_t b)
{
    double v;
    memcpy(&v, &b, 8);
    return v;
}

static uint64_t to_bits(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

// fmt.Sprintf(mode 0: "%e", else "%.2f") by way of the C library
static std::string go_format(double v, int mode)
{
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "+Inf" : "-Inf";
    char tmp[400];
    snprintf(tmp, sizeof tmp, mode == 0 ? "%e" : "%.2f", v);
    return tmp;
}

static std::string lib_format(double v, int mode)
{
    const uint64_t need = kaamer_format_double(v, mode, nullptr, 0);
    std::vector<char> buf((size_t)need + 1);   // exactly: one byte more would hide an overrun from the sanitizer
    const uint64_t got = kaamer_format_double(v, mode, buf.data(), need + 1);
    CHECK(got == need && buf[(size_t)need] == '\0', "kaamer_format_double lengths");
    return std::string(buf.data(), (size_t)need);
}

static uint64_t g_values = 0;
static void check_value(double v)
{
    for (int mode = 0; mode < 2; mode++) {
        const std::string want = go_format(v, mode), got = lib_format(v, mode);
        CHECK(want == got, "mode %d of %a (%016llx): %s, expected %s", mode, v, (unsigned long long)to_bits(v), got.c_str(), want.c_str());
    }
    g_values++;
}

static void check_around(double v)
{
    check_value(std::nextafter(v, -INFINITY));
    check_value(v);
    check_value(std::nextafter(v, INFINITY));
    check_value(-v);
}

static void numbers()
{
    check_value(0.0);
    check_value(-0.0);
    check_value(from_bits(1));
    check_value(from_bits(0x7FEFFFFFFFFFFFFFull));
    check_value(from_bits(0xFFEFFFFFFFFFFFFFull));
    for (int k = -1074; k <= 1023; k++) check_around(std::ldexp(1.0, k));
    for (int k = -300; k <= 300; k++) {
        char tmp[16];
        snprintf(tmp, sizeof tmp, "1e%d", k);
        check_around(strtod(tmp, nullptr));
    }
    for (double v : { 999999.95, 9.9999995e5, 1000000.5, 1000001.5, 0.125, 0.375, 2.5e-3, -0.125, 0.005, 0.015, 0.995, 1.005, 99.995, 1e7, 9999999.5,
                      4503599627370496.0, 18446744073709551616.0, 1e17, 1e18, 1e19, 1e20, 123456789012345678.0 })
        check_around(v);
    check_value(INFINITY);
    check_value(-INFINITY);
    check_value(NAN);
    uint64_t x = 20261003;
    for (int i = 0; i < 200000; i++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        uint64_t b = x ^ (x >> 29);
        check_value(from_bits(b));
        // ... and bit patterns with short mantissas: exact ties are among them
        check_value(from_bits(b & 0xFFFFFF0000000000ull));
    }
}

struct Hit {
    uint32_t pid;
    kaamer_alignment a;
};

static kaamer_alignment aln(float identity, int len, int mm, int go, double bits, double ev, int qs, int qe, int ss, int se, int status = 0)
{
    kaamer_alignment a;
    memset(&a, 0, sizeof a);
    a.identity = identity; a.length = len; a.mismatches = mm; a.gap_openings = go; a.bitscore = bits; a.evalue = ev;
    a.query_start = qs; a.query_end = qe; a.subject_start = ss; a.subject_end = se; a.status = status;
    return a;
}

static void rows()
{
    const std::string db = "EntryID\tSequence\tOrganism\tEC\nA1\tMKTAYIAKQR\tE. coli\t1.1.1.1\nB2\tACDEFGHIKLMN\t\tnone\nC3\tMKTAYIAKQRACD\tyeast\t\n";
    kaamer_proteins *table = nullptr;
    CHECK(kaamer_makedb_tsv(db.data(), db.size(), &table) == KAAMER_OK, "makedb: %s", g_err);
    if (!table) return;
    const char *eid[3] = { "A1", "B2", "C3" };
    const char *feat[3][2] = { { "E. coli", "1.1.1.1" }, { "", "none" }, { "yeast", "" } };
    const std::string names = "@read/1 first\n@tab\tname here\n@\n";
    const kaamer_text_span spans[3] = { { 1, 12, 0, 0 }, { 15, 13, 0, 0 }, { 30, 0, 0, 0 } };
    // three reported queries; a missing id in the middle of the second; an empty AlignmentResult; n_ops == 0 (NaN)
    std::vector<std::vector<Hit>> hits = {
        { { 0, aln(87.5f, 8, 1, 0, 21.17, 4.3e-5, 1, 8, 3, 10) }, { 2, aln(33.333332f, 30, 18, 2, 4.61, 5712.0, 2, 29, 1, 13) } },
        { { 1, aln(100.0f, 12, 0, 0, 1234567.895, 0.0, 1, 12, 1, 12) }, { 1000, aln(0.0f, 0, 0, 0, 0.0, 0.0, 0, 0, 0, 0, 4) }, { 2, aln(0.0f, 0, 0, 0, 0.0, 0.0, 0, 0, 0, 0, 4) } },
        { { 2, aln(NAN, 0, 0, 0, 4.6073, 9.999995e-310, 1, 0, 1, 0) }, { 0, aln(12.125f, 2147483647, 2147483647, 7, -0.125, 1.5e300, 2147483647, 5, 6, 7) } },
    };
    const int32_t starts[3] = { 4, -7, 0 }, ends[3] = { 33, 2147483647, 9 };
    const int32_t bits_len[3] = { 10, 0, 70 };
    std::vector<kaamer_query_meta> q(3);
    std::vector<uint64_t> top_off(4, 0), pos_off, pos_bits;
    std::vector<uint32_t> pid;
    std::vector<kaamer_alignment> alns;
    memset(q.data(), 0, sizeof(kaamer_query_meta) * 3);
    for (uint32_t i = 0; i < 3; i++) {
        q[i].src_seq = i == 2 ? 7 : i;   // (a record beyond the names: an empty QueryId)
        q[i].start_position = starts[i]; q[i].end_position = ends[i];
        for (const Hit &h : hits[i]) {
            pid.push_back(h.pid);
            alns.push_back(h.a);
            pos_off.push_back(pos_bits.size());
            for (int w = 0; w < (bits_len[i] + 63) / 64; w++) pos_bits.push_back(w == 0 ? 0x8000000000000337ull : 0x21ull);
        }
        top_off[i + 1] = pid.size();
    }
    pos_bits.push_back(0);
    kaamer_batch_top top;
    memset(&top, 0, sizeof top);
    top.n_queries = 5; top.n_reported = 3; top.max_results = 3;
    top.q = q.data(); top.top_off = top_off.data(); top.top_pid = pid.data();
    for (int protein = 0; protein < 2; protein++)
        for (int positions = 0; positions < 2; positions++)
            for (int annotations = 0; annotations < 2; annotations++) {
                std::string want;
                std::vector<uint64_t> want_off;
                for (uint32_t i = 0; i < 3; i++) {
                    const std::string id = i == 0 ? "read/1" : i == 1 ? "tab\tname" : "";
                    bool gone = false;
                    for (uint64_t e = top_off[i]; e < top_off[i + 1]; e++) {
                        want_off.push_back(want.size());
                        const kaamer_alignment &a = alns[(size_t)e];
                        gone = gone || pid[(size_t)e] > 2;
                        want += id + "\t" + (gone ? "" : eid[pid[(size_t)e]]) + "\t" + go_format((double)a.identity, 1) + "\t" + std::to_string(a.length) + "\t" +
                                std::to_string(a.mismatches) + "\t" + std::to_string(a.gap_openings) + "\t" +
                                std::to_string(protein ? a.query_start : starts[i]) + "\t" + std::to_string(protein ? a.query_end : ends[i]) + "\t" +
                                std::to_string(a.subject_start) + "\t" + std::to_string(a.subject_end) + "\t" + go_format(a.evalue, 0) + "\t" +
                                go_format(a.bitscore, 1);
                        if (positions) {
                            char tmp[512];
                            const uint64_t n = kaamer_format_positions(pos_bits.data() + pos_off[(size_t)e], bits_len[i], 1, tmp, sizeof tmp);
                            want += "\t" + std::string(tmp, (size_t)n);
                        }
                        if (annotations)
                            for (int f = 0; f < 2; f++) want += std::string("\t") + (gone ? "" : feat[pid[(size_t)e]][f]);
                        want += "\n";
                    }
                }
                want_off.push_back(want.size());
                const int32_t seq_type = protein ? KAAMER_PROTEIN : (KAAMER_READS | (4 << 8));
                std::vector<uint64_t> off(pid.size() + 1, 99);
                const int64_t need = kaamer_format_tsv_aln_arrays(&top, alns.data(), bits_len, pos_off.data(), pos_bits.data(), names.data(), names.size(), spans,
                                                                  2, table, seq_type, positions, annotations, nullptr, 0, off.data());
                CHECK(need == (int64_t)want.size(), "needed %lld, expected %zu", (long long)need, want.size());
                CHECK(off == want_off, "line offsets");
                if (need < 0) continue;
                for (uint64_t cap : { (uint64_t)1, (uint64_t)17, (uint64_t)need, (uint64_t)need + 1 }) {
                    std::vector<char> buf((size_t)cap);
                    const int64_t got = kaamer_format_tsv_aln_arrays(&top, alns.data(), bits_len, pos_off.data(), pos_bits.data(), names.data(), names.size(),
                                                                     spans, 2, table, seq_type, positions, annotations, buf.data(), cap, nullptr);
                    const size_t n = (size_t)(cap - 1 < (uint64_t)need ? cap - 1 : (uint64_t)need);
                    CHECK(got == need && std::string(buf.data(), n) == want.substr(0, n) && buf[n] == '\0', "rows into %llu bytes:\n%s\nexpected\n%s",
                          (unsigned long long)cap, std::string(buf.data(), n).c_str(), want.c_str());
                }
                char hdr[256];
                const uint64_t hn = kaamer_format_tsv_aln_header(positions, annotations, table, hdr, sizeof hdr);
                std::string hw = "QueryId\tSubjectId\t%Identity\tAlnLength\tMismatches\tGapOpen\tQStart\tQEnd\tSStart\tSEnd\tEvalue\tBitscore";
                if (positions) hw += "\tQueryPositions";
                if (annotations) hw += "\tOrganism\tEC";
                hw += "\n";
                CHECK(std::string(hdr, (size_t)hn) == hw, "header: %s", hdr);
            }
    // a result without alignments; ExtractPositions without bitmaps
    CHECK(kaamer_format_tsv_aln_arrays(&top, nullptr, nullptr, nullptr, nullptr, names.data(), names.size(), spans, 2, table, KAAMER_PROTEIN, 0, 0, nullptr, 0,
                                       nullptr) == KAAMER_E_ARG, "no alignments");
    CHECK(kaamer_format_tsv_aln_arrays(&top, alns.data(), nullptr, nullptr, nullptr, names.data(), names.size(), spans, 2, table, KAAMER_PROTEIN, 1, 0, nullptr, 0,
                                       nullptr) == KAAMER_E_ARG, "no bitmaps");
    kaamer_proteins_free(table);
}

int main()
{
    numbers();
    rows();
    if (g_failed) {
        fprintf(stderr, "%d checks FAILED\n", g_failed);
        return 1;
    }
    printf("tsv_aln_check: %llu doubles in both formats and the rows of 8 option sets agree with the C library\n", (unsigned long long)g_values);
    return 0;
}
