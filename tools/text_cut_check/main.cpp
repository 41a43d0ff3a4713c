// text_cut_check — the host half of the device FASTQ and FASTA readers under AddressSanitizer + UBSan, as a stand-alone
// program: kaamer_text_cut_fastq / kaamer_text_cut_fasta and the chunk reader of kaamer_search_text_file /
// kaamer_search_fasta_file (byte source -> chunks cut before an '@' / a '>' that opens a line) over hand cases and random
// texts, plain and gzip; every chunk is parsed with the host reader (FASTA: every chunk but the last with its last record
// upper-cased, as upper_last = 1 does on the device) and the concatenation must equal the host parse of the whole text.
// The FASTA cut is also held against a straight restatement of its rule.  kaamer_text_cut_embl (the cut of the device EMBL
// reader's pieces) goes the same way: hand cases and random texts against a restatement, and the host tables of the two pieces
// a cut leaves (kaamer_makedb_embl, ids moved on by the terminators in front) against the whole text's.  CPU only.
//   make -C tools/text_cut_check test
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>
#include <zlib.h>

#include "../../kaamer_amd/csrc/kaamer_internal.h"

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
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
            g_failed++;                                         \
        }                                                       \
    } while (0)

struct Records {
    std::vector<std::string> seq, name;
    std::vector<int32_t> size;
    bool operator==(const Records &o) const { return seq == o.seq && name == o.name && size == o.size; }
};

static void parse_into(const std::string &text, Records *out, bool fasta = false, bool upper_last = false)
{
    kaamer_reads *r = nullptr;
    const int rc = fasta ? kaamer_parse_fasta(text.data(), text.size(), &r) : kaamer_parse_fastq(text.data(), text.size(), &r);
    CHECK(rc == KAAMER_OK, "parse: %d", rc);
    if (rc) return;
    const uint32_t n = kaamer_reads_count(r);
    const uint64_t *off = kaamer_reads_offsets(r), *noff = kaamer_reads_name_offsets(r);
    const char *seqs = (const char *)kaamer_reads_seqs(r), *names = kaamer_reads_names(r);
    for (uint32_t i = 0; i < n; i++) {
        out->seq.emplace_back(seqs + off[i], seqs + off[i + 1]);
        out->name.emplace_back(names + noff[i], names + noff[i + 1]);
        out->size.push_back(kaamer_reads_size_in_kmer(r)[i]);
        // (PlusStrand is 1 on the first record of what was parsed: per FILE it is host bookkeeping, not compared here)
    }
    if (upper_last && n)
        for (char &c : out->seq.back())
            if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    kaamer_reads_free(r);
}

// ---- kaamer_text_cut_fasta, restated straight from its rule (quadratic: small texts only)
static bool fa_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }
// [p, len) holds a line, complete or not, that does not start with '>' and holds a non-space byte
static bool fa_has_s_line(const std::string &t, size_t p)
{
    while (p < t.size()) {
        size_t e = t.find('\n', p);
        if (e == std::string::npos) e = t.size();
        if (t[p] != '>')
            for (size_t q = p; q < e; q++)
                if (!fa_space(t[q])) return true;
        p = e + 1;
    }
    return false;
}
static bool fa_valid_cut(const std::string &t, size_t p) { return p >= 1 && p < t.size() && t[p - 1] == '\n' && t[p] == '>' && fa_has_s_line(t, p); }
static uint64_t fa_ref_cut(const std::string &t)
{
    for (size_t p = t.size(); p-- > 1;)
        if (fa_valid_cut(t, p)) return p;
    return 0;
}
// the chunk reader restated: a window of 1 to 4 budgets behind the last cut, cut at the greatest valid place INSIDE the
// window (the S line must lie in it too); a window that reaches beyond the text is the rest of the text.  false: some window
// of four budgets holds no cut (KAAMER_E_CAPACITY by design)
static bool fa_ref_chunks(const std::string &t, size_t budget, std::vector<size_t> *lens)
{
    for (size_t a = 0; a < t.size();) {
        size_t take = 0;
        for (size_t w = budget; !take; w += budget) {
            if (a + w > t.size()) { take = t.size() - a; break; }
            take = (size_t)fa_ref_cut(t.substr(a, w));
            if (!take && w >= 4 * budget) return false;
        }
        lens->push_back(take);
        a += take;
    }
    return true;
}

// ---- kaamer_text_cut_embl, restated: the end of the last line that is exactly "//" once one trailing '\r' is dropped
static uint64_t embl_ref_cut(const std::string &t, uint64_t *n_terms = nullptr)
{
    uint64_t best = 0, n = 0;
    for (size_t at = 0; at < t.size();) {
        const size_t nl = t.find('\n', at);
        const size_t end = nl == std::string::npos ? t.size() : nl, next = nl == std::string::npos ? t.size() : nl + 1;
        size_t e = end;
        if (e > at && t[e - 1] == '\r') e--;
        if (e - at == 2 && t[at] == '/' && t[at + 1] == '/') { best = next; n++; }
        at = next;
    }
    if (n_terms) *n_terms = n;
    return best;
}
// every record of the host's table of an EMBL text: id + id_shift, EntryId, what is indexed, the stored Sequence, the cells
static void embl_dump(const std::string &text, uint64_t id_shift, std::vector<std::string> *out, kaamer_proteins **keep)
{
    kaamer_proteins *p = nullptr;
    const int rc = kaamer_makedb_embl(text.data(), text.size(), &p);
    CHECK(rc == KAAMER_OK, "makedb_embl: %d", rc);
    if (rc) return;
    const uint32_t n = kaamer_proteins_count(p);
    const uint32_t *ids = kaamer_proteins_ids(p);
    const uint64_t *off = kaamer_proteins_offsets(p);
    std::vector<kaamer_protein_entry> ent(n ? n : 1);
    CHECK(kaamer_fetch_hits(p, ids, n, ent.data()) == KAAMER_OK, "fetch_hits");
    for (uint32_t i = 0; i < n; i++) {
        const kaamer_protein_entry &e = ent[i];
        std::string r = std::to_string((uint32_t)(ids[i] + id_shift)) + "|" + std::string(e.entry_id, e.entry_id_len) + "|" +
                        std::to_string(off[i + 1] - off[i]) + "|" + std::string((const char *)e.sequence, e.sequence_len);
        for (uint32_t j = 0; j < e.n_features; j++) r += "|" + std::string(e.features + e.feature_off[j], e.features + e.feature_off[j + 1]);
        out->push_back(r);
    }
    if (keep) *keep = p; else kaamer_proteins_free(p);
}

static std::string gzip_members(const std::string &text, size_t split)
{
    std::string out;
    const std::string parts[2] = { text.substr(0, split), text.substr(split) };
    for (const std::string &p : parts) {
        z_stream z;
        memset(&z, 0, sizeof z);
        if (deflateInit2(&z, 1, Z_DEFLATED, 16 + MAX_WBITS, 8, Z_DEFAULT_STRATEGY) != Z_OK) abort();
        std::vector<unsigned char> buf(deflateBound(&z, p.size()) + 64);
        z.next_in = (Bytef *)p.data(); z.avail_in = (uInt)p.size();
        z.next_out = buf.data(); z.avail_out = (uInt)buf.size();
        if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
        out.append((const char *)buf.data(), buf.size() - z.avail_out);
        deflateEnd(&z);
    }
    return out;
}

// the file's bytes through the byte source and the chunk reader; expect_rc: what the reader must end with
static void through_chunker(const std::string &file_bytes, const std::string &text, size_t budget, int expect_rc, const char *what,
                            bool fasta = false, const std::vector<size_t> *want_lens = nullptr)
{
    std::vector<size_t> lens;
    FILE *f = tmpfile();
    if (!f) { perror("tmpfile"); exit(2); }
    if (!file_bytes.empty() && fwrite(file_bytes.data(), 1, file_bytes.size(), f) != file_bytes.size()) { perror("fwrite"); exit(2); }
    fflush(f);
    rewind(f);
    kaamer_bytes *src = nullptr;
    int rc = kaamer_bytes_open_fd(fileno(f), &src);
    CHECK(rc == KAAMER_OK, "%s: bytes_open_fd %d", what, rc);
    kaamer_text_chunker *ck = kaamer_text_chunker_new(src, budget, fasta);
    Records got, whole;
    std::string joined;
    std::vector<char> spare;
    size_t n_chunks = 0;
    while (!rc && !kaamer_text_chunker_done(ck)) {
        size_t len = 0;
        rc = kaamer_text_chunker_next(ck, &spare, &len);
        if (rc || !len) continue;
        n_chunks++;
        lens.push_back(len);
        CHECK(len <= 4 * budget || kaamer_text_chunker_done(ck), "%s: a chunk of %zu bytes with budget %zu", what, len, budget);
        CHECK(joined.empty() || spare[0] == (fasta ? '>' : '@'), "%s: chunk %zu does not start with '%c'", what, n_chunks, fasta ? '>' : '@');
        CHECK(kaamer_text_chunker_done(ck) || spare[len - 1] == '\n', "%s: chunk %zu does not end with a newline", what, n_chunks);
        const std::string piece(spare.data(), len);
        joined += piece;
        // FASTA: a chunk in front of a cut is parsed with upper_last = 1 -- a record follows it
        parse_into(piece, &got, fasta, fasta && !kaamer_text_chunker_done(ck));
    }
    CHECK(rc == expect_rc, "%s: the reader ended with %d (%s), expected %d", what, rc, g_err, expect_rc);
    if (!rc && !expect_rc) {
        CHECK(joined == text, "%s: the chunks do not add up to the text (%zu of %zu bytes)", what, joined.size(), text.size());
        CHECK(!want_lens || lens == *want_lens, "%s: %zu chunks, the restated reader cuts %zu (budget %zu)", what, lens.size(), want_lens->size(), budget);
        parse_into(text, &whole, fasta);
        CHECK(got == whole, "%s: %zu records piecewise, %zu at once (budget %zu, %zu chunks)", what, got.seq.size(), whole.seq.size(), budget, n_chunks);
    }
    kaamer_text_chunker_free(ck);
    kaamer_bytes_close(src);
    fclose(f);
}

// a text may hold a stretch without a cut that four budgets cannot hold (KAAMER_E_CAPACITY by design): such a text goes
// through in one chunk
static size_t budget_that_fits(const std::string &text, size_t budget)
{
    for (size_t at = 1, last_cut = 0; at <= text.size(); at++)
        if (at == text.size() || (text[at] == '@' && text[at - 1] == '\n')) {
            if (at - last_cut > 3 * budget) return text.size() + 1;
            last_cut = at;
        }
    return budget;
}

int main()
{
    // kaamer_text_cut_fastq by hand
    struct { const char *text; uint64_t cut; } hand[] = {
        { "", 0 }, { "@r1 ACGT", 0 }, { "@r1\nACGT\n+\nIIII\n", 0 }, { "@a\nAC\r\n@b\nGT\n", 7 }, { "@a\nAC\n@", 6 },
        { "@a\nAC@GT\n+\nII@I\n", 0 }, { "\n@", 1 }, { "@a\nAC\n+\n@@II\n@b\nGT\n", 13 }, { "@", 0 }, { "\n", 0 },
    };
    for (auto &h : hand) {
        const std::string t(h.text);
        // (an exact-size heap copy: a read past either end is the sanitizer's to find)
        std::vector<char> exact(t.begin(), t.end());
        const uint64_t cut = kaamer_text_cut_fastq(exact.data(), exact.size());
        CHECK(cut == h.cut, "cut of the hand case \"%s\": %llu, expected %llu", h.text, (unsigned long long)cut, (unsigned long long)h.cut);
        for (size_t budget : { (size_t)1, (size_t)3, (size_t)8, (size_t)64 }) through_chunker(t, t, budget_that_fits(t, budget), KAAMER_OK, "hand case");
    }
    CHECK(kaamer_text_cut_fastq(nullptr, 0) == 0, "NULL text");
    // a record that no four budgets hold, and one they do
    const std::string long_read = "@long\n" + std::string(8000, 'A') + "\n+\n" + std::string(8000, 'I') + "\n@next\nACGT\n+\nIIII\n@z\nAC\n";
    through_chunker(long_read, long_read, 1000, KAAMER_E_CAPACITY, "long record, small budget");
    through_chunker(long_read, long_read, 4100, KAAMER_OK, "long record, four budgets");
    // 2 000 random texts over the alphabet of the tests, seed 20261003 (a 64-bit LCG: the texts need not be Python's)
    const char alphabet[] = "@ACNax+\r\n!G";
    const size_t n_alpha = sizeof alphabet - 1;
    uint64_t state = 20261003ull;
    auto rnd = [&](uint64_t n) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (state >> 33) % n; };
    for (int it = 0; it < 2000; it++) {
        const size_t n = (size_t)rnd(400);
        const uint64_t nl_weight = 1 + rnd(4), at_weight = 1 + rnd(2);
        std::string text;
        for (size_t i = 0; i < n; i++) {
            const uint64_t k = rnd(n_alpha + nl_weight + at_weight);
            text += k < n_alpha ? alphabet[k] : (k < n_alpha + nl_weight ? '\n' : '@');
        }
        if (!text.empty() && (uint8_t)text[0] == 0x1F) text[0] = 'A';
        const size_t budgets[] = { 1, 7, 16, 50 };
        const size_t budget = budgets[rnd(4)];
        const size_t use = budget_that_fits(text, budget);
        through_chunker(text, text, use, KAAMER_OK, "random text");
        if (it % 4 == 0) through_chunker(gzip_members(text, text.size() / 2), text, use, KAAMER_OK, "random text, two gzip members");
    }
    // ---- FASTA: the cut by hand, against the restatement, and through the chunk reader
    struct { const char *text; uint64_t cut; } fa_hand[] = {
        { "", 0 }, { ">", 0 }, { "\n", 0 }, { "\n>", 0 }, { "ACGT\nACGT\n", 0 }, { "AC>GT\nA>C\n", 0 }, { ">a\nAC\n>b\n>c\n", 0 },
        { ">a\nAC\n>b\n>c\nG\n", 9 }, { ">a\nAC\n>b\n \t\n\r\n\n", 0 }, { ">a\nAC\n>b\nGG\n>c", 6 }, { ">a\nAC\n>b\nG", 6 },
        { ">a\nAC\n>b\n  ", 0 }, { ">a\r\nAC\r\n>b\r\nGG\r\n", 8 }, { "\n>a\nAC\n", 1 }, { ">a\nAC\n>b\n >x\n", 6 }, { ">a\nacgt\n>b\n", 0 },
    };
    for (auto &h : fa_hand) {
        const std::string t(h.text);
        std::vector<char> exact(t.begin(), t.end());
        const uint64_t cut = kaamer_text_cut_fasta(exact.data(), exact.size());
        CHECK(cut == h.cut, "FASTA cut of the hand case \"%s\": %llu, expected %llu", h.text, (unsigned long long)cut, (unsigned long long)h.cut);
        CHECK(fa_ref_cut(t) == h.cut, "the restated FASTA cut of the hand case \"%s\"", h.text);
        for (size_t budget : { (size_t)1, (size_t)3, (size_t)8, (size_t)64 }) {
            std::vector<size_t> want;
            const bool fits = fa_ref_chunks(t, budget, &want);
            through_chunker(t, t, budget, fits ? KAAMER_OK : KAAMER_E_CAPACITY, "FASTA hand case", true, &want);
        }
    }
    CHECK(kaamer_text_cut_fasta(nullptr, 0) == 0, "NULL text");
    std::string long_rec = ">long\n";
    for (int i = 0; i < 100; i++) long_rec += std::string(80, "ACgt"[i & 3]) + "\n";
    long_rec += ">next\nacgt\n>z\nac\n";
    through_chunker(long_rec, long_rec, 1000, KAAMER_E_CAPACITY, "long FASTA record, small budget", true);
    through_chunker(long_rec, long_rec, 2100, KAAMER_OK, "long FASTA record, four budgets", true);
    const char fa_alphabet[] = ">>AAcg*  \t\r\n\n\n\v\f";
    const size_t n_fa = sizeof fa_alphabet - 1;
    size_t fa_with_cut = 0, fa_fit = 0;
    for (int it = 0; it < 2000; it++) {
        const size_t n = (size_t)rnd(300);
        std::string text;
        for (size_t i = 0; i < n; i++) text += fa_alphabet[rnd(n_fa)];
        std::vector<char> exact(text.begin(), text.end());
        const uint64_t cut = kaamer_text_cut_fasta(exact.data(), exact.size()), want = fa_ref_cut(text);
        CHECK(cut == want, "FASTA cut of random text %d: %llu, the rule says %llu", it, (unsigned long long)cut, (unsigned long long)want);
        fa_with_cut += want != 0;
        const size_t budgets[] = { 1, 7, 16, 50 };
        const size_t use = 2 * budgets[rnd(4)] + 14;   // (16 to 114: records of this alphabet are longer than FASTQ's)
        std::vector<size_t> want_lens;
        const bool fits = fa_ref_chunks(text, use, &want_lens);
        fa_fit += fits;
        through_chunker(text, text, use, fits ? KAAMER_OK : KAAMER_E_CAPACITY, "random FASTA text", true, &want_lens);
        if (it % 4 == 0)
            through_chunker(gzip_members(text, text.size() / 2), text, use, fits ? KAAMER_OK : KAAMER_E_CAPACITY, "random FASTA text, two gzip members", true,
                            &want_lens);
    }
    CHECK(fa_fit * 2 >= 2000, "only %zu of 2000 random FASTA texts go through the chunk reader", fa_fit);
    CHECK(fa_with_cut * 4 >= 2000, "only %zu of 2000 random FASTA texts hold a cut", fa_with_cut);
    // ---- EMBL: the cut by hand, against the restatement, and the pieces' tables against the whole text's
    struct { const char *text; uint64_t cut; } em_hand[] = {
        { "", 0 }, { "//", 2 }, { "//\n", 3 }, { "//\r\n", 4 }, { "//\r", 3 }, { "//\nID   x\n", 3 }, { "ID   x\n//", 9 }, { "ID   x\n//\n", 10 },
        { "ID   x\r\n//\r\nID   y\r\n", 12 }, { "// \n", 0 }, { "///\n", 0 }, { " //\n", 0 }, { "//\r\r\n", 0 }, { "ID   x\nSQ\n", 0 }, { "\n", 0 },
        { "\n\n//", 4 }, { "//\n//", 5 }, { "//\n//x", 3 }, { "a//\n//\nb//", 7 }, { "/", 0 }, { "/\n/\n", 0 },
    };
    for (auto &h : em_hand) {
        const std::string t(h.text);
        std::vector<char> exact(t.begin(), t.end());
        const uint64_t cut = kaamer_text_cut_embl(exact.data(), exact.size());
        CHECK(cut == h.cut, "EMBL cut of the hand case \"%s\": %llu, expected %llu", h.text, (unsigned long long)cut, (unsigned long long)h.cut);
        CHECK(embl_ref_cut(t) == h.cut, "the restated EMBL cut of the hand case \"%s\"", h.text);
    }
    CHECK(kaamer_text_cut_embl(nullptr, 0) == 0, "NULL text");
    const char *em_tokens[] = { "//", "//", "\n", "\n", "\r", "\r\n", "/", " ", "x", "ID   P1 x\n", "ID   P2 y\r\n", "SQ   SEQUENCE 8 AA;\n", "SQ   SEQUENCE 12 AA;\n",
                                "     MAFSAEDVLK EYD\n", "     MKTAYIAK\r\n", "DE   RecName: Full=n {e};\n", "DR   GO; GO:1;\n", "OS   Org.\n", "//\n", "//\r\n" };
    const size_t n_em = sizeof em_tokens / sizeof em_tokens[0];
    size_t em_with_cut = 0, em_records = 0, em_second = 0;
    for (int it = 0; it < 3000; it++) {
        std::string text;
        for (size_t i = 0, n = 10 + (size_t)rnd(60); i < n; i++) text += em_tokens[rnd(n_em)];
        const std::string prefix = text.substr(0, (size_t)rnd(text.size() + 1));
        std::vector<char> exact(prefix.begin(), prefix.end());
        uint64_t n_terms = 0;
        const uint64_t cut = kaamer_text_cut_embl(exact.data(), exact.size()), want = embl_ref_cut(prefix, &n_terms);
        CHECK(cut == want, "EMBL cut of random text %d: %llu, the rule says %llu", it, (unsigned long long)cut, (unsigned long long)want);
        em_with_cut += want != 0;
        // (a prefix that ends inside a line: its last "//" is a terminator only if the input ends there, which the whole text denies)
        if (cut == prefix.size() && cut < text.size() && prefix.back() != '\n') continue;
        // the pieces [0, cut) and [cut, len) of the whole text: their tables, the second with its ids moved on, are the whole's
        std::vector<std::string> whole, pieces;
        kaamer_proteins *pw = nullptr, *pp[2] = { nullptr, nullptr }, *merged = nullptr;
        embl_dump(text, 0, &whole, &pw);
        embl_dump(text.substr(0, (size_t)cut), 0, &pieces, &pp[0]);
        const size_t n_first = pieces.size();
        embl_dump(text.substr((size_t)cut), n_terms, &pieces, &pp[1]);
        CHECK(pieces == whole, "random EMBL text %d cut at %llu: %zu records piecewise, %zu at once", it, (unsigned long long)cut, pieces.size(), whole.size());
        em_records += whole.size();
        em_second += cut ? whole.size() - n_first : 0;
        if (pw && pp[0] && pp[1]) {
            CHECK(kaamer_proteins_merge(pp, 2, &merged) == KAAMER_OK, "proteins_merge");
            const uint32_t n = merged ? kaamer_proteins_count(merged) : 0;
            CHECK(merged && n == kaamer_proteins_count(pw), "merged records");
            if (merged && n == kaamer_proteins_count(pw)) {
                const bool same_off = !memcmp(kaamer_proteins_offsets(merged), kaamer_proteins_offsets(pw), ((size_t)n + 1) * 8);
                CHECK(same_off, "merged offsets");
                CHECK(!n || !same_off || !memcmp(kaamer_proteins_seqs(merged), kaamer_proteins_seqs(pw), (size_t)kaamer_proteins_offsets(pw)[n]), "merged sequences");
            }
        }
        for (kaamer_proteins *q : { pw, pp[0], pp[1], merged }) if (q) kaamer_proteins_free(q);
    }
    CHECK(em_with_cut * 2 >= 3000, "only %zu of 3000 random EMBL texts hold a cut", em_with_cut);
    CHECK(em_records >= 300 && em_second >= 50, "the random EMBL texts keep %zu records, %zu of them behind a cut", em_records, em_second);
    // the byte source's gzip rules: a stream that breaks off reads as what inflated before; a bad first header: nothing
    const std::string two = "@a\nACGT\n+\nIIII\n@b\nGGCC\n+\nIIII\n";
    std::string gz = gzip_members(two, 15);
    through_chunker(gz + "trailing bytes that are no gzip header", two, 1 << 20, KAAMER_OK, "gzip with trailing garbage");
    through_chunker(std::string("\x1f\x8b\x08\xff\xff\xff\xff", 7) + " no gzip header", "", 64, KAAMER_OK, "bad first gzip header");
    through_chunker("", "", 64, KAAMER_OK, "empty file");
    if (g_failed) { fprintf(stderr, "%d check(s) failed\n", g_failed); return 1; }
    printf("text_cut_check: ok\n");
    return 0;
}
