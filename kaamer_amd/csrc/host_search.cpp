// host_search.cpp — host-side pieces of pkg/search kept next to the kernels so that
// non-Go callers get the reference's behaviour bit for bit:
//
//   kaamer_parse_fasta / kaamer_parse_fastq   GetQueriesFasta / GetQueriesFastq
//                                             (search.go:222-412), from a text buffer
//   kaamer_set_best_start_codon               SetBestStartCodon (dna.go:198-272), driven by
//                                             the per-hit lowest matching position
//
// In the Go integration these stay the reference's own Go code.
#include "kaamer_internal.h"
#include "gcodes.h"

#include <zlib.h>

#include <errno.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

struct kaamer_reads {
    std::vector<uint8_t> seqs;
    std::vector<uint64_t> offsets;  // n + 1
    std::vector<int32_t> size_in_kmer;
    std::vector<char> names;
    std::vector<uint64_t> name_off;  // n + 1
    std::vector<int32_t> plus_strand;  // Location.PlusStrand as the reference's reader leaves it
};

namespace {

// bufio.Scanner with ScanLines: split at '\n', drop one trailing '\r'
struct LineReader {
    const char *p, *end;
    bool next(const char *&b, const char *&e)
    {
        if (p >= end) return false;
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        b = p;
        e = nl ? nl : end;
        p = nl ? nl + 1 : end;
        if (e > b && e[-1] == '\r') e--;
        return true;
    }
};

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// GetQueriesFasta / GetQueriesFastq (search.go:222-412) as a state machine over lines, so that a whole buffer and a file
// read in pieces go through ONE statement of the rules:
//   FASTA  blank lines are skipped (:285-287); a '>' line closes the pending record and names the next; sequence lines
//          are TrimSpace'd and concatenated (:309); every record but the LAST of the input is upper-cased (:295 vs
//          :313-320); SizeInKmer = len - 6, minus 1 when the sequence ends in '*' (:290-293)
//   FASTQ  a line starting with '@' opens a record (also a quality line that happens to start with '@'); a line
//          matching ^[ATGCNatgcn]+$ REPLACES the record's sequence; no case change; SizeInKmer = len - 6 (:395,407)
//   both   the first Query of the input is built with Location{PlusStrand: true}, every following one as
//          Query{Sequence: "", ...} (search.go:297,399): Location is then Go's zero value, PlusStrand false
struct RecordParser {
    bool fastq = false;
    bool first_done = false;
    std::string seq, name;

    void push(kaamer_reads *r, bool upper, bool star_rule)
    {
        int32_t size = (int32_t)seq.size() - KAAMER_KMER_SIZE + 1;          // search.go:290,314,395,407
        if (star_rule && !seq.empty() && seq.back() == '*') size--;         // search.go:291-293,315-317
        const size_t at = r->seqs.size();
        r->seqs.resize(at + seq.size());
        if (!upper) {
            memcpy(r->seqs.data() + at, seq.data(), seq.size());
        } else {
            for (size_t i = 0; i < seq.size(); i++) {
                const char c = seq[i];
                r->seqs[at + i] = (uint8_t)((c >= 'a' && c <= 'z') ? c - 32 : c);  // strings.ToUpper (:295)
            }
        }
        r->offsets.push_back(r->seqs.size());
        r->size_in_kmer.push_back(size);
        r->names.insert(r->names.end(), name.begin(), name.end());
        r->name_off.push_back(r->names.size());
        r->plus_strand.push_back(first_done ? 0 : 1);
        first_done = true;
    }

    void line(kaamer_reads *r, const char *b, const char *e)
    {
        if (e - b < 1) return;
        if (!fastq) {
            if (*b == '>') {
                if (!seq.empty()) { push(r, /*upper=*/true, /*star_rule=*/true); seq.clear(); }
                name.assign(b + 1, e);
            } else {
                while (b < e && is_space(*b)) b++;
                while (e > b && is_space(e[-1])) e--;
                seq.append(b, e);
            }
            return;
        }
        if (*b == '@') {
            if (!seq.empty()) { push(r, false, false); seq.clear(); name.clear(); }
            name.assign(b + 1, e);
        } else {
            static const struct NtTable {   // ^[ATGCNatgcn]+$ (search.go:340,386)
                bool ok[256];
                NtTable() { memset(ok, 0, sizeof ok); for (const char *c = "ATGCNatgcn"; *c; c++) ok[(uint8_t)*c] = true; }
            } nt;
            bool is_seq = true;
            for (const char *c = b; c < e && is_seq; c++) is_seq = nt.ok[(uint8_t)*c];
            if (is_seq) seq.assign(b, e);
        }
    }

    // end of the input: the pending record is the LAST one (FASTA: not upper-cased)
    void finish(kaamer_reads *r)
    {
        if (!seq.empty()) { push(r, false, !fastq); seq.clear(); }
    }
};

kaamer_reads *new_reads()
{
    kaamer_reads *r = new (std::nothrow) kaamer_reads();
    if (r) { r->offsets.push_back(0); r->name_off.push_back(0); }
    return r;
}

// bufio.Scanner with Buffer(buf, 1 MiB) (search.go:273-274, inputFASTA.go:88-89): a line of 1 048 576 bytes or more
// (its '\r' included, its '\n' not) fills the scanner's buffer without a token; Scan() returns false and the reference
// goes on as if the input had ended there
const size_t SCANNER_MAX = 1024u * 1024u;

}  // namespace

bool kaamer_is_gzip(const char *text, uint64_t len)
{
    return len >= 3 && (uint8_t)text[0] == 0x1F && (uint8_t)text[1] == 0x8B && (uint8_t)text[2] == 0x08;
}

int kaamer_gunzip(const char *text, uint64_t len, std::string *out)
{
    out->clear();
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) return kaamer_fail(KAAMER_E_NOMEM, "gzip: inflateInit2");
    z.next_in = (Bytef *)const_cast<char *>(text);
    uint64_t left = len;
    bool first_header_seen = false;
    std::string buf(1u << 20, '\0');
    for (;;) {
        if (z.avail_in == 0 && left) {
            const uInt take = left > (1u << 30) ? (1u << 30) : (uInt)left;
            z.avail_in = take;
            left -= take;
        }
        z.next_out = (Bytef *)&buf[0];
        z.avail_out = (uInt)buf.size();
        const int rc = inflate(&z, Z_NO_FLUSH);
        const size_t got = buf.size() - z.avail_out;
        if (got) { out->append(buf.data(), got); first_header_seen = true; }
        if (rc == Z_STREAM_END) {
            first_header_seen = true;
            if (z.avail_in == 0 && left == 0) break;          // the last member ended with the input
            // another member follows (gzip.Reader multistream); bytes that are not a gzip header end the text here
            const Bytef *next = z.next_in;
            const uInt avail = z.avail_in;
            if (inflateReset(&z) != Z_OK) break;
            z.next_in = const_cast<Bytef *>(next);
            z.avail_in = avail;
            continue;
        }
        if (rc == Z_OK) continue;
        if (rc == Z_BUF_ERROR && z.avail_in == 0 && left == 0) break;   // the stream breaks off: what was read stays
        break;                                                           // damaged data: the same
    }
    inflateEnd(&z);
    if (!first_header_seen && out->empty()) {
        // (an empty member is fine; a first header that is no gzip header is gzip.NewReader's error)
        z_stream t;
        memset(&t, 0, sizeof t);
        bool ok = false;
        if (inflateInit2(&t, 16 + MAX_WBITS) == Z_OK) {
            Bytef sink[64];
            t.next_in = (Bytef *)const_cast<char *>(text);
            t.avail_in = len > 4096 ? 4096u : (uInt)len;
            t.next_out = sink; t.avail_out = sizeof sink;
            const int rc = inflate(&t, Z_NO_FLUSH);
            ok = rc == Z_OK || rc == Z_STREAM_END || rc == Z_BUF_ERROR;
            inflateEnd(&t);
        }
        if (!ok) return kaamer_fail(KAAMER_E_FORMAT, "gzip: invalid header");
    }
    return KAAMER_OK;
}

extern "C" {

static int parse_buffer(const char *text, uint64_t len, bool fastq, kaamer_reads **out)
{
    std::string inflated;   // (search.go:259-263, 361-366: gzipped input)
    if (kaamer_is_gzip(text, len)) {
        const int zrc = kaamer_gunzip(text, len, &inflated);
        // gzip.NewReader fails on a first header that is no gzip header: the reference prints the error and returns
        // without a query (search.go:259-263) -- an empty read set, not an error of the call
        if (zrc == KAAMER_E_FORMAT) inflated.clear();
        else if (zrc) return zrc;
        text = inflated.data(); len = inflated.size();
    }
    kaamer_reads *r = new_reads();
    if (!r) return kaamer_fail(KAAMER_E_NOMEM, "parse");
    RecordParser ps;
    ps.fastq = fastq;
    LineReader lr{ text, text + len };
    const char *b, *e;
    while (lr.next(b, e)) ps.line(r, b, e);
    ps.finish(r);
    *out = r;
    return KAAMER_OK;
}

// GetQueriesFasta, search.go:222-322 (rules: RecordParser above)
int kaamer_parse_fasta(const char *text, uint64_t len, kaamer_reads **out)
{
    if (!out || (!text && len)) return kaamer_fail(KAAMER_E_ARG, "parse_fasta: bad argument");
    return parse_buffer(text, len, false, out);
}

// GetQueriesFastq, search.go:324-412
int kaamer_parse_fastq(const char *text, uint64_t len, kaamer_reads **out)
{
    if (!out || (!text && len)) return kaamer_fail(KAAMER_E_ARG, "parse_fastq: bad argument");
    return parse_buffer(text, len, true, out);
}

// Where a FASTQ text may be cut so that its pieces, parsed one by one, give the records of the whole (the rules per line:
// include/kaamer_hip.h): before an '@' that opens a line.  That line is an H whatever it holds, an H closes the record
// pending before it and names whatever follows, so nothing of the reader's state crosses the cut -- a quality line that
// starts with '@' is an H to the reader too (search.go:380), which is why it is as good a place as a header.
uint64_t kaamer_text_cut_fastq(const char *text, uint64_t len)
{
    if (!text) return 0;
    for (uint64_t p = len; p-- > 1;)
        if (text[p] == '@' && text[p - 1] == '\n') return p;
    return 0;
}

// Where a FASTA text may be cut (the rules: include/kaamer_hip.h): before a '>' that opens a line, provided an S line --
// a line that does not start with '>' and holds a non-space byte, complete or not -- lies behind it.  The H closes the
// record pending before it and names what follows, and the S line behind it guarantees that the piece in front does not
// hold the input's last record: it is parsed with upper_last = 1.  One walk over the lines from the end.
uint64_t kaamer_text_cut_fasta(const char *text, uint64_t len)
{
    if (!text) return 0;
    bool has_s = false;
    uint64_t le = len;   // the end of the line being looked at: the position of its '\n', or len
    if (len && text[len - 1] == '\n') le = len - 1;
    while (len) {
        const char *nl = le ? (const char *)memrchr(text, '\n', (size_t)le) : nullptr;
        const uint64_t ls = nl ? (uint64_t)(nl - text) + 1 : 0;
        if (ls < le && text[ls] == '>') {
            if (has_s && ls) return ls;
        } else if (!has_s) {
            for (uint64_t q = ls; q < le && !has_s; q++) has_s = !is_space(text[q]);
        }
        if (!ls) break;
        le = ls - 1;
    }
    return 0;
}

// Where an EMBL text may be cut (the rules: include/kaamer_hip.h): behind the line end of a line that is exactly "//" once
// its trailing '\r' is dropped.  Such a line closes an entry and takes a number; nothing else of the reader's state crosses
// it.  One walk over the lines from the end.
uint64_t kaamer_text_cut_embl(const char *text, uint64_t len)
{
    if (!text) return 0;
    uint64_t le = len;   // the end of the line being looked at: the position of its '\n', or len
    if (len && text[len - 1] == '\n') le = len - 1;
    while (len) {
        const char *nl = le ? (const char *)memrchr(text, '\n', (size_t)le) : nullptr;
        const uint64_t ls = nl ? (uint64_t)(nl - text) + 1 : 0;
        const uint64_t e = (le > ls && text[le - 1] == '\r') ? le - 1 : le;
        if (e - ls == 2 && text[ls] == '/' && text[ls + 1] == '/') return le < len ? le + 1 : len;
        if (!ls) break;
        le = ls - 1;
    }
    return 0;
}

// The blocks of a BGZF stream, found without inflating (the rules: include/kaamer_hip.h).  A member is
//   1f 8b 08 FLG=4 MTIME(4) XFL OS XLEN(2) | extra field of XLEN bytes: subfields SI1 SI2 SLEN(2) data | deflate | CRC32 ISIZE
// and the subfield 'B' 'C' with SLEN 2 holds BSIZE = the member's size - 1.
int kaamer_bgzf_scan(const uint8_t *bytes, uint64_t len, kaamer_bgzf_block *blocks, uint64_t cap, uint64_t *n_blocks, uint64_t *consumed)
{
    if (!n_blocks || !consumed || (!bytes && len) || (!blocks && cap)) return kaamer_fail(KAAMER_E_ARG, "bgzf_scan: bad argument");
    uint64_t at = 0, n = 0;
    auto u16 = [&](uint64_t p) { return (uint32_t)bytes[p] | (uint32_t)bytes[p + 1] << 8; };
    auto u32 = [&](uint64_t p) { return u16(p) | u16(p + 2) << 16; };
    while (len - at >= 12) {
        if (bytes[at] != 0x1F || bytes[at + 1] != 0x8B || bytes[at + 2] != 0x08 || bytes[at + 3] != 4) break;
        const uint64_t xlen = u16(at + 10), extra = at + 12;
        if (len - extra < xlen) break;
        uint64_t bsize1 = 0;   // BSIZE + 1; 0: no BC subfield
        for (uint64_t f = 0; xlen - f >= 4;) {
            const uint64_t slen = u16(extra + f + 2);
            if (xlen - f - 4 < slen) break;   // a subfield that leaves the extra field
            if (bytes[extra + f] == 'B' && bytes[extra + f + 1] == 'C' && slen == 2) { bsize1 = (uint64_t)u16(extra + f + 4) + 1; break; }
            f += 4 + slen;
        }
        const uint64_t head = 12 + xlen;
        if (!bsize1 || bsize1 < head + 8 || len - at < bsize1) break;
        const uint32_t isize = u32(at + bsize1 - 4);
        if (isize > 65536) break;
        if (n < cap) {
            kaamer_bgzf_block &b = blocks[n];
            b.comp_off = at + head;
            b.comp_len = (uint32_t)(bsize1 - head - 8);
            b.isize = isize;
            b.crc = u32(at + bsize1 - 8);
            b.reserved = 0;
        }
        n++;
        at += bsize1;
    }
    *n_blocks = n;
    *consumed = at;
    return KAAMER_OK;
}

// ---- the same readers over a FILE, in chunks: search.go:240-283 opens the file, sniffs the first 32 bytes, wraps a
// gzip.Reader around it when they carry the gzip signature and scans line by line; a 100 M-read file is never in
// memory as a whole (configs[4]).  kaamer_reader_next hands out up to max_seqs records / about max_bytes of sequence
// as a kaamer_reads (the accessors below), which goes straight into kaamer_stream_push.
// The bytes of a query file as text, one copy for every reader of a file (kaamer_reader_* below, kaamer_search_text_file):
// search.go:240-283 opens the file, sniffs the first 32 bytes and wraps a gzip.Reader around it when they carry the gzip
// signature.  gzip: every member is read (gzip.Reader is multistream); a stream that breaks off or is damaged reads as
// what inflated before (gzip.Reader returns the error and the scanner stops); a first header that is no gzip header
// yields nothing.
struct kaamer_bytes {
    int fd = -1;
    bool gz = false, eof = false;
    z_stream z;
    bool z_live = false;
    std::vector<uint8_t> raw;     // bytes as read from the file (gzip only)
    size_t raw_pos = 0, raw_len = 0;
    uint8_t head[32];             // the sniffed bytes
    size_t n_head = 0, head_pos = 0;
};

static ssize_t fd_read(int fd, void *dst, size_t n)
{
    for (;;) {
        const ssize_t k = read(fd, dst, n);
        if (k < 0 && errno == EINTR) continue;
        return k;
    }
}

}  // extern "C"

int kaamer_bytes_open_fd(int fd, kaamer_bytes **out)
{
    *out = nullptr;
    kaamer_bytes *b = new (std::nothrow) kaamer_bytes();
    if (!b) return kaamer_fail(KAAMER_E_NOMEM, "byte source");
    b->fd = fd;
    // the first 32 bytes decide how the file is read (http.DetectContentType, search.go:246-270)
    while (b->n_head < sizeof b->head) {
        const ssize_t k = fd_read(fd, b->head + b->n_head, sizeof b->head - b->n_head);
        if (k <= 0) break;
        b->n_head += (size_t)k;
    }
    if (b->n_head == 0) b->eof = true;
    if (kaamer_is_gzip((const char *)b->head, b->n_head)) {
        b->gz = true;
        b->raw.resize(1u << 20);
        memcpy(b->raw.data(), b->head, b->n_head);
        b->raw_len = b->n_head;
        memset(&b->z, 0, sizeof b->z);
        if (inflateInit2(&b->z, 16 + MAX_WBITS) != Z_OK) { delete b; return kaamer_fail(KAAMER_E_NOMEM, "gzip: inflateInit2"); }
        b->z_live = true;
    }
    *out = b;
    return KAAMER_OK;
}

const uint8_t *kaamer_bytes_head(const kaamer_bytes *b, size_t *n) { *n = b->n_head; return b->head; }
bool kaamer_bytes_is_gzip(const kaamer_bytes *b) { return b->gz; }
void kaamer_bytes_end(kaamer_bytes *b) { b->eof = true; }

void kaamer_bytes_close(kaamer_bytes *b)
{
    if (!b) return;
    if (b->z_live) inflateEnd(&b->z);
    delete b;
}

// the next block of decoded text into dst[0, cap): its length; 0: the input is over (EOF, a gzip stream that broke off or
// is damaged: what was read before stays)
size_t kaamer_bytes_read(kaamer_bytes *b, char *dst, size_t cap)
{
    if (b->eof || cap == 0) return 0;
    if (!b->gz) {
        if (b->head_pos < b->n_head) {   // the sniffed bytes first
            const size_t k = b->n_head - b->head_pos < cap ? b->n_head - b->head_pos : cap;
            memcpy(dst, b->head + b->head_pos, k);
            b->head_pos += k;
            return k;
        }
        const ssize_t k = fd_read(b->fd, dst, cap);
        if (k <= 0) { b->eof = true; return 0; }
        return (size_t)k;
    }
    if (cap > (1u << 30)) cap = 1u << 30;
    for (;;) {
        if (b->raw_pos == b->raw_len) {
            const ssize_t k = fd_read(b->fd, b->raw.data(), b->raw.size());
            b->raw_pos = 0;
            b->raw_len = k > 0 ? (size_t)k : 0;
        }
        const bool file_over = b->raw_len == 0;
        b->z.next_in = b->raw.data() + b->raw_pos;
        b->z.avail_in = (uInt)(b->raw_len - b->raw_pos);
        b->z.next_out = (Bytef *)dst;
        b->z.avail_out = (uInt)cap;
        const int rc = inflate(&b->z, Z_NO_FLUSH);
        b->raw_pos = b->raw_len - b->z.avail_in;
        const size_t got = cap - b->z.avail_out;
        if (rc == Z_STREAM_END) {
            // another member may follow (gzip.Reader is multistream); bytes that are no gzip header end the text here
            if (b->raw_pos == b->raw_len) {
                const ssize_t k = fd_read(b->fd, b->raw.data(), b->raw.size());
                b->raw_pos = 0;
                b->raw_len = k > 0 ? (size_t)k : 0;
            }
            if (b->raw_len == b->raw_pos || inflateReset(&b->z) != Z_OK) b->eof = true;
            if (got) return got;
            if (b->eof) return 0;
            continue;
        }
        if (rc != Z_OK && !(rc == Z_BUF_ERROR && !file_over && got == 0 && b->z.avail_in == 0)) b->eof = true;  // broke off / damaged
        if (file_over && got == 0) b->eof = true;
        if (got) return got;
        if (b->eof) return 0;
    }
}

// The chunk reader of kaamer_search_text_file: text from a byte source in pieces of about `budget` bytes, each cut at
// the reader's cut rule (kaamer_text_cut_fastq or kaamer_text_cut_fasta), the tail behind the cut carried into the next.
// *chunk comes in as a spare buffer (any size) and goes out holding the chunk in its first *len bytes; *len = 0: the input is over.  A piece without a cut goes on reading
// up to 4 budgets, then KAAMER_E_CAPACITY.
struct TextCutRule {
    uint64_t (*cut)(const char *text, uint64_t len);
    const char *driver, *no_cut;   // "<driver>: <no_cut> within N bytes of text ..."
};
struct kaamer_text_chunker {
    kaamer_bytes *src = nullptr;
    size_t budget = 0;
    std::vector<char> acc;        // text read and not yet handed out: the tail behind the last cut, then what follows
    size_t acc_len = 0;
    bool over = false;            // the byte source is exhausted
    const TextCutRule *rule = nullptr;   // the cut rule of the text's format
};

kaamer_text_chunker *kaamer_text_chunker_new(kaamer_bytes *src, uint64_t budget, bool fasta)
{
    // a format's cut rule, with what the reader says when four budgets hold no cut
    static const TextCutRule rules[2] = {
        { kaamer_text_cut_fastq, "search_text_file", "no line starts with '@'" },
        { kaamer_text_cut_fasta, "search_fasta_file", "no record starts behind a '>' line (kaamer_text_cut_fasta)" },
    };
    kaamer_text_chunker *c = new (std::nothrow) kaamer_text_chunker();
    if (c) { c->src = src; c->budget = (size_t)budget; c->rule = &rules[fasta ? 1 : 0]; }
    return c;
}

void kaamer_text_chunker_free(kaamer_text_chunker *c) { delete c; }
// text that precedes what the byte source will give (a reader that takes over in the middle of a file)
void kaamer_text_chunker_prime(kaamer_text_chunker *c, const char *text, size_t len)
{
    if (c->acc.size() < c->acc_len + len) c->acc.resize(c->acc_len + len);
    if (len) memcpy(c->acc.data() + c->acc_len, text, len);
    c->acc_len += len;
}
bool kaamer_text_chunker_done(const kaamer_text_chunker *c) { return c->over && c->acc_len == 0; }

int kaamer_text_chunker_next(kaamer_text_chunker *c, std::vector<char> *chunk, size_t *len)
{
    *len = 0;
    size_t want = c->budget, cut = 0;
    for (;;) {
        if (c->acc.size() < want) c->acc.resize(want);
        while (!c->over && c->acc_len < want) {
            const size_t got = kaamer_bytes_read(c->src, c->acc.data() + c->acc_len, want - c->acc_len);
            if (!got) c->over = true;
            else c->acc_len += got;
        }
        if (c->acc_len == 0) return KAAMER_OK;
        if (c->over) { cut = c->acc_len; break; }   // the rest of the file
        cut = (size_t)c->rule->cut(c->acc.data(), c->acc_len);
        if (cut) break;
        if (want >= 4 * c->budget)
            return kaamer_fail(KAAMER_E_CAPACITY, "%s: %s within %zu bytes of text (4 chunk_text_bytes): "
                                                  "use kaamer_search_file, whose reader takes records of any length", c->rule->driver, c->rule->no_cut, want);
        want += c->budget;
    }
    // the chunk takes the buffer, the tail moves to the front of the spare one
    const size_t tail = c->acc_len - cut;
    if (chunk->size() < c->budget) chunk->resize(c->budget);
    if (chunk->size() < tail) chunk->resize(tail);
    memcpy(chunk->data(), c->acc.data() + cut, tail);
    chunk->swap(c->acc);
    c->acc_len = tail;
    *len = cut;
    return KAAMER_OK;
}

extern "C" {

struct kaamer_reader {
    int fd = -1;
    bool own_fd = false;
    bool ended = false, strict = false;
    kaamer_bytes *src = nullptr;  // plain or gzip: the file as text
    std::vector<char> text;       // decoded text not yet split into lines
    size_t text_pos = 0, text_len = 0;
    std::string carry;            // a line that began in an earlier block
    RecordParser ps;
    uint64_t n_records = 0;
};

// fills rd->text with the next block of decoded text; false: the input is over
static bool reader_fill(kaamer_reader *rd)
{
    rd->text_pos = 0;
    rd->text_len = kaamer_bytes_read(rd->src, rd->text.data(), rd->text.size());
    return rd->text_len != 0;
}

int kaamer_reader_open_fd(int fd, int format, int strict_scanner, kaamer_reader **out)
{
    if (!out || fd < 0 || (format != 0 && format != 1)) return kaamer_fail(KAAMER_E_ARG, "reader_open: bad argument (format 0 = FASTA, 1 = FASTQ)");
    *out = nullptr;
    kaamer_reader *rd = new (std::nothrow) kaamer_reader();
    if (!rd) return kaamer_fail(KAAMER_E_NOMEM, "reader");
    rd->fd = fd;
    rd->ps.fastq = format == 1;
    rd->strict = strict_scanner != 0;
    rd->text.resize(4u << 20);
    const int rc = kaamer_bytes_open_fd(fd, &rd->src);
    if (rc) { delete rd; return rc; }
    size_t nh = 0;
    const uint8_t *head = kaamer_bytes_head(rd->src, &nh);
    if (nh == 0) rd->ended = true;   // (the reference exits on the read error of an empty file)
    if (!kaamer_bytes_is_gzip(rd->src) && rd->strict) {
        // anything DetectContentType does not call "text/plain; charset=utf-8" yields no query (search.go:266-270):
        // a UTF-16 / UTF-32 byte-order mark, or a byte the sniffer counts as binary among the first 32
        bool text_utf8 = !(nh >= 2 && ((head[0] == 0xFE && head[1] == 0xFF) || (head[0] == 0xFF && head[1] == 0xFE)));
        for (size_t i = 0; i < nh && text_utf8; i++) {
            const uint8_t c = head[i];
            if (c <= 0x08 || c == 0x0B || (c >= 0x0E && c <= 0x1A) || (c >= 0x1C && c <= 0x1F)) text_utf8 = false;
        }
        if (!text_utf8) { kaamer_bytes_end(rd->src); rd->ended = true; }
    }
    *out = rd;
    return KAAMER_OK;
}

int kaamer_reader_open(const char *path, int format, int strict_scanner, kaamer_reader **out)
{
    if (!path || !out) return kaamer_fail(KAAMER_E_ARG, "reader_open: bad argument");
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return kaamer_fail(KAAMER_E_IO, "reader_open: cannot open %s", path);
    const int rc = kaamer_reader_open_fd(fd, format, strict_scanner, out);
    if (rc) { close(fd); return rc; }
    (*out)->own_fd = true;
    return KAAMER_OK;
}

int kaamer_reader_next(kaamer_reader *rd, uint32_t max_seqs, uint64_t max_bytes, kaamer_reads **out)
{
    if (!rd || !out || max_seqs == 0) return kaamer_fail(KAAMER_E_ARG, "reader_next: bad argument");
    *out = nullptr;
    kaamer_reads *r = new_reads();
    if (!r) return kaamer_fail(KAAMER_E_NOMEM, "reader_next");
    while (!rd->ended && r->size_in_kmer.size() < max_seqs && r->seqs.size() < max_bytes) {
        if (rd->text_pos == rd->text_len && !reader_fill(rd)) {
            // the end of the input: an unterminated last line, then the pending record as the LAST one
            if (!rd->carry.empty()) {
                if (!(rd->strict && rd->carry.size() >= SCANNER_MAX)) {
                    size_t n = rd->carry.size();
                    if (n && rd->carry[n - 1] == '\r') n--;
                    rd->ps.line(r, rd->carry.data(), rd->carry.data() + n);
                }
                rd->carry.clear();
            }
            rd->ps.finish(r);
            rd->ended = true;
            break;
        }
        const char *p = rd->text.data() + rd->text_pos, *end = rd->text.data() + rd->text_len;
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        if (!nl) {   // the line goes on in the next block
            rd->carry.append(p, end);
            rd->text_pos = rd->text_len;
            if (rd->strict && rd->carry.size() >= SCANNER_MAX) {   // the scanner gives up here: the pending record is the last
                rd->carry.clear();
                rd->ps.finish(r);
                rd->ended = true;
            }
            continue;
        }
        rd->text_pos = (size_t)(nl + 1 - rd->text.data());
        const char *b = p, *e = nl;
        if (!rd->carry.empty()) {
            rd->carry.append(p, nl);
            b = rd->carry.data();
            e = b + rd->carry.size();
        }
        if (rd->strict && (size_t)(e - b) >= SCANNER_MAX) {
            rd->carry.clear();
            rd->ps.finish(r);
            rd->ended = true;
            break;
        }
        if (e > b && e[-1] == '\r') e--;
        rd->ps.line(r, b, e);
        rd->carry.clear();
    }
    rd->n_records += r->size_in_kmer.size();
    *out = r;
    return KAAMER_OK;
}

int kaamer_reader_done(const kaamer_reader *rd) { return (!rd || rd->ended) ? 1 : 0; }
uint64_t kaamer_reader_records(const kaamer_reader *rd) { return rd ? rd->n_records : 0; }

void kaamer_reader_close(kaamer_reader *rd)
{
    if (!rd) return;
    kaamer_bytes_close(rd->src);
    if (rd->own_fd && rd->fd >= 0) close(rd->fd);
    delete rd;
}

uint32_t kaamer_reads_count(const kaamer_reads *r) { return r ? (uint32_t)r->size_in_kmer.size() : 0; }
const uint8_t *kaamer_reads_seqs(const kaamer_reads *r) { return r ? r->seqs.data() : nullptr; }
const uint64_t *kaamer_reads_offsets(const kaamer_reads *r) { return r ? r->offsets.data() : nullptr; }
const int32_t *kaamer_reads_size_in_kmer(const kaamer_reads *r) { return r ? r->size_in_kmer.data() : nullptr; }
const char *kaamer_reads_names(const kaamer_reads *r) { return r ? r->names.data() : nullptr; }
const uint64_t *kaamer_reads_name_offsets(const kaamer_reads *r) { return r ? r->name_off.data() : nullptr; }
const int32_t *kaamer_reads_plus_strand(const kaamer_reads *r) { return r ? r->plus_strand.data() : nullptr; }
void kaamer_reads_free(kaamer_reads *r) { delete r; }

// the library's own table of a genetic code (gcodes.h), as tests and a Go host see it; 0 = the reference's behaviour = table 11
int kaamer_genetic_code(int32_t code, char aa[64], char start[64])
{
    if (!aa || !start) return kaamer_fail(KAAMER_E_ARG, "genetic_code: bad argument");
    const int slot = kt_gcode_slot(code);
    if (slot < 0) return kaamer_fail(KAAMER_E_ARG, "genetic_code: unknown genetic code %d (one of 1-6, 9-15; 0 = table 11)", (int)code);
    memcpy(aa, kt_tables()[slot].aa, 64);
    memcpy(start, kt_tables()[slot].start, 64);
    return KAAMER_OK;
}

// SetBestStartCodon, dna.go:198-272.  hits must be in sortMapByValue order (Kmatch
// descending; kaamer_sort_hits).  The reference scans PositionHits of the best hits; the only
// thing it reads from them is the lowest matching position of the first best hit and whether
// position 0 matches for the following ones (its `exit` flag is never reset, dna.go:224-237),
// which is exactly hit_first_pos.  Returns the number of residues trimmed from the ORF head
// (0: unchanged) and updates start_position / size_in_kmer like dna.go:252-267.
int32_t kaamer_set_best_start_codon(const uint32_t *kmatch_sorted, const uint32_t *first_pos_sorted, int64_t n_hits,
                                    const int32_t *starts_alt, int32_t n_starts, int32_t plus_strand,
                                    const uint8_t *orf_aa, uint32_t aa_len, int32_t *start_position, int32_t *size_in_kmer)
{
    if (n_starts < 1 || !starts_alt || !start_position || !size_in_kmer) return 0;  // dna.go:210-212
    int64_t best_hit_score = 0;
    int64_t first_best_hit_pos = 999999999;                                        // dna.go:219
    bool exit_ = false;
    for (int64_t h = 0; h < n_hits; h++) {
        if ((int64_t)kmatch_sorted[h] < best_hit_score) continue;                  // dna.go:203-208
        best_hit_score = kmatch_sorted[h];
        // dna.go:225-237 on this best hit's PositionHits
        if (!exit_) {
            if ((int64_t)first_pos_sorted[h] < first_best_hit_pos) first_best_hit_pos = first_pos_sorted[h];
            exit_ = true;
        } else if (first_pos_sorted[h] == 0) {
            first_best_hit_pos = 0;  // only position 0 is examined once exit is set
        }
    }
    int32_t best_start = starts_alt[0];
    const int32_t first_start = starts_alt[0];
    for (int32_t s = 0; s < n_starts; s++) {                                       // dna.go:240-249
        if ((int64_t)starts_alt[s] <= first_best_hit_pos) best_start = starts_alt[s];
        else break;
    }
    if (best_start == first_start) return 0;
    *start_position = plus_strand ? *start_position + 3 * best_start : *start_position - 3 * best_start;  // dna.go:254-258
    const int64_t new_len = (int64_t)aa_len - best_start;
    int32_t s = (int32_t)(new_len - KAAMER_KMER_SIZE + 1);                         // dna.go:263
    if (new_len > 0 && orf_aa && orf_aa[aa_len - 1] == '*') s--;                   // dna.go:264-266
    *size_in_kmer = s;
    return best_start;
}

}  // extern "C"

// ---- host post-steps kept bit-compatible with the reference (moved here from search.hip: pure host code, part of
// the sanitized CPU build, tools/asan) -------------------------------------------------------------------------
extern "C" {

int64_t kaamer_filter_results(const uint32_t *kmatch_sorted, int64_t n_hits, int32_t size_in_kmer, double min_k_ratio,
                              int64_t min_k_match, int64_t max_results)
{
    // search.go:189-220
    int64_t last_good = n_hits - 1;
    for (int64_t i = 0; i < n_hits; i++) {
        const int64_t km = (int64_t)kmatch_sorted[i];
        if (((double)km / (double)size_in_kmer) < min_k_ratio || km < min_k_match) {
            if (last_good == n_hits - 1) last_good = i - 1;
        }
    }
    if (last_good >= max_results) last_good = max_results - 1;
    return last_good < 0 ? 0 : last_good + 1;
}

void kaamer_sort_hits(const uint32_t *pid, const uint32_t *kmatch, int64_t n_hits, uint32_t *order)
{
    std::vector<uint32_t> idx((size_t)n_hits);
    for (int64_t i = 0; i < n_hits; i++) idx[(size_t)i] = (uint32_t)i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        if (kmatch[a] != kmatch[b]) return kmatch[a] > kmatch[b];
        return pid[a] < pid[b];
    });
    for (int64_t i = 0; i < n_hits; i++) order[i] = idx[(size_t)i];
}

// FormatPositionsToString, search.go:694-742, byte for byte.  A run is closed by the first unset position `pos` and
// printed as start-end with start = first set position + 1 and end = pos + 1 (one past the run's last position as the
// reference counts from 1); a run that reaches the end prints len(positions); with_alignment adds KMER_SIZE - 1 to the
// end.  (The reference's single-number branch needs pos + 1 <= currentStart and can never be taken.)
uint64_t kaamer_format_positions(const uint64_t *bits, int32_t n_bits, int32_t with_alignment, char *buf, uint64_t cap)
{
    uint64_t len = 0;
    auto put = [&](char c) { if (buf && len < cap) buf[len] = c; len++; };
    auto put_int = [&](long long v) {
        char tmp[24];
        int n = 0;
        do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (n) put(tmp[--n]);
    };
    auto put_run = [&](long long start, long long end) {
        if (len) put(',');
        put_int(start);
        put('-');
        put_int(with_alignment ? end + KAAMER_KMER_SIZE - 1 : end);
    };
    long long current_start = 0;
    bool in_sequence = false;
    const long long n = (bits && n_bits > 0) ? n_bits : 0;
    for (long long pos = 0; pos < n; pos++) {
        const bool match = (bits[pos >> 6] >> (pos & 63)) & 1ull;
        if (match) {
            if (!in_sequence) { current_start = pos + 1; in_sequence = true; }
        } else if (in_sequence) {
            put_run(current_start, pos + 1);
            in_sequence = false;
        }
    }
    if (in_sequence) put_run(current_start, n);
    if (buf && cap) buf[len < cap ? len : cap - 1] = '\0';
    return len;
}

}  // extern "C"
