// host_text_file.hip.inc — FastqSearch over a FILE (search_fastq.go:60-136) with the reader on the device (included by
// search.hip inside its extern "C" block, after host_replicas.hip.inc): raw bytes -> chunks cut at kaamer_text_cut_fastq ->
// the replicas' text call, round-robin -> a callback per chunk, in input order.  The loop is host_replicas.hip.inc's
// chunk_loop; this file holds the two sources it runs over (TextSource: text the host chunk reader cut, FASTQ or FASTA;
// BgzfSource: whole BGZF blocks for the device's inflater), and what the three exported calls share:
//   text_file_check    what a call refuses, under its own name
//   text_file_run      open the file and the replica stream, chunk_loop over the source, close both
//   text_file_deliver  a chunk's result to the callback

// chunk k -> replica k mod n, as kaamer_replica_stream_push deals packed chunks
static int replica_stream_push_text(kaamer_replica_stream *rs, const TextRequest &rq)
{
    const int rc = stream_push_text((*rs->st)[rs->pushed % rs->st->size()], rq);
    if (rc == KAAMER_OK) rs->pushed++;
    return rc;
}

// the records of a chunk (`text`: what the spans index) and its hits to the callback; n_seen: records delivered so far
static int text_file_deliver(kaamer_text_chunk_cb cb, void *user, uint64_t *n_seen, const char *text, uint64_t len, const kaamer_batch_top *top)
{
    const kaamer_text_span *spans = nullptr;
    uint32_t n = 0;
    (void)kaamer_batch_top_text_spans(top, &spans, &n);
    const uint64_t first = *n_seen;
    *n_seen += n;
    return cb ? cb(user, first, text, len, spans, n, top) : 0;
}

struct TextChunk { std::vector<char> text; size_t len; bool last; };
struct TextSource {
    typedef TextChunk Chunk;
    uint64_t budget;
    bool fasta;                   // kaamer_search_fasta_file: the chunks are FASTA, every one but the file's last with upper_last
    kaamer_text_chunk_cb cb;
    void *user;
    kaamer_replica_stream *rs = nullptr;
    kaamer_bytes *bytes = nullptr;
    kaamer_text_chunker *reader = nullptr;   // the file's text, cut into chunks (host_search.cpp)
    uint64_t n_seen = 0;          // records delivered so far
    std::vector<std::vector<char>> pool;   // buffers of chunks that were delivered

    ~TextSource() { if (reader) kaamer_text_chunker_free(reader); if (bytes) kaamer_bytes_close(bytes); }
    int open(int fd)
    {
        const int rc = kaamer_bytes_open_fd(fd, &bytes);
        if (rc) return rc;
        reader = kaamer_text_chunker_new(bytes, budget, fasta);
        return reader ? KAAMER_OK : kaamer_fail(KAAMER_E_NOMEM, "%s: chunk reader", fasta ? "search_fasta_file" : "search_text_file");
    }
    bool done() const { return kaamer_text_chunker_done(reader); }
    int next(Chunk **out)
    {
        Chunk *c = new (std::nothrow) Chunk();
        if (!c) return kaamer_fail(KAAMER_E_NOMEM, "search_text_file: chunk");
        if (!pool.empty()) { c->text.swap(pool.back()); pool.pop_back(); }
        const int rc = kaamer_text_chunker_next(reader, &c->text, &c->len);
        if (rc || c->len == 0) { drop(c); return rc; }
        c->last = kaamer_text_chunker_done(reader);   // (the reader hands out the rest of the input only once it has seen its end)
        *out = c;
        return KAAMER_OK;
    }
    int push(Chunk *c)
    {
        return replica_stream_push_text(rs, fasta ? fasta_request(c->text.data(), c->len, !c->last) : fastq_request(c->text.data(), c->len));
    }
    int pop(kaamer_batch_top **top) { return kaamer_replica_stream_pop(rs, top); }
    uint32_t pending() const { return kaamer_replica_stream_pending(rs); }
    int deliver(Chunk *c, const kaamer_batch_top *top) { return text_file_deliver(cb, user, &n_seen, c->text.data(), c->len, top); }
    void drop(Chunk *c)
    {
        if (pool.size() < 64) pool.emplace_back(std::move(c->text));
        delete c;
    }
};

// ---- the third source: a BGZF file whose blocks are inflated on the device (kaamer_search_text_file_opts, device_inflate).
// The file is read RAW; kaamer_bgzf_scan finds whole blocks, which are grouped until their ISIZEs reach the budget.  The
// device text of chunk k is the tail of chunk k-1 (a short plain upload) followed by its blocks' output; the device cuts
// it (the last chunk: at its end), parses and searches [0, cut) and hands back [cut, end) as the next tail, and the text
// [0, cut) with the result: that copy is what the callback sees.  A chunk without a cut takes one more budget of blocks,
// up to four, then fails as the host chunk reader does.
// FALLBACK.  As soon as a chunk reports a bad block, or the scan meets a member that is no BGZF block (ordinary gzip,
// FNAME set, ...), or the file ends inside a block, the file's position at that chunk's first block goes to the host
// inflater (kaamer_bytes) with the pending tail in front, and the rest of the file runs on kaamer_search_text_file's
// route.  Members are independent, so zlib started there yields what it yields there in a run from the file's start: the
// device never has to imitate zlib on a damaged stream, and the concatenated text equals the flag-0 run's for every file.
struct BgzfChunk {
    bool host = false;
    std::vector<char> text;                   // a host chunk (after the fallback)
    size_t len = 0;
    std::vector<kaamer_bgzf_block> blocks;    // a device chunk: comp_off relative to the chunk's first block
    size_t comp_len = 0;                      // raw bytes of those blocks
    uint64_t isize_sum = 0;
    bool last = false, stopped = false;       // the file ends with it / what follows is no whole BGZF block
};
struct BgzfSource {
    typedef BgzfChunk Chunk;
    uint64_t budget;
    kaamer_text_chunk_cb cb;
    void *user;
    kaamer_replica_stream *rs = nullptr;
    int fd = -1;
    uint64_t n_seen = 0;
    std::vector<uint8_t> raw;                 // file bytes [raw_off, raw_off + raw_len); the next chunk starts at raw_pos
    size_t raw_pos = 0, raw_len = 0;
    uint64_t raw_off = 0;
    bool file_eof = false, finished = false;
    std::vector<char> tail, next_tail;        // the text behind the last chunk's cut
    bool no_cut = false;
    kaamer_bytes *bytes = nullptr;            // after the fallback
    kaamer_text_chunker *reader = nullptr;
    std::vector<kaamer_bgzf_block> tab;

    ~BgzfSource() { if (reader) kaamer_text_chunker_free(reader); if (bytes) kaamer_bytes_close(bytes); }
    int open(int file) { fd = file; return KAAMER_OK; }
    bool done() const { return reader ? kaamer_text_chunker_done(reader) : finished; }

    // at least `want` unread bytes in raw, or the file's end
    void fill(size_t want)
    {
        if (raw_pos) { memmove(raw.data(), raw.data() + raw_pos, raw_len - raw_pos); raw_off += raw_pos; raw_len -= raw_pos; raw_pos = 0; }
        if (raw.size() < want) raw.resize(want);
        while (!file_eof && raw_len < want) {
            ssize_t k;
            do k = read(fd, raw.data() + raw_len, raw.size() - raw_len); while (k < 0 && errno == EINTR);
            if (k <= 0) file_eof = true; else raw_len += (size_t)k;
        }
    }
    // whole blocks from raw_pos on until their ISIZEs reach `want` (nothing is consumed before the push succeeds)
    int gather(Chunk *c, uint64_t want)
    {
        size_t need = (size_t)(want / 2) + (1u << 16);
        for (;;) {
            if (raw_len - raw_pos < need) fill(need);
            const size_t avail = raw_len - raw_pos;
            if (tab.size() < avail / 28 + 1) tab.resize(avail / 28 + 1);
            uint64_t n = 0, used = 0;
            const int rc = kaamer_bgzf_scan(raw.data() + raw_pos, avail, tab.data(), tab.size(), &n, &used);
            if (rc) return rc;
            size_t k = 0;
            uint64_t sum = 0;
            while (k < n && sum < want) sum += tab[k++].isize;
            const size_t comp = k ? (size_t)(tab[k - 1].comp_off + tab[k - 1].comp_len + 8) : 0;   // the end of block k - 1's trailer
            // every scanned block is taken and fewer than 64 KiB (a block's most) lie behind them: what follows is not known yet
            if (k == n && !file_eof && avail - used < (1u << 16)) { need = avail + need; continue; }
            c->blocks.assign(tab.begin(), tab.begin() + k);
            c->comp_len = comp;
            c->isize_sum = sum;
            c->stopped = k == n && used < avail;                       // (here: 64 KiB or the file's end lie behind `used`)
            c->last = file_eof && k == n && used == avail;
            return KAAMER_OK;
        }
    }
    // the host inflater takes over at the file's byte `at`, the pending tail in front
    int fall_back(uint64_t at)
    {
        if (lseek(fd, (off_t)at, SEEK_SET) < 0) return kaamer_fail(KAAMER_E_IO, "search_text_file: cannot seek");
        int rc = kaamer_bytes_open_fd(fd, &bytes);
        if (rc) return rc;
        if (!kaamer_bytes_is_gzip(bytes)) kaamer_bytes_end(bytes);   // bytes that are no gzip header end a multi-member stream
        reader = kaamer_text_chunker_new(bytes, budget);
        if (!reader) return kaamer_fail(KAAMER_E_NOMEM, "search_text_file: chunk reader");
        kaamer_text_chunker_prime(reader, tail.data(), tail.size());
        tail.clear();
        return KAAMER_OK;
    }
    int next_host(Chunk *c)
    {
        c->host = true;
        c->blocks.clear();
        return kaamer_text_chunker_next(reader, &c->text, &c->len);
    }
    int next(Chunk **out)
    {
        Chunk *c = new (std::nothrow) Chunk();
        if (!c) return kaamer_fail(KAAMER_E_NOMEM, "search_text_file: chunk");
        int rc = KAAMER_OK;
        if (!reader) {
            const uint64_t want = budget > tail.size() ? budget - tail.size() : 1;
            rc = gather(c, want);
            if (!rc && c->blocks.empty()) {
                if (c->stopped || !tail.empty()) rc = fall_back(raw_off + raw_pos);   // (a tail without blocks: the host route flushes it)
                else finished = true;
            }
        }
        if (!rc && reader) rc = next_host(c);
        if (rc || (c->host ? c->len == 0 : c->blocks.empty())) { delete c; return rc; }
        *out = c;
        return KAAMER_OK;
    }
    int push(Chunk *c)
    {
        for (;;) {
            if (c->host) return replica_stream_push_text(rs, fastq_request(c->text.data(), c->len));
            TextRequest bz = bgzf_request(raw.data() + raw_pos, c->comp_len);
            bz.blocks = &c->blocks;
            bz.file = true; bz.last = c->last; bz.tail = tail.data(); bz.tail_len = tail.size();
            bz.tail_out = &next_tail; bz.no_cut = &no_cut;
            no_cut = false;
            const uint64_t text_len = bz.len = tail.size() + c->isize_sum;
            int rc = replica_stream_push_text(rs, bz);
            if (rc == KAAMER_OK) {
                raw_pos += c->comp_len;
                tail.swap(next_tail);
                if (c->last) finished = true;
                return KAAMER_OK;
            }
            if (rc == KAAMER_E_CAPACITY && no_cut) {
                if (text_len >= 4 * budget)
                    return kaamer_fail(KAAMER_E_CAPACITY, "search_text_file: no line starts with '@' within %llu bytes of text (4 chunk_text_bytes): "
                                                          "use kaamer_search_file, whose reader takes records of any length", (unsigned long long)text_len);
                const size_t had = c->blocks.size();
                rc = gather(c, c->isize_sum + budget);
                if (rc) return rc;
                if (c->blocks.size() > had || c->last) continue;   // one more budget of blocks (or: the file ends here after all)
                rc = KAAMER_E_FORMAT;                               // nothing more to take: what follows is for the host
            }
            if (rc != KAAMER_E_FORMAT) return rc;
            rc = fall_back(raw_off + raw_pos);
            if (!rc) rc = next_host(c);
            if (rc) return rc;
        }
    }
    int pop(kaamer_batch_top **top) { return kaamer_replica_stream_pop(rs, top); }
    uint32_t pending() const { return kaamer_replica_stream_pending(rs); }
    int deliver(Chunk *c, const kaamer_batch_top *top)
    {
        const char *text = c->text.data();
        uint64_t len = c->len;
        if (!c->host) (void)kaamer_batch_top_text(top, &text, &len);   // the copy brought back from the device
        return text_file_deliver(cb, user, &n_seen, text, len, top);
    }
    void drop(Chunk *c) { delete c; }
};

// what the file calls refuse before they open anything (fasta: kaamer_search_fasta_file, which takes any sequence type)
static int text_file_check(const char *who, bool fasta, kaamer_replicas *r, const char *path, int format, int32_t seq_type, uint32_t max_results,
                           uint64_t chunk_text_bytes)
{
    if (!r || !path || chunk_text_bytes == 0 || max_results < 1) return kaamer_fail(KAAMER_E_ARG, "%s: bad argument", who);
    if (!fasta) {
        if (format == 0)
            return kaamer_fail(KAAMER_E_ARG, "%s: FASTA is not parsed on the device by this call: use kaamer_search_fasta_file, or the host reader (kaamer_search_file)", who);
        if (format != 1) return kaamer_fail(KAAMER_E_ARG, "%s: unknown format %d (1 = FASTQ)", who, format);
    }
    SEQ_TYPE_CHK(seq_type, who);
    if (!fasta && !is_nucl(seq_type)) return kaamer_fail(KAAMER_E_ARG, "%s: FASTQ text is READS or NUCLEOTIDE input, not PROTEIN", who);
    if (chunk_text_bytes > 0xFFFFFFFFull / 4)
        return kaamer_fail(KAAMER_E_ARG, "%s: chunk_text_bytes above 2^30 - 1 (a chunk may grow to four times that and spans are 32-bit)", who);
    return KAAMER_OK;
}

// the file `path` and a replica stream opened, chunk_loop over `src` (a TextSource or a BgzfSource), both closed
extern "C++" {
template <class Src> static int text_file_run(Src &src, const char *who, kaamer_replicas *r, const char *path, int32_t seq_type, double min_k_ratio,
                                              int64_t min_k_match, uint32_t max_results, uint32_t in_flight, kaamer_counters *total)
{
    if (total) memset(total, 0, sizeof *total);
    if (in_flight < 1) in_flight = 3;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return kaamer_fail(KAAMER_E_IO, "%s: cannot open %s", who, path);
    int rc = src.open(fd);
    if (!rc) rc = kaamer_replica_stream_open_flat(r, seq_type, min_k_ratio, min_k_match, max_results, &src.rs);
    if (!rc) {
        rc = chunk_loop(src, in_flight * kaamer_replicas_count(r), total);
        kaamer_replica_stream_close(src.rs);
    }
    close(fd);
    return rc;
}
}  // extern "C++"

// ProteinSearch / NucleotideSearch / FastqSearch over a FASTA file (search_protein.go, search_nucleotide.go, search_fastq.go:
// each calls GetQueriesFasta when the request is not FASTQ) with the reader on the device
int kaamer_search_fasta_file(kaamer_replicas *r, const char *path, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                             uint32_t max_results, uint64_t chunk_text_bytes, uint32_t in_flight, kaamer_text_chunk_cb cb, void *user,
                             kaamer_counters *total)
{
    const int rc = text_file_check("search_fasta_file", true, r, path, 0, seq_type, max_results, chunk_text_bytes);
    if (rc) return rc;
    TextSource src = { chunk_text_bytes, true, cb, user };
    return text_file_run(src, "search_fasta_file", r, path, seq_type, min_k_ratio, min_k_match, max_results, in_flight, total);
}

int kaamer_search_text_file(kaamer_replicas *r, const char *path, int format, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                            uint32_t max_results, uint64_t chunk_text_bytes, uint32_t in_flight, kaamer_text_chunk_cb cb, void *user,
                            kaamer_counters *total)
{
    return kaamer_search_text_file_opts(r, path, format, seq_type, min_k_ratio, min_k_match, max_results, chunk_text_bytes, in_flight, 0, cb, user, total);
}

// device_inflate: a file that starts with the gzip signature goes through BgzfSource; flag 0, and plain files: TextSource
int kaamer_search_text_file_opts(kaamer_replicas *r, const char *path, int format, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                 uint32_t max_results, uint64_t chunk_text_bytes, uint32_t in_flight, int32_t device_inflate,
                                 kaamer_text_chunk_cb cb, void *user, kaamer_counters *total)
{
    const int rc = text_file_check("search_text_file", false, r, path, format, seq_type, max_results, chunk_text_bytes);
    if (rc) return rc;
    bool gz = false;
    if (device_inflate) {
        const int fd = open(path, O_RDONLY | O_CLOEXEC);
        uint8_t head[3];
        if (fd >= 0) { gz = read(fd, head, 3) == 3 && kaamer_is_gzip((const char *)head, 3); close(fd); }
    }
    if (gz) {
        BgzfSource src = { chunk_text_bytes, cb, user };
        return text_file_run(src, "search_text_file", r, path, seq_type, min_k_ratio, min_k_match, max_results, in_flight, total);
    }
    TextSource src = { chunk_text_bytes, false, cb, user };
    return text_file_run(src, "search_text_file", r, path, seq_type, min_k_ratio, min_k_match, max_results, in_flight, total);
}
