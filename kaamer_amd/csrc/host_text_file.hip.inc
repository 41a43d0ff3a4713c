// host_text_file.hip.inc — FastqSearch over a FILE (search_fastq.go:60-136) with the reader on the device (included by
// search.hip inside its extern "C" block, after host_replicas.hip.inc): raw bytes -> chunks cut at kaamer_text_cut_fastq ->
// the replicas' text call, round-robin -> a callback per chunk, in input order.  The loop is host_replicas.hip.inc's
// chunk_loop; this file is the source it runs over.

// chunk k -> replica k mod n, as kaamer_replica_stream_push deals packed chunks
static int replica_stream_push_text(kaamer_replica_stream *rs, const char *text, uint64_t len)
{
    const int rc = stream_push_text((*rs->st)[rs->pushed % rs->st->size()], text, len);
    if (rc == KAAMER_OK) rs->pushed++;
    return rc;
}

struct TextChunk { std::vector<char> text; size_t len; };
struct TextSource {
    typedef TextChunk Chunk;
    kaamer_text_chunker *reader;  // the file's text, cut into chunks (host_search.cpp)
    kaamer_replica_stream *rs;
    kaamer_text_chunk_cb cb;
    void *user;
    uint64_t n_seen;              // records delivered so far
    std::vector<std::vector<char>> pool;   // buffers of chunks that were delivered

    bool done() const { return kaamer_text_chunker_done(reader); }
    int next(Chunk **out)
    {
        Chunk *c = new (std::nothrow) Chunk();
        if (!c) return kaamer_fail(KAAMER_E_NOMEM, "search_text_file: chunk");
        if (!pool.empty()) { c->text.swap(pool.back()); pool.pop_back(); }
        const int rc = kaamer_text_chunker_next(reader, &c->text, &c->len);
        if (rc || c->len == 0) { drop(c); return rc; }
        *out = c;
        return KAAMER_OK;
    }
    int push(Chunk *c) { return replica_stream_push_text(rs, c->text.data(), c->len); }
    int pop(kaamer_batch_top **top) { return kaamer_replica_stream_pop(rs, top); }
    uint32_t pending() const { return kaamer_replica_stream_pending(rs); }
    int deliver(Chunk *c, const kaamer_batch_top *top)
    {
        const kaamer_text_span *spans = nullptr;
        uint32_t n = 0;
        (void)kaamer_batch_top_text_spans(top, &spans, &n);
        const uint64_t first = n_seen;
        n_seen += n;
        return cb ? cb(user, first, c->text.data(), c->len, spans, n, top) : 0;
    }
    void drop(Chunk *c)
    {
        if (pool.size() < 64) pool.emplace_back(std::move(c->text));
        delete c;
    }
};

int kaamer_search_text_file(kaamer_replicas *r, const char *path, int format, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                            uint32_t max_results, uint64_t chunk_text_bytes, uint32_t in_flight, kaamer_text_chunk_cb cb, void *user,
                            kaamer_counters *total)
{
    if (!r || !path || chunk_text_bytes == 0 || max_results < 1) return kaamer_fail(KAAMER_E_ARG, "search_text_file: bad argument");
    if (format == 0)
        return kaamer_fail(KAAMER_E_ARG, "search_text_file: FASTA is not parsed on the device: use the host reader (kaamer_search_file)");
    if (format != 1) return kaamer_fail(KAAMER_E_ARG, "search_text_file: unknown format %d (1 = FASTQ)", format);
    SEQ_TYPE_CHK(seq_type, "search_text_file");
    if (!is_nucl(seq_type)) return kaamer_fail(KAAMER_E_ARG, "search_text_file: FASTQ text is READS or NUCLEOTIDE input, not PROTEIN");
    if (chunk_text_bytes > 0xFFFFFFFFull / 4)
        return kaamer_fail(KAAMER_E_ARG, "search_text_file: chunk_text_bytes above 2^30 - 1 (a chunk may grow to four times that and spans are 32-bit)");
    if (total) memset(total, 0, sizeof *total);
    if (in_flight < 1) in_flight = 3;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return kaamer_fail(KAAMER_E_IO, "search_text_file: cannot open %s", path);
    kaamer_bytes *bytes = nullptr;
    int rc = kaamer_bytes_open_fd(fd, &bytes);
    if (rc) { close(fd); return rc; }
    kaamer_replica_stream *rs = nullptr;
    rc = kaamer_replica_stream_open_flat(r, seq_type, min_k_ratio, min_k_match, max_results, &rs);
    if (!rc) {
        kaamer_text_chunker *reader = kaamer_text_chunker_new(bytes, chunk_text_bytes);
        if (!reader) rc = kaamer_fail(KAAMER_E_NOMEM, "search_text_file: chunk reader");
        if (!rc) {
            TextSource src = { reader, rs, cb, user, 0, {} };
            rc = chunk_loop(src, in_flight * kaamer_replicas_count(r), total);
        }
        kaamer_text_chunker_free(reader);
        kaamer_replica_stream_close(rs);
    }
    kaamer_bytes_close(bytes);
    close(fd);
    return rc;
}
