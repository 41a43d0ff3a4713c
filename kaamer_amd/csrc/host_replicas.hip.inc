// host_replicas.hip.inc — ONE process, the same database resident on several devices (included by search.hip inside
// its extern "C" block, after host_sharded_collect.hip.inc).
//
// SURVEY 8e: a database that fits one device is not sharded, the QUERY stream is split -- "replicas only", no
// collective.  The reference is one server process (api/server.go:47-65) whose FastqSearch takes a file
// (search_fastq.go:60-136): here that process opens the index once per device (kaamer_index_open_replicas) and
// deals the chunks of the read set round-robin over the devices (kaamer_replica_stream_*: chunk k goes to replica
// k mod n, results come back in input order), or hands the whole job to kaamer_search_file, which is the reader
// (kaamer_reader_*: incremental, gzip) + the dealing + a callback per chunk -- BASELINE configs[4] behind the ABI.
struct kaamer_replicas {
    std::vector<kaamer_index *> *ix = nullptr;
};

void kaamer_replicas_close(kaamer_replicas *r)
{
    if (!r) return;
    if (r->ix) {
        for (kaamer_index *ix : *r->ix) if (ix) kaamer_index_close(ix);
        delete r->ix;
    }
    delete r;
}

static int replicas_open_common(const int *devices, uint32_t n, kaamer_replicas **out, const kaamer_image *img)
{
    if (!out || !devices || n == 0 || n > 64 || !img) return kaamer_fail(KAAMER_E_ARG, "index_open_replicas: bad argument");
    *out = nullptr;
    kaamer_replicas *r = new (std::nothrow) kaamer_replicas();
    if (!r) return kaamer_fail(KAAMER_E_NOMEM, "replicas");
    r->ix = new (std::nothrow) std::vector<kaamer_index *>(n, nullptr);
    if (!r->ix) { delete r; return kaamer_fail(KAAMER_E_NOMEM, "replicas"); }
    for (uint32_t i = 0; i < n; i++) {
        const int rc = kaamer_index_open_image(img, devices[i], &(*r->ix)[i]);
        if (rc) { kaamer_replicas_close(r); return rc; }
    }
    *out = r;
    return KAAMER_OK;
}

int kaamer_index_open_replicas_image(const kaamer_image *img, const int *devices, uint32_t n, kaamer_replicas **out)
{
    return replicas_open_common(devices, n, out, img);
}

int kaamer_index_open_replicas(const char *path, const int *devices, uint32_t n, kaamer_replicas **out)
{
    if (!path) return kaamer_fail(KAAMER_E_ARG, "index_open_replicas: bad argument");
    kaamer_image *img = nullptr;   // read once, uploaded n times
    int rc = kaamer_image_load(path, &img);
    if (rc) return rc;
    rc = replicas_open_common(devices, n, out, img);
    kaamer_image_free(img);
    return rc;
}

uint32_t kaamer_replicas_count(const kaamer_replicas *r) { return (r && r->ix) ? (uint32_t)r->ix->size() : 0u; }
kaamer_index *kaamer_replicas_index(const kaamer_replicas *r, uint32_t i) { return (r && r->ix && i < r->ix->size()) ? (*r->ix)[i] : nullptr; }

// ---- a FIFO of chunks over the set: chunk k -> replica k mod n; pop returns the chunks in push order
struct kaamer_replica_stream {
    std::vector<kaamer_stream *> *st = nullptr;
    uint64_t pushed = 0, popped = 0;
};

void kaamer_replica_stream_close(kaamer_replica_stream *rs)
{
    if (!rs) return;
    if (rs->st) {
        for (kaamer_stream *s : *rs->st) if (s) kaamer_stream_close(s);
        delete rs->st;
    }
    delete rs;
}

// the fixed options of a stream, in the three forms the ABI has: plain, with the bitmaps, with the alignments
struct StreamForm {
    int32_t seq_type;
    double min_k_ratio;
    int64_t min_k_match;
    uint32_t max_results;
    int32_t want_positions, want_aln;
    const char *sub_matrix;   // want_aln only
    int32_t gap_open, gap_extend, want_text;
};

// one kaamer_stream per replica
static int replica_stream_open_form(kaamer_replicas *r, const StreamForm &f, kaamer_replica_stream **out)
{
    if (!r || !r->ix || !out) return kaamer_fail(KAAMER_E_ARG, "replica_stream_open: bad argument");
    *out = nullptr;
    SEQ_TYPE_CHK(f.seq_type, "replica_stream_open");
    kaamer_replica_stream *rs = new (std::nothrow) kaamer_replica_stream();
    if (!rs) return kaamer_fail(KAAMER_E_NOMEM, "replica stream");
    rs->st = new (std::nothrow) std::vector<kaamer_stream *>(r->ix->size(), nullptr);
    if (!rs->st) { delete rs; return kaamer_fail(KAAMER_E_NOMEM, "replica stream"); }
    for (size_t i = 0; i < r->ix->size(); i++) {
        kaamer_index *ix = (*r->ix)[i];
        kaamer_stream **st = &(*rs->st)[i];
        int rc;
        if (f.want_aln) rc = kaamer_stream_open_aln_flat(ix, f.seq_type, f.min_k_ratio, f.min_k_match, f.max_results, f.want_positions, f.sub_matrix,
                                                         f.gap_open, f.gap_extend, f.want_text, st);
        else if (f.want_positions) rc = kaamer_stream_open_pos_flat(ix, f.seq_type, f.min_k_ratio, f.min_k_match, f.max_results, st);
        else rc = kaamer_stream_open_flat(ix, f.seq_type, f.min_k_ratio, f.min_k_match, f.max_results, st);
        if (rc) { kaamer_replica_stream_close(rs); return rc; }
    }
    *out = rs;
    return KAAMER_OK;
}

int kaamer_replica_stream_open_flat(kaamer_replicas *r, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                    kaamer_replica_stream **out)
{
    const StreamForm f = { seq_type, min_k_ratio, min_k_match, max_results, 0, 0, nullptr, 0, 0, 0 };
    return replica_stream_open_form(r, f, out);
}

// the chunks' results carry the bitmaps of the reported hits (kaamer_stream_open_pos_flat on every replica)
int kaamer_replica_stream_open_pos_flat(kaamer_replicas *r, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                        kaamer_replica_stream **out)
{
    const StreamForm f = { seq_type, min_k_ratio, min_k_match, max_results, 1, 0, nullptr, 0, 0, 0 };
    return replica_stream_open_form(r, f, out);
}

// ... and the alignments (kaamer_stream_open_aln_flat on every replica: KAAMER_E_ARG unless each has its table,
// kaamer_replicas_attach_proteins)
int kaamer_replica_stream_open_aln_flat(kaamer_replicas *r, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                        int32_t want_positions, const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text,
                                        kaamer_replica_stream **out)
{
    const StreamForm f = { seq_type, min_k_ratio, min_k_match, max_results, want_positions, 1, sub_matrix, gap_open, gap_extend, want_text };
    return replica_stream_open_form(r, f, out);
}

// kaamer_index_attach_proteins on every replica (HitEntries next to every copy of the index, search.go:454-470); a failure
// on replica i is reported as such and leaves replicas 0 .. i-1 attached
int kaamer_replicas_attach_proteins(kaamer_replicas *r, const kaamer_proteins *p)
{
    if (!r || !r->ix || !p) return kaamer_fail(KAAMER_E_ARG, "replicas_attach_proteins: bad argument");
    for (size_t i = 0; i < r->ix->size(); i++) {
        const int rc = kaamer_index_attach_proteins((*r->ix)[i], p);
        if (rc) {
            char why[400];
            snprintf(why, sizeof why, "%s", kaamer_last_error());
            return kaamer_fail(rc, "replicas_attach_proteins: replica %zu of %zu: %s", i, r->ix->size(), why);
        }
    }
    return KAAMER_OK;
}

// KAAMER_E_BUSY: every slot of the replica whose turn it is holds one of this stream's chunks -- pop first
int kaamer_replica_stream_push(kaamer_replica_stream *rs, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs)
{
    if (!rs || !rs->st) return kaamer_fail(KAAMER_E_ARG, "replica_stream_push: bad argument");
    const int rc = kaamer_stream_push((*rs->st)[rs->pushed % rs->st->size()], seqs, offsets, n_seqs);
    if (rc == KAAMER_OK) rs->pushed++;
    return rc;
}

int kaamer_replica_stream_pop(kaamer_replica_stream *rs, kaamer_batch_top **out)
{
    if (!rs || !rs->st || !out) return kaamer_fail(KAAMER_E_ARG, "replica_stream_pop: bad argument");
    *out = nullptr;
    if (rs->popped == rs->pushed) return kaamer_fail(KAAMER_E_ARG, "replica_stream_pop: nothing was pushed");
    const int rc = kaamer_stream_pop((*rs->st)[rs->popped % rs->st->size()], out);
    rs->popped++;   // (a failed chunk is consumed too: the FIFO stays aligned with the input)
    return rc;
}

uint32_t kaamer_replica_stream_pending(const kaamer_replica_stream *rs) { return rs ? (uint32_t)(rs->pushed - rs->popped) : 0u; }

// ---- FastqSearch / ProteinSearch over a FILE of any size (search_fastq.go:60-136: reader goroutine -> queryChan ->
// worker goroutines -> result writer): chunks of at most chunk_seqs records / about chunk_bytes of sequence, up to
// max_pending chunks in flight, the callback once per chunk, in input order, with the chunk's records (names, sequences:
// what QueryResultHandler needs next to the hits) and its reported hits.  first_seq = index of the chunk's first record in
// the file.  A non-zero return of the callback ends the run with KAAMER_E_ARG.
// The loop is written once, over a source of chunks that also searches them (chunk_loop): records from kaamer_reader_*
// through a replica stream or a sharded stream (ReadsSource over a ChunkFifo), or raw text through the replicas' text
// call (host_text_file.hip.inc).  What it needs of a source:
//   Chunk                      what is in flight and goes to the callback with its hits
//   bool done()                the input is over
//   int  next(Chunk **)        the next chunk (NULL with KAAMER_OK: none this time)
//   int  push(Chunk *)         KAAMER_E_BUSY: pop first
//   int  pop(top **)           the oldest chunk's result; a failed chunk is consumed too
//   uint32_t pending()
//   int  deliver(Chunk *, top) the callback (non-zero: stop)
//   void drop(Chunk *)
extern "C++" {
template <class Src> static int chunk_loop(Src &src, uint32_t max_pending, kaamer_counters *total)
{
    int rc = KAAMER_OK;
    std::vector<typename Src::Chunk *> fifo;   // the chunks in flight, oldest first (the callback gets the records with the hits)
    auto pop_one = [&]() -> int {
        kaamer_batch_top *top = nullptr;
        int prc = src.pop(&top);
        typename Src::Chunk *chunk = fifo.front();
        fifo.erase(fifo.begin());
        if (!prc) {
            if (total) {
                const kaamer_counters &c = top->counters;
                total->n_in += c.n_in; total->n_queries += c.n_queries; total->n_lookup += c.n_lookup; total->n_probe += c.n_probe;
                total->n_found += c.n_found; total->n_post += c.n_post; total->n_hits += c.n_hits; total->n_overflow += c.n_overflow;
                total->n_lists += c.n_lists; total->n_list_ids += c.n_list_ids;
            }
            if (src.deliver(chunk, top) != 0) prc = kaamer_fail(KAAMER_E_ARG, "search_file: stopped by the callback");
            kaamer_batch_top_free(top);
        }
        src.drop(chunk);
        return prc;
    };
    while (!rc && !src.done()) {
        typename Src::Chunk *chunk = nullptr;
        rc = src.next(&chunk);
        if (rc) break;
        if (!chunk) continue;
        for (;;) {
            int prc = KAAMER_E_BUSY;
            if (src.pending() < max_pending) prc = src.push(chunk);
            if (prc == KAAMER_OK) break;
            if (prc != KAAMER_E_BUSY || fifo.empty()) { rc = prc; break; }
            rc = pop_one();
            if (rc) break;
        }
        if (rc) { src.drop(chunk); break; }
        fifo.push_back(chunk);
    }
    while (!fifo.empty()) {   // (after an error: the chunks in flight are drained and dropped)
        const int prc = pop_one();
        if (!rc) rc = prc;
    }
    return rc;
}
}  // extern "C++"

struct ChunkFifo {
    void *st;
    int (*push)(void *st, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs);   // KAAMER_E_BUSY: pop first
    int (*pop)(void *st, kaamer_batch_top **out);                                           // a failed chunk is consumed too
    uint32_t (*pending)(const void *st);
    uint32_t max_pending;
};

// records of a kaamer_reader, searched through a ChunkFifo
struct ReadsChunk { kaamer_reads *reads; uint64_t first; };
struct ReadsSource {
    typedef ReadsChunk Chunk;
    kaamer_reader *rd;
    const ChunkFifo &q;
    uint32_t chunk_seqs;
    uint64_t chunk_bytes;
    kaamer_chunk_cb cb;
    void *user;
    uint64_t n_seen;
    bool done() const { return kaamer_reader_done(rd) != 0; }
    int next(Chunk **out)
    {
        kaamer_reads *reads = nullptr;
        const int rc = kaamer_reader_next(rd, chunk_seqs, chunk_bytes, &reads);
        if (rc) return rc;
        const uint32_t n = kaamer_reads_count(reads);
        if (n == 0) { kaamer_reads_free(reads); return KAAMER_OK; }
        Chunk *c = new (std::nothrow) Chunk{ reads, n_seen };
        if (!c) { kaamer_reads_free(reads); return kaamer_fail(KAAMER_E_NOMEM, "search_file: chunk"); }
        n_seen += n;
        *out = c;
        return KAAMER_OK;
    }
    int push(Chunk *c) { return q.push(q.st, kaamer_reads_seqs(c->reads), kaamer_reads_offsets(c->reads), kaamer_reads_count(c->reads)); }
    int pop(kaamer_batch_top **top) { return q.pop(q.st, top); }
    uint32_t pending() const { return q.pending(q.st); }
    int deliver(Chunk *c, const kaamer_batch_top *top) { return cb ? cb(user, c->first, c->reads, top) : 0; }
    void drop(Chunk *c) { kaamer_reads_free(c->reads); delete c; }
};

static int search_file_loop(kaamer_reader *rd, const ChunkFifo &q, uint32_t chunk_seqs, uint64_t chunk_bytes, kaamer_chunk_cb cb, void *user,
                            kaamer_counters *total)
{
    ReadsSource src = { rd, q, chunk_seqs, chunk_bytes, cb, user, 0 };
    return chunk_loop(src, q.max_pending, total);
}

static int replica_fifo_push(void *st, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs)
{
    return kaamer_replica_stream_push(static_cast<kaamer_replica_stream *>(st), seqs, offsets, n_seqs);
}
static int replica_fifo_pop(void *st, kaamer_batch_top **out) { return kaamer_replica_stream_pop(static_cast<kaamer_replica_stream *>(st), out); }
static uint32_t replica_fifo_pending(const void *st) { return kaamer_replica_stream_pending(static_cast<const kaamer_replica_stream *>(st)); }

// reader -> stream of form `f` -> loop
static int search_file_replicas(kaamer_replicas *r, const char *path, int format, int strict_scanner, const StreamForm &f, uint32_t chunk_seqs,
                                uint64_t chunk_bytes, uint32_t in_flight, kaamer_chunk_cb cb, void *user, kaamer_counters *total)
{
    if (!r || !path || chunk_seqs == 0 || (f.want_aln && !f.sub_matrix)) return kaamer_fail(KAAMER_E_ARG, "search_file: bad argument");
    SEQ_TYPE_CHK(f.seq_type, "search_file");
    if (total) memset(total, 0, sizeof *total);
    if (in_flight < 1) in_flight = 3;
    kaamer_reader *rd = nullptr;
    int rc = kaamer_reader_open(path, format, strict_scanner, &rd);
    if (rc) return rc;
    kaamer_replica_stream *rs = nullptr;
    rc = replica_stream_open_form(r, f, &rs);
    if (rc) { kaamer_reader_close(rd); return rc; }
    const ChunkFifo q = { rs, replica_fifo_push, replica_fifo_pop, replica_fifo_pending, in_flight * kaamer_replicas_count(r) };
    rc = search_file_loop(rd, q, chunk_seqs, chunk_bytes, cb, user, total);
    kaamer_replica_stream_close(rs);
    kaamer_reader_close(rd);
    return rc;
}

int kaamer_search_file(kaamer_replicas *r, const char *path, int format, int strict_scanner, int32_t seq_type, double min_k_ratio,
                       int64_t min_k_match, uint32_t max_results, uint32_t chunk_seqs, uint64_t chunk_bytes, uint32_t in_flight,
                       kaamer_chunk_cb cb, void *user, kaamer_counters *total)
{
    const StreamForm f = { seq_type, min_k_ratio, min_k_match, max_results, 0, 0, nullptr, 0, 0, 0 };
    return search_file_replicas(r, path, format, strict_scanner, f, chunk_seqs, chunk_bytes, in_flight, cb, user, total);
}

// the same with -pos (search.go:416,442-452) and -aln (search.go:483-494): `top` of the callback carries the chunk's bitmaps
// (kaamer_batch_top_positions) and alignments (kaamer_batch_top_alignments)
int kaamer_search_file_opts(kaamer_replicas *r, const char *path, int format, int strict_scanner, int32_t seq_type, double min_k_ratio,
                            int64_t min_k_match, uint32_t max_results, int32_t want_positions, int32_t want_aln, const char *sub_matrix,
                            int32_t gap_open, int32_t gap_extend, int32_t want_text, uint32_t chunk_seqs, uint64_t chunk_bytes, uint32_t in_flight,
                            kaamer_chunk_cb cb, void *user, kaamer_counters *total)
{
    const StreamForm f = { seq_type, min_k_ratio, min_k_match, max_results, want_positions, want_aln, sub_matrix, gap_open, gap_extend, want_text };
    return search_file_replicas(r, path, format, strict_scanner, f, chunk_seqs, chunk_bytes, in_flight, cb, user, total);
}
