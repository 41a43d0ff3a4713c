// host_sharded_stream.hip.inc — the stream and the whole-file driver on the one-process sharded handle (included by
// search.hip inside its extern "C" block, after host_replicas.hip.inc, whose file loop it calls).
//
// The reference's search is one server call over a file of any size, whatever the size of the database
// (search_fastq.go:60-136, search_protein.go:40-118, search_nucleotide.go:27-160), with -pos (search.go:416,442-452) and
// -aln (search.go:483-494).  A database larger than one device lives on a kaamer_sharded_index; here its per-batch calls
// get the drivers kaamer_stream_* and kaamer_search_file give an unsharded index: a FIFO of kaamer_sharded_ticket with
// fixed options, and the reader + that FIFO + one callback per chunk (BASELINE configs[3] behind the ABI).  Host code
// only: every chunk goes the way kaamer_sharded_submit_batch_top*_flat / kaamer_sharded_wait_batch_top go.
struct kaamer_sharded_stream {
    kaamer_sharded_index *sx = nullptr;
    int32_t seq_type = 0;
    kaamer_topn_opts top;
    bool want_pos = false, want_aln = false;
    TopAlnRequest aln;
    std::vector<kaamer_sharded_ticket *> *fifo = nullptr;
};

static int sharded_stream_open(kaamer_sharded_index *sx, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                               bool want_pos, const TopAlnRequest *aln, kaamer_sharded_stream **out)
{
    if (!sx || !out || max_results < 1) return kaamer_fail(KAAMER_E_ARG, "sharded_stream_open: bad argument");
    *out = nullptr;
    SEQ_TYPE_CHK(seq_type, "sharded_stream_open");
    kaamer_sharded_stream *st = new (std::nothrow) kaamer_sharded_stream();
    if (!st) return kaamer_fail(KAAMER_E_NOMEM, "sharded stream");
    st->sx = sx; st->seq_type = seq_type; st->want_pos = want_pos;
    flat_top(&st->top, min_k_ratio, min_k_match, max_results);
    if (aln) { st->want_aln = true; st->aln = *aln; }
    st->fifo = new (std::nothrow) std::vector<kaamer_sharded_ticket *>();
    if (!st->fifo) { delete st; return kaamer_fail(KAAMER_E_NOMEM, "sharded stream"); }
    *out = st;
    return KAAMER_OK;
}

int kaamer_sharded_stream_open_flat(kaamer_sharded_index *sx, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                    kaamer_sharded_stream **out)
{
    return sharded_stream_open(sx, seq_type, min_k_ratio, min_k_match, max_results, false, nullptr, out);
}

int kaamer_sharded_stream_open_pos_flat(kaamer_sharded_index *sx, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                        kaamer_sharded_stream **out)
{
    return sharded_stream_open(sx, seq_type, min_k_ratio, min_k_match, max_results, true, nullptr, out);
}

int kaamer_sharded_stream_open_aln_flat(kaamer_sharded_index *sx, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                        int32_t want_positions, const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text,
                                        kaamer_sharded_stream **out)
{
    if (!sx || !sub_matrix || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_stream_open_aln: bad argument");
    *out = nullptr;
    {
        std::lock_guard<std::mutex> lock(sx->mu);
        if (!sx->aln) return kaamer_fail(KAAMER_E_ARG, "sharded_stream_open_aln: no protein table is attached to the handle (kaamer_sharded_index_attach_proteins)");
    }
    const TopAlnRequest rq = top_aln_request(sub_matrix, gap_open, gap_extend, want_text);
    return sharded_stream_open(sx, seq_type, min_k_ratio, min_k_match, max_results, want_positions != 0, &rq, out);
}

// KAAMER_E_BUSY: every set of the handle holds a chunk (of this stream: at once, nothing is waited for; of other callers
// while this stream holds chunks of its own: likewise) -- pop first.  A stream that holds nothing waits for a set like
// every other caller of the handle.
int kaamer_sharded_stream_push(kaamer_sharded_stream *st, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs)
{
    if (!st || !offsets) return kaamer_fail(KAAMER_E_ARG, "sharded_stream_push: bad argument");
    if (st->fifo->size() >= KAAMER_SHARDED_SETS)
        return kaamer_fail(KAAMER_E_BUSY, "all %d sets of the handle hold chunks of this stream: pop first", KAAMER_SHARDED_SETS);
    kaamer_batch_in in;
    flat_in(&in, seqs, offsets, n_seqs, st->seq_type, st->want_pos ? 1 : 0);
    kaamer_sharded_ticket *t = nullptr;
    // never wait for a set this stream itself holds
    const int rc = sharded_submit_top(st->sx, &in, &st->top, st->want_pos, &t, st->want_aln ? &st->aln : nullptr, st->fifo->empty());
    if (rc) return rc;
    st->fifo->push_back(t);
    return KAAMER_OK;
}

// the oldest chunk's result; the retry with grown bounds stays inside kaamer_sharded_wait_batch_top
int kaamer_sharded_stream_pop(kaamer_sharded_stream *st, kaamer_batch_top **out)
{
    if (!st || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_stream_pop: bad argument");
    *out = nullptr;
    if (st->fifo->empty()) return kaamer_fail(KAAMER_E_ARG, "sharded_stream_pop: nothing was pushed");
    kaamer_sharded_ticket *t = st->fifo->front();
    st->fifo->erase(st->fifo->begin());   // (a failed chunk is consumed too: the FIFO stays aligned with the input)
    return kaamer_sharded_wait_batch_top(t, out);
}

uint32_t kaamer_sharded_stream_pending(const kaamer_sharded_stream *st) { return st ? (uint32_t)st->fifo->size() : 0u; }

void kaamer_sharded_stream_close(kaamer_sharded_stream *st)
{
    if (!st) return;
    for (kaamer_sharded_ticket *t : *st->fifo) kaamer_sharded_ticket_discard(t);   // chunks nobody popped: let run out, dropped
    delete st->fifo;
    delete st;
}

static int sharded_fifo_push(void *st, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs)
{
    return kaamer_sharded_stream_push(static_cast<kaamer_sharded_stream *>(st), seqs, offsets, n_seqs);
}
static int sharded_fifo_pop(void *st, kaamer_batch_top **out) { return kaamer_sharded_stream_pop(static_cast<kaamer_sharded_stream *>(st), out); }
static uint32_t sharded_fifo_pending(const void *st) { return kaamer_sharded_stream_pending(static_cast<const kaamer_sharded_stream *>(st)); }

// kaamer_search_file_opts on the sharded handle: the same reader, the same loop (search_file_loop), the same callback
int kaamer_sharded_search_file(kaamer_sharded_index *sx, const char *path, int format, int strict_scanner, int32_t seq_type, double min_k_ratio,
                               int64_t min_k_match, uint32_t max_results, int32_t want_positions, int32_t want_aln, const char *sub_matrix,
                               int32_t gap_open, int32_t gap_extend, int32_t want_text, uint32_t chunk_seqs, uint64_t chunk_bytes,
                               uint32_t in_flight, kaamer_chunk_cb cb, void *user, kaamer_counters *total)
{
    if (!sx || !path || chunk_seqs == 0 || (want_aln && !sub_matrix)) return kaamer_fail(KAAMER_E_ARG, "sharded_search_file: bad argument");
    SEQ_TYPE_CHK(seq_type, "sharded_search_file");
    if (total) memset(total, 0, sizeof *total);
    if (in_flight < 1) in_flight = 3;
    if (in_flight > KAAMER_SHARDED_SETS) in_flight = KAAMER_SHARDED_SETS;
    kaamer_reader *rd = nullptr;
    int rc = kaamer_reader_open(path, format, strict_scanner, &rd);
    if (rc) return rc;
    kaamer_sharded_stream *st = nullptr;
    if (want_aln) rc = kaamer_sharded_stream_open_aln_flat(sx, seq_type, min_k_ratio, min_k_match, max_results, want_positions, sub_matrix, gap_open,
                                                           gap_extend, want_text, &st);
    else rc = sharded_stream_open(sx, seq_type, min_k_ratio, min_k_match, max_results, want_positions != 0, nullptr, &st);
    if (rc) { kaamer_reader_close(rd); return rc; }
    const ChunkFifo q = { st, sharded_fifo_push, sharded_fifo_pop, sharded_fifo_pending, in_flight };
    rc = search_file_loop(rd, q, chunk_seqs, chunk_bytes, cb, user, total);
    kaamer_sharded_stream_close(st);
    kaamer_reader_close(rd);
    return rc;
}
