// host_top.hip.inc — the pipelined host-buffer boundary (included by search.hip inside its extern "C" block).
//
// What a Go caller uses: host buffers in, the reported hits out (search_protein.go:105-112, search_fastq.go:118-126).
// The reference runs N worker goroutines against shared read-only stores (search_protein.go:58-118); here N callers run
// against one index concurrently, each call on its own SLOT (workspace + stream + pinned staging + result block):
//
//   kaamer_submit_batch_top   takes a free slot (blocks while all are busy), copies the caller's buffers into the
//                             slot's pinned staging (the caller's pointers are not kept), enqueues H2D -> search ->
//                             top-N -> result block -> ONE D2H copy on the slot's stream, returns a ticket
//   kaamer_wait_batch_top     waits for the slot's stream, reads the block header, fetches what the speculative copy
//                             missed (rare after the first call), hands out the result as views of the pinned block
//   kaamer_search_batch_top   = submit + wait
//   kaamer_stream_*           a FIFO of tickets with fixed options: push chunk i+1 while chunk i is searched
//                             (configs[4]'s double-buffered host -> GPU streaming behind the C ABI)
// No per-call device allocation, no index-wide lock around the device work, one host synchronisation per call.

struct batch_top_owner {
    kaamer_batch_top pub;
    uint8_t *block = nullptr;  // everything pub points to
    size_t block_cap = 0;
    bool pinned = true;        // from the pinned cache (else malloc: the interleaved result of a sharded index)
    bool has_pos = false;      // the block carries the bitmap sections (RepPosExt, topn.hip.inc)
    // ... or, in the interleaved result of a sharded index (no RepBlockHdr), the three arrays are at these places
    const int32_t *m_pos_len = nullptr;
    const uint64_t *m_pos_off = nullptr, *m_pos_bits = nullptr;
    // the alignments of the reported hits (host_top_align.hip.inc), parallel to the CSR entries
    bool has_aln = false, has_text = false;
    std::vector<kaamer_alignment> aln;
    std::vector<char> aln_text;
    // the records of a text call (host_text.hip.inc): one span each, pinned
    kaamer_text_span *spans = nullptr;
    size_t spans_cap = 0;
    uint32_t n_spans = 0;
    // the text of a BGZF call, inflated on the device and brought back with the result (the spans index it): pinned
    char *text = nullptr;
    size_t text_cap = 0;
    uint64_t text_len = 0;
    // the response text of a *_tsv_flat / *_json_flat call (host_out_text.hip.inc), pinned: the offsets of its rows or objects
    // (out_units + 1 of them), then the text
    OutFormat out_fmt = OUT_PLAIN;
    uint8_t *out = nullptr;
    size_t out_cap = 0;
    uint64_t out_units = 0, out_len = 0;
    const char *out_text = nullptr;
};

// the alignment half of a request (kaamer_*_batch_top_aln_flat)
struct TopAlnRequest {
    bool on = false;               // the options have a row in AllMatrixScores and name BLOSUM62
    double lambda = 0, kk = 0;
    int32_t gap_open = 0, gap_extend = 0;
    bool text = false;
};

static TopAlnRequest top_aln_request(const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text)
{
    TopAlnRequest rq;
    rq.on = kaamer_align_options(sub_matrix, gap_open, gap_extend, &rq.lambda, &rq.kk);
    rq.gap_open = gap_open; rq.gap_extend = gap_extend; rq.text = want_text != 0;
    return rq;
}

// residues of the batch's longest query (a bound for ORFs): sizes the direction slabs
static uint32_t batch_max_query_len(const kaamer_batch_in *in)
{
    uint64_t longest = 0;
    for (uint32_t i = 0; i < in->n_seqs; i++)
        if (in->offsets[i + 1] >= in->offsets[i] && in->offsets[i + 1] - in->offsets[i] > longest) longest = in->offsets[i + 1] - in->offsets[i];
    if (is_nucl(in->seq_type)) longest = longest / 3 + 2;   // an ORF holds at most a frame's codons
    return longest > 0x3FFFFFFFull ? 0x3FFFFFFFu : (uint32_t)longest;
}

struct kaamer_ticket {
    kaamer_index *ix;
    int slot;
    uint32_t n_seqs;
    int32_t seq_type;
    uint64_t seq_bytes;
    kaamer_topn_opts top;
    uint8_t *h_block;
    size_t h_block_cap, copied;
    BatchBounds b;
    int attempt;
    bool want_pos;   // PositionHits of the reported hits ride in the block (the *_pos_flat calls)
    bool want_aln;   // the alignments of the reported hits ride in the block (the *_aln_flat calls)
    TopAlnRequest aln;
    uint32_t max_query_len;   // batch_max_query_len
    uint64_t aln_cap;         // bytes the block's two sections may take
    // a text call (host_text.hip.inc): the batch is what the slot's parser left on the device, nothing is uploaded
    bool text;
    const uint8_t *d_text_seqs;
    const uint64_t *d_text_off;
    kaamer_text_span *h_spans;   // pinned; goes to the result
    size_t h_spans_cap;
    char *h_text_out;            // a BGZF call: the inflated text, pinned; goes to the result
    size_t h_text_out_cap;
    uint64_t text_len;
    // a call that returns response text (host_out_text.hip.inc; text calls only): the format and the request (out_pos:
    // ExtractPositions, out_ann: Annotations, json_fasta: the records are FASTA), the names on the device, the bounds of this
    // attempt (bytes; rows or objects; 0: the slot's guess) and the pinned buffer that goes to the result
    OutFormat out_fmt;
    bool out_pos, out_ann, json_fasta;
    const uint8_t *d_names;
    uint64_t names_len;
    const kaamer_text_span *d_spans;
    uint64_t out_bytes_cap, out_units_cap;
    uint8_t *h_out;
    size_t h_out_cap;
};
// the pinned buffers a ticket still holds (those that went to a result are NULL by then) back to the cache
static void ticket_put_pinned(kaamer_ticket *t)
{
    if (t->h_block) pinned_put(t->h_block, t->h_block_cap);
    if (t->h_spans) pinned_put(t->h_spans, t->h_spans_cap);
    if (t->h_text_out) pinned_put(t->h_text_out, t->h_text_out_cap);
    if (t->h_out) pinned_put(t->h_out, t->h_out_cap);
}
static int top_enqueue_out(kaamer_ticket *t, TopSlot &h, const kaamer_topn_result *tr, hipStream_t s);
static int out_needs_repeat(kaamer_ticket *t, TopSlot &h, int *rc);
static void out_finish_host(kaamer_ticket *t, TopSlot &h, batch_top_owner *bo);
static int tsv_aln_host_rows(kaamer_ticket *t, TopSlot &h, batch_top_owner *bo);
extern "C" void kaamer_json_stage_free(kaamer_json_stage *st);
static int top_enqueue_alignments(kaamer_ticket *t, TopSlot &h, const kaamer_topn_result *tr, hipStream_t s);
static uint64_t ta_first_cap(const kaamer_ticket *t, const TopSlot &h);
static int ta_needs_repeat(kaamer_ticket *t, TopSlot &h);
static int ta_finish_host(const kaamer_ticket *t, const TopSlot &h, batch_top_owner *bo);

// upper bound of the result block of a batch searched on `ws`, whose queries belong to `src` (ws itself, or the
// workspace that translated the batch: merged results of a sharded index)
static size_t rep_block_bound(const kaamer_workspace *ws, const kaamer_workspace *src, uint32_t K, uint64_t pos_words = 0)
{
    const size_t nq = ws->q_cap;
    // the bitmap sections: bit length per query, CSR per entry, the words
    const size_t pos = pos_words ? nq * 4 + 8 + (nq * (size_t)K + 1) * 8 + (size_t)pos_words * 8 : 0;
    return pos + sizeof(RepBlockHdr) + nq * (4 + 4 + sizeof(kaamer_query_meta) + 8) + 64 + nq * (size_t)K * 12 + (src->nucleotide ? (size_t)src->aa_cap + 64 : 0) + 64;
}

// packs the reported queries of the last kaamer_topn_device call on `ws` into `d_block` (topn.hip.inc); `src`: the
// workspace whose queries the results belong to (result i = its query q_first + i q_stride)
static int topn_pack_block(kaamer_workspace *ws, const kaamer_workspace *src, uint32_t q_first, uint32_t q_stride,
                           const kaamer_topn_result *tr, hipStream_t s, uint8_t *d_block, size_t block_cap)
{
    {   // (q_cap is fixed per workspace: the group is made at the first call)
        const size_t qc = ws->q_cap;
        const int rc = reserve_group(s, GROW_EXACT, { want(ws->d_rep_flag, qc), want(ws->d_rep_aalen, qc), want(ws->d_rep_rank, qc + 1),
                                                      want(ws->d_rep_eoff, qc + 1), want(ws->d_rep_aoff, qc + 1) });
        if (rc) return rc;
    }
    RepParams p;
    memset(&p, 0, sizeof p);
    p.d_nq = ws->d_nq; p.q = src->d_q; p.q_first = q_first; p.q_stride = q_stride ? q_stride : 1u;
    p.top_cnt = tr->d_top_cnt;
    p.trim = tr->d_trim; p.start_pos = tr->d_start_position; p.size_out = tr->d_size_in_kmer;
    p.K = tr->max_results;
    p.top_pid = tr->d_top_pid; p.top_km = tr->d_top_kmatch; p.top_fp = tr->d_top_first_pos;
    p.orf_aa = src->nucleotide ? src->d_orf_aa : nullptr;
    p.flag = ws->d_rep_flag; p.aalen = ws->d_rep_aalen;
    p.rank = ws->d_rep_rank; p.eoff = ws->d_rep_eoff; p.aoff = ws->d_rep_aoff;
    p.block = d_block; p.block_cap = block_cap;
    p.ctr = ws->d_counters; p.status_out = ws->d_status_out;
    const uint64_t bound = ws->q_cap;
    hipLaunchKernelGGL(rep_flags_kernel, dim3(ws->n_cu * 4), dim3(256), 0, s, p);
    scan_u32_on(ws, ws->d_rep_flag, ws->d_nq, bound, ws->d_rep_rank, s);
    scan_u32_on(ws, tr->d_top_cnt, ws->d_nq, bound, ws->d_rep_eoff, s);
    scan_u32_on(ws, ws->d_rep_aalen, ws->d_nq, bound, ws->d_rep_aoff, s);
    hipLaunchKernelGGL(rep_block_kernel, dim3(ws->n_cu * 8), dim3(256), 0, s, p);
    HIPCHK(hipGetLastError());
    return KAAMER_OK;
}

// the bitmaps of the reported hits behind the sections topn_pack_block just laid out (top_positions.hip.inc); a block
// that cannot hold them gets ST_POS_CAP in its header: the caller repeats the batch with a larger bound
static int topn_pack_positions(kaamer_index *ix, kaamer_workspace *ws, const kaamer_topn_result *tr, hipStream_t s, uint8_t *d_block,
                               size_t block_cap, uint64_t pos_words)
{
    int rc = tp_check(ix, ws, tr, "search_batch_top_pos");
    if (!rc) rc = tp_prepare(ws);
    if (rc) return rc;
    TopPosParams p = tp_params(ix, ws, tr);
    p.cap = pos_words;
    p.block = d_block; p.block_cap = block_cap;
    p.rank = ws->d_rep_rank; p.eoff = ws->d_rep_eoff; p.aoff = ws->d_rep_aoff;
    tp_enqueue_layout(ws, p, s);
    hipLaunchKernelGGL(top_pos_bits_kernel, dim3(ws->n_cu * 8), dim3(64 * TP_WAVES), 0, s, p);
    HIPCHK(hipGetLastError());
    return KAAMER_OK;
}

// a pinned block -> the public result (views into the block)
static void top_owner_fill(batch_top_owner *bo)
{
    const RepBlockHdr *h = reinterpret_cast<const RepBlockHdr *>(bo->block);
    memset(&bo->pub, 0, sizeof bo->pub);
    bo->pub.n_queries = h->n_queries;
    bo->pub.n_reported = h->n_rep;
    bo->pub.rep_query = reinterpret_cast<const uint32_t *>(bo->block + h->off_rep_query);
    bo->pub.trim = reinterpret_cast<const int32_t *>(bo->block + h->off_trim);
    bo->pub.q = reinterpret_cast<const kaamer_query_meta *>(bo->block + h->off_q);
    bo->pub.top_off = reinterpret_cast<const uint64_t *>(bo->block + h->off_top_off);
    bo->pub.top_pid = reinterpret_cast<const uint32_t *>(bo->block + h->off_pid);
    bo->pub.top_kmatch = reinterpret_cast<const uint32_t *>(bo->block + h->off_km);
    bo->pub.top_first_pos = reinterpret_cast<const uint32_t *>(bo->block + h->off_fp);
    bo->pub.orf_aa = bo->block + h->off_aa;
    bo->pub.counters = h->counters;
}

// The host protocol of a packed block, on both handles: copy a guess -- as much as the previous call's block took (plus a
// quarter), never more than the `usable` bytes of d_block -- into a pinned block, read the header once the stream is done
// (the caller), fetch the rest only when the guess was short.
static int rep_block_copy_guess(const uint8_t *d_block, size_t usable, size_t guess, uint8_t **h_block, size_t *h_block_cap, size_t *copied, hipStream_t s)
{
    size_t want = guess < sizeof(RepBlockHdr) ? sizeof(RepBlockHdr) : guess;
    if (want > usable) want = usable;
    if (*h_block_cap < want) {
        if (*h_block) pinned_put(*h_block, *h_block_cap);
        *h_block = (uint8_t *)pinned_get(want, h_block_cap);
        if (!*h_block) { *h_block_cap = 0; return kaamer_fail(KAAMER_E_NOMEM, "pinned result block (%zu bytes)", want); }
    }
    const hipError_t e = hipMemcpyAsync(*h_block, d_block, want, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(e));
    *copied = want;
    return KAAMER_OK;
}

// ... the header (in *h_block) is fine: what the guess missed, and the next call's guess
static int rep_block_fetch_rest(const uint8_t *d_block, size_t *guess, uint8_t **h_block, size_t *h_block_cap, size_t *copied, hipStream_t s)
{
    const size_t total = (size_t)reinterpret_cast<const RepBlockHdr *>(*h_block)->total_bytes;
    *guess = total + total / 4 + 4096;
    if (total <= *copied) return KAAMER_OK;
    size_t cap = 0;
    uint8_t *nb = (uint8_t *)pinned_get(total, &cap);
    if (!nb) return kaamer_fail(KAAMER_E_NOMEM, "pinned result block (%zu bytes)", total);
    memcpy(nb, *h_block, *copied);
    hipError_t e = hipMemcpyAsync(nb + *copied, d_block + *copied, total - *copied, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    pinned_put(*h_block, *h_block_cap);
    *h_block = nb; *h_block_cap = cap;
    if (e != hipSuccess) return kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(e));
    *copied = total;
    return KAAMER_OK;
}

static int status_to_error(uint32_t status, const kaamer_workspace *ws)
{
    if (!status) return KAAMER_OK;
    if (status & ST_CHAIN_TIMEOUT) return kaamer_fail(KAAMER_E_HIP, "table layout: a tile never published its total");
    if (status & (ST_QUERY_CAP | ST_AA_CAP)) return kaamer_fail(KAAMER_E_CAPACITY, "more ORFs than the workspace holds (max_queries %u)", ws->q_cap);
    return kaamer_fail(KAAMER_E_CAPACITY, "a workspace bound was exceeded (device status 0x%x)", status);
}

static void top_slot_release(kaamer_index *ix, int slot)
{
    {
        std::lock_guard<std::mutex> lock(ix->pool_mu);
        ix->top[slot].busy = false;
    }
    ix->pool_cv.notify_all();   // (two kinds of waiters share the condition: slots of this pool and of kaamer_search_batch's)
}

static void top_slot_free(TopSlot &h)
{
    if (h.ws) kaamer_workspace_free(h.ws);
    if (h.parser) kaamer_text_parser_free(h.parser);
    if (h.inflater) kaamer_inflater_free(h.inflater);
    if (h.tsv) kaamer_tsv_stage_free(h.tsv);
    if (h.json) kaamer_json_stage_free(h.json);
    if (h.stream) (void)hipStreamDestroy(h.stream);
    h = TopSlot();   // (its buffers go here)
}

// the pinned staging of a packed batch: the sequences, then (8-byte aligned) the n_seqs + 1 offsets
static int top_slot_staging(TopSlot &h, uint64_t seq_bytes, uint32_t n_seqs)
{
    const size_t in_need = (((size_t)seq_bytes + 7) & ~(size_t)7) + ((size_t)n_seqs + 1) * 8;
    return reserve(h.h_in, in_need, GROW_SLOT, h.stream);
}

// workspace, staging and result block of a slot: rebuilt only when the batch outgrows them
static int top_slot_prepare(kaamer_index *ix, TopSlot &h, const kaamer_workspace_opts &need, uint64_t seq_bytes, uint32_t n_seqs, uint32_t K,
                            bool want_pos = false, uint32_t pos_scale = 0, uint64_t aln_bytes = 0)
{
    if (!h.stream) HIPCHK(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
    const kaamer_workspace_opts &o = h.opts;
    const bool fits = h.ws && o.seq_type == need.seq_type && o.max_seq_bytes >= need.max_seq_bytes && o.max_seqs >= need.max_seqs &&
                      o.max_hits >= need.max_hits && o.g_tier_slots >= need.g_tier_slots && o.max_queries >= need.max_queries &&
                      (need.max_hits != 0 || o.max_hits == 0);
    if (!fits) {
        if (h.ws) { HIPCHK(hipStreamSynchronize(h.stream)); kaamer_workspace_free(h.ws); h.ws = nullptr; }
        kaamer_workspace_opts g = need;  // some headroom so that slightly larger batches do not rebuild it
        g.max_seq_bytes = need.max_seq_bytes + need.max_seq_bytes / 4 + 4096;
        g.max_seqs = need.max_seqs + need.max_seqs / 4 + 16;
        if (need.max_hits) g.max_hits = need.max_hits + need.max_hits / 4;
        const int rc = kaamer_workspace_create(ix, &g, &h.ws);
        if (rc) { h.ws = nullptr; return rc; }
        h.opts = g;
    }
    int rc = reserve(h.d_seqs, (size_t)seq_bytes, GROW_SLOT_SEQS, h.stream);
    if (!rc) rc = reserve(h.d_off, (size_t)n_seqs, GROW_SLOT_OFF, h.stream);
    if (!rc) rc = top_slot_staging(h, seq_bytes, n_seqs);
    if (rc) return rc;
    // the bitmap bound (the rule next to kaamer_topn_positions_device); a first bound set on the index holds for the
    // first attempt only: the repeat of a batch that exceeded it takes the rule's
    h.pos_words = 0;
    if (want_pos) {
        uint64_t first = 0;
        { std::lock_guard<std::mutex> lock(ix->pool_mu); first = ix->top_pos_words; }
        const uint64_t hard = tp_hard_words(h.ws, K);
        h.pos_words = (first && pos_scale <= 1) ? (first < hard ? first : hard) : tp_default_words(h.ws, K, pos_scale);
    }
    const size_t bneed = rep_block_bound(h.ws, h.ws, K, h.pos_words) + (aln_bytes ? (size_t)aln_bytes + 64 : 0);
    h.block_use = bneed;
    return reserve(h.d_block, bneed, GROW_EXACT, h.stream);
}

// everything of one call onto the slot's stream; the inputs are in the slot's pinned staging
static int top_enqueue(kaamer_ticket *t)
{
    kaamer_index *ix = t->ix;
    TopSlot &h = ix->top[t->slot];
    const bool nucl = is_nucl(t->seq_type);
    kaamer_workspace_opts o;
    memset(&o, 0, sizeof o);
    o.max_seq_bytes = t->seq_bytes;
    o.max_seqs = t->n_seqs ? t->n_seqs : 1;
    o.max_hits = t->b.max_hits;
    o.g_tier_slots = t->b.g_slots;
    o.seq_type = seq_base(t->seq_type);
    o.first_pos = 0;  // as the reference fills PositionHits: nucleotide / reads input only (search.go:416)
    o.max_queries = t->b.max_queries;
    o.concurrent_batches = (uint32_t)ix->n_top;   // the slots exist so that batches overlap
    const bool aligns = t->want_aln && t->aln.on;   // (without a matrix row nothing is aligned: the host marks every item)
    if (aligns && !t->aln_cap) t->aln_cap = ta_first_cap(t, h);
    // (a text call stages nothing: its batch is on the device already)
    int rc = top_slot_prepare(ix, h, o, t->text ? 0 : t->seq_bytes, t->text ? 0 : t->n_seqs, t->top.max_results, t->want_pos, t->b.pos_scale,
                              aligns ? t->aln_cap : 0);
    if (rc) return rc;
    hipStream_t s = h.stream;
    const uint8_t *d_seqs = h.d_seqs;
    const uint64_t *d_off = h.d_off;
    if (t->text) {
        d_seqs = t->d_text_seqs; d_off = t->d_text_off;
    } else {
        const size_t off_at = ((size_t)t->seq_bytes + 7) & ~(size_t)7;
        hipError_t e = hipSuccess;
        if (t->seq_bytes) e = hipMemcpyAsync(h.d_seqs, h.h_in, (size_t)t->seq_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h.d_off, h.h_in + off_at, ((size_t)t->n_seqs + 1) * 8, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return kaamer_fail(KAAMER_E_HIP, "H2D: %s", hipGetErrorString(e));
    }
    kaamer_device_result dr;
    kaamer_topn_result tr;
    kaamer_topn_opts top = t->top;
    top.best_start_codon = nucl ? 1u : 0u;  // search_fastq.go:121, search_nucleotide.go:118; not in search_protein.go
    top.d_size_in_kmer = nullptr; top.orf_source = nullptr;
    rc = kaamer_search_device(ix, h.ws, d_seqs, d_off, t->n_seqs, t->seq_bytes, t->seq_type, s, &dr);
    if (!rc) rc = kaamer_topn_device(h.ws, &top, s, &tr);
    if (!rc) rc = topn_pack_block(h.ws, h.ws, 0u, 1u, &tr, s, h.d_block, h.block_use);
    if (!rc && t->want_pos) rc = topn_pack_positions(ix, h.ws, &tr, s, h.d_block, h.block_use, h.pos_words);
    if (!rc && aligns) rc = top_enqueue_alignments(t, h, &tr, s);
    if (!rc && t->out_fmt) rc = top_enqueue_out(t, h, &tr, s);
    if (rc) return rc;
    return rep_block_copy_guess(h.d_block, h.block_use, h.guess, &t->h_block, &t->h_block_cap, &t->copied, s);
}

// a free slot of the pool, marked busy; blocking: waits while all are busy, else KAAMER_E_BUSY
static int top_slot_take(kaamer_index *ix, bool blocking, int *slot_out)
{
    int slot = -1;
    std::unique_lock<std::mutex> lock(ix->pool_mu);
    for (;;) {
        for (int i = 0; i < ix->n_top; i++)
            if (!ix->top[i].busy) { slot = i; break; }
        if (slot >= 0) break;
        if (!blocking) return kaamer_fail(KAAMER_E_BUSY, "all %d host slots are busy: wait for / pop an earlier batch first", ix->n_top);
        ix->pool_cv.wait(lock);
    }
    ix->top[slot].busy = true;
    *slot_out = slot;
    return KAAMER_OK;
}

static int top_submit(kaamer_index *ix, const kaamer_batch_in *in, const kaamer_topn_opts *top, bool blocking, kaamer_ticket **out,
                      bool want_pos = false, const TopAlnRequest *aln = nullptr)
{
    if (!ix || !in || !top || !out || !in->offsets || (in->n_seqs && !in->seqs) || top->max_results < 1)
        return kaamer_fail(KAAMER_E_ARG, "submit_batch_top: bad argument");
    *out = nullptr;
    SEQ_TYPE_CHK(in->seq_type, "submit_batch_top");
    int slot = -1;
    const int src = top_slot_take(ix, blocking, &slot);
    if (src) return src;
    kaamer_ticket *t = new (std::nothrow) kaamer_ticket();
    if (!t) { top_slot_release(ix, slot); return kaamer_fail(KAAMER_E_NOMEM, "ticket"); }
    memset(t, 0, sizeof *t);
    t->ix = ix; t->slot = slot; t->n_seqs = in->n_seqs; t->seq_type = in->seq_type; t->seq_bytes = in->offsets[in->n_seqs];
    t->top = *top;
    t->want_pos = want_pos;
    if (aln) {
        t->want_aln = true; t->aln = *aln;
        t->max_query_len = batch_max_query_len(in);
    }
    int rc = KAAMER_OK;
    hipError_t he = hipSetDevice(ix->device);
    if (he != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "hipSetDevice: %s", hipGetErrorString(he));
    if (!rc) {
        // the caller's buffers are only borrowed for this call: into the slot's pinned staging now.  (Sizing the staging
        // is part of top_slot_prepare, which needs the workspace options: a first pass with the default bounds.)
        TopSlot &h = ix->top[slot];
        const size_t off_at = ((size_t)t->seq_bytes + 7) & ~(size_t)7;
        rc = top_slot_staging(h, t->seq_bytes, in->n_seqs);
        if (!rc) {
            if (t->seq_bytes) memcpy(h.h_in, in->seqs, (size_t)t->seq_bytes);
            memcpy(h.h_in + off_at, in->offsets, ((size_t)in->n_seqs + 1) * 8);
            rc = top_enqueue(t);
        }
    }
    if (rc) {
        // part of the call may be on the slot's stream already (copies out of the pinned staging the next caller overwrites)
        if (ix->top[slot].stream) (void)hipStreamSynchronize(ix->top[slot].stream);
        ticket_put_pinned(t);
        delete t;
        top_slot_release(ix, slot);
        return rc;
    }
    *out = t;
    return KAAMER_OK;
}

int kaamer_submit_batch_top(kaamer_index *ix, const kaamer_batch_in *in, const kaamer_topn_opts *top, kaamer_ticket **ticket)
{
    return top_submit(ix, in, top, true, ticket);
}

int kaamer_wait_batch_top(kaamer_ticket *t, kaamer_batch_top **out)
{
    if (!t || !out) return kaamer_fail(KAAMER_E_ARG, "wait_batch_top: bad argument");
    *out = nullptr;
    kaamer_index *ix = t->ix;
    TopSlot &h = ix->top[t->slot];
    const bool nucl = is_nucl(t->seq_type);
    int rc = KAAMER_OK;
    hipError_t e = hipSetDevice(ix->device);
    if (e != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
    while (!rc) {
        e = hipStreamSynchronize(h.stream);
        if (e != hipSuccess) { rc = kaamer_fail(KAAMER_E_HIP, "stream: %s", hipGetErrorString(e)); break; }
        const RepBlockHdr *hdr = reinterpret_cast<const RepBlockHdr *>(t->h_block);
        const uint32_t status = hdr->status & 0x7FFFFFFFu;
        if (status) h.ws->clean = false;  // an aborted batch may leave per-batch state behind
        rc = status_to_error(status, h.ws);
        if (!rc && (hdr->status & 0x80000000u)) rc = kaamer_fail(KAAMER_E_CAPACITY, "result block capacity exceeded");
        if (rc == KAAMER_E_CAPACITY && t->attempt < MAX_BOUND_RETRIES) {
            // enlarge the bounds and run the batch again from the staging copy
            t->attempt++;
            bounds_grow(t->b, t->seq_bytes, t->n_seqs, nucl);
            rc = top_enqueue(t);   // (an error here ends the loop, E_CAPACITY included: kept as it was)
            continue;
        }
        if (rc) break;
        if (t->want_aln && t->aln.on && ta_needs_repeat(t, h)) {   // the alignment sections were too small: once more, with what they needed
            if (t->attempt >= MAX_BOUND_RETRIES + 2) { rc = kaamer_fail(KAAMER_E_CAPACITY, "alignment sections of the result block"); break; }
            t->attempt++;
            rc = top_enqueue(t);
            continue;
        }
        if (t->out_fmt && out_needs_repeat(t, h, &rc)) {   // the response text's bounds were too small: once more, with what it needed
            if (t->attempt >= MAX_BOUND_RETRIES + 2) { rc = kaamer_fail(KAAMER_E_CAPACITY, "%s of the result", t->out_fmt == OUT_TSV ? "TSV rows" : "JSON objects"); break; }
            t->attempt++;
            rc = top_enqueue(t);
            continue;
        }
        if (rc) break;
        rc = rep_block_fetch_rest(h.d_block, &h.guess, &t->h_block, &t->h_block_cap, &t->copied, h.stream);
        break;
    }
    batch_top_owner *bo = nullptr;
    if (!rc) {
        bo = new (std::nothrow) batch_top_owner();
        if (!bo) rc = kaamer_fail(KAAMER_E_NOMEM, "batch_top");
    }
    if (!rc) {
        bo->block = t->h_block; bo->block_cap = t->h_block_cap;
        t->h_block = nullptr;
        top_owner_fill(bo);
        if (ix->top[t->slot].ws) ws_note_density(ix->top[t->slot].ws, bo->pub.counters);
        bo->pub.max_results = t->top.max_results;
        bo->has_pos = t->want_pos;
        if (t->text) { bo->spans = t->h_spans; bo->spans_cap = t->h_spans_cap; bo->n_spans = t->n_seqs; t->h_spans = nullptr; }
        if (t->h_text_out) { bo->text = t->h_text_out; bo->text_cap = t->h_text_out_cap; bo->text_len = t->text_len; t->h_text_out = nullptr; }
        if (t->out_fmt) out_finish_host(t, h, bo);
        if (t->want_aln) rc = ta_finish_host(t, h, bo);   // (reads protein queries from the slot's staging: before the release)
        if (!rc && t->want_aln && t->out_fmt == OUT_TSV) rc = tsv_aln_host_rows(t, h, bo);   // (only a batch the stage flagged)
        if (!nucl) bo->pub.orf_aa = nullptr;
        if (!rc) *out = &bo->pub;
        else kaamer_batch_top_free(&bo->pub);
    }
    ticket_put_pinned(t);
    top_slot_release(ix, t->slot);
    delete t;
    return rc;
}

// a ticket nobody will wait for (the caller gave up between submit and wait): the batch is let run out, its result
// dropped, the slot and the pinned block given back
void kaamer_ticket_discard(kaamer_ticket *t)
{
    if (!t) return;
    kaamer_index *ix = t->ix;
    (void)hipSetDevice(ix->device);
    TopSlot &h = ix->top[t->slot];
    if (h.stream) (void)hipStreamSynchronize(h.stream);
    if (h.ws) h.ws->clean = false;  // its status was not looked at: the next batch starts from cleared per-batch state
    ticket_put_pinned(t);
    top_slot_release(ix, t->slot);
    delete t;
}

static void stream_set_positions(kaamer_stream *st);
static void flat_in(kaamer_batch_in *in, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type, int32_t want_positions)
{
    memset(in, 0, sizeof *in);
    in->seqs = seqs; in->offsets = offsets; in->n_seqs = n_seqs; in->seq_type = seq_type; in->want_positions = want_positions;
}
static void flat_top(kaamer_topn_opts *top, double min_k_ratio, int64_t min_k_match, uint32_t max_results)
{
    memset(top, 0, sizeof *top);
    top->min_k_ratio = min_k_ratio; top->min_k_match = min_k_match; top->max_results = max_results;
}

int kaamer_submit_batch_top_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                 double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket)
{
    kaamer_batch_in in;
    kaamer_topn_opts top;
    flat_in(&in, seqs, offsets, n_seqs, seq_type, 0);
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    return top_submit(ix, &in, &top, true, ticket);
}

int kaamer_search_batch_top_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                 double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_ticket *t = nullptr;
    const int rc = kaamer_submit_batch_top_flat(ix, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, &t);
    if (rc) return rc;
    return kaamer_wait_batch_top(t, out);
}

// ---- the same calls with the PositionHits bitmaps of the reported hits in the block (search.go:442-452,520-522) ----
int kaamer_submit_batch_top_pos_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                     double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket)
{
    kaamer_batch_in in;
    kaamer_topn_opts top;
    flat_in(&in, seqs, offsets, n_seqs, seq_type, 1);
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    return top_submit(ix, &in, &top, true, ticket, true);
}

int kaamer_search_batch_top_pos_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                     double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_ticket *t = nullptr;
    const int rc = kaamer_submit_batch_top_pos_flat(ix, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, &t);
    if (rc) return rc;
    return kaamer_wait_batch_top(t, out);
}

int kaamer_batch_top_positions(const kaamer_batch_top *out, const int32_t **pos_bits_len, const uint64_t **pos_off, const uint64_t **pos_bits)
{
    if (pos_bits_len) *pos_bits_len = nullptr;
    if (pos_off) *pos_off = nullptr;
    if (pos_bits) *pos_bits = nullptr;
    if (!out) return kaamer_fail(KAAMER_E_ARG, "batch_top_positions: bad argument");
    const batch_top_owner *bo = reinterpret_cast<const batch_top_owner *>(out);  // pub is the first member
    if (!bo->has_pos || !bo->block) return KAAMER_OK;   // not asked for positions: all NULL
    if (bo->m_pos_off) {
        if (pos_bits_len) *pos_bits_len = bo->m_pos_len;
        if (pos_off) *pos_off = bo->m_pos_off;
        if (pos_bits) *pos_bits = bo->m_pos_bits;
        return KAAMER_OK;
    }
    const RepPosExt *x = rep_pos_ext(reinterpret_cast<const RepBlockHdr *>(bo->block));
    if (!x->off_pos_bits) return KAAMER_OK;
    if (pos_bits_len) *pos_bits_len = reinterpret_cast<const int32_t *>(bo->block + x->off_pos_len);
    if (pos_off) *pos_off = reinterpret_cast<const uint64_t *>(bo->block + x->off_pos_off);
    if (pos_bits) *pos_bits = reinterpret_cast<const uint64_t *>(bo->block + x->off_pos_bits);
    return KAAMER_OK;
}

int kaamer_search_batch_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                             int32_t want_positions, kaamer_batch_out **out)
{
    kaamer_batch_in in;
    flat_in(&in, seqs, offsets, n_seqs, seq_type, want_positions);
    return kaamer_search_batch(ix, &in, out);
}

int kaamer_stream_open_flat(kaamer_index *ix, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_stream **out)
{
    kaamer_topn_opts top;
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    return kaamer_stream_open(ix, seq_type, &top, out);
}

int kaamer_stream_open_pos_flat(kaamer_index *ix, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_stream **out)
{
    const int rc = kaamer_stream_open_flat(ix, seq_type, min_k_ratio, min_k_match, max_results, out);
    if (!rc) stream_set_positions(*out);
    return rc;
}

int kaamer_search_batch_top(kaamer_index *ix, const kaamer_batch_in *in, const kaamer_topn_opts *top, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_ticket *t = nullptr;
    const int rc = top_submit(ix, in, top, true, &t);
    if (rc) return rc;
    return kaamer_wait_batch_top(t, out);
}

void kaamer_batch_top_free(kaamer_batch_top *out)
{
    if (!out) return;
    batch_top_owner *bo = reinterpret_cast<batch_top_owner *>(out);  // pub is the first member
    if (bo->block) { if (bo->pinned) pinned_put(bo->block, bo->block_cap); else free(bo->block); }
    if (bo->spans) pinned_put(bo->spans, bo->spans_cap);
    if (bo->text) pinned_put(bo->text, bo->text_cap);
    if (bo->out) pinned_put(bo->out, bo->out_cap);
    delete bo;
}

// ---- streaming: a FIFO of tickets --------------------------------------------------------------------
struct kaamer_stream {
    kaamer_index *ix;
    int32_t seq_type;
    kaamer_topn_opts top;
    std::vector<kaamer_ticket *> *fifo;
    bool want_pos;
    bool want_aln;       // kaamer_stream_open_aln_flat (host_top_align.hip.inc): every chunk is a TopAlnRequest
    TopAlnRequest aln;
};
static void stream_set_positions(kaamer_stream *st) { st->want_pos = true; }

int kaamer_stream_open(kaamer_index *ix, int32_t seq_type, const kaamer_topn_opts *top, kaamer_stream **out)
{
    if (!ix || !top || !out || top->max_results < 1) return kaamer_fail(KAAMER_E_ARG, "stream_open: bad argument");
    *out = nullptr;
    SEQ_TYPE_CHK(seq_type, "stream_open");
    kaamer_stream *st = new (std::nothrow) kaamer_stream();
    if (!st) return kaamer_fail(KAAMER_E_NOMEM, "stream");
    st->ix = ix; st->seq_type = seq_type; st->top = *top; st->want_pos = false; st->want_aln = false;
    st->fifo = new (std::nothrow) std::vector<kaamer_ticket *>();
    if (!st->fifo) { delete st; return kaamer_fail(KAAMER_E_NOMEM, "stream"); }
    *out = st;
    return KAAMER_OK;
}

int kaamer_stream_push(kaamer_stream *st, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs)
{
    if (!st || !offsets) return kaamer_fail(KAAMER_E_ARG, "stream_push: bad argument");
    kaamer_batch_in in;
    memset(&in, 0, sizeof in);
    in.seqs = seqs; in.offsets = offsets; in.n_seqs = n_seqs; in.seq_type = st->seq_type;
    kaamer_ticket *t = nullptr;
    // never block on a slot this stream itself holds: when every slot is busy the caller pops first
    const int rc = top_submit(st->ix, &in, &st->top, st->fifo->empty(), &t, st->want_pos, st->want_aln ? &st->aln : nullptr);
    if (rc) return rc;
    st->fifo->push_back(t);
    return KAAMER_OK;
}

int kaamer_stream_pop(kaamer_stream *st, kaamer_batch_top **out)
{
    if (!st || !out) return kaamer_fail(KAAMER_E_ARG, "stream_pop: bad argument");
    *out = nullptr;
    if (st->fifo->empty()) return kaamer_fail(KAAMER_E_ARG, "stream_pop: nothing was pushed");
    kaamer_ticket *t = st->fifo->front();
    st->fifo->erase(st->fifo->begin());
    return kaamer_wait_batch_top(t, out);
}

uint32_t kaamer_stream_pending(const kaamer_stream *st) { return st ? (uint32_t)st->fifo->size() : 0u; }

void kaamer_stream_close(kaamer_stream *st)
{
    if (!st) return;
    for (kaamer_ticket *t : *st->fifo) {  // chunks nobody popped: finished and dropped
        kaamer_batch_top *o = nullptr;
        if (kaamer_wait_batch_top(t, &o) == KAAMER_OK) kaamer_batch_top_free(o);
    }
    delete st->fifo;
    delete st;
}
