// host_text.hip.inc — the host-buffer boundary for callers that hold TEXT (included by search.hip inside its extern "C"
// block, after host_top.hip.inc): search_fastq.go:60-136 with the reader (search.go:324-412) on the device.
//
//   kaamer_submit_text_top_flat   takes a free slot, copies the caller's text into the slot's pinned staging, uploads it,
//                                 parses it on the slot's stream (parse_text.hip.inc), waits for the two counts, then
//                                 enqueues what kaamer_submit_batch_top_flat enqueues -- on the parser's buffers
//   kaamer_wait_batch_top         as for every ticket; the result carries the records' spans
//   kaamer_submit_bgzf_top_flat   the same call for whole BGZF blocks: the COMPRESSED bytes and the block table go up, the
//                                 slot's inflater (inflate.hip.inc) writes the text where the upload would have put it, and
//                                 the text comes back with the result (kaamer_batch_top_text), since the caller never had it
// The slot's parser starts from an estimate of the record count and, as every other bound of these calls, grows when the
// device reports KAAMER_E_CAPACITY: the text is on the device by then, only the parse is repeated.

// a text holds at most one record per two bytes (an S line and its '\n'), and one line per byte
static uint32_t text_hard_records(uint64_t len) { return (uint32_t)(len / 2 + 1); }

// parser and staging of a slot for `len` bytes of text with the bounds (recs, lines)
static int text_slot_prepare(kaamer_index *ix, TopSlot &h, uint64_t len, uint32_t recs, uint64_t lines, bool host_staging = true)
{
    if (!h.stream) HIPCHK(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
    if (host_staging && h.h_text_cap < len) {
        HIPCHK(hipStreamSynchronize(h.stream));
        if (h.h_text) (void)hipHostFree(h.h_text);
        h.h_text = nullptr; h.h_text_cap = 0;
        const size_t cap = (size_t)len + (size_t)len / 4 + 4096;
        if (hipHostMalloc((void **)&h.h_text, cap, hipHostMallocDefault) != hipSuccess) return kaamer_fail(KAAMER_E_NOMEM, "pinned text staging (%zu bytes)", cap);
        h.h_text_cap = cap;
    }
    if (h.d_text_cap < len) {
        HIPCHK(hipStreamSynchronize(h.stream));
        if (h.d_text) (void)hipFree(h.d_text);
        h.d_text = nullptr; h.d_text_cap = 0;
        const size_t cap = (size_t)len + (size_t)len / 4 + 4096;
        const int rc = dev_alloc(&h.d_text, cap);
        if (rc) return rc;
        h.d_text_cap = cap;
    }
    if (!h.parser || h.parser_text < len || h.parser_recs < recs || h.parser_lines < lines) {
        HIPCHK(hipStreamSynchronize(h.stream));
        if (h.parser) kaamer_text_parser_free(h.parser);
        h.parser = nullptr;
        uint64_t text_cap = len + len / 4 + 4096;   // some headroom, as for the other buffers of a slot
        if (text_cap > 0xFFFFFFFFull) text_cap = 0xFFFFFFFFull;
        const int rc = text_parser_create_lines(ix->device, text_cap, recs, lines, &h.parser);
        if (rc) { h.parser = nullptr; return rc; }
        h.parser_text = text_cap; h.parser_recs = recs; h.parser_lines = lines;
    }
    return KAAMER_OK;
}

// whole BGZF blocks as the input of a text call: `len` of text_submit is then the sum of the blocks' isize
struct BgzfInput {
    const uint8_t *bytes;
    uint64_t len;
    const std::vector<kaamer_bgzf_block> *blocks;
    // the file form (host_text_file.hip.inc): the text on the device is `tail` (what the previous chunk left behind its cut)
    // followed by the blocks' output; it is cut on the device (last: at its end) and only [0, cut) is parsed and searched
    bool file = false, last = false;
    const char *tail = nullptr;
    uint64_t tail_len = 0;
    std::vector<char> *tail_out = nullptr;   // the text behind the cut, for the next chunk
    bool *no_cut = nullptr;                  // set with KAAMER_E_CAPACITY: no line of the text starts with '@'
};

// staging (pinned + device: the compressed bytes, then the block table at the next multiple of 8) and inflater of a slot
static int bgzf_slot_prepare(kaamer_index *ix, TopSlot &h, uint64_t comp_len, size_t n_blocks)
{
    if (!h.stream) HIPCHK(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
    const size_t need = (size_t)((comp_len + 7) & ~7ull) + n_blocks * sizeof(kaamer_bgzf_block);
    if (h.h_comp_cap < need || h.d_comp_cap < need) {
        HIPCHK(hipStreamSynchronize(h.stream));
        if (h.h_comp) (void)hipHostFree(h.h_comp);
        if (h.d_comp) (void)hipFree(h.d_comp);
        h.h_comp = nullptr; h.d_comp = nullptr; h.h_comp_cap = h.d_comp_cap = 0;
        const size_t cap = need + need / 4 + 4096;
        if (hipHostMalloc((void **)&h.h_comp, cap, hipHostMallocDefault) != hipSuccess) return kaamer_fail(KAAMER_E_NOMEM, "pinned BGZF staging (%zu bytes)", cap);
        h.h_comp_cap = cap;
        const int rc = dev_alloc(&h.d_comp, cap);
        if (rc) return rc;
        h.d_comp_cap = cap;
    }
    if (!h.inflater || h.inflater_comp < comp_len || h.inflater_blocks < n_blocks) {
        HIPCHK(hipStreamSynchronize(h.stream));
        if (h.inflater) kaamer_inflater_free(h.inflater);
        h.inflater = nullptr;
        const uint64_t comp_cap = comp_len + comp_len / 4 + 4096;
        const uint32_t blocks_cap = (uint32_t)(n_blocks + n_blocks / 4 + 64);
        const int rc = kaamer_inflater_create(ix->device, comp_cap, blocks_cap, &h.inflater);
        if (rc) { h.inflater = nullptr; return rc; }
        h.inflater_comp = comp_cap; h.inflater_blocks = blocks_cap;
    }
    return KAAMER_OK;
}

// compressed bytes and block table up, the text into h.d_text (behind the tail of the file form); waits once for the
// status words' summary and, in the file form, the cut.  A bad block: KAAMER_E_FORMAT.
static int bgzf_inflate_to_slot(TopSlot &h, const BgzfInput &bz, uint64_t text_len, uint64_t *cut)
{
    const size_t n = bz.blocks->size(), table_at = (size_t)((bz.len + 7) & ~7ull);
    if (bz.len) memcpy(h.h_comp, bz.bytes, (size_t)bz.len);   // the caller's buffer is only borrowed for this call
    if (n) memcpy(h.h_comp + table_at, bz.blocks->data(), n * sizeof(kaamer_bgzf_block));
    if (table_at + n) HIPCHK(hipMemcpyAsync(h.d_comp, h.h_comp, table_at + n * sizeof(kaamer_bgzf_block), hipMemcpyHostToDevice, h.stream));
    if (bz.tail_len) HIPCHK(hipMemcpyAsync(h.d_text, bz.tail, (size_t)bz.tail_len, hipMemcpyHostToDevice, h.stream));
    const bool want_cut = bz.file && !bz.last;
    int rc = inf_enqueue(h.inflater, h.d_comp, bz.len, reinterpret_cast<const kaamer_bgzf_block *>(h.d_comp + table_at), (uint32_t)n,
                         h.d_text + bz.tail_len, text_len - bz.tail_len, h.d_text, want_cut ? text_len : 0, h.stream);
    kaamer_inflate_result res;
    if (!rc) rc = kaamer_inflater_finish(h.inflater, h.stream, &res);
    if (rc) return rc;
    if (res.n_bad)
        return kaamer_fail(KAAMER_E_FORMAT, "search_bgzf_top: BGZF block %u does not inflate: status %u (%u bad of %zu blocks)", res.first_bad,
                           res.first_bad_status, res.n_bad, n);
    *cut = want_cut ? h.inflater->h_res[INF_R_CUT] : text_len;
    return KAAMER_OK;
}

// FASTA text as the input of a text call (kaamer_submit_fasta_top_flat, kaamer_search_fasta_file): the `format` of
// text_submit is then not looked at, and PROTEIN is as good a sequence type as the other two
struct FastaInput { bool upper_last; };
// the TSV rows of the reported hits as part of a text call (the *_tsv_flat calls, host_tsv.hip.inc)
struct TsvRequest { bool positions, annotations; };

static int text_submit(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, const kaamer_topn_opts *top,
                       bool blocking, kaamer_ticket **out, const BgzfInput *bz = nullptr, const FastaInput *fa = nullptr,
                       const TsvRequest *tsv = nullptr)
{
    const char *who = fa ? "submit_fasta_top" : "submit_text_top";
    if (!ix || !top || !out || (!text && len && !bz) || top->max_results < 1) return kaamer_fail(KAAMER_E_ARG, "%s: bad argument", who);
    *out = nullptr;
    if (tsv && !ix->d_st_bytes)
        return kaamer_fail(KAAMER_E_ARG, "%s: TSV rows need the subject text on the device (kaamer_index_attach_subject_text)", who);
    if (!fa) {
        if (format == 0)
            return kaamer_fail(KAAMER_E_ARG, "submit_text_top: FASTA is not parsed on the device by this call: use kaamer_submit_fasta_top_flat, or the host reader "
                                             "(kaamer_parse_fasta, then kaamer_submit_batch_top_flat)");
        if (format != 1) return kaamer_fail(KAAMER_E_ARG, "submit_text_top: unknown format %d (1 = FASTQ)", (int)format);
    }
    SEQ_TYPE_CHK(seq_type, who);
    if (!fa && !is_nucl(seq_type)) return kaamer_fail(KAAMER_E_ARG, "submit_text_top: FASTQ text is READS or NUCLEOTIDE input, not PROTEIN");
    if (!bz && kaamer_is_gzip(text, len))
        return kaamer_fail(KAAMER_E_ARG, "%s: the text starts with the gzip signature: inflate it first (%s does)", who,
                           fa ? "kaamer_search_fasta_file" : "kaamer_search_text_file");
    if (len > 0xFFFFFFFFull)
        return kaamer_fail(KAAMER_E_ARG, "%s: a text holds at most 2^32 - 1 bytes (spans are 32-bit): cut it (%s)", who,
                           fa ? "kaamer_text_cut_fasta" : "kaamer_text_cut_fastq");
    int slot = -1;
    const int src = top_slot_take(ix, blocking, &slot);
    if (src) return src;
    kaamer_ticket *t = new (std::nothrow) kaamer_ticket();
    if (!t) { top_slot_release(ix, slot); return kaamer_fail(KAAMER_E_NOMEM, "ticket"); }
    memset(t, 0, sizeof *t);
    t->ix = ix; t->slot = slot; t->seq_type = seq_type; t->top = *top; t->text = true;
    if (tsv) { t->want_tsv = true; t->tsv_pos = tsv->positions; t->tsv_ann = tsv->annotations; t->want_pos = tsv->positions; }
    TopSlot &h = ix->top[slot];
    int rc = KAAMER_OK;
    hipError_t he = hipSetDevice(ix->device);
    if (he != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "hipSetDevice: %s", hipGetErrorString(he));
    // where the bounds start: a record of a read set is a header, the read, '+' and as many quality bytes -- 32 bytes
    // would be a 10-base read; four lines per record.  Kept when the slot's parser already holds more.  (FASTA starts from
    // the same figures: they hold for two-line reads and for 60-column files, and narrower ones grow them.)
    const uint32_t hard_recs = text_hard_records(len);
    uint32_t recs = (uint32_t)(len / 32 + 1024);
    if (recs > hard_recs) recs = hard_recs;
    uint64_t lines = pt_default_line_cap(len, recs);
    if (!rc && h.parser && h.parser_text >= len) {
        if (h.parser_recs > recs) recs = h.parser_recs;
        if (h.parser_lines > lines) lines = h.parser_lines;
    }
    kaamer_text_parse_result pr;
    memset(&pr, 0, sizeof pr);
    bool uploaded = false;
    while (!rc) {
        rc = text_slot_prepare(ix, h, len, recs, lines, !bz);
        if (rc) break;
        if (!uploaded && bz) {
            rc = bgzf_slot_prepare(ix, h, bz->len, bz->blocks->size());
            uint64_t cut = len;
            if (!rc) rc = bgzf_inflate_to_slot(h, *bz, len, &cut);
            if (!rc && bz->file) {
                if (cut == 0 && !bz->last && len) { *bz->no_cut = true; rc = KAAMER_E_CAPACITY; }   // (the source grows the chunk or gives up)
                else {
                    // the tail goes home with the wait for the parse's counts; from here on the text is [0, cut)
                    bz->tail_out->resize((size_t)(len - cut));
                    if (len > cut) {
                        he = hipMemcpyAsync(bz->tail_out->data(), h.d_text + cut, (size_t)(len - cut), hipMemcpyDeviceToHost, h.stream);
                        if (he != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(he));
                    }
                    len = cut;
                }
            }
            if (rc) break;
            uploaded = true;
        }
        if (!uploaded) {
            if (len) {
                memcpy(h.h_text, text, (size_t)len);   // the caller's buffer is only borrowed for this call
                he = hipMemcpyAsync(h.d_text, h.h_text, (size_t)len, hipMemcpyHostToDevice, h.stream);
                if (he != hipSuccess) { rc = kaamer_fail(KAAMER_E_HIP, "H2D: %s", hipGetErrorString(he)); break; }
            }
            uploaded = true;
        }
        rc = fa ? kaamer_parse_fasta_device(h.parser, h.d_text, len, fa->upper_last ? 1 : 0, h.stream)
                : kaamer_parse_fastq_device(h.parser, h.d_text, len, h.stream);
        if (!rc) rc = kaamer_text_parser_finish(h.parser, h.stream, &pr);   // the one wait of the submit call: n_seqs comes from the host
        if (rc != KAAMER_E_CAPACITY) break;
        if (recs >= hard_recs && lines >= len + 1) break;   // (cannot happen: these bounds hold for any text)
        recs = recs > hard_recs / 4 ? hard_recs : recs * 4;
        lines = lines > (len + 1) / 4 ? len + 1 : lines * 4;
        rc = KAAMER_OK;
    }
    if (!rc) {
        t->n_seqs = pr.n_records; t->seq_bytes = pr.seq_bytes;
        t->d_text_seqs = pr.d_seqs; t->d_text_off = pr.d_offsets;
        t->d_names = h.d_text; t->names_len = len; t->d_spans = pr.d_spans;
        t->h_spans = (kaamer_text_span *)pinned_get(((size_t)pr.n_records + 1) * sizeof(kaamer_text_span), &t->h_spans_cap);
        if (!t->h_spans) rc = kaamer_fail(KAAMER_E_NOMEM, "pinned spans (%u records)", pr.n_records);
    }
    if (!rc && pr.n_records) {
        he = hipMemcpyAsync(t->h_spans, pr.d_spans, (size_t)pr.n_records * sizeof(kaamer_text_span), hipMemcpyDeviceToHost, h.stream);
        if (he != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(he));
    }
    if (!rc && bz) {   // the caller never held the text: it rides back with the result
        t->text_len = len;
        t->h_text_out = (char *)pinned_get((size_t)len + 1, &t->h_text_out_cap);
        if (!t->h_text_out) rc = kaamer_fail(KAAMER_E_NOMEM, "pinned text (%llu bytes)", (unsigned long long)len);
        if (!rc && len) {
            he = hipMemcpyAsync(t->h_text_out, h.d_text, (size_t)len, hipMemcpyDeviceToHost, h.stream);
            if (he != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(he));
        }
    }
    if (!rc) rc = top_enqueue(t);
    if (rc) {
        if (h.stream) (void)hipStreamSynchronize(h.stream);
        if (t->h_block) pinned_put(t->h_block, t->h_block_cap);
        if (t->h_spans) pinned_put(t->h_spans, t->h_spans_cap);
        if (t->h_text_out) pinned_put(t->h_text_out, t->h_text_out_cap);
        if (t->h_tsv) pinned_put(t->h_tsv, t->h_tsv_cap);
        delete t;
        top_slot_release(ix, slot);
        return rc;
    }
    *out = t;
    return KAAMER_OK;
}

int kaamer_submit_text_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket)
{
    kaamer_topn_opts top;
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    return text_submit(ix, text, len, format, seq_type, &top, true, ticket);
}

int kaamer_search_text_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_ticket *t = nullptr;
    const int rc = kaamer_submit_text_top_flat(ix, text, len, format, seq_type, min_k_ratio, min_k_match, max_results, &t);
    if (rc) return rc;
    return kaamer_wait_batch_top(t, out);
}

// the text call for FASTA (search_protein.go / search_nucleotide.go / search_fastq.go with GetQueriesFasta inside): one more
// caller of text_submit
int kaamer_submit_fasta_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                 int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket)
{
    kaamer_topn_opts top;
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    const FastaInput fa = { upper_last != 0 };
    return text_submit(ix, text, len, 0, seq_type, &top, true, ticket, nullptr, &fa);
}

int kaamer_search_fasta_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                 int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_ticket *t = nullptr;
    const int rc = kaamer_submit_fasta_top_flat(ix, text, len, seq_type, upper_last, min_k_ratio, min_k_match, max_results, &t);
    if (rc) return rc;
    return kaamer_wait_batch_top(t, out);
}

// whole BGZF blocks: scanned on the host (no inflate), inflated, parsed and searched on the slot's stream
static int bgzf_submit(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                       uint32_t max_results, kaamer_ticket **ticket, const TsvRequest *tsv)
{
    if (ticket) *ticket = nullptr;
    if (!ix || !ticket || (!bytes && len)) return kaamer_fail(KAAMER_E_ARG, "submit_bgzf_top: bad argument");
    std::vector<kaamer_bgzf_block> blocks;
    uint64_t n = 0, used = 0;
    int rc = kaamer_bgzf_scan(bytes, len, nullptr, 0, &n, &used);
    if (rc) return rc;
    if (used != len)
        return kaamer_fail(KAAMER_E_ARG, "submit_bgzf_top: the bytes are not whole BGZF blocks (%llu blocks in the first %llu of %llu bytes): "
                                         "ordinary gzip and plain text go through the host (kaamer_search_text_file, kaamer_search_text_top_flat)",
                           (unsigned long long)n, (unsigned long long)used, (unsigned long long)len);
    if (n > 0xFFFFFFF0ull) return kaamer_fail(KAAMER_E_ARG, "submit_bgzf_top: too many blocks");
    blocks.resize((size_t)n);
    rc = kaamer_bgzf_scan(bytes, len, blocks.data(), n, &n, &used);
    if (rc) return rc;
    uint64_t text_len = 0;
    for (const kaamer_bgzf_block &b : blocks) text_len += b.isize;
    kaamer_topn_opts top;
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    const BgzfInput bz = { bytes, len, &blocks };
    return text_submit(ix, nullptr, text_len, 1, seq_type, &top, true, ticket, &bz, nullptr, tsv);
}

int kaamer_submit_bgzf_top_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                uint32_t max_results, kaamer_ticket **ticket)
{
    return bgzf_submit(ix, bytes, len, seq_type, min_k_ratio, min_k_match, max_results, ticket, nullptr);
}

int kaamer_search_bgzf_top_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                uint32_t max_results, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_ticket *t = nullptr;
    const int rc = kaamer_submit_bgzf_top_flat(ix, bytes, len, seq_type, min_k_ratio, min_k_match, max_results, &t);
    if (rc) return rc;
    return kaamer_wait_batch_top(t, out);
}

int kaamer_batch_top_text(const kaamer_batch_top *out, const char **text, uint64_t *len)
{
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!out) return kaamer_fail(KAAMER_E_ARG, "batch_top_text: bad argument");
    const batch_top_owner *bo = reinterpret_cast<const batch_top_owner *>(out);  // pub is the first member
    if (!bo->text) return KAAMER_OK;   // the caller of any other call holds the text (or the batch) itself
    if (text) *text = bo->text;
    if (len) *len = bo->text_len;
    return KAAMER_OK;
}

int kaamer_batch_top_text_spans(const kaamer_batch_top *out, const kaamer_text_span **spans, uint32_t *n_records)
{
    if (spans) *spans = nullptr;
    if (n_records) *n_records = 0;
    if (!out) return kaamer_fail(KAAMER_E_ARG, "batch_top_text_spans: bad argument");
    const batch_top_owner *bo = reinterpret_cast<const batch_top_owner *>(out);  // pub is the first member
    if (!bo->spans) return KAAMER_OK;   // the call took a packed batch
    if (spans) *spans = bo->spans;
    if (n_records) *n_records = bo->n_spans;
    return KAAMER_OK;
}

// whole BGZF blocks of a file (with the tail in front) into the FIFO of a stream: as stream_push_text
static int stream_push_bgzf(kaamer_stream *st, const BgzfInput &bz, uint64_t text_len)
{
    kaamer_ticket *t = nullptr;
    const int rc = text_submit(st->ix, nullptr, text_len, 1, st->seq_type, &st->top, st->fifo->empty(), &t, &bz);
    if (rc) return rc;
    st->fifo->push_back(t);
    return KAAMER_OK;
}

// a text chunk into the FIFO of a stream (kaamer_search_text_file): as kaamer_stream_push, never blocking on a slot the
// stream itself holds
static int stream_push_text(kaamer_stream *st, const char *text, uint64_t len, const FastaInput *fa = nullptr)
{
    kaamer_ticket *t = nullptr;
    const int rc = text_submit(st->ix, text, len, 1, st->seq_type, &st->top, st->fifo->empty(), &t, nullptr, fa);
    if (rc) return rc;
    st->fifo->push_back(t);
    return KAAMER_OK;
}
