// host_text.hip.inc — the host-buffer boundary for callers that hold TEXT (included by search.hip inside its extern "C"
// block, after host_top.hip.inc): search_fastq.go:60-136 with the reader (search.go:324-412) on the device.
//
// Every text call is a TextRequest -- where the text comes from (the caller's buffer, or BGZF blocks that the slot's
// inflater, inflate.hip.inc, turns into text on the device), which parser reads it (parse_text.hip.inc, parse_fasta.hip.inc)
// and whether the TSV rows of the reported hits come back too (host_out_text.hip.inc) -- handed to text_submit, whose phases are
//   text_check            what is refused, before anything is taken
//   text_take_ticket      a free slot and the ticket that holds it
//   text_first_bounds     records and lines the slot's parser starts with
//   text_stage            the text onto the device: text_upload through pinned staging, or bgzf_stage (inflate; the file
//                         form cuts the text and hands the tail behind the cut back)
//   text_parse_growing    the parse and the one wait of the call, for the two counts; repeated with four times the bounds
//                         while the device reports KAAMER_E_CAPACITY (the text is on the device by then)
//   text_attach_results   the records' spans, and the text of a BGZF call, ride back with the result block
//   top_enqueue           what kaamer_submit_batch_top_flat enqueues -- on the parser's buffers
//   text_submit_failed    the one failure exit
// kaamer_wait_batch_top takes the ticket as every other; the twelve kaamer_{submit,search}_{text,fasta,bgzf}_top[_tsv]_flat
// build a request and go through flat_submit / flat_search.

// one text call
struct TextRequest {
    const char *who = "submit_text_top";   // the call's name in messages
    // the source: the caller's text ...
    const char *text = nullptr;
    uint64_t len = 0;                       // bytes of text on the device; BGZF: tail_len + the sum of the blocks' isize
    // ... or whole BGZF blocks of FASTQ (text is NULL then): `blocks` is their table, comp_off relative to `comp`
    bool bgzf = false;
    const uint8_t *comp = nullptr;
    uint64_t comp_len = 0;
    const std::vector<kaamer_bgzf_block> *blocks = nullptr;
    // the file form of BGZF (host_text_file.hip.inc): the text on the device is `tail` (what the previous chunk left behind its
    // cut) followed by the blocks' output; it is cut on the device (last: at its end) and only [0, cut) is parsed and searched
    bool file = false, last = false;
    const char *tail = nullptr;
    uint64_t tail_len = 0;
    std::vector<char> *tail_out = nullptr;  // the text behind the cut, for the next chunk
    bool *no_cut = nullptr;                 // set with KAAMER_E_CAPACITY: no line of the text starts with '@'
    // the parser: FASTQ (format: the caller's, 1 is FASTQ), or FASTA (format is not looked at, and PROTEIN is as good a
    // sequence type as the other two)
    int32_t format = 1;
    bool fasta = false, upper_last = false;
    // the TSV rows of the reported hits come back with the result (the *_tsv_flat calls, host_out_text.hip.inc)
    bool tsv = false, tsv_positions = false, tsv_annotations = false;
    // ... or the JSON objects of the reported queries (the *_json_flat calls); tsv_positions is ExtractPositions
    bool json = false;
    // ... behind the alignment of the reported hits, as the -aln rows (the *_aln_tsv_flat calls): numbers only, no operations
    bool aln = false;
    TopAlnRequest aln_rq;
};

static TextRequest fastq_request(const char *text, uint64_t len, int32_t format = 1)
{
    TextRequest rq;
    rq.text = text; rq.len = len; rq.format = format;
    return rq;
}
static TextRequest fasta_request(const char *text, uint64_t len, bool upper_last)
{
    TextRequest rq;
    rq.who = "submit_fasta_top";
    rq.text = text; rq.len = len; rq.format = 0; rq.fasta = true; rq.upper_last = upper_last;
    return rq;
}
// (without the table and the text's length: bgzf_submit scans the bytes, the file source knows both)
static TextRequest bgzf_request(const uint8_t *comp, uint64_t comp_len)
{
    TextRequest rq;
    rq.bgzf = true; rq.comp = comp; rq.comp_len = comp_len;
    return rq;
}
static TextRequest with_rows(TextRequest rq, int32_t extract_positions, int32_t annotations)
{
    rq.tsv = true; rq.tsv_positions = extract_positions != 0; rq.tsv_annotations = annotations != 0;
    return rq;
}

static TextRequest with_objects(TextRequest rq, int32_t extract_positions)
{
    rq.json = true; rq.tsv_positions = extract_positions != 0;
    return rq;
}

static TextRequest with_alignment(TextRequest rq, const char *sub_matrix, int32_t gap_open, int32_t gap_extend)
{
    rq.aln = true;
    rq.aln_rq = top_aln_request(sub_matrix ? sub_matrix : "", gap_open, gap_extend, 0);
    return rq;
}

// what a submit knows between its phases: the length of the text on the device (the file form: up to its cut), the
// parser's bounds and what the parse found
struct TextParse {
    uint64_t len;
    uint32_t recs, hard_recs;
    uint64_t lines;
    kaamer_text_parse_result pr;
};

// a text holds at most one record per two bytes (an S line and its '\n'), and one line per byte
static uint32_t text_hard_records(uint64_t len) { return (uint32_t)(len / 2 + 1); }

// parser and staging of a slot for `len` bytes of text with the bounds (recs, lines)
static int text_slot_prepare(kaamer_index *ix, TopSlot &h, uint64_t len, uint32_t recs, uint64_t lines, bool host_staging)
{
    if (!h.stream) HIPCHK(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
    int rc = host_staging ? reserve(h.h_text, (size_t)len, GROW_SLOT, h.stream) : KAAMER_OK;
    if (!rc) rc = reserve(h.d_text, (size_t)len, GROW_SLOT, h.stream);
    if (rc) return rc;
    if (!h.parser || h.parser_text < len || h.parser_recs < recs || h.parser_lines < lines) {
        HIPCHK(hipStreamSynchronize(h.stream));
        if (h.parser) kaamer_text_parser_free(h.parser);
        h.parser = nullptr;
        uint64_t text_cap = grow_capacity(GROW_SLOT, len);   // some headroom, as for the other buffers of a slot
        if (text_cap > 0xFFFFFFFFull) text_cap = 0xFFFFFFFFull;
        rc = text_parser_create_lines(ix->device, text_cap, recs, lines, &h.parser);
        if (rc) { h.parser = nullptr; return rc; }
        h.parser_text = text_cap; h.parser_recs = recs; h.parser_lines = lines;
    }
    return KAAMER_OK;
}

// staging (pinned + device: the compressed bytes, then the block table at the next multiple of 8) and inflater of a slot
static int bgzf_slot_prepare(kaamer_index *ix, TopSlot &h, uint64_t comp_len, size_t n_blocks)
{
    if (!h.stream) HIPCHK(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
    const size_t need = (size_t)((comp_len + 7) & ~7ull) + n_blocks * sizeof(kaamer_bgzf_block);
    int rc = reserve(h.h_comp, need, GROW_SLOT, h.stream);
    if (!rc) rc = reserve(h.d_comp, need, GROW_SLOT, h.stream);
    if (rc) return rc;
    if (!h.inflater || h.inflater_comp < comp_len || h.inflater_blocks < n_blocks) {
        HIPCHK(hipStreamSynchronize(h.stream));
        if (h.inflater) kaamer_inflater_free(h.inflater);
        h.inflater = nullptr;
        const uint64_t comp_cap = grow_capacity(GROW_SLOT, comp_len);
        const uint32_t blocks_cap = (uint32_t)(n_blocks + n_blocks / 4 + 64);
        rc = kaamer_inflater_create(ix->device, comp_cap, blocks_cap, &h.inflater);
        if (rc) { h.inflater = nullptr; return rc; }
        h.inflater_comp = comp_cap; h.inflater_blocks = blocks_cap;
    }
    return KAAMER_OK;
}

// compressed bytes and block table up, the text into h.d_text (behind the tail of the file form); waits once for the
// status words' summary and, in the file form, the cut.  A bad block: KAAMER_E_FORMAT.
static int bgzf_inflate_to_slot(TopSlot &h, const TextRequest &rq, uint64_t *cut)
{
    const size_t n = rq.blocks->size(), table_at = (size_t)((rq.comp_len + 7) & ~7ull);
    if (rq.comp_len) memcpy(h.h_comp, rq.comp, (size_t)rq.comp_len);   // the caller's buffer is only borrowed for this call
    if (n) memcpy(h.h_comp + table_at, rq.blocks->data(), n * sizeof(kaamer_bgzf_block));
    if (table_at + n) HIPCHK(hipMemcpyAsync(h.d_comp, h.h_comp, table_at + n * sizeof(kaamer_bgzf_block), hipMemcpyHostToDevice, h.stream));
    if (rq.tail_len) HIPCHK(hipMemcpyAsync(h.d_text, rq.tail, (size_t)rq.tail_len, hipMemcpyHostToDevice, h.stream));
    const bool want_cut = rq.file && !rq.last;
    int rc = inf_enqueue(h.inflater, h.d_comp, rq.comp_len, reinterpret_cast<const kaamer_bgzf_block *>(h.d_comp + table_at), (uint32_t)n,
                         h.d_text + rq.tail_len, rq.len - rq.tail_len, h.d_text, want_cut ? rq.len : 0, h.stream);
    kaamer_inflate_result res;
    if (!rc) rc = kaamer_inflater_finish(h.inflater, h.stream, &res);
    if (rc) return rc;
    if (res.n_bad)
        return kaamer_fail(KAAMER_E_FORMAT, "search_bgzf_top: BGZF block %u does not inflate: status %u (%u bad of %zu blocks)", res.first_bad,
                           res.first_bad_status, res.n_bad, n);
    *cut = want_cut ? h.inflater->h_res[INF_R_CUT] : rq.len;
    return KAAMER_OK;
}

// ---- the phases of text_submit ------------------------------------------------------------------------------------------
static int text_check(kaamer_index *ix, const TextRequest &rq, int32_t seq_type, const kaamer_topn_opts *top, kaamer_ticket **out)
{
    const char *who = rq.who;
    if (!ix || !top || !out || (!rq.text && rq.len && !rq.bgzf) || top->max_results < 1) return kaamer_fail(KAAMER_E_ARG, "%s: bad argument", who);
    *out = nullptr;
    if (rq.tsv && !ix->st.d_bytes)
        return kaamer_fail(KAAMER_E_ARG, "%s: TSV rows need the subject text on the device (kaamer_index_attach_subject_text)", who);
    if (rq.json && !ix->sj.d_bytes)
        return kaamer_fail(KAAMER_E_ARG, "%s: JSON objects need the subject entries on the device (kaamer_index_attach_subject_json)", who);
    if (!rq.fasta) {
        if (rq.format == 0)
            return kaamer_fail(KAAMER_E_ARG, "%s: FASTA is not parsed on the device by this call: use kaamer_submit_fasta_top_flat, or the host reader "
                                             "(kaamer_parse_fasta, then kaamer_submit_batch_top_flat)", who);
        if (rq.format != 1) return kaamer_fail(KAAMER_E_ARG, "%s: unknown format %d (1 = FASTQ)", who, (int)rq.format);
    }
    if (rq.aln && !ix->d_aln_raw)
        return kaamer_fail(KAAMER_E_ARG, "%s: the -aln rows need the protein table on the device (kaamer_index_attach_proteins)", who);
    SEQ_TYPE_CHK(seq_type, who);
    if (!rq.fasta && !is_nucl(seq_type)) return kaamer_fail(KAAMER_E_ARG, "%s: FASTQ text is READS or NUCLEOTIDE input, not PROTEIN", who);
    if (!rq.bgzf && kaamer_is_gzip(rq.text, rq.len))
        return kaamer_fail(KAAMER_E_ARG, "%s: the text starts with the gzip signature: inflate it first (%s does)", who,
                           rq.fasta ? "kaamer_search_fasta_file" : "kaamer_search_text_file");
    if (rq.len > 0xFFFFFFFFull)
        return kaamer_fail(KAAMER_E_ARG, "%s: a text holds at most 2^32 - 1 bytes (spans are 32-bit): cut it (%s)", who,
                           rq.fasta ? "kaamer_text_cut_fasta" : "kaamer_text_cut_fastq");
    return KAAMER_OK;
}

static int text_take_ticket(kaamer_index *ix, const TextRequest &rq, int32_t seq_type, const kaamer_topn_opts *top, bool blocking, kaamer_ticket **out)
{
    int slot = -1;
    const int src = top_slot_take(ix, blocking, &slot);
    if (src) return src;
    kaamer_ticket *t = new (std::nothrow) kaamer_ticket();
    if (!t) { top_slot_release(ix, slot); return kaamer_fail(KAAMER_E_NOMEM, "ticket"); }
    memset(t, 0, sizeof *t);
    t->ix = ix; t->slot = slot; t->seq_type = seq_type; t->top = *top; t->text = true;
    if (rq.tsv) { t->out_fmt = OUT_TSV; t->out_pos = rq.tsv_positions; t->out_ann = rq.tsv_annotations; t->want_pos = rq.tsv_positions; }
    if (rq.json) {   // nucleotide / reads requests always print PositionHits (search.go:416)
        t->out_fmt = OUT_JSON; t->json_fasta = rq.fasta; t->out_pos = rq.tsv_positions || is_nucl(seq_type); t->want_pos = t->out_pos;
    }
    if (rq.aln) { t->want_aln = true; t->aln = rq.aln_rq; }
    *out = t;
    return KAAMER_OK;
}

// where the bounds start: a record of a read set is a header, the read, '+' and as many quality bytes -- 32 bytes
// would be a 10-base read; four lines per record.  Kept when the slot's parser already holds more.  (FASTA starts from
// the same figures: they hold for two-line reads and for 60-column files, and narrower ones grow them.)
static TextParse text_first_bounds(const TopSlot &h, uint64_t len)
{
    TextParse ps;
    memset(&ps, 0, sizeof ps);
    ps.len = len;
    ps.hard_recs = text_hard_records(len);
    ps.recs = (uint32_t)(len / 32 + 1024);
    if (ps.recs > ps.hard_recs) ps.recs = ps.hard_recs;
    ps.lines = pt_default_line_cap(len, ps.recs);
    if (h.parser && h.parser_text >= len) {
        if (h.parser_recs > ps.recs) ps.recs = h.parser_recs;
        if (h.parser_lines > ps.lines) ps.lines = h.parser_lines;
    }
    return ps;
}

static int text_upload(TopSlot &h, const TextRequest &rq)
{
    if (!rq.len) return KAAMER_OK;
    memcpy(h.h_text, rq.text, (size_t)rq.len);   // the caller's buffer is only borrowed for this call
    const hipError_t he = hipMemcpyAsync(h.d_text, h.h_text, (size_t)rq.len, hipMemcpyHostToDevice, h.stream);
    return he == hipSuccess ? KAAMER_OK : kaamer_fail(KAAMER_E_HIP, "H2D: %s", hipGetErrorString(he));
}

// the blocks inflated into the slot's text; the file form: from here on the text is [0, cut), what lies behind goes home
// with the wait for the parse's counts
static int bgzf_stage(kaamer_index *ix, TopSlot &h, const TextRequest &rq, TextParse &ps)
{
    int rc = bgzf_slot_prepare(ix, h, rq.comp_len, rq.blocks->size());
    uint64_t cut = rq.len;
    if (!rc) rc = bgzf_inflate_to_slot(h, rq, &cut);
    if (rc || !rq.file) return rc;
    if (cut == 0 && !rq.last && rq.len) { *rq.no_cut = true; return KAAMER_E_CAPACITY; }   // (the source grows the chunk or gives up)
    rq.tail_out->resize((size_t)(rq.len - cut));
    if (rq.len > cut) {
        const hipError_t he = hipMemcpyAsync(rq.tail_out->data(), h.d_text + cut, (size_t)(rq.len - cut), hipMemcpyDeviceToHost, h.stream);
        if (he != hipSuccess) return kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(he));
    }
    ps.len = cut;
    return KAAMER_OK;
}

static int text_stage(kaamer_index *ix, TopSlot &h, const TextRequest &rq, TextParse &ps)
{
    const int rc = text_slot_prepare(ix, h, ps.len, ps.recs, ps.lines, !rq.bgzf);
    if (rc) return rc;
    return rq.bgzf ? bgzf_stage(ix, h, rq, ps) : text_upload(h, rq);
}

// the parse of the staged text; bounds the device reports as too small grow fourfold, up to those that hold for any text
static int text_parse_growing(kaamer_index *ix, TopSlot &h, const TextRequest &rq, TextParse &ps)
{
    for (;;) {
        int rc = rq.fasta ? kaamer_parse_fasta_device(h.parser, h.d_text, ps.len, rq.upper_last ? 1 : 0, h.stream)
                          : kaamer_parse_fastq_device(h.parser, h.d_text, ps.len, h.stream);
        if (!rc) rc = kaamer_text_parser_finish(h.parser, h.stream, &ps.pr);   // the one wait of the submit call: n_seqs comes from the host
        if (rc != KAAMER_E_CAPACITY) return rc;
        if (ps.recs >= ps.hard_recs && ps.lines >= ps.len + 1) return rc;   // (cannot happen: these bounds hold for any text)
        ps.recs = ps.recs > ps.hard_recs / 4 ? ps.hard_recs : ps.recs * 4;
        ps.lines = ps.lines > (ps.len + 1) / 4 ? ps.len + 1 : ps.lines * 4;
        rc = text_slot_prepare(ix, h, ps.len, ps.recs, ps.lines, !rq.bgzf);
        if (rc) return rc;
    }
}

// the batch of the ticket is what the parser left on the device; the spans, and the text the caller of a BGZF call never
// held, go into pinned buffers of the ticket behind the parse
static int text_attach_results(kaamer_ticket *t, TopSlot &h, const TextRequest &rq, const TextParse &ps)
{
    const kaamer_text_parse_result &pr = ps.pr;
    t->n_seqs = pr.n_records; t->seq_bytes = pr.seq_bytes;
    t->d_text_seqs = pr.d_seqs; t->d_text_off = pr.d_offsets;
    t->d_names = h.d_text; t->names_len = ps.len; t->d_spans = pr.d_spans;
    t->h_spans = (kaamer_text_span *)pinned_get(((size_t)pr.n_records + 1) * sizeof(kaamer_text_span), &t->h_spans_cap);
    if (!t->h_spans) return kaamer_fail(KAAMER_E_NOMEM, "pinned spans (%u records)", pr.n_records);
    hipError_t he = hipSuccess;
    if (pr.n_records) he = hipMemcpyAsync(t->h_spans, pr.d_spans, (size_t)pr.n_records * sizeof(kaamer_text_span), hipMemcpyDeviceToHost, h.stream);
    if (he == hipSuccess && rq.bgzf) {
        t->text_len = ps.len;
        t->h_text_out = (char *)pinned_get((size_t)ps.len + 1, &t->h_text_out_cap);
        if (!t->h_text_out) return kaamer_fail(KAAMER_E_NOMEM, "pinned text (%llu bytes)", (unsigned long long)ps.len);
        if (ps.len) he = hipMemcpyAsync(t->h_text_out, h.d_text, (size_t)ps.len, hipMemcpyDeviceToHost, h.stream);
    }
    return he == hipSuccess ? KAAMER_OK : kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(he));
}

// The alignment stage sizes its direction slabs by the batch's longest query.  A text call learns the records' lengths
// from the spans, which are on their way home: one more wait, in the aligning calls only.
static int text_max_query_len(kaamer_ticket *t, TopSlot &h)
{
    HIPCHK(hipStreamSynchronize(h.stream));
    uint64_t longest = 0;
    for (uint32_t i = 0; i < t->n_seqs; i++)
        if (t->h_spans[i].seq_len > longest) longest = t->h_spans[i].seq_len;
    if (is_nucl(t->seq_type)) longest = longest / 3 + 2;   // an ORF holds at most a frame's codons
    t->max_query_len = longest > 0x3FFFFFFFull ? 0x3FFFFFFFu : (uint32_t)longest;
    return KAAMER_OK;
}

// part of the call may be on the slot's stream already
static int text_submit_failed(kaamer_ticket *t, int rc)
{
    kaamer_index *ix = t->ix;
    const int slot = t->slot;
    if (ix->top[slot].stream) (void)hipStreamSynchronize(ix->top[slot].stream);
    ticket_put_pinned(t);
    delete t;
    top_slot_release(ix, slot);
    return rc;
}

static int text_submit(kaamer_index *ix, const TextRequest &rq, int32_t seq_type, const kaamer_topn_opts *top, bool blocking, kaamer_ticket **out)
{
    int rc = text_check(ix, rq, seq_type, top, out);
    if (rc) return rc;
    kaamer_ticket *t = nullptr;
    rc = text_take_ticket(ix, rq, seq_type, top, blocking, &t);
    if (rc) return rc;
    TopSlot &h = ix->top[t->slot];
    const hipError_t he = hipSetDevice(ix->device);
    if (he != hipSuccess) return text_submit_failed(t, kaamer_fail(KAAMER_E_HIP, "hipSetDevice: %s", hipGetErrorString(he)));
    TextParse ps = text_first_bounds(h, rq.len);
    rc = text_stage(ix, h, rq, ps);
    if (!rc) rc = text_parse_growing(ix, h, rq, ps);
    if (!rc) rc = text_attach_results(t, h, rq, ps);
    if (!rc && rq.aln) rc = text_max_query_len(t, h);
    if (!rc) rc = top_enqueue(t);
    if (rc) return text_submit_failed(t, rc);
    *out = t;
    return KAAMER_OK;
}

// ---- the exported calls: build the request, submit, and (kaamer_search_*) wait --------------------------------------------
// whole BGZF blocks: scanned on the host (no inflate), inflated, parsed and searched on the slot's stream
static int bgzf_submit(kaamer_index *ix, TextRequest rq, int32_t seq_type, const kaamer_topn_opts *top, kaamer_ticket **ticket)
{
    const uint8_t *bytes = rq.comp;
    const uint64_t len = rq.comp_len;
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
    rq.blocks = &blocks;
    for (const kaamer_bgzf_block &b : blocks) rq.len += b.isize;
    return text_submit(ix, rq, seq_type, top, true, ticket);
}

static int flat_submit(kaamer_index *ix, const TextRequest &rq, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                       kaamer_ticket **ticket)
{
    kaamer_topn_opts top;
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    return rq.bgzf ? bgzf_submit(ix, rq, seq_type, &top, ticket) : text_submit(ix, rq, seq_type, &top, true, ticket);
}

// ... and the wait for that submit's ticket
static int flat_search(kaamer_index *ix, const TextRequest &rq, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                       kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_ticket *t = nullptr;
    const int rc = flat_submit(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, &t);
    if (rc) return rc;
    return kaamer_wait_batch_top(t, out);
}

// FASTQ text (search_fastq.go with GetQueriesFastq inside); the _tsv_ forms: with the rows of the reported hits
int kaamer_submit_text_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket)
{
    return flat_submit(ix, fastq_request(text, len, format), seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_text_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    return flat_search(ix, fastq_request(text, len, format), seq_type, min_k_ratio, min_k_match, max_results, out);
}

int kaamer_submit_text_top_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                    int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations, kaamer_ticket **ticket)
{
    const TextRequest rq = with_rows(fastq_request(text, len, format), extract_positions, annotations);
    return flat_submit(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_text_top_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                    int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations, kaamer_batch_top **out)
{
    const TextRequest rq = with_rows(fastq_request(text, len, format), extract_positions, annotations);
    return flat_search(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, out);
}

// FASTA text (search_protein.go / search_nucleotide.go / search_fastq.go with GetQueriesFasta inside)
int kaamer_submit_fasta_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                 int64_t min_k_match, uint32_t max_results, kaamer_ticket **ticket)
{
    return flat_submit(ix, fasta_request(text, len, upper_last != 0), seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_fasta_top_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                 int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    return flat_search(ix, fasta_request(text, len, upper_last != 0), seq_type, min_k_ratio, min_k_match, max_results, out);
}

int kaamer_submit_fasta_top_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                     int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations, kaamer_ticket **ticket)
{
    const TextRequest rq = with_rows(fasta_request(text, len, upper_last != 0), extract_positions, annotations);
    return flat_submit(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_fasta_top_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                     int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations, kaamer_batch_top **out)
{
    const TextRequest rq = with_rows(fasta_request(text, len, upper_last != 0), extract_positions, annotations);
    return flat_search(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, out);
}

// whole BGZF blocks of FASTQ: the text comes back with the result (kaamer_batch_top_text), since the caller never had it
int kaamer_submit_bgzf_top_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                uint32_t max_results, kaamer_ticket **ticket)
{
    return flat_submit(ix, bgzf_request(bytes, len), seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_bgzf_top_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                uint32_t max_results, kaamer_batch_top **out)
{
    return flat_search(ix, bgzf_request(bytes, len), seq_type, min_k_ratio, min_k_match, max_results, out);
}

int kaamer_submit_bgzf_top_tsv_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                    uint32_t max_results, int32_t extract_positions, int32_t annotations, kaamer_ticket **ticket)
{
    const TextRequest rq = with_rows(bgzf_request(bytes, len), extract_positions, annotations);
    return flat_submit(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_bgzf_top_tsv_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                    uint32_t max_results, int32_t extract_positions, int32_t annotations, kaamer_batch_top **out)
{
    const TextRequest rq = with_rows(bgzf_request(bytes, len), extract_positions, annotations);
    return flat_search(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, out);
}

// ... and the three with the JSON objects of the reported queries (-fmt json, search.go:497-503)
int kaamer_submit_text_top_json_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                     int64_t min_k_match, uint32_t max_results, int32_t extract_positions, kaamer_ticket **ticket)
{
    return flat_submit(ix, with_objects(fastq_request(text, len, format), extract_positions), seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_text_top_json_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                     int64_t min_k_match, uint32_t max_results, int32_t extract_positions, kaamer_batch_top **out)
{
    return flat_search(ix, with_objects(fastq_request(text, len, format), extract_positions), seq_type, min_k_ratio, min_k_match, max_results, out);
}

int kaamer_submit_fasta_top_json_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                      int64_t min_k_match, uint32_t max_results, int32_t extract_positions, kaamer_ticket **ticket)
{
    return flat_submit(ix, with_objects(fasta_request(text, len, upper_last != 0), extract_positions), seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_fasta_top_json_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                      int64_t min_k_match, uint32_t max_results, int32_t extract_positions, kaamer_batch_top **out)
{
    return flat_search(ix, with_objects(fasta_request(text, len, upper_last != 0), extract_positions), seq_type, min_k_ratio, min_k_match, max_results, out);
}

int kaamer_submit_bgzf_top_json_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                     uint32_t max_results, int32_t extract_positions, kaamer_ticket **ticket)
{
    return flat_submit(ix, with_objects(bgzf_request(bytes, len), extract_positions), seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_bgzf_top_json_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                     uint32_t max_results, int32_t extract_positions, kaamer_batch_top **out)
{
    return flat_search(ix, with_objects(bgzf_request(bytes, len), extract_positions), seq_type, min_k_ratio, min_k_match, max_results, out);
}

// ... and with the alignment of the reported hits, the rows in the -aln form (search.go:556-604)
int kaamer_submit_text_top_aln_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                        int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations,
                                        const char *sub_matrix, int32_t gap_open, int32_t gap_extend, kaamer_ticket **ticket)
{
    const TextRequest rq = with_alignment(with_rows(fastq_request(text, len, format), extract_positions, annotations), sub_matrix, gap_open, gap_extend);
    return flat_submit(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_text_top_aln_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t format, int32_t seq_type, double min_k_ratio,
                                        int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations,
                                        const char *sub_matrix, int32_t gap_open, int32_t gap_extend, kaamer_batch_top **out)
{
    const TextRequest rq = with_alignment(with_rows(fastq_request(text, len, format), extract_positions, annotations), sub_matrix, gap_open, gap_extend);
    return flat_search(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, out);
}

int kaamer_submit_fasta_top_aln_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                         int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations,
                                         const char *sub_matrix, int32_t gap_open, int32_t gap_extend, kaamer_ticket **ticket)
{
    const TextRequest rq = with_alignment(with_rows(fasta_request(text, len, upper_last != 0), extract_positions, annotations), sub_matrix, gap_open, gap_extend);
    return flat_submit(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_fasta_top_aln_tsv_flat(kaamer_index *ix, const char *text, uint64_t len, int32_t seq_type, int32_t upper_last, double min_k_ratio,
                                         int64_t min_k_match, uint32_t max_results, int32_t extract_positions, int32_t annotations,
                                         const char *sub_matrix, int32_t gap_open, int32_t gap_extend, kaamer_batch_top **out)
{
    const TextRequest rq = with_alignment(with_rows(fasta_request(text, len, upper_last != 0), extract_positions, annotations), sub_matrix, gap_open, gap_extend);
    return flat_search(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, out);
}

int kaamer_submit_bgzf_top_aln_tsv_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                        uint32_t max_results, int32_t extract_positions, int32_t annotations, const char *sub_matrix, int32_t gap_open,
                                        int32_t gap_extend, kaamer_ticket **ticket)
{
    const TextRequest rq = with_alignment(with_rows(bgzf_request(bytes, len), extract_positions, annotations), sub_matrix, gap_open, gap_extend);
    return flat_submit(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, ticket);
}

int kaamer_search_bgzf_top_aln_tsv_flat(kaamer_index *ix, const uint8_t *bytes, uint64_t len, int32_t seq_type, double min_k_ratio, int64_t min_k_match,
                                        uint32_t max_results, int32_t extract_positions, int32_t annotations, const char *sub_matrix, int32_t gap_open,
                                        int32_t gap_extend, kaamer_batch_top **out)
{
    const TextRequest rq = with_alignment(with_rows(bgzf_request(bytes, len), extract_positions, annotations), sub_matrix, gap_open, gap_extend);
    return flat_search(ix, rq, seq_type, min_k_ratio, min_k_match, max_results, out);
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

// a request into the FIFO of a stream (the chunks of kaamer_search_text_file and its kin): as kaamer_stream_push, never
// blocking on a slot the stream itself holds
static int stream_push_text(kaamer_stream *st, const TextRequest &rq)
{
    kaamer_ticket *t = nullptr;
    const int rc = text_submit(st->ix, rq, st->seq_type, &st->top, st->fifo->empty(), &t);
    if (rc) return rc;
    st->fifo->push_back(t);
    return KAAMER_OK;
}
