// host_tsv.hip.inc — the host side of the TSV response rows (included by search.hip inside its extern "C" block, after
// host_out.hip.inc, whose attach skeleton and stage base it uses; the kernels are in tsv_rows.hip.inc and
// tsv_aln_rows.hip.inc, the contract and the host formatter in tsv_format.cpp):
//   kaamer_index_attach_subject_text  EntryId, Length and the annotation columns of every entry, resident next to the index
//   kaamer_tsv_stage_* / kaamer_tsv_rows_device / kaamer_tsv_rows_finish   the stage on a stream
//   kaamer_tsv_aln_rows_device        the -aln rows on the same stage, kaamer_tsv_aln_info, kaamer_tsv_format_doubles_device
//   kaamer_format_tsv / kaamer_format_tsv_aln   the host formatters on a result of this library (bitmaps and alignments come
//                                     from the result)
//   tsv_aln_host_rows                 the -aln rows of a text call's batch the stage gave up on; kaamer_batch_top_tsv

// entry i: EntryId, then '\t' + value per KStats.Features name (the device only copies bytes); len: the EntryId's length, plen:
// Protein.Length; longest: the longest of what a row prints of an entry (its bytes and the digits of Length)
static int subject_text_render(const kaamer_proteins *p, const std::vector<kaamer_protein_entry> &ent, const char *, SubjectHost &h)
{
    const uint32_t n = (uint32_t)ent.size(), nf = kaamer_proteins_n_features(p);
    h.off.assign((size_t)n + 1, 0); h.len.assign((size_t)n + 1, 0); h.plen.assign((size_t)n + 1, 0);
    h.pad = 1; h.features = nf;
    for (uint32_t i = 0; i < n; i++) {
        const kaamer_protein_entry &e = ent[i];
        h.off[i] = h.bytes.size();
        h.len[i] = e.entry_id_len;
        h.plen[i] = e.length;
        h.bytes.insert(h.bytes.end(), e.entry_id, e.entry_id + e.entry_id_len);
        for (uint32_t f = 0; f < nf; f++) {
            h.bytes.push_back((uint8_t)'\t');
            if (f < e.n_features) h.bytes.insert(h.bytes.end(), e.features + e.feature_off[f], e.features + e.feature_off[f + 1]);
        }
        uint64_t digits = 1;
        for (uint32_t v = e.length; v >= 10; v /= 10) digits++;
        const uint64_t suffix = h.bytes.size() - h.off[i] + digits;
        if (suffix > h.longest) h.longest = suffix;
    }
    h.off[n] = h.bytes.size();
    return KAAMER_OK;
}

int kaamer_index_attach_subject_text(kaamer_index *ix, const kaamer_proteins *p)
{
    if (!ix || !p) return kaamer_fail(KAAMER_E_ARG, "index_attach_subject_text: bad argument");
    return subject_attach(ix, p, "index_attach_subject_text", "subject text", ix->st, { &ix->aln_idmap }, subject_text_render);
}

int kaamer_index_subject_text_info(const kaamer_index *ix, uint64_t out[4])
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "index_subject_text_info: bad argument");
    out[0] = ix->st.table_bytes; out[1] = ix->st.entries; out[2] = ix->st.longest; out[3] = ix->st.features;
    return KAAMER_OK;
}

void kaamer_tsv_geometry(uint32_t out[4])
{
    out[0] = OUT_TILE; out[1] = TSV_WINDOW; out[2] = 16; out[3] = OUT_TILE;
}

// the -aln form (kaamer_tsv_aln_rows_device) adds BitScore / 2^BitScore per raw score for the options of the last call
struct kaamer_tsv_stage : OutStage {
    bool last_aln = false;
    DevBuf<double> d_tab;                     // [2 * TSV_ALN_RAW_N]: BitScore, then 2^BitScore
    std::vector<double> h_tab;
    double tab_lambda = 0, tab_kk = 0;
    uint32_t tab_n = 0;                       // raw scores [TSV_ALN_RAW_MIN, + tab_n) are tabulated; 0: no table yet
    uint64_t tabs_filled = 0;
    uint32_t tab_limit = 0;                   // the index's tsv_aln_raw_count the table was filled under
};

void kaamer_tsv_stage_free(kaamer_tsv_stage *st) { out_stage_free(st); }

int kaamer_tsv_stage_create(kaamer_index *ix, uint32_t max_queries, uint64_t max_lines, kaamer_tsv_stage **out)
{
    return out_stage_create(ix, max_queries, max_lines, "tsv", out);
}

// the argument checks and the kernels' parameters of both forms (out_params, and the subject text)
static int tsv_params(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, char *d_out, uint64_t out_cap, unsigned long long *d_line_off,
                      uint64_t line_cap, const uint8_t *block, TsvParams *p)
{
    const SubjectTable &t = st->ix->st;
    if (!t.d_bytes) return kaamer_fail(KAAMER_E_ARG, "tsv_rows: no subject text is attached to the index (kaamer_index_attach_subject_text)");
    const int rc = out_params(st, "tsv_rows", in, in && in->extract_positions, "ExtractPositions", t, d_out, out_cap, d_line_off, line_cap, block, p);
    if (rc) return rc;
    p->annotations = in->annotations ? 1 : 0;
    p->st_bytes = t.d_bytes; p->st_off = t.d_off; p->st_idlen = t.d_len; p->st_length = t.d_plen; p->n_features = t.features;
    return KAAMER_OK;
}

// the four launches and the copy of the counts
static int tsv_enqueue(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, char *d_out, uint64_t out_cap, unsigned long long *d_line_off,
                       uint64_t line_cap, hipStream_t s, const uint8_t *block = nullptr)
{
    st->last_aln = false;
    TsvParams p;
    memset(&p, 0, sizeof p);
    int rc = tsv_params(st, in, d_out, out_cap, d_line_off, line_cap, block, &p);
    if (!rc) rc = out_clear_counts(st, s);
    if (rc) return rc;
    const uint32_t tiles = in->n_queries_cap / OUT_TILE + 1;
    hipLaunchKernelGGL(tsv_len_kernel<TsvPlain>, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    hipLaunchKernelGGL(out_scan_kernel, dim3(1), dim3(OUT_TILE), 0, s, p, 0u);
    hipLaunchKernelGGL(tsv_off_kernel<TsvPlain>, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_write_kernel<TsvPlain>, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    return out_launch_tail(st, s);
}

// BitScore and 2^BitScore per raw score for (lambda, K), by kaamer_align_finish's own arithmetic; kept while the options
// stay.  The table ends before the first BitScore the rows' 64-bit "%.2f" would not take (none with the reference's rows).
static int tsv_aln_table(kaamer_tsv_stage *st, double lambda, double kk, hipStream_t s)
{
    if (st->tab_n && st->tab_lambda == lambda && st->tab_kk == kk && st->tab_limit == st->ix->tsv_aln_raw_count) return KAAMER_OK;
    st->tab_limit = st->ix->tsv_aln_raw_count;
    int rc = reserve(st->d_tab, (size_t)2 * TSV_ALN_RAW_N, GROW_EXACT, s);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));   // (an earlier call's copy reads h_tab)
    st->h_tab.assign((size_t)2 * TSV_ALN_RAW_N, 0.0);
    uint32_t n = 0;
    kaamer_align_ints t;
    memset(&t, 0, sizeof t);
    const uint32_t limit = st->ix->tsv_aln_raw_count && st->ix->tsv_aln_raw_count < TSV_ALN_RAW_N ? st->ix->tsv_aln_raw_count : TSV_ALN_RAW_N;
    for (; n < limit; n++) {
        kaamer_alignment a;
        t.raw = TSV_ALN_RAW_MIN + (int32_t)n;
        kaamer_align_finish(&a, &t, 1, 1, lambda, kk);
        if (!(std::fabs(a.bitscore) < 9.0e18)) break;
        st->h_tab[n] = a.bitscore;
        st->h_tab[(size_t)TSV_ALN_RAW_N + n] = kaamer_align_pow2(a.bitscore);
    }
    if (!n) return kaamer_fail(KAAMER_E_ARG, "tsv_aln_rows: the options give no finite BitScore");
    HIPCHK(hipMemcpyAsync(st->d_tab, st->h_tab.data(), st->h_tab.size() * 8, hipMemcpyHostToDevice, s));
    st->tab_lambda = lambda; st->tab_kk = kk; st->tab_n = n;
    st->tabs_filled++;
    return KAAMER_OK;
}

// where the pair records of a batch are: plain arrays (the device-resident form), the section of the packed block the
// alignment stage laid out (lay, on the device), or nowhere -- options without a row in AllMatrixScores: every hit keeps
// the empty AlignmentResult with status 1
struct TsvAlnSource {
    const uint64_t *pair_off = nullptr;
    const kaamer_align_pair *pairs = nullptr;
    uint64_t pair_cap = 0;
    const TaLayout *lay = nullptr;
    bool on = true;
    double lambda = 0, kk = 0;
    int32_t seq_type = 0;
};

// the five launches and the copy of the counts, for both callers
static int tsv_aln_enqueue(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, const TsvAlnSource &src, char *d_out, uint64_t out_cap,
                           unsigned long long *d_line_off, uint64_t line_cap, hipStream_t s, const uint8_t *block)
{
    const kaamer_index *ix = st->ix;
    if (!ix->d_aln_raw) return kaamer_fail(KAAMER_E_ARG, "tsv_aln_rows: no protein table is attached to the index (kaamer_index_attach_proteins)");
    TsvAlnParams p;
    memset(&p, 0, sizeof p);
    int rc = tsv_params(st, in, d_out, out_cap, d_line_off, line_cap, block, &p);
    if (rc) return rc;
    if (in->top.max_results > 65535u) return kaamer_fail(KAAMER_E_ARG, "tsv_aln_rows: max_results %u, the stage orders up to 65535 hits per query", in->top.max_results);
    if (src.on) rc = tsv_aln_table(st, src.lambda, src.kk, s);
    if (!rc) rc = reserve(st->d_order, (size_t)in->n_queries_cap * in->top.max_results, GROW_EXACT, s);
    if (rc) return rc;
    p.pair_off = src.pair_off; p.pairs = src.pairs; p.pair_cap = src.pair_cap; p.lay = src.lay; p.unaligned = src.on ? 0 : 1;
    p.order = st->d_order;
    if (src.on) { p.tab_bits = st->d_tab; p.tab_pow = st->d_tab + TSV_ALN_RAW_N; p.tab_n = st->tab_n; }
    p.protein = KAAMER_SEQ_TYPE_BASE(src.seq_type) == KAAMER_PROTEIN ? 1 : 0;
    p.number_of_aa = (double)ix->aln_number_of_aa;
    st->last_aln = true;
    const uint32_t tiles = in->n_queries_cap / OUT_TILE + 1;
    rc = out_clear_counts(st, s);
    if (rc) return rc;
    hipLaunchKernelGGL(tsv_aln_order_kernel, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_len_kernel<TsvAln>, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    hipLaunchKernelGGL(out_scan_kernel, dim3(1), dim3(OUT_TILE), 0, s, p, 0u);
    hipLaunchKernelGGL(tsv_off_kernel<TsvAln>, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_write_kernel<TsvAln>, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    return out_launch_tail(st, s);
}

int kaamer_tsv_aln_rows_device(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, const kaamer_topn_alignments *alns, const kaamer_tsv_aln_opts *opts,
                               char *d_out, uint64_t out_cap, void *stream, kaamer_tsv_rows_result *out)
{
    if (!st || !out || !alns || !opts || !alns->d_pair_off || !alns->d_pairs) return kaamer_fail(KAAMER_E_ARG, "tsv_aln_rows_device: bad argument");
    memset(out, 0, sizeof *out);
    HIPCHK(hipSetDevice(st->ix->device));
    char name[sizeof opts->sub_matrix + 1];
    memcpy(name, opts->sub_matrix, sizeof opts->sub_matrix);
    name[sizeof opts->sub_matrix] = 0;
    TsvAlnSource src;
    if (!kaamer_align_options(name, opts->gap_open, opts->gap_extend, &src.lambda, &src.kk))
        return kaamer_fail(KAAMER_E_ARG, "tsv_aln_rows_device: No matrix found (or not BLOSUM62)");
    src.pair_off = alns->d_pair_off; src.pairs = alns->d_pairs; src.pair_cap = alns->pair_capacity; src.seq_type = opts->seq_type;
    const int rc = tsv_aln_enqueue(st, in, src, d_out, out_cap, st->d_unit_off, st->max_units + 1, (hipStream_t)stream, nullptr);
    if (rc) return rc;
    out->d_line_off = reinterpret_cast<const uint64_t *>(st->d_unit_off.get());
    out->d_counts = reinterpret_cast<const uint64_t *>(st->d_counts.get());
    out->line_off_capacity = st->max_units + 1;
    return KAAMER_OK;
}

int kaamer_tsv_aln_info(const kaamer_tsv_stage *st, uint64_t out[4])
{
    if (!st || !out) return kaamer_fail(KAAMER_E_ARG, "tsv_aln_info: bad argument");
    out[0] = st->last_aln ? st->h_counts[OUT_C_RAW] : 0; out[1] = st->tab_n; out[2] = st->tabs_filled; out[3] = 0;
    return KAAMER_OK;
}

int kaamer_tsv_format_doubles_device(const double *d_values, uint64_t n, int32_t mode, char *d_out)
{
    if ((n && (!d_values || !d_out)) || (mode != 0 && mode != 1) || n > 0xFFFFFFFFull * OUT_TILE) return kaamer_fail(KAAMER_E_ARG, "tsv_format_doubles_device: bad argument");
    if (n) hipLaunchKernelGGL(tsv_format_doubles_kernel, dim3((uint32_t)((n + OUT_TILE - 1) / OUT_TILE)), dim3(OUT_TILE), 0, nullptr, d_values, n, (int)mode, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return KAAMER_OK;
}

int kaamer_tsv_rows_device(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, char *d_out, uint64_t out_cap, void *stream,
                           kaamer_tsv_rows_result *out)
{
    if (!st || !out) return kaamer_fail(KAAMER_E_ARG, "tsv_rows_device: bad argument");
    memset(out, 0, sizeof *out);
    HIPCHK(hipSetDevice(st->ix->device));
    const int rc = tsv_enqueue(st, in, d_out, out_cap, st->d_unit_off, st->max_units + 1, (hipStream_t)stream);
    if (rc) return rc;
    out->d_line_off = reinterpret_cast<const uint64_t *>(st->d_unit_off.get());
    out->d_counts = reinterpret_cast<const uint64_t *>(st->d_counts.get());
    out->line_off_capacity = st->max_units + 1;
    return KAAMER_OK;
}

// the counts of the last enqueue, once its stream is done
static int stage_counts(const kaamer_tsv_stage *st, uint64_t counts[2])
{
    const int rc = out_counts(st, "tsv_rows", "rows", counts);
    if (st->last_aln && st->h_counts[OUT_C_RAW])   // (whatever the status says)
        return kaamer_fail(KAAMER_E_RANGE, "tsv_aln_rows: %llu pairs with a raw score outside the table [%d, %d): format this batch on the host (kaamer_format_tsv_aln)",
                           st->h_counts[OUT_C_RAW], TSV_ALN_RAW_MIN, TSV_ALN_RAW_MIN + (int)st->tab_n);
    return rc;
}

int kaamer_tsv_rows_finish(kaamer_tsv_stage *st, void *stream, uint64_t counts[2]) { return out_finish(st, "tsv_rows_finish", stream, counts); }

int64_t kaamer_format_tsv(const kaamer_batch_top *top, const char *name_bytes, uint64_t name_bytes_len, const kaamer_text_span *name_spans,
                          uint32_t n_names, const kaamer_proteins *proteins, int32_t extract_positions, int32_t annotations, char *buf, uint64_t cap,
                          uint64_t *line_off)
{
    if (!top) return kaamer_fail(KAAMER_E_ARG, "format_tsv: bad argument");
    const int32_t *len = nullptr;
    const uint64_t *off = nullptr, *bits = nullptr;
    if (extract_positions) {
        const int rc = kaamer_batch_top_positions(top, &len, &off, &bits);
        if (rc) return rc;
    }
    return kaamer_format_tsv_arrays(top, len, off, bits, name_bytes, name_bytes_len, name_spans, n_names, proteins, extract_positions, annotations,
                                    buf, cap, line_off);
}

int64_t kaamer_format_tsv_aln(const kaamer_batch_top *top, const char *name_bytes, uint64_t name_bytes_len, const kaamer_text_span *name_spans,
                              uint32_t n_names, const kaamer_proteins *proteins, int32_t seq_type, int32_t extract_positions, int32_t annotations,
                              char *buf, uint64_t cap, uint64_t *line_off)
{
    if (!top) return kaamer_fail(KAAMER_E_ARG, "format_tsv_aln: bad argument");
    const kaamer_alignment *alns = nullptr;
    int rc = kaamer_batch_top_alignments(top, &alns, nullptr);
    if (rc) return rc;
    const int32_t *len = nullptr;
    const uint64_t *off = nullptr, *bits = nullptr;
    if (extract_positions) {
        rc = kaamer_batch_top_positions(top, &len, &off, &bits);
        if (rc) return rc;
    }
    return kaamer_format_tsv_aln_arrays(top, alns, len, off, bits, name_bytes, name_bytes_len, name_spans, n_names, proteins, seq_type, extract_positions,
                                        annotations, buf, cap, line_off);
}

// A batch of an *_aln_tsv_flat call in which a raw score lay outside the stage's table: the device printed nothing; the rows
// are the host formatter's, on the finished result (alignments in, hits in BitScore order), into a buffer of the same form.
// The names: the text a BGZF call brought back, else the slot's staging copy of the caller's text (the slot is still the
// ticket's).  The entries come from the table of kaamer_index_attach_proteins.
static int tsv_aln_host_rows(kaamer_ticket *t, TopSlot &h, batch_top_owner *bo)
{
    kaamer_index *ix = t->ix;
    if (!t->aln.on || !h.tsv->h_counts[OUT_C_RAW]) return KAAMER_OK;
    const char *names = bo->text ? bo->text : reinterpret_cast<const char *>(h.h_text.get());
    const kaamer_batch_top &r = bo->pub;
    const uint64_t lines = r.n_reported ? r.top_off[r.n_reported] : 0;
    const int64_t need = kaamer_format_tsv_aln(&r, names, t->names_len, bo->spans, bo->n_spans, ix->aln_host, t->seq_type, t->out_pos, t->out_ann, nullptr, 0, nullptr);
    if (need < 0) return (int)need;
    size_t cap = 0;
    const size_t off_bytes = ((size_t)lines + 1) * 8;
    uint8_t *buf = (uint8_t *)pinned_get(off_bytes + (size_t)need + 1, &cap);
    if (!buf) return kaamer_fail(KAAMER_E_NOMEM, "pinned TSV rows (%zu bytes)", off_bytes + (size_t)need + 1);
    (void)kaamer_format_tsv_aln(&r, names, t->names_len, bo->spans, bo->n_spans, ix->aln_host, t->seq_type, t->out_pos, t->out_ann,
                                reinterpret_cast<char *>(buf + off_bytes), (uint64_t)need + 1, reinterpret_cast<uint64_t *>(buf));
    if (bo->out) pinned_put(bo->out, bo->out_cap);
    bo->out = buf; bo->out_cap = cap;
    bo->out_units = lines; bo->out_len = (uint64_t)need;
    bo->out_text = reinterpret_cast<const char *>(buf + off_bytes);
    { std::lock_guard<std::mutex> lock(ix->pool_mu); ix->tsv_aln_host_batches++; }
    return KAAMER_OK;
}

int kaamer_index_tsv_aln_info(kaamer_index *ix, uint64_t out[2])
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "index_tsv_aln_info: bad argument");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    out[0] = ix->tsv_aln_host_batches; out[1] = ix->tsv_aln_raw_count ? ix->tsv_aln_raw_count : TSV_ALN_RAW_N;
    return KAAMER_OK;
}

int kaamer_index_set_tsv_aln_raw_count(kaamer_index *ix, uint32_t n)
{
    if (!ix) return kaamer_fail(KAAMER_E_ARG, "index_set_tsv_aln_raw_count: bad argument");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    for (int i = 0; i < ix->n_top; i++)
        if (ix->top[i].busy) return kaamer_fail(KAAMER_E_BUSY, "index_set_tsv_aln_raw_count: calls are in flight on the index");
    ix->tsv_aln_raw_count = n;
    return KAAMER_OK;
}

// the first bounds of the rows on a slot that has not run a TSV call yet (tests: a first bound too small); 0: the rule
int kaamer_index_set_tsv_bounds(kaamer_index *ix, uint64_t bytes, uint64_t lines)
{
    if (!ix) return kaamer_fail(KAAMER_E_ARG, "index_set_tsv_bounds: bad argument");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    for (int i = 0; i < ix->n_top; i++) {
        if (ix->top[i].busy) return kaamer_fail(KAAMER_E_BUSY, "index_set_tsv_bounds: calls are in flight on the index");
        ix->top[i].guess_bytes[OUT_TSV] = bytes; ix->top[i].guess_units[OUT_TSV] = lines;
    }
    return KAAMER_OK;
}
