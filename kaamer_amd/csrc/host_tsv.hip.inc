// host_tsv.hip.inc — the host side of the TSV response rows (included by search.hip inside its extern "C" block, after
// host_text.hip.inc; the kernels are in tsv_rows.hip.inc, the contract and the host formatter in tsv_format.cpp):
//   kaamer_index_attach_subject_text  EntryId, Length and the annotation columns of every entry, resident next to the index
//   kaamer_tsv_stage_* / kaamer_tsv_rows_device / kaamer_tsv_rows_finish   the stage on a stream
//   kaamer_tsv_aln_rows_device        the -aln rows on the same stage (kernels: tsv_aln_rows.hip.inc), kaamer_tsv_aln_info,
//                                     kaamer_tsv_format_doubles_device
//   kaamer_format_tsv / kaamer_format_tsv_aln   the host formatters on a result of this library (bitmaps and alignments come
//                                     from the result)
//   top_enqueue_tsv / tsv_needs_repeat / tsv_finish_host   the rows as part of a text call (the kaamer_*_top_tsv_flat calls
//                                     themselves stand next to their twins in host_text.hip.inc); kaamer_batch_top_tsv

int kaamer_index_attach_subject_text(kaamer_index *ix, const kaamer_proteins *p)
{
    if (!ix || !p) return kaamer_fail(KAAMER_E_ARG, "index_attach_subject_text: bad argument");
    HIPCHK(hipSetDevice(ix->device));
    std::vector<uint32_t> uniq;
    std::vector<kaamer_protein_entry> ent;
    int rc = proteins_distinct(p, uniq, ent);   // the entry order of kaamer_index_attach_proteins: one map serves both
    if (rc) return rc;
    const uint32_t n = (uint32_t)uniq.size(), nf = kaamer_proteins_n_features(p);
    const uint64_t map_n = n ? (uint64_t)uniq.back() + 1 : 0;
    if (map_n > (1ull << 31)) return kaamer_fail(KAAMER_E_ARG, "index_attach_subject_text: protein ids up to %llu: the id map is dense", (unsigned long long)map_n);
    std::vector<uint64_t> off((size_t)n + 1, 0);
    std::vector<uint32_t> idlen((size_t)n + 1, 0), length((size_t)n + 1, 0);
    std::vector<uint8_t> bytes;
    uint64_t max_suffix = 0;
    for (uint32_t i = 0; i < n; i++) {
        const kaamer_protein_entry &e = ent[i];
        off[i] = bytes.size();
        idlen[i] = e.entry_id_len;
        length[i] = e.length;
        bytes.insert(bytes.end(), e.entry_id, e.entry_id + e.entry_id_len);
        for (uint32_t f = 0; f < nf; f++) {   // '\t' + value per KStats.Features name: the device only copies bytes
            bytes.push_back((uint8_t)'\t');
            if (f < e.n_features) bytes.insert(bytes.end(), e.features + e.feature_off[f], e.features + e.feature_off[f + 1]);
        }
        uint64_t digits = 1;
        for (uint32_t v = e.length; v >= 10; v /= 10) digits++;
        const uint64_t suffix = bytes.size() - off[i] + digits;
        if (suffix > max_suffix) max_suffix = suffix;
    }
    off[n] = bytes.size();
    {   // nothing of the index may be running: the slots' streams are idle when no slot is busy
        std::lock_guard<std::mutex> lock(ix->pool_mu);
        for (int i = 0; i < ix->n_top; i++)
            if (ix->top[i].busy) return kaamer_fail(KAAMER_E_BUSY, "index_attach_subject_text: calls are in flight on the index");
    }
    HIPCHK(hipDeviceSynchronize());
    subject_text_free(ix);   // a second attach replaces the first
    const bool share = ix->d_aln_idmap && ix->aln_host == p && ix->aln_entries == n && ix->aln_idmap_n == (uint32_t)map_n;
    std::vector<uint32_t> idmap;
    rc = reserve_group(nullptr, GROW_EXACT, { want(ix->d_st_bytes, bytes.size() + 1), want(ix->d_st_off, off.size()), want(ix->d_st_idlen, idlen.size()),
                                              want(ix->d_st_length, length.size()) });
    if (!rc && !share) {
        idmap.assign((size_t)map_n + 1, TSV_NONE);
        for (uint32_t i = 0; i < n; i++) idmap[uniq[i]] = i;
        rc = reserve(ix->d_st_idmap_own, idmap.size(), GROW_EXACT, nullptr);
    }
    if (rc) { subject_text_free(ix); return rc; }
    hipError_t e = bytes.empty() ? hipSuccess : hipMemcpy(ix->d_st_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_st_off, off.data(), off.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_st_idlen, idlen.data(), idlen.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_st_length, length.data(), length.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !share) e = hipMemcpy(ix->d_st_idmap_own, idmap.data(), idmap.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { subject_text_free(ix); return kaamer_fail(KAAMER_E_HIP, "subject text upload: %s", hipGetErrorString(e)); }
    ix->d_st_idmap = share ? ix->d_aln_idmap.get() : ix->d_st_idmap_own.get();   // (borrowed: aln_table_free hands it over)
    ix->st_idmap_n = (uint32_t)map_n; ix->st_entries = n; ix->st_features = nf;
    ix->st_max_suffix = max_suffix;
    ix->st_host = p;
    ix->st_bytes = bytes.size() + 1 + off.size() * 8 + idlen.size() * 4 + length.size() * 4 + (share ? 0 : idmap.size() * 4);
    return KAAMER_OK;
}

int kaamer_index_subject_text_info(const kaamer_index *ix, uint64_t out[4])
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "index_subject_text_info: bad argument");
    out[0] = ix->st_bytes; out[1] = ix->st_entries; out[2] = ix->st_max_suffix; out[3] = ix->st_features;
    return KAAMER_OK;
}

void kaamer_tsv_geometry(uint32_t out[4])
{
    out[0] = TSV_TILE; out[1] = TSV_WINDOW; out[2] = 16; out[3] = TSV_TILE;
}

struct kaamer_tsv_stage {
    kaamer_index *ix = nullptr;
    uint32_t max_queries = 0;
    uint64_t max_lines = 0;
    DevBuf<unsigned long long> d_tile_bytes, d_tile_lines, d_line_off, d_counts;
    PinnedBuf<unsigned long long> h_counts;
    uint64_t out_cap = 0;                     // of the last call
    // the -aln form (kaamer_tsv_aln_rows_device): the order of every query's hits, and BitScore / 2^BitScore per raw score
    // for the options of the last call
    bool last_aln = false;
    DevBuf<uint16_t> d_order;
    DevBuf<double> d_tab;                     // [2 * TSV_ALN_RAW_N]: BitScore, then 2^BitScore
    std::vector<double> h_tab;
    double tab_lambda = 0, tab_kk = 0;
    uint32_t tab_n = 0;                       // raw scores [TSV_ALN_RAW_MIN, + tab_n) are tabulated; 0: no table yet
    uint64_t tabs_filled = 0;
    uint32_t tab_limit = 0;                   // the index's tsv_aln_raw_count the table was filled under
    ~kaamer_tsv_stage() { if (ix) (void)hipSetDevice(ix->device); }   // (before the buffers go)
};

void kaamer_tsv_stage_free(kaamer_tsv_stage *st) { delete st; }

int kaamer_tsv_stage_create(kaamer_index *ix, uint32_t max_queries, uint64_t max_lines, kaamer_tsv_stage **out)
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "tsv_stage_create: bad argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(ix->device));
    kaamer_tsv_stage *st = new (std::nothrow) kaamer_tsv_stage();
    if (!st) return kaamer_fail(KAAMER_E_NOMEM, "tsv stage");
    st->ix = ix; st->max_queries = max_queries; st->max_lines = max_lines;
    const size_t tiles = (size_t)max_queries / TSV_TILE + 1;
    const int rc = reserve_group(nullptr, GROW_EXACT, { want(st->d_tile_bytes, tiles), want(st->d_tile_lines, tiles), want(st->d_line_off, (size_t)max_lines + 1),
                                                        want(st->d_counts, (size_t)TSV_C_N), want(st->h_counts, (size_t)TSV_C_N) });
    if (rc) { delete st; return rc; }
    *out = st;
    return KAAMER_OK;
}

// the argument checks and the kernels' parameters of both forms; d_line_off / line_cap: where the line offsets go; block:
// the packed result block of the same batch (the host-buffer calls), see TsvParams
static int tsv_params(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, char *d_out, uint64_t out_cap, unsigned long long *d_line_off,
                      uint64_t line_cap, const uint8_t *block, TsvParams *out)
{
    const kaamer_index *ix = st->ix;
    if (!ix->d_st_bytes) return kaamer_fail(KAAMER_E_ARG, "tsv_rows: no subject text is attached to the index (kaamer_index_attach_subject_text)");
    if (!in || !in->d_n_queries || !in->d_q || !in->top.d_top_cnt || !in->top.d_top_pid || !in->top.d_top_kmatch || !in->top.d_start_position ||
        !in->top.d_size_in_kmer || in->top.max_results < 1 || (in->n_names && (!in->d_spans || !in->d_name_bytes)) || (!d_out && out_cap) ||
        ((uintptr_t)d_out & 15u) || line_cap < 1)
        return kaamer_fail(KAAMER_E_ARG, "tsv_rows: bad argument");
    if (in->extract_positions && (!in->pos || !in->pos->d_pos_base || !in->pos->d_pos_bits_len || !in->pos->d_pos_bits))
        return kaamer_fail(KAAMER_E_ARG, "tsv_rows: ExtractPositions without the bitmaps of the reported hits (kaamer_topn_positions_device)");
    if (in->n_queries_cap > st->max_queries) return kaamer_fail(KAAMER_E_ARG, "tsv_rows: %u queries, the stage holds %u", in->n_queries_cap, st->max_queries);
    TsvParams p;
    memset(&p, 0, sizeof p);
    p.d_nq = in->d_n_queries; p.nq_cap = in->n_queries_cap; p.q = in->d_q;
    p.top_cnt = in->top.d_top_cnt; p.top_pid = in->top.d_top_pid; p.top_km = in->top.d_top_kmatch;
    p.start_pos = in->top.d_start_position; p.size_out = in->top.d_size_in_kmer; p.K = in->top.max_results;
    p.names = in->d_name_bytes; p.names_len = in->name_bytes_len; p.spans = in->d_spans; p.n_names = in->n_names;
    p.positions = in->extract_positions ? 1 : 0; p.annotations = in->annotations ? 1 : 0;
    if (p.positions) { p.pos_base = in->pos->d_pos_base; p.pos_len = in->pos->d_pos_bits_len; p.pos_bits = in->pos->d_pos_bits; }
    p.st_bytes = ix->d_st_bytes; p.st_off = ix->d_st_off; p.st_idlen = ix->d_st_idlen; p.st_length = ix->d_st_length;
    p.idmap = ix->d_st_idmap; p.idmap_n = ix->st_idmap_n; p.n_features = ix->st_features;
    p.tile_bytes = st->d_tile_bytes; p.tile_lines = st->d_tile_lines;
    p.line_off = d_line_off; p.line_cap = line_cap;
    p.out = d_out; p.out_cap = out_cap;
    p.counts = st->d_counts;
    p.block = block;
    st->out_cap = out_cap;
    *out = p;
    return KAAMER_OK;
}

// the four launches and the copy of the counts
static int tsv_enqueue(kaamer_tsv_stage *st, const kaamer_tsv_rows_in *in, char *d_out, uint64_t out_cap, unsigned long long *d_line_off,
                       uint64_t line_cap, hipStream_t s, const uint8_t *block = nullptr)
{
    st->last_aln = false;
    TsvParams p;
    const int rc = tsv_params(st, in, d_out, out_cap, d_line_off, line_cap, block, &p);
    if (rc) return rc;
    const uint32_t tiles = in->n_queries_cap / TSV_TILE + 1;
    hipLaunchKernelGGL(tsv_len_kernel, dim3(tiles), dim3(TSV_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_scan_kernel, dim3(1), dim3(TSV_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_off_kernel, dim3(tiles), dim3(TSV_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_write_kernel, dim3(tiles), dim3(TSV_TILE), 0, s, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(st->h_counts, st->d_counts, TSV_C_N * 8, hipMemcpyDeviceToHost, s));
    return KAAMER_OK;
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
    int rc = tsv_params(st, in, d_out, out_cap, d_line_off, line_cap, block, &p.base);
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
    const uint32_t tiles = in->n_queries_cap / TSV_TILE + 1;
    HIPCHK(hipMemsetAsync(st->d_counts, 0, TSV_C_N * 8, s));
    hipLaunchKernelGGL(tsv_aln_order_kernel, dim3(tiles), dim3(TSV_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_aln_len_kernel, dim3(tiles), dim3(TSV_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_scan_kernel, dim3(1), dim3(TSV_TILE), 0, s, p.base);
    hipLaunchKernelGGL(tsv_aln_off_kernel, dim3(tiles), dim3(TSV_TILE), 0, s, p);
    hipLaunchKernelGGL(tsv_aln_write_kernel, dim3(tiles), dim3(TSV_TILE), 0, s, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(st->h_counts, st->d_counts, TSV_C_N * 8, hipMemcpyDeviceToHost, s));
    return KAAMER_OK;
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
    const int rc = tsv_aln_enqueue(st, in, src, d_out, out_cap, st->d_line_off, st->max_lines + 1, (hipStream_t)stream, nullptr);
    if (rc) return rc;
    out->d_line_off = reinterpret_cast<const uint64_t *>(st->d_line_off.get());
    out->d_counts = reinterpret_cast<const uint64_t *>(st->d_counts.get());
    out->line_off_capacity = st->max_lines + 1;
    return KAAMER_OK;
}

int kaamer_tsv_aln_info(const kaamer_tsv_stage *st, uint64_t out[4])
{
    if (!st || !out) return kaamer_fail(KAAMER_E_ARG, "tsv_aln_info: bad argument");
    out[0] = st->last_aln ? st->h_counts[TSV_C_RAW] : 0; out[1] = st->tab_n; out[2] = st->tabs_filled; out[3] = 0;
    return KAAMER_OK;
}

int kaamer_tsv_format_doubles_device(const double *d_values, uint64_t n, int32_t mode, char *d_out)
{
    if ((n && (!d_values || !d_out)) || (mode != 0 && mode != 1) || n > 0xFFFFFFFFull * TSV_TILE) return kaamer_fail(KAAMER_E_ARG, "tsv_format_doubles_device: bad argument");
    if (n) hipLaunchKernelGGL(tsv_format_doubles_kernel, dim3((uint32_t)((n + TSV_TILE - 1) / TSV_TILE)), dim3(TSV_TILE), 0, nullptr, d_values, n, (int)mode, d_out);
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
    const int rc = tsv_enqueue(st, in, d_out, out_cap, st->d_line_off, st->max_lines + 1, (hipStream_t)stream);
    if (rc) return rc;
    out->d_line_off = reinterpret_cast<const uint64_t *>(st->d_line_off.get());
    out->d_counts = reinterpret_cast<const uint64_t *>(st->d_counts.get());
    out->line_off_capacity = st->max_lines + 1;
    return KAAMER_OK;
}

// the counts of the last enqueue, once its stream is done
static int tsv_counts(const kaamer_tsv_stage *st, uint64_t counts[2])
{
    if (counts) { counts[0] = st->h_counts[TSV_C_LINES]; counts[1] = st->h_counts[TSV_C_BYTES]; }
    const unsigned long long status = st->h_counts[TSV_C_STATUS];
    if (st->last_aln && st->h_counts[TSV_C_RAW])
        return kaamer_fail(KAAMER_E_RANGE, "tsv_aln_rows: %llu pairs with a raw score outside the table [%d, %d): format this batch on the host (kaamer_format_tsv_aln)",
                           st->h_counts[TSV_C_RAW], TSV_ALN_RAW_MIN, TSV_ALN_RAW_MIN + (int)st->tab_n);
    if (status)
        return kaamer_fail(KAAMER_E_CAPACITY, "tsv_rows: %llu rows of %llu bytes do not fit (%llu bytes, %llu rows)", st->h_counts[TSV_C_LINES],
                           st->h_counts[TSV_C_BYTES], (unsigned long long)st->out_cap, (unsigned long long)st->max_lines);
    return KAAMER_OK;
}

int kaamer_tsv_rows_finish(kaamer_tsv_stage *st, void *stream, uint64_t counts[2])
{
    if (!st) return kaamer_fail(KAAMER_E_ARG, "tsv_rows_finish: bad argument");
    HIPCHK(hipSetDevice(st->ix->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return tsv_counts(st, counts);
}

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

// ---- the rows as part of a text call (kaamer_*_top_tsv_flat): behind the packed block on the slot's stream ----------------
// The rows and their line offsets have a buffer of their own next to the block (the block's format is unchanged): one
// more device-to-host copy per call.  Both bounds -- bytes and rows -- start from what the slot's previous call needed plus
// a quarter; a batch beyond them reports how much it needs, and is repeated from the parsed buffers with exactly that.

static int top_enqueue_tsv(kaamer_ticket *t, TopSlot &h, const kaamer_topn_result *tr, hipStream_t s)
{
    kaamer_index *ix = t->ix;
    const uint64_t hard_lines = (uint64_t)h.ws->q_cap * tr->max_results;
    uint64_t lines = t->tsv_lines_cap ? t->tsv_lines_cap : (h.tsv_guess_lines ? h.tsv_guess_lines : (uint64_t)t->n_seqs + 1024);
    if (lines > hard_lines) lines = hard_lines;
    const uint64_t bytes = t->tsv_bytes_cap ? t->tsv_bytes_cap : (h.tsv_guess_bytes ? h.tsv_guess_bytes : lines * 64);
    t->tsv_lines_cap = lines; t->tsv_bytes_cap = bytes;
    if (!h.tsv || h.tsv_queries < h.ws->q_cap || h.tsv_lines < lines) {
        HIPCHK(hipStreamSynchronize(s));
        if (h.tsv) kaamer_tsv_stage_free(h.tsv);
        h.tsv = nullptr;
        const int rc = kaamer_tsv_stage_create(ix, h.ws->q_cap, lines, &h.tsv);
        if (rc) { h.tsv = nullptr; return rc; }
        h.tsv_queries = h.ws->q_cap; h.tsv_lines = lines;
    }
    { const int rc = reserve(h.d_tsv, (size_t)bytes + 16, GROW_EXACT, s); if (rc) return rc; }
    const size_t off_bytes = ((size_t)lines + 1) * 8, need = off_bytes + (size_t)bytes;
    if (t->h_tsv_cap < need) {
        if (t->h_tsv) pinned_put(t->h_tsv, t->h_tsv_cap);
        t->h_tsv = (uint8_t *)pinned_get(need, &t->h_tsv_cap);
        if (!t->h_tsv) { t->h_tsv_cap = 0; return kaamer_fail(KAAMER_E_NOMEM, "pinned TSV rows (%zu bytes)", need); }
    }
    kaamer_tsv_rows_in in;
    memset(&in, 0, sizeof in);
    in.top = *tr;
    in.d_q = h.ws->d_q; in.d_n_queries = h.ws->d_nq; in.n_queries_cap = h.ws->q_cap;
    in.n_names = t->n_seqs; in.d_name_bytes = t->d_names; in.name_bytes_len = t->names_len; in.d_spans = t->d_spans;
    kaamer_topn_positions pos;
    memset(&pos, 0, sizeof pos);
    if (t->tsv_pos) {   // the bitmaps are in the block (topn_pack_positions); the per-query layout is the workspace's
        pos.d_pos_base = h.ws->d_tp_base; pos.d_pos_bits_len = h.ws->d_tp_len;
        pos.d_pos_bits = reinterpret_cast<const uint64_t *>(h.d_block.get());   // (replaced on the device by the block's section)
        in.pos = &pos;
    }
    in.extract_positions = t->tsv_pos; in.annotations = t->tsv_ann;
    int rc;
    if (t->want_aln) {   // the -aln rows: behind the alignment stage, on the pair records it laid out in the block
        TsvAlnSource src;
        src.on = t->aln.on; src.lambda = t->aln.lambda; src.kk = t->aln.kk; src.seq_type = t->seq_type;
        src.pair_off = h.ws->d_rep_eoff;
        if (src.on) src.lay = h.ws->d_ta_lay;
        rc = tsv_aln_enqueue(h.tsv, &in, src, h.d_tsv, bytes, h.tsv->d_line_off, lines + 1, s, h.d_block);
    } else rc = tsv_enqueue(h.tsv, &in, h.d_tsv, bytes, h.tsv->d_line_off, lines + 1, s, h.d_block);
    if (rc) return rc;
    // the bounds are what the previous call needed plus a quarter: all of both goes home with the block
    HIPCHK(hipMemcpyAsync(t->h_tsv, h.tsv->d_line_off, off_bytes, hipMemcpyDeviceToHost, s));
    if (bytes) HIPCHK(hipMemcpyAsync(t->h_tsv + off_bytes, h.d_tsv, (size_t)bytes, hipMemcpyDeviceToHost, s));
    return KAAMER_OK;
}

// after the stream is done and the block was fine: 1 when the rows did not fit (the ticket's bounds are then what they need)
static int tsv_needs_repeat(kaamer_ticket *t, TopSlot &h, int *rc)
{
    const unsigned long long status = h.tsv->h_counts[TSV_C_STATUS], lines = h.tsv->h_counts[TSV_C_LINES], bytes = h.tsv->h_counts[TSV_C_BYTES];
    if (status & TSV_ST_UPSTREAM) { *rc = kaamer_fail(KAAMER_E_HIP, "tsv rows: the block carries no bitmaps"); return 0; }
    if (t->want_aln && h.tsv->h_counts[TSV_C_RAW]) return 0;   // a raw score outside the table: the host prints this batch (tsv_aln_host_rows)
    if (!status) return 0;
    t->tsv_lines_cap = lines + 1; t->tsv_bytes_cap = bytes + 16;
    return 1;
}

static void tsv_finish_host(kaamer_ticket *t, TopSlot &h, batch_top_owner *bo)
{
    const uint64_t lines = h.tsv->h_counts[TSV_C_LINES], bytes = h.tsv->h_counts[TSV_C_BYTES];
    h.tsv_guess_lines = lines + lines / 4 + 64; h.tsv_guess_bytes = bytes + bytes / 4 + 4096;
    bo->tsv = t->h_tsv; bo->tsv_cap = t->h_tsv_cap;
    bo->tsv_lines = lines; bo->tsv_len = bytes;
    bo->tsv_text = reinterpret_cast<const char *>(t->h_tsv + ((size_t)t->tsv_lines_cap + 1) * 8);
    t->h_tsv = nullptr;
}

// A batch of an *_aln_tsv_flat call in which a raw score lay outside the stage's table: the device printed nothing; the rows
// are the host formatter's, on the finished result (alignments in, hits in BitScore order), into a buffer of the same form.
// The names: the text a BGZF call brought back, else the slot's staging copy of the caller's text (the slot is still the
// ticket's).  The entries come from the table of kaamer_index_attach_proteins.
static int tsv_aln_host_rows(kaamer_ticket *t, TopSlot &h, batch_top_owner *bo)
{
    kaamer_index *ix = t->ix;
    if (!t->aln.on || !h.tsv->h_counts[TSV_C_RAW]) return KAAMER_OK;
    const char *names = bo->text ? bo->text : reinterpret_cast<const char *>(h.h_text.get());
    const kaamer_batch_top &r = bo->pub;
    const uint64_t lines = r.n_reported ? r.top_off[r.n_reported] : 0;
    const int64_t need = kaamer_format_tsv_aln(&r, names, t->names_len, bo->spans, bo->n_spans, ix->aln_host, t->seq_type, t->tsv_pos, t->tsv_ann, nullptr, 0, nullptr);
    if (need < 0) return (int)need;
    size_t cap = 0;
    const size_t off_bytes = ((size_t)lines + 1) * 8;
    uint8_t *buf = (uint8_t *)pinned_get(off_bytes + (size_t)need + 1, &cap);
    if (!buf) return kaamer_fail(KAAMER_E_NOMEM, "pinned TSV rows (%zu bytes)", off_bytes + (size_t)need + 1);
    (void)kaamer_format_tsv_aln(&r, names, t->names_len, bo->spans, bo->n_spans, ix->aln_host, t->seq_type, t->tsv_pos, t->tsv_ann,
                                reinterpret_cast<char *>(buf + off_bytes), (uint64_t)need + 1, reinterpret_cast<uint64_t *>(buf));
    if (bo->tsv) pinned_put(bo->tsv, bo->tsv_cap);
    bo->tsv = buf; bo->tsv_cap = cap;
    bo->tsv_lines = lines; bo->tsv_len = (uint64_t)need;
    bo->tsv_text = reinterpret_cast<const char *>(buf + off_bytes);
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

int kaamer_batch_top_tsv(const kaamer_batch_top *out, const char **text, uint64_t *len, const uint64_t **line_off)
{
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (line_off) *line_off = nullptr;
    if (!out) return kaamer_fail(KAAMER_E_ARG, "batch_top_tsv: bad argument");
    const batch_top_owner *bo = reinterpret_cast<const batch_top_owner *>(out);  // pub is the first member
    if (!bo->tsv || bo->json) return KAAMER_OK;   // any other call: format the rows on the host (kaamer_format_tsv)
    if (text) *text = bo->tsv_text;
    if (len) *len = bo->tsv_len;
    if (line_off) *line_off = reinterpret_cast<const uint64_t *>(bo->tsv);
    return KAAMER_OK;
}

// the first bounds of the rows on a slot that has not run a TSV call yet (tests: a first bound too small); 0: the rule
int kaamer_index_set_tsv_bounds(kaamer_index *ix, uint64_t bytes, uint64_t lines)
{
    if (!ix) return kaamer_fail(KAAMER_E_ARG, "index_set_tsv_bounds: bad argument");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    for (int i = 0; i < ix->n_top; i++) {
        if (ix->top[i].busy) return kaamer_fail(KAAMER_E_BUSY, "index_set_tsv_bounds: calls are in flight on the index");
        ix->top[i].tsv_guess_bytes = bytes; ix->top[i].tsv_guess_lines = lines;
    }
    return KAAMER_OK;
}
