// host_json.hip.inc — the host side of the JSON response (included by search.hip inside its extern "C" block, after
// host_tsv.hip.inc; the kernels are in json_rows.hip.inc, the contract and the host formatter in json_format.cpp):
//   kaamer_format_json                the host formatter on a result of this library (bitmaps and alignments come from it)
//   kaamer_index_attach_subject_json  every entry's HitEntries value, resident next to the index
//   kaamer_json_stage_* / kaamer_json_rows_device / kaamer_json_rows_finish   the stage on a stream

int64_t kaamer_format_json(const kaamer_batch_top *top, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, const char *name_bytes,
                           uint64_t name_bytes_len, const kaamer_text_span *name_spans, uint32_t n_names, const kaamer_proteins *proteins, int32_t seq_type,
                           int32_t text_format, int32_t extract_positions, char *buf, uint64_t cap, uint64_t *obj_off)
{
    if (!top) return kaamer_fail(KAAMER_E_ARG, "format_json: bad argument");
    const kaamer_alignment *alns = nullptr;
    int rc = kaamer_batch_top_alignments(top, &alns, nullptr);
    if (rc) return rc;
    const int32_t *len = nullptr;
    const uint64_t *off = nullptr, *bits = nullptr;
    if (extract_positions || KAAMER_SEQ_TYPE_BASE(seq_type) != KAAMER_PROTEIN) {
        rc = kaamer_batch_top_positions(top, &len, &off, &bits);
        if (rc) return rc;
    }
    return kaamer_format_json_arrays(top, alns, len, off, bits, seqs, offsets, n_seqs, name_bytes, name_bytes_len, name_spans, n_names, proteins, seq_type,
                                     text_format, extract_positions, buf, cap, obj_off);
}

int kaamer_index_attach_subject_json(kaamer_index *ix, const kaamer_proteins *p)
{
    if (!ix || !p) return kaamer_fail(KAAMER_E_ARG, "index_attach_subject_json: bad argument");
    HIPCHK(hipSetDevice(ix->device));
    std::vector<uint32_t> uniq;
    std::vector<kaamer_protein_entry> ent;
    int rc = proteins_distinct(p, uniq, ent);   // the entry order of the other two attaches: one map serves all three
    if (rc) return rc;
    const uint32_t n = (uint32_t)uniq.size();
    const uint64_t map_n = n ? (uint64_t)uniq.back() + 1 : 0;
    if (map_n > (1ull << 31)) return kaamer_fail(KAAMER_E_ARG, "index_attach_subject_json: protein ids up to %llu: the id map is dense", (unsigned long long)map_n);
    std::vector<const char *> names;
    for (uint32_t f = 0, nf = kaamer_proteins_n_features(p); f < nf; f++) names.push_back(kaamer_proteins_feature_name(p, f));
    std::vector<uint64_t> off((size_t)n + 1, 0);
    std::vector<uint32_t> len((size_t)n + 1, 0);
    std::vector<uint8_t> bytes;
    uint64_t max_entry = 0;
    for (uint32_t i = 0; i < n; i++) {   // the formatter's own code renders every value: the device only copies
        const uint64_t need = kaamer_json_protein_value(&ent[i], names.empty() ? nullptr : names.data(), nullptr, 0);
        if (need > 0xFFFFFFF0ull) return kaamer_fail(KAAMER_E_ARG, "index_attach_subject_json: an entry of %llu bytes", (unsigned long long)need);
        off[i] = bytes.size();
        len[i] = (uint32_t)need;
        bytes.resize((size_t)((off[i] + need + 1 + 15) & ~15ull), 0);   // (the NUL, then up to the next 16-byte boundary)
        (void)kaamer_json_protein_value(&ent[i], names.empty() ? nullptr : names.data(), reinterpret_cast<char *>(bytes.data() + off[i]), need + 1);
        if (need > max_entry) max_entry = need;
    }
    off[n] = bytes.size();
    {   // nothing of the index may be running: the slots' streams are idle when no slot is busy
        std::lock_guard<std::mutex> lock(ix->pool_mu);
        for (int i = 0; i < ix->n_top; i++)
            if (ix->top[i].busy) return kaamer_fail(KAAMER_E_BUSY, "index_attach_subject_json: calls are in flight on the index");
    }
    HIPCHK(hipDeviceSynchronize());
    subject_json_free(ix);   // a second attach replaces the first
    const uint32_t *lend = nullptr;
    if (ix->d_st_idmap && ix->st_host == p && ix->st_entries == n && ix->st_idmap_n == (uint32_t)map_n) lend = ix->d_st_idmap;
    else if (ix->d_aln_idmap && ix->aln_host == p && ix->aln_entries == n && ix->aln_idmap_n == (uint32_t)map_n) lend = ix->d_aln_idmap.get();
    std::vector<uint32_t> idmap;
    rc = reserve_group(nullptr, GROW_EXACT, { want(ix->d_sj_bytes, bytes.size() + 16), want(ix->d_sj_off, off.size()), want(ix->d_sj_len, len.size()) });
    if (!rc && !lend) {
        idmap.assign((size_t)map_n + 1, TSV_NONE);
        for (uint32_t i = 0; i < n; i++) idmap[uniq[i]] = i;
        rc = reserve(ix->d_sj_idmap_own, idmap.size(), GROW_EXACT, nullptr);
    }
    if (rc) { subject_json_free(ix); return rc; }
    hipError_t e = bytes.empty() ? hipSuccess : hipMemcpy(ix->d_sj_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_sj_off, off.data(), off.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_sj_len, len.data(), len.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !lend) e = hipMemcpy(ix->d_sj_idmap_own, idmap.data(), idmap.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { subject_json_free(ix); return kaamer_fail(KAAMER_E_HIP, "subject json upload: %s", hipGetErrorString(e)); }
    ix->d_sj_idmap = lend ? lend : ix->d_sj_idmap_own.get();
    ix->sj_idmap_n = (uint32_t)map_n; ix->sj_entries = n; ix->sj_max_entry = max_entry;
    ix->sj_bytes = bytes.size() + 16 + off.size() * 8 + len.size() * 4 + (lend ? 0 : idmap.size() * 4);
    return KAAMER_OK;
}

int kaamer_index_subject_json_info(const kaamer_index *ix, uint64_t out[4])
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "index_subject_json_info: bad argument");
    out[0] = ix->sj_bytes; out[1] = ix->sj_entries; out[2] = ix->sj_max_entry; out[3] = 0;
    return KAAMER_OK;
}

void kaamer_json_geometry(uint32_t out[4])
{
    out[0] = JSON_TILE; out[1] = JSON_WIN; out[2] = 16; out[3] = JSON_TILE;
}

struct kaamer_json_stage {
    kaamer_index *ix = nullptr;
    uint32_t max_queries = 0;
    uint64_t max_objects = 0;
    DevBuf<unsigned long long> d_tile_bytes, d_tile_objs, d_obj_off, d_counts;
    DevBuf<uint32_t> d_obj_len;
    DevBuf<uint16_t> d_order;              // [queries x max_results] of the last call
    PinnedBuf<unsigned long long> h_counts;
    uint64_t out_cap = 0;                  // of the last call
    ~kaamer_json_stage() { if (ix) (void)hipSetDevice(ix->device); }   // (before the buffers go)
};

void kaamer_json_stage_free(kaamer_json_stage *st) { delete st; }

int kaamer_json_stage_create(kaamer_index *ix, uint32_t max_queries, uint64_t max_objects, kaamer_json_stage **out)
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "json_stage_create: bad argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(ix->device));
    kaamer_json_stage *st = new (std::nothrow) kaamer_json_stage();
    if (!st) return kaamer_fail(KAAMER_E_NOMEM, "json stage");
    st->ix = ix; st->max_queries = max_queries; st->max_objects = max_objects;
    const size_t tiles = (size_t)max_queries / JSON_TILE + 1;
    const int rc = reserve_group(nullptr, GROW_EXACT, { want(st->d_tile_bytes, tiles), want(st->d_tile_objs, tiles), want(st->d_obj_off, (size_t)max_objects + 1),
                                                        want(st->d_obj_len, (size_t)max_queries + 1), want(st->d_counts, (size_t)JSON_C_N),
                                                        want(st->h_counts, (size_t)JSON_C_N) });
    if (rc) { delete st; return rc; }
    *out = st;
    return KAAMER_OK;
}

// the argument checks, the three launches and the copy of the counts; d_obj_off / obj_cap: where the objects' offsets go;
// block: the packed result block of the same batch (the text calls), see TsvParams
static int json_enqueue(kaamer_json_stage *st, const kaamer_json_rows_in *jin, char *d_out, uint64_t out_cap, unsigned long long *d_obj_off, uint64_t obj_cap,
                        hipStream_t s, const uint8_t *block = nullptr)
{
    const kaamer_index *ix = st->ix;
    if (!ix->d_sj_bytes) return kaamer_fail(KAAMER_E_ARG, "json_rows: no subject entries are attached to the index (kaamer_index_attach_subject_json)");
    if (!jin) return kaamer_fail(KAAMER_E_ARG, "json_rows: bad argument");
    const kaamer_tsv_rows_in *in = &jin->rows;
    if (!in->d_n_queries || !in->d_q || !in->top.d_top_cnt || !in->top.d_top_pid || !in->top.d_top_kmatch || !in->top.d_start_position ||
        !in->top.d_size_in_kmer || in->top.max_results < 1 || (in->n_names && (!in->d_spans || !in->d_name_bytes)) || (!d_out && out_cap) ||
        ((uintptr_t)d_out & 15u) || obj_cap < 1 || (jin->aa_len && !jin->d_aa) || (jin->text_format != 0 && jin->text_format != 1))
        return kaamer_fail(KAAMER_E_ARG, "json_rows: bad argument");
    if (in->top.max_results > 65535u) return kaamer_fail(KAAMER_E_ARG, "json_rows: max_results %u, the stage orders up to 65535 keys per query", in->top.max_results);
    const bool protein = KAAMER_SEQ_TYPE_BASE(jin->seq_type) == KAAMER_PROTEIN;
    const bool positions = !protein || in->extract_positions;   // search.go:416
    if (positions && (!in->pos || !in->pos->d_pos_base || !in->pos->d_pos_bits_len || !in->pos->d_pos_bits))
        return kaamer_fail(KAAMER_E_ARG, "json_rows: PositionHits without the bitmaps of the reported hits (kaamer_topn_positions_device)");
    if (in->n_queries_cap > st->max_queries) return kaamer_fail(KAAMER_E_ARG, "json_rows: %u queries, the stage holds %u", in->n_queries_cap, st->max_queries);
    const int rc = reserve(st->d_order, (size_t)in->n_queries_cap * in->top.max_results + 1, GROW_EXACT, s);
    if (rc) return rc;
    JsonParams p;
    memset(&p, 0, sizeof p);
    p.t.d_nq = in->d_n_queries; p.t.nq_cap = in->n_queries_cap; p.t.q = in->d_q;
    p.t.top_cnt = in->top.d_top_cnt; p.t.top_pid = in->top.d_top_pid; p.t.top_km = in->top.d_top_kmatch;
    p.t.start_pos = in->top.d_start_position; p.t.size_out = in->top.d_size_in_kmer; p.t.K = in->top.max_results;
    p.t.names = in->d_name_bytes; p.t.names_len = in->name_bytes_len; p.t.spans = in->d_spans; p.t.n_names = in->n_names;
    p.t.positions = positions ? 1 : 0;
    if (positions) { p.t.pos_base = in->pos->d_pos_base; p.t.pos_len = in->pos->d_pos_bits_len; p.t.pos_bits = in->pos->d_pos_bits; }
    p.t.idmap = ix->d_sj_idmap; p.t.idmap_n = ix->sj_idmap_n;
    p.t.tile_bytes = st->d_tile_bytes; p.t.tile_lines = st->d_tile_objs;
    p.t.line_off = d_obj_off; p.t.line_cap = obj_cap;
    p.t.out = d_out; p.t.out_cap = out_cap;
    p.t.counts = st->d_counts;
    p.t.block = block;
    p.trim = in->top.d_trim; p.aa = jin->d_aa; p.aa_len = jin->aa_len;
    p.protein = protein ? 1 : 0; p.fasta = jin->text_format == 0 ? 1 : 0;
    p.sj_bytes = ix->d_sj_bytes; p.sj_off = ix->d_sj_off; p.sj_len = ix->d_sj_len;
    p.obj_len = st->d_obj_len; p.order = st->d_order;
    st->out_cap = out_cap;
    const uint32_t tiles = in->n_queries_cap / JSON_TILE + 1;
    HIPCHK(hipMemsetAsync(st->d_counts, 0, JSON_C_N * 8, s));
    hipLaunchKernelGGL(json_len_kernel, dim3(tiles), dim3(JSON_TILE), 0, s, p);
    hipLaunchKernelGGL(json_scan_kernel, dim3(1), dim3(JSON_TILE), 0, s, p);
    hipLaunchKernelGGL(json_write_kernel, dim3(tiles), dim3(JSON_TILE), 0, s, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(st->h_counts, st->d_counts, JSON_C_N * 8, hipMemcpyDeviceToHost, s));
    return KAAMER_OK;
}

int kaamer_json_rows_device(kaamer_json_stage *st, const kaamer_json_rows_in *in, char *d_out, uint64_t out_cap, void *stream, kaamer_json_rows_result *out)
{
    if (!st || !out) return kaamer_fail(KAAMER_E_ARG, "json_rows_device: bad argument");
    memset(out, 0, sizeof *out);
    HIPCHK(hipSetDevice(st->ix->device));
    const int rc = json_enqueue(st, in, d_out, out_cap, st->d_obj_off, st->max_objects + 1, (hipStream_t)stream);
    if (rc) return rc;
    out->d_obj_off = reinterpret_cast<const uint64_t *>(st->d_obj_off.get());
    out->d_counts = reinterpret_cast<const uint64_t *>(st->d_counts.get());
    out->obj_off_capacity = st->max_objects + 1;
    return KAAMER_OK;
}

// the counts of the last enqueue, once its stream is done
static int json_counts(const kaamer_json_stage *st, uint64_t counts[2])
{
    if (counts) { counts[0] = st->h_counts[JSON_C_OBJECTS]; counts[1] = st->h_counts[JSON_C_BYTES]; }
    const unsigned long long status = st->h_counts[JSON_C_STATUS];
    if (status & (JSON_ST_OBJECT | JSON_ST_MISMATCH))
        return kaamer_fail(KAAMER_E_HIP, "json_rows: status %llu (8: an object of 4 GB; 16: the two passes disagree about an object)", status);
    if (status)
        return kaamer_fail(KAAMER_E_CAPACITY, "json_rows: %llu objects of %llu bytes do not fit (%llu bytes, %llu objects)", st->h_counts[JSON_C_OBJECTS],
                           st->h_counts[JSON_C_BYTES], (unsigned long long)st->out_cap, (unsigned long long)st->max_objects);
    return KAAMER_OK;
}

int kaamer_json_rows_finish(kaamer_json_stage *st, void *stream, uint64_t counts[2])
{
    if (!st) return kaamer_fail(KAAMER_E_ARG, "json_rows_finish: bad argument");
    HIPCHK(hipSetDevice(st->ix->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return json_counts(st, counts);
}

// ---- the objects as part of a text call (kaamer_*_top_json_flat): behind the packed block on the slot's stream ------------
// As the TSV rows (host_tsv.hip.inc): a buffer of their own next to the block, one more device-to-host copy per call; the two
// bounds -- bytes and objects -- start from what the slot's previous call needed plus a quarter; a batch beyond them reports
// how much it needs and is repeated from the parsed buffers with exactly that.  The ticket's and the result's fields are
// those of the rows.

static int top_enqueue_json(kaamer_ticket *t, TopSlot &h, const kaamer_topn_result *tr, hipStream_t s)
{
    kaamer_index *ix = t->ix;
    const uint64_t hard = h.ws->q_cap;
    uint64_t objects = t->tsv_lines_cap ? t->tsv_lines_cap : (h.json_guess_objects ? h.json_guess_objects : (uint64_t)t->n_seqs + 1024);
    if (objects > hard) objects = hard;
    const uint64_t bytes = t->tsv_bytes_cap ? t->tsv_bytes_cap : (h.json_guess_bytes ? h.json_guess_bytes : objects * 2048);
    t->tsv_lines_cap = objects; t->tsv_bytes_cap = bytes;
    if (!h.json || h.json_queries < h.ws->q_cap || h.json_objects < objects) {
        HIPCHK(hipStreamSynchronize(s));
        if (h.json) kaamer_json_stage_free(h.json);
        h.json = nullptr;
        const int rc = kaamer_json_stage_create(ix, h.ws->q_cap, objects, &h.json);
        if (rc) { h.json = nullptr; return rc; }
        h.json_queries = h.ws->q_cap; h.json_objects = objects;
    }
    { const int rc = reserve(h.d_json, (size_t)bytes + 16, GROW_EXACT, s); if (rc) return rc; }
    const size_t off_bytes = ((size_t)objects + 1) * 8, need = off_bytes + (size_t)bytes;
    if (t->h_tsv_cap < need) {
        if (t->h_tsv) pinned_put(t->h_tsv, t->h_tsv_cap);
        t->h_tsv = (uint8_t *)pinned_get(need, &t->h_tsv_cap);
        if (!t->h_tsv) { t->h_tsv_cap = 0; return kaamer_fail(KAAMER_E_NOMEM, "pinned JSON objects (%zu bytes)", need); }
    }
    const bool nucl = is_nucl(t->seq_type);
    kaamer_json_rows_in in;
    memset(&in, 0, sizeof in);
    in.rows.top = *tr;
    in.rows.d_q = h.ws->d_q; in.rows.d_n_queries = h.ws->d_nq; in.rows.n_queries_cap = h.ws->q_cap;
    in.rows.n_names = t->n_seqs; in.rows.d_name_bytes = t->d_names; in.rows.name_bytes_len = t->names_len; in.rows.d_spans = t->d_spans;
    kaamer_topn_positions pos;
    memset(&pos, 0, sizeof pos);
    if (t->tsv_pos) {   // the bitmaps are in the block (topn_pack_positions); the per-query layout is the workspace's
        pos.d_pos_base = h.ws->d_tp_base; pos.d_pos_bits_len = h.ws->d_tp_len;
        pos.d_pos_bits = reinterpret_cast<const uint64_t *>(h.d_block.get());   // (replaced on the device by the block's section)
        in.rows.pos = &pos;
    }
    in.rows.extract_positions = t->tsv_pos;
    in.d_aa = nucl ? h.ws->d_orf_aa.get() : t->d_text_seqs;
    in.aa_len = nucl ? h.ws->aa_cap : t->seq_bytes;
    in.seq_type = t->seq_type; in.text_format = t->json_fasta ? 0 : 1;
    const int rc = json_enqueue(h.json, &in, h.d_json, bytes, h.json->d_obj_off, objects + 1, s, h.d_block);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(t->h_tsv, h.json->d_obj_off, off_bytes, hipMemcpyDeviceToHost, s));
    if (bytes) HIPCHK(hipMemcpyAsync(t->h_tsv + off_bytes, h.d_json, (size_t)bytes, hipMemcpyDeviceToHost, s));
    return KAAMER_OK;
}

// after the stream is done and the block was fine: 1 when the objects did not fit (the ticket's bounds are then what they need)
static int json_needs_repeat(kaamer_ticket *t, TopSlot &h, int *rc)
{
    const unsigned long long status = h.json->h_counts[JSON_C_STATUS], objects = h.json->h_counts[JSON_C_OBJECTS], bytes = h.json->h_counts[JSON_C_BYTES];
    if (status & (JSON_ST_UPSTREAM | JSON_ST_OBJECT | JSON_ST_MISMATCH)) { *rc = kaamer_fail(KAAMER_E_HIP, "json objects: status %llu", status); return 0; }
    if (!status) return 0;
    t->tsv_lines_cap = objects + 1; t->tsv_bytes_cap = bytes + 16;
    return 1;
}

static void json_finish_host(kaamer_ticket *t, TopSlot &h, batch_top_owner *bo)
{
    const uint64_t objects = h.json->h_counts[JSON_C_OBJECTS], bytes = h.json->h_counts[JSON_C_BYTES];
    h.json_guess_objects = objects + objects / 4 + 64; h.json_guess_bytes = bytes + bytes / 4 + 4096;
    bo->tsv = t->h_tsv; bo->tsv_cap = t->h_tsv_cap;
    bo->tsv_lines = objects; bo->tsv_len = bytes;
    bo->tsv_text = reinterpret_cast<const char *>(t->h_tsv + ((size_t)t->tsv_lines_cap + 1) * 8);
    bo->json = true;
    t->h_tsv = nullptr;
}

int kaamer_batch_top_json(const kaamer_batch_top *out, const char **text, uint64_t *len, const uint64_t **obj_off)
{
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (obj_off) *obj_off = nullptr;
    if (!out) return kaamer_fail(KAAMER_E_ARG, "batch_top_json: bad argument");
    const batch_top_owner *bo = reinterpret_cast<const batch_top_owner *>(out);  // pub is the first member
    if (!bo->tsv || !bo->json) return KAAMER_OK;   // any other call: format the objects on the host (kaamer_format_json)
    if (text) *text = bo->tsv_text;
    if (len) *len = bo->tsv_len;
    if (obj_off) *obj_off = reinterpret_cast<const uint64_t *>(bo->tsv);
    return KAAMER_OK;
}

// the first bounds of the objects on every slot (tests: a first bound too small); 0: the rule
int kaamer_index_set_json_bounds(kaamer_index *ix, uint64_t bytes, uint64_t objects)
{
    if (!ix) return kaamer_fail(KAAMER_E_ARG, "index_set_json_bounds: bad argument");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    for (int i = 0; i < ix->n_top; i++) {
        if (ix->top[i].busy) return kaamer_fail(KAAMER_E_BUSY, "index_set_json_bounds: calls are in flight on the index");
        ix->top[i].json_guess_bytes = bytes; ix->top[i].json_guess_objects = objects;
    }
    return KAAMER_OK;
}
