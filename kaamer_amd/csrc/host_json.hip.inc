// host_json.hip.inc — the host side of the JSON response (included by search.hip inside its extern "C" block, after
// host_tsv.hip.inc; the attach skeleton and the stage base are host_out.hip.inc's, the kernels are in json_rows.hip.inc, the
// contract and the host formatter in json_format.cpp):
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

// entry i: its HitEntries value at a 16-byte boundary, by the formatter's own code (the device only copies); len: its length
static int subject_json_render(const kaamer_proteins *p, const std::vector<kaamer_protein_entry> &ent, const char *who, SubjectHost &h)
{
    const uint32_t n = (uint32_t)ent.size();
    std::vector<const char *> names;
    for (uint32_t f = 0, nf = kaamer_proteins_n_features(p); f < nf; f++) names.push_back(kaamer_proteins_feature_name(p, f));
    h.off.assign((size_t)n + 1, 0); h.len.assign((size_t)n + 1, 0);
    h.pad = 16;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t need = kaamer_json_protein_value(&ent[i], names.empty() ? nullptr : names.data(), nullptr, 0);
        if (need > 0xFFFFFFF0ull) return kaamer_fail(KAAMER_E_ARG, "%s: an entry of %llu bytes", who, (unsigned long long)need);
        h.off[i] = h.bytes.size();
        h.len[i] = (uint32_t)need;
        h.bytes.resize((size_t)((h.off[i] + need + 1 + 15) & ~15ull), 0);   // (the NUL, then up to the next 16-byte boundary)
        (void)kaamer_json_protein_value(&ent[i], names.empty() ? nullptr : names.data(), reinterpret_cast<char *>(h.bytes.data() + h.off[i]), need + 1);
        if (need > h.longest) h.longest = need;
    }
    h.off[n] = h.bytes.size();
    return KAAMER_OK;
}

int kaamer_index_attach_subject_json(kaamer_index *ix, const kaamer_proteins *p)
{
    if (!ix || !p) return kaamer_fail(KAAMER_E_ARG, "index_attach_subject_json: bad argument");
    return subject_attach(ix, p, "index_attach_subject_json", "subject json", ix->sj, { &ix->st.idmap, &ix->aln_idmap }, subject_json_render);
}

int kaamer_index_subject_json_info(const kaamer_index *ix, uint64_t out[4])
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "index_subject_json_info: bad argument");
    out[0] = ix->sj.table_bytes; out[1] = ix->sj.entries; out[2] = ix->sj.longest; out[3] = 0;
    return KAAMER_OK;
}

void kaamer_json_geometry(uint32_t out[4])
{
    out[0] = OUT_TILE; out[1] = JSON_WIN; out[2] = 16; out[3] = OUT_TILE;
}

struct kaamer_json_stage : OutStage {
    DevBuf<uint32_t> d_obj_len;            // per query
};

void kaamer_json_stage_free(kaamer_json_stage *st) { out_stage_free(st); }

int kaamer_json_stage_create(kaamer_index *ix, uint32_t max_queries, uint64_t max_objects, kaamer_json_stage **out)
{
    int rc = out_stage_create(ix, max_queries, max_objects, "json", out);
    if (!rc) rc = reserve((*out)->d_obj_len, (size_t)max_queries + 1, GROW_EXACT, nullptr);
    if (rc && out && *out) { kaamer_json_stage_free(*out); *out = nullptr; }
    return rc;
}

// the argument checks, the three launches and the copy of the counts; d_obj_off / obj_cap: where the objects' offsets go;
// block: the packed result block of the same batch (the text calls), see OutParams
static int json_enqueue(kaamer_json_stage *st, const kaamer_json_rows_in *jin, char *d_out, uint64_t out_cap, unsigned long long *d_obj_off, uint64_t obj_cap,
                        hipStream_t s, const uint8_t *block = nullptr)
{
    const SubjectTable &t = st->ix->sj;
    if (!t.d_bytes) return kaamer_fail(KAAMER_E_ARG, "json_rows: no subject entries are attached to the index (kaamer_index_attach_subject_json)");
    if (!jin || (jin->aa_len && !jin->d_aa) || (jin->text_format != 0 && jin->text_format != 1)) return kaamer_fail(KAAMER_E_ARG, "json_rows: bad argument");
    const kaamer_tsv_rows_in *in = &jin->rows;
    const bool protein = KAAMER_SEQ_TYPE_BASE(jin->seq_type) == KAAMER_PROTEIN;
    JsonParams p;
    memset(&p, 0, sizeof p);
    int rc = out_params(st, "json_rows", in, !protein || in->extract_positions /* search.go:416 */, "PositionHits", t, d_out, out_cap, d_obj_off, obj_cap, block, &p);
    if (rc) return rc;
    if (in->top.max_results > 65535u) return kaamer_fail(KAAMER_E_ARG, "json_rows: max_results %u, the stage orders up to 65535 keys per query", in->top.max_results);
    rc = reserve(st->d_order, (size_t)in->n_queries_cap * in->top.max_results + 1, GROW_EXACT, s);
    if (!rc) rc = out_clear_counts(st, s);
    if (rc) return rc;
    p.trim = in->top.d_trim; p.aa = jin->d_aa; p.aa_len = jin->aa_len;
    p.protein = protein ? 1 : 0; p.fasta = jin->text_format == 0 ? 1 : 0;
    p.sj_bytes = t.d_bytes; p.sj_off = t.d_off; p.sj_len = t.d_len;
    p.obj_len = st->d_obj_len; p.order = st->d_order;
    const uint32_t tiles = in->n_queries_cap / OUT_TILE + 1;
    hipLaunchKernelGGL(json_len_kernel, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    hipLaunchKernelGGL(out_scan_kernel, dim3(1), dim3(OUT_TILE), 0, s, p, 1u);
    hipLaunchKernelGGL(json_write_kernel, dim3(tiles), dim3(OUT_TILE), 0, s, p);
    return out_launch_tail(st, s);
}

int kaamer_json_rows_device(kaamer_json_stage *st, const kaamer_json_rows_in *in, char *d_out, uint64_t out_cap, void *stream, kaamer_json_rows_result *out)
{
    if (!st || !out) return kaamer_fail(KAAMER_E_ARG, "json_rows_device: bad argument");
    memset(out, 0, sizeof *out);
    HIPCHK(hipSetDevice(st->ix->device));
    const int rc = json_enqueue(st, in, d_out, out_cap, st->d_unit_off, st->max_units + 1, (hipStream_t)stream);
    if (rc) return rc;
    out->d_obj_off = reinterpret_cast<const uint64_t *>(st->d_unit_off.get());
    out->d_counts = reinterpret_cast<const uint64_t *>(st->d_counts.get());
    out->obj_off_capacity = st->max_units + 1;
    return KAAMER_OK;
}

static int stage_counts(const kaamer_json_stage *st, uint64_t counts[2]) { return out_counts(st, "json_rows", "objects", counts); }

int kaamer_json_rows_finish(kaamer_json_stage *st, void *stream, uint64_t counts[2]) { return out_finish(st, "json_rows_finish", stream, counts); }

// the first bounds of the objects on every slot (tests: a first bound too small); 0: the rule
int kaamer_index_set_json_bounds(kaamer_index *ix, uint64_t bytes, uint64_t objects)
{
    if (!ix) return kaamer_fail(KAAMER_E_ARG, "index_set_json_bounds: bad argument");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    for (int i = 0; i < ix->n_top; i++) {
        if (ix->top[i].busy) return kaamer_fail(KAAMER_E_BUSY, "index_set_json_bounds: calls are in flight on the index");
        ix->top[i].guess_bytes[OUT_JSON] = bytes; ix->top[i].guess_units[OUT_JSON] = objects;
    }
    return KAAMER_OK;
}
