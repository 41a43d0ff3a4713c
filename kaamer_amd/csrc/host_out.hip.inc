// host_out.hip.inc — what the host sides of the response writers share (included by search.hip inside its extern "C" block,
// after host_text.hip.inc and before host_tsv.hip.inc and host_json.hip.inc; the kernels' shared part is out_rows.hip.inc):
//   subject_attach                 the skeleton of the two subject attaches (idmap_build, index_idle: host_top_align.hip.inc)
//   OutStage, out_stage_* / out_params / out_launch_tail / out_counts / out_finish   the base of both stages on a stream
// The part of a text call that returns response text is host_out_text.hip.inc, behind both stages.
// the host arrays of a subject table (SubjectTable names them); pad: bytes the device buffer holds behind `bytes`
struct SubjectHost {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len, plen;
    size_t pad = 0;
    uint64_t longest = 0;
    uint32_t features = 0;
};

// The two subject attaches: the distinct entries in the entry order of kaamer_index_attach_proteins (one map serves all
// three), the dense-map limit, the format's host arrays (render), the index idle, the old attach gone, the id map -- the
// first lender that holds this table's, else a new one --, the buffers, the upload; on a failure nothing stays attached.
static int subject_attach(kaamer_index *ix, const kaamer_proteins *p, const char *who, const char *what, SubjectTable &t,
                          std::initializer_list<const std::shared_ptr<IdMap> *> lenders,
                          int (*render)(const kaamer_proteins *, const std::vector<kaamer_protein_entry> &, const char *, SubjectHost &))
{
    HIPCHK(hipSetDevice(ix->device));
    std::vector<uint32_t> uniq;
    std::vector<kaamer_protein_entry> ent;
    int rc = proteins_distinct(p, uniq, ent);
    if (rc) return rc;
    const uint32_t n = (uint32_t)uniq.size();
    const uint64_t map_n = n ? (uint64_t)uniq.back() + 1 : 0;
    if (map_n > (1ull << 31)) return kaamer_fail(KAAMER_E_ARG, "%s: protein ids up to %llu: the id map is dense", who, (unsigned long long)map_n);
    SubjectHost h;
    rc = render(p, ent, who, h);
    if (!rc) rc = index_idle(ix, who);
    if (rc) return rc;
    subject_free(t);   // a second attach replaces the first
    std::shared_ptr<IdMap> map;
    for (const std::shared_ptr<IdMap> *l : lenders)
        if (!map && *l && (*l)->serves(p, n, map_n)) map = *l;
    const bool own = !map;
    rc = reserve_group(nullptr, GROW_EXACT, { want(t.d_bytes, h.bytes.size() + h.pad), want(t.d_off, h.off.size()), want(t.d_len, h.len.size()) });
    if (!rc && !h.plen.empty()) rc = reserve(t.d_plen, h.plen.size(), GROW_EXACT, nullptr);
    if (!rc && own) map = idmap_build(p, uniq, map_n, what, &rc);
    if (rc) { subject_free(t); return rc; }
    hipError_t e = h.bytes.empty() ? hipSuccess : hipMemcpy(t.d_bytes, h.bytes.data(), h.bytes.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t.d_off, h.off.data(), h.off.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t.d_len, h.len.data(), h.len.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !h.plen.empty()) e = hipMemcpy(t.d_plen, h.plen.data(), h.plen.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { subject_free(t); return kaamer_fail(KAAMER_E_HIP, "%s upload: %s", what, hipGetErrorString(e)); }
    t.idmap = map;
    t.entries = n; t.features = h.features; t.longest = h.longest;
    t.table_bytes = h.bytes.size() + h.pad + h.off.size() * 8 + (h.len.size() + h.plen.size()) * 4 + (own ? ((size_t)map_n + 1) * 4 : 0);
    return KAAMER_OK;
}

// ---- the stage base ---------------------------------------------------------------------------------------------------
// What kaamer_tsv_stage and kaamer_json_stage share.  A stage is freed through out_stage_free, which selects the device
// before the buffers go.
struct OutStage {
    kaamer_index *ix = nullptr;
    uint32_t max_queries = 0;
    uint64_t max_units = 0;                   // rows, objects
    DevBuf<unsigned long long> d_tile_bytes, d_tile_units, d_unit_off, d_counts;
    PinnedBuf<unsigned long long> h_counts;
    uint64_t out_cap = 0;                     // of the last call
    DevBuf<uint16_t> d_order;                 // [queries x max_results] of the last call: the -aln rows' hits, the objects' keys
};

extern "C++" {   // (templates: this file is included inside search.hip's extern "C" block)
template <class Stage> static void out_stage_free(Stage *st)
{
    if (!st) return;
    (void)hipSetDevice(st->ix->device);
    delete st;
}

// what: "tsv" / "json"
template <class Stage> static int out_stage_create(kaamer_index *ix, uint32_t max_queries, uint64_t max_units, const char *what, Stage **out)
{
    if (!ix || !out) return kaamer_fail(KAAMER_E_ARG, "%s_stage_create: bad argument", what);
    *out = nullptr;
    HIPCHK(hipSetDevice(ix->device));
    Stage *st = new (std::nothrow) Stage();
    if (!st) return kaamer_fail(KAAMER_E_NOMEM, "%s stage", what);
    st->ix = ix; st->max_queries = max_queries; st->max_units = max_units;
    const size_t tiles = (size_t)max_queries / OUT_TILE + 1;
    const int rc = reserve_group(nullptr, GROW_EXACT, { want(st->d_tile_bytes, tiles), want(st->d_tile_units, tiles), want(st->d_unit_off, (size_t)max_units + 1),
                                                        want(st->d_counts, (size_t)OUT_C_N), want(st->h_counts, (size_t)OUT_C_N) });
    if (rc) { delete st; return rc; }
    *out = st;
    return KAAMER_OK;
}

}   // extern "C++"

// the argument checks every writer makes and the common part of the kernels' parameters.  who: "tsv_rows" / "json_rows";
// positions: the bitmaps are printed (asked: the option's name in the error text); d_unit_off / unit_cap: where the units'
// offsets go; block: the packed result block of the same batch (the text calls), see OutParams
static int out_params(OutStage *st, const char *who, const kaamer_tsv_rows_in *in, bool positions, const char *asked, const SubjectTable &subject, char *d_out,
                      uint64_t out_cap, unsigned long long *d_unit_off, uint64_t unit_cap, const uint8_t *block, OutParams *p)
{
    if (!in || !in->d_n_queries || !in->d_q || !in->top.d_top_cnt || !in->top.d_top_pid || !in->top.d_top_kmatch || !in->top.d_start_position ||
        !in->top.d_size_in_kmer || in->top.max_results < 1 || (in->n_names && (!in->d_spans || !in->d_name_bytes)) || (!d_out && out_cap) ||
        ((uintptr_t)d_out & 15u) || unit_cap < 1)
        return kaamer_fail(KAAMER_E_ARG, "%s: bad argument", who);
    if (positions && (!in->pos || !in->pos->d_pos_base || !in->pos->d_pos_bits_len || !in->pos->d_pos_bits))
        return kaamer_fail(KAAMER_E_ARG, "%s: %s without the bitmaps of the reported hits (kaamer_topn_positions_device)", who, asked);
    if (in->n_queries_cap > st->max_queries) return kaamer_fail(KAAMER_E_ARG, "%s: %u queries, the stage holds %u", who, in->n_queries_cap, st->max_queries);
    p->d_nq = in->d_n_queries; p->nq_cap = in->n_queries_cap; p->q = in->d_q;
    p->top_cnt = in->top.d_top_cnt; p->top_pid = in->top.d_top_pid; p->top_km = in->top.d_top_kmatch;
    p->start_pos = in->top.d_start_position; p->size_out = in->top.d_size_in_kmer; p->K = in->top.max_results;
    p->names = in->d_name_bytes; p->names_len = in->name_bytes_len; p->spans = in->d_spans; p->n_names = in->n_names;
    p->positions = positions ? 1 : 0;
    if (positions) { p->pos_base = in->pos->d_pos_base; p->pos_len = in->pos->d_pos_bits_len; p->pos_bits = in->pos->d_pos_bits; }
    p->idmap = subject.idmap->d; p->idmap_n = subject.idmap->n;
    p->tile_bytes = st->d_tile_bytes; p->tile_units = st->d_tile_units;
    p->unit_off = d_unit_off; p->unit_cap = unit_cap;
    p->out = d_out; p->out_cap = out_cap;
    p->counts = st->d_counts;
    p->block = block;
    st->out_cap = out_cap;
    return KAAMER_OK;
}

// before a writer's first pass: the counts start from 0 (a length pass may set status bits, the scan kernel adds to them)
static int out_clear_counts(OutStage *st, hipStream_t s)
{
    HIPCHK(hipMemsetAsync(st->d_counts, 0, OUT_C_N * 8, s));
    return KAAMER_OK;
}

// behind a writer's last pass: launch errors, and the counts on their way home
static int out_launch_tail(OutStage *st, hipStream_t s)
{
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(st->h_counts, st->d_counts, OUT_C_N * 8, hipMemcpyDeviceToHost, s));
    return KAAMER_OK;
}

// the counts of the last enqueue, once its stream is done; noun: what a unit is called ("rows", "objects")
static int out_counts(const OutStage *st, const char *who, const char *noun, uint64_t counts[2])
{
    if (counts) { counts[0] = st->h_counts[OUT_C_UNITS]; counts[1] = st->h_counts[OUT_C_BYTES]; }
    const unsigned long long status = st->h_counts[OUT_C_STATUS];
    if (status & (OUT_ST_OBJECT | OUT_ST_MISMATCH))
        return kaamer_fail(KAAMER_E_HIP, "%s: status %llu (8: an object of 4 GB; 16: the two passes disagree about an object)", who, status);
    if (status)
        return kaamer_fail(KAAMER_E_CAPACITY, "%s: %llu %s of %llu bytes do not fit (%llu bytes, %llu %s)", who, st->h_counts[OUT_C_UNITS], noun,
                           st->h_counts[OUT_C_BYTES], (unsigned long long)st->out_cap, (unsigned long long)st->max_units, noun);
    return KAAMER_OK;
}

// kaamer_*_rows_finish: the stream done, then the stage's stage_counts(st, counts) (out_counts, and what the stage adds)
extern "C++" template <class Stage> static int out_finish(Stage *st, const char *who, void *stream, uint64_t counts[2])
{
    if (!st) return kaamer_fail(KAAMER_E_ARG, "%s: bad argument", who);
    HIPCHK(hipSetDevice(st->ix->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return stage_counts(st, counts);
}
