// host_top_align.hip.inc — the host side of the alignment of the reported hits (included by search.hip inside its
// extern "C" block, after host_top.hip.inc; the kernels are in top_align.hip.inc):
//   kaamer_index_attach_proteins      HitEntries (search.go:454-470) made resident next to the index
//   ta_stage / ta_enqueue             the stage on a stream: sizing and launches (shared with the sharded handle), one-device form
//   kaamer_topn_align_device          the device-resident form
//   kaamer_*_batch_top_aln_flat       the host-buffer form: top-N + alignment, one packed block, one D2H copy
//   ta_finish_rows / ta_finish_host   floats, the sort by BitScore (search.go:492) and the three rows, on the host, through
//                                     the code kaamer_align_pairs uses (align.hip)
#define TA_DEFAULT_BUDGET (4ull << 30)
#define TA_WAVES_PER_CU 5          /* a sizing rule, not a requirement: AlnWaveLds is 29 KB, five workgroups share a CU's 160 KB of
                                      LDS, and slabs beyond what runs at once would only hold memory (waves take pairs by ticket) */
#define TA_LONG_WAVES_MAX 256u       /* the long-subject kernel: as many slabs as the budget allows, up to this */

// the entries of a protein table, both handles': one per distinct id (uniq, ascending), resolved as kaamer_fetch_hits
// resolves it (a later record with the same id wins)
static int proteins_distinct(const kaamer_proteins *p, std::vector<uint32_t> &uniq, std::vector<kaamer_protein_entry> &ent)
{
    const uint32_t *ids = kaamer_proteins_ids(p);
    uniq = std::vector<uint32_t>(ids, ids + kaamer_proteins_count(p));
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    ent = std::vector<kaamer_protein_entry>(uniq.size());
    return kaamer_fetch_hits(p, uniq.data(), (uint32_t)uniq.size(), ent.data());
}

static_assert(TA_NONE == OUT_NONE, "one id map serves the alignment stage and the response writers");

// a new map for the distinct ids of table p (uniq, ascending; map_n ids), on the device; NULL: *rc.  what: the attach, for
// the error text
static std::shared_ptr<IdMap> idmap_build(const kaamer_proteins *p, const std::vector<uint32_t> &uniq, uint64_t map_n, const char *what, int *rc)
{
    std::shared_ptr<IdMap> m(new (std::nothrow) IdMap());
    if (!m) { *rc = kaamer_fail(KAAMER_E_NOMEM, "id map"); return nullptr; }
    std::vector<uint32_t> host((size_t)map_n + 1, OUT_NONE);
    for (size_t i = 0; i < uniq.size(); i++) host[uniq[i]] = (uint32_t)i;
    *rc = reserve(m->d, host.size(), GROW_EXACT, nullptr);
    if (*rc) return nullptr;
    const hipError_t e = hipMemcpy(m->d, host.data(), host.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { *rc = kaamer_fail(KAAMER_E_HIP, "%s upload: %s", what, hipGetErrorString(e)); return nullptr; }
    m->n = (uint32_t)map_n; m->host = p; m->entries = (uint32_t)uniq.size();
    return m;
}

// nothing of the index may be running when an attach changes: the slots' streams are idle when no slot is busy
static int index_idle(kaamer_index *ix, const char *who)
{
    {
        std::lock_guard<std::mutex> lock(ix->pool_mu);
        for (int i = 0; i < ix->n_top; i++)
            if (ix->top[i].busy) return kaamer_fail(KAAMER_E_BUSY, "%s: calls are in flight on the index", who);
    }
    HIPCHK(hipDeviceSynchronize());
    return KAAMER_OK;
}

int kaamer_index_attach_proteins(kaamer_index *ix, const kaamer_proteins *p)
{
    if (!ix || !p) return kaamer_fail(KAAMER_E_ARG, "index_attach_proteins: bad argument");
    HIPCHK(hipSetDevice(ix->device));
    std::vector<uint32_t> uniq;
    std::vector<kaamer_protein_entry> ent;
    int rc = proteins_distinct(p, uniq, ent);
    if (rc) return rc;
    const uint32_t n = (uint32_t)uniq.size();
    const uint64_t map_n = n ? (uint64_t)uniq.back() + 1 : 0;
    if (map_n > (1ull << 31)) return kaamer_fail(KAAMER_E_ARG, "index_attach_proteins: protein ids up to %llu: the id map is dense", (unsigned long long)map_n);
    std::vector<uint64_t> off((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; i++) off[i + 1] = off[i] + ent[i].sequence_len;
    std::vector<uint8_t> raw((size_t)off[n] + 1, 0), codes((size_t)off[n] + 1, 0), bad((size_t)n + 1, 0);
    uint32_t max_ns = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (ent[i].sequence_len > max_ns) max_ns = ent[i].sequence_len;
        for (uint32_t j = 0; j < ent[i].sequence_len; j++) {
            const int c = ent[i].sequence[j];
            int k = aln_code(c);
            if (k < 0) { bad[i] = 1; k = 0; }
            raw[(size_t)off[i] + j] = (uint8_t)c;
            codes[(size_t)off[i] + j] = (uint8_t)k;
        }
    }
    uint64_t st[3] = {0, 0, 0};
    kaamer_proteins_stats(p, st);
    rc = index_idle(ix, "index_attach_proteins");
    if (rc) return rc;
    const uint64_t budget = ix->aln_budget;
    aln_table_free(ix);   // a second attach replaces the first
    ix->aln_budget = budget;
    rc = reserve_group(nullptr, GROW_EXACT, { want(ix->d_aln_raw, raw.size()), want(ix->d_aln_codes, codes.size()), want(ix->d_aln_bad, bad.size()),
                                              want(ix->d_aln_off, off.size()), want(ix->d_aln_matrix, (size_t)ALN_NL * ALN_NL) });
    if (!rc) ix->aln_idmap = idmap_build(p, uniq, map_n, "protein table", &rc);   // (always its own: the subject attaches take it over)
    if (rc) { aln_table_free(ix); return rc; }
    kaamer_align_matrix(ix->aln_matrix);
    hipError_t e = hipMemcpy(ix->d_aln_raw, raw.data(), raw.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_aln_codes, codes.data(), codes.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_aln_bad, bad.data(), bad.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_aln_off, off.data(), off.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ix->d_aln_matrix, ix->aln_matrix, sizeof ix->aln_matrix, hipMemcpyHostToDevice);
    if (e != hipSuccess) { aln_table_free(ix); return kaamer_fail(KAAMER_E_HIP, "protein table upload: %s", hipGetErrorString(e)); }
    ix->aln_host = p;
    ix->aln_entries = n; ix->aln_max_ns = max_ns;
    ix->aln_number_of_aa = st[1];
    ix->aln_bytes = raw.size() + codes.size() + bad.size() + off.size() * 8 + ((size_t)map_n + 1) * 4 + sizeof ix->aln_matrix;
    return KAAMER_OK;
}

int kaamer_index_align_info(const kaamer_index *cix, uint64_t out[8])
{
    if (!cix || !out) return kaamer_fail(KAAMER_E_ARG, "index_align_info: bad argument");
    kaamer_index *ix = const_cast<kaamer_index *>(cix);
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    out[0] = ix->aln_bytes; out[1] = ix->aln_entries; out[2] = ix->aln_max_ns; out[3] = ix->aln_number_of_aa;
    out[4] = ix->aln_budget ? ix->aln_budget : TA_DEFAULT_BUDGET;
    out[5] = ix->aln_last[0]; out[6] = ix->aln_last[1]; out[7] = ix->aln_last[2];
    return KAAMER_OK;
}

int kaamer_index_set_align_budget(kaamer_index *ix, uint64_t bytes)
{
    if (!ix) return kaamer_fail(KAAMER_E_ARG, "index_set_align_budget: bad argument");
    std::lock_guard<std::mutex> lock(ix->pool_mu);
    ix->aln_budget = bytes;
    return KAAMER_OK;
}

static int ta_check(const kaamer_index *ix, const kaamer_workspace *ws, const kaamer_topn_result *tr, const char *who)
{
    int rc = tp_check(ix, ws, tr, who);   // (a merged result: the queries' residues live on the owner's search workspace)
    if (rc) return rc;
    if (!ix->d_aln_raw) return kaamer_fail(KAAMER_E_ARG, "%s: no protein table is attached to the index (kaamer_index_attach_proteins)", who);
    return KAAMER_OK;
}

// What both forms of the stage share, on one device or on an owner of the sharded handle: first-use buffers, the sizing of
// the direction slabs (the batch's longest query against the table's longest subject, the number of waves from the byte
// budget) and the launches.  `ws` holds the stage's buffers; `p` arrives with the result it aligns, the table, the matrix
// and where the output goes.  sharded != NULL: the pairs come from tas_pairs_kernel (top_align_sharded.hip.inc) instead
// of ta_pairs_kernel.
// marks: NULL, or three timing events recorded before the layout, behind the pairs kernel and behind the last kernel.
static int ta_stage(kaamer_workspace *ws, TaParams p, uint64_t budget, uint32_t table_max_ns, uint32_t max_query_len, const TasParams *sharded,
                    hipStream_t s, uint64_t info[3], const hipEvent_t *marks = nullptr)
{
    {   // first use (pos_cap is fixed per workspace)
        const int rc = reserve_group(s, GROW_EXACT, { want(ws->d_ta_lay, 1), want(ws->d_ta_ctr, 4), want(ws->d_ta_qcodes, (size_t)ws->pos_cap + 64) });
        if (rc) return rc;
    }
    // slabs: the batch's longest query against the table's longest subject, capped at the wave kernel's LDS row
    const uint64_t mq = max_query_len ? max_query_len : 1, strips = (mq + 63) / 64;
    const uint64_t sub = table_max_ns < ALN_WAVE_NS ? (table_max_ns ? table_max_ns : 1) : ALN_WAVE_NS;
    const uint64_t slab = strips * (sub + 63) * 64, opsb = (mq + sub + 63) & ~63ull;
    uint64_t n_waves = budget / (slab + opsb);
    const uint64_t resident = (uint64_t)ws->n_cu * TA_WAVES_PER_CU;
    n_waves = n_waves < 1 ? 1 : (n_waves > resident ? resident : n_waves);
    // (grow-only, each on its own: a buffer that is large enough stays as large as it is)
    int rc = reserve(ws->d_ta_dirs, (size_t)(n_waves * slab), GROW_EXACT, s);
    if (!rc) rc = reserve(ws->d_ta_ops, (size_t)(n_waves * opsb), GROW_EXACT, s);
    uint64_t n_long = 0, lslab = 0, lops = 0, lbnd = 0;
    if (!rc && table_max_ns > ALN_WAVE_NS) {   // the table holds subjects beyond the LDS row: slabs of its longest one
        const uint64_t ns = table_max_ns;
        lslab = strips * (ns + 63) * 64; lops = (mq + ns + 63) & ~63ull; lbnd = 3 * (ns + 1);
        n_long = budget / (lslab + lops + 4 * lbnd);
        n_long = n_long < 1 ? 1 : (n_long > TA_LONG_WAVES_MAX ? TA_LONG_WAVES_MAX : n_long);
        rc = reserve(ws->d_ta_ldirs, (size_t)(n_long * lslab), GROW_EXACT, s);
        if (!rc) rc = reserve(ws->d_ta_lops, (size_t)(n_long * lops), GROW_EXACT, s);
        if (!rc) rc = reserve(ws->d_ta_lbnd, (size_t)(n_long * lbnd), GROW_EXACT, s);
    }
    if (rc) return rc;
    p.qcodes = ws->d_ta_qcodes;
    p.dp_open = kaamer_align_dp_open();
    p.lay = ws->d_ta_lay; p.ctr = ws->d_ta_ctr;
    p.dirs = ws->d_ta_dirs; p.opsbuf = ws->d_ta_ops; p.slab_bytes = slab; p.ops_bytes = opsb;
    if (marks) HIPCHK(hipEventRecord(marks[0], s));
    hipLaunchKernelGGL(ta_layout_kernel, dim3(1), dim3(1), 0, s, p);
    if (sharded) {
        TasParams sp = *sharded;
        sp.qcodes = ws->d_ta_qcodes; sp.tlay = ws->d_ta_lay;
        hipLaunchKernelGGL(tas_pairs_kernel, dim3(ws->n_cu * 8), dim3(256), 0, s, sp);
    } else hipLaunchKernelGGL(ta_pairs_kernel, dim3(ws->n_cu * 8), dim3(256), 0, s, p);
    if (marks) HIPCHK(hipEventRecord(marks[1], s));
    hipLaunchKernelGGL(ta_wave_kernel<false>, dim3((unsigned)n_waves), dim3(64), 0, s, p);
    if (n_long) {
        TaParams pl = p;
        pl.dirs = ws->d_ta_ldirs; pl.opsbuf = ws->d_ta_lops; pl.slab_bytes = lslab; pl.ops_bytes = lops;
        pl.bnd = ws->d_ta_lbnd; pl.bnd_ints = lbnd;
        hipLaunchKernelGGL(ta_wave_kernel<true>, dim3((unsigned)n_long), dim3(64), 0, s, pl);
    }
    if (p.block) hipLaunchKernelGGL(ta_finish_kernel, dim3(1), dim3(1), 0, s, p);
    if (marks) HIPCHK(hipEventRecord(marks[2], s));
    HIPCHK(hipGetLastError());
    info[0] = n_waves; info[1] = slab; info[2] = n_long;
    return KAAMER_OK;
}

// The stage on `s`, behind kaamer_topn_device (and, for the host-buffer form, topn_pack_block / topn_pack_positions).
// eoff: the exclusive scan of top_cnt.  block != NULL: the two sections go behind the packed block; else pair records
// into items[items_cap].
static int ta_enqueue(kaamer_index *ix, kaamer_workspace *ws, const kaamer_topn_result *tr, const uint64_t *eoff, hipStream_t s,
                      uint8_t *block, uint64_t block_cap, uint64_t aln_cap, bool want_text, int gap_open, int gap_extend,
                      uint32_t max_query_len, kaamer_align_pair *items, uint64_t items_cap, uint64_t info[3])
{
    uint64_t budget;
    { std::lock_guard<std::mutex> lock(ix->pool_mu); budget = ix->aln_budget ? ix->aln_budget : TA_DEFAULT_BUDGET; }
    TaParams p;
    memset(&p, 0, sizeof p);
    p.d_nq = ws->d_nq; p.q = ws->d_q;
    p.top_cnt = tr->d_top_cnt; p.top_pid = tr->d_top_pid; p.trim = tr->d_trim; p.K = tr->max_results;
    p.eoff = eoff;
    p.qraw = ws->nucleotide ? ws->d_orf_aa : ws->last_seqs;
    p.tab.raw = ix->d_aln_raw; p.tab.codes = ix->d_aln_codes; p.tab.off = ix->d_aln_off; p.tab.bad = ix->d_aln_bad;
    p.tab.idmap = ix->aln_idmap->d; p.tab.idmap_n = ix->aln_idmap->n;
    p.matrix = ix->d_aln_matrix;
    p.gap_open = gap_open; p.gap_extend = gap_extend;
    p.block = block; p.block_cap = block_cap; p.aln_cap = aln_cap; p.want_text = want_text ? 1 : 0;
    p.items = items; p.items_cap = items_cap;
    p.status = ws->d_status_out;
    const int rc = ta_stage(ws, p, budget, ix->aln_max_ns, max_query_len, nullptr, s, info);
    if (rc) return rc;
    { std::lock_guard<std::mutex> lock(ix->pool_mu); ix->aln_last[0] = info[0]; ix->aln_last[1] = info[1]; ix->aln_last[2] = info[2]; }
    return KAAMER_OK;
}

int kaamer_topn_align_device(kaamer_index *ix, kaamer_workspace *ws, const kaamer_topn_result *top, const kaamer_topn_align_opts *opts,
                             void *stream, kaamer_topn_alignments *out)
{
    if (!opts || !out) return kaamer_fail(KAAMER_E_ARG, "topn_align_device: bad argument");
    int rc = ta_check(ix, ws, top, "topn_align_device");
    if (rc) return rc;
    char name[sizeof opts->sub_matrix + 1];
    memcpy(name, opts->sub_matrix, sizeof opts->sub_matrix);
    name[sizeof opts->sub_matrix] = 0;
    double lambda = 0, kk = 0;
    if (!kaamer_align_options(name, opts->gap_open, opts->gap_extend, &lambda, &kk))
        return kaamer_fail(KAAMER_E_ARG, "topn_align_device: No matrix found (or not BLOSUM62)");
    HIPCHK(hipSetDevice(ws->device));
    const bool on_count_stream = ws->split_pending && ws->count_stream;
    hipStream_t s = on_count_stream ? ws->count_stream : (hipStream_t)stream;
    uint64_t cap = opts->max_pairs;
    if (!cap) { cap = (uint64_t)ws->q_cap * top->max_results; if (ws->hit_cap && ws->hit_cap < cap) cap = ws->hit_cap; }
    rc = reserve(ws->d_ta_eoff, (size_t)ws->q_cap + 1, GROW_EXACT, s);   // (q_cap is fixed per workspace)
    if (!rc) rc = reserve(ws->d_ta_items, (size_t)cap, GROW_EXACT, s);
    if (rc) return rc;
    scan_u32_on(ws, top->d_top_cnt, ws->d_nq, ws->q_cap, ws->d_ta_eoff, s);
    uint64_t mq = opts->max_query_len ? opts->max_query_len : ws->opts.max_seq_bytes;
    if (mq > 0x3FFFFFFFull) mq = 0x3FFFFFFFull;
    uint64_t info[3];
    rc = ta_enqueue(ix, ws, top, ws->d_ta_eoff, s, nullptr, 0, 0, false, opts->gap_open, opts->gap_extend, (uint32_t)mq, ws->d_ta_items, cap, info);
    if (rc) return rc;
    if (on_count_stream) HIPCHK(hipEventRecord(ws->ev_count, s));
    out->d_pair_off = ws->d_ta_eoff;
    out->d_pairs = ws->d_ta_items;
    out->pair_capacity = cap;
    out->n_waves = (uint32_t)info[0]; out->n_long_waves = (uint32_t)info[2];
    out->slab_bytes = info[1];
    return KAAMER_OK;
}

// ---- the host-buffer form ---------------------------------------------------------------------------------------------
// the stage of one ticket, behind its packed block (called by top_enqueue)
static int top_enqueue_alignments(kaamer_ticket *t, TopSlot &h, const kaamer_topn_result *tr, hipStream_t s)
{
    int rc = ta_check(t->ix, h.ws, tr, "search_batch_top_aln");
    if (rc) return rc;
    uint64_t info[3];
    return ta_enqueue(t->ix, h.ws, tr, h.ws->d_rep_eoff, s, h.d_block, h.block_use, t->aln_cap, t->aln.text, t->aln.gap_open, t->aln.gap_extend,
                      t->max_query_len, nullptr, 0, info);
}

// what the block's two sections may take on the first attempt (a batch beyond it is repeated with what it needed)
static uint64_t ta_first_cap(const kaamer_ticket *t, const TopSlot &h)
{
    if (h.aln_guess) return h.aln_guess;
    const uint64_t K = t->top.max_results;
    if (is_nucl(t->seq_type)) return (1ull << 20) + t->seq_bytes / 4;
    return (uint64_t)t->n_seqs * K * sizeof(kaamer_align_pair) + (t->aln.text ? 2 * K * t->seq_bytes : 0) + 4096;
}

// after the stream is done and the batch's status is fine: 1 = the sections were too small, repeat with t->aln_cap grown
static int ta_needs_repeat(kaamer_ticket *t, TopSlot &h)
{
    const RepAlnExt *x = rep_aln_ext(reinterpret_cast<const RepBlockHdr *>(t->h_block));
    h.aln_guess = x->need_bytes + x->need_bytes / 4 + 4096;
    if (x->need_bytes <= x->cap_bytes && x->off_items) return 0;
    t->aln_cap = x->need_bytes + x->need_bytes / 4 + 65536;
    return 1;
}

// what the host finish needs beside the result: the request, the borrowed table, and where protein queries' residues are
struct TaFinish {
    const kaamer_proteins *table;
    const int *matrix;
    uint64_t number_of_aa;
    TopAlnRequest rq;
    bool nucl;
    const uint8_t *h_in;   // the staging copy of the batch input (protein queries)
};

// floats, sort and rows of a finished result, for both forms: bo->pub is complete; items / ops are the pair records and
// operations parallel to its CSR entries; pos_off: the bitmaps' offsets to permute with the hits (or NULL)
static int ta_finish_rows(const TaFinish &f, batch_top_owner *bo, const kaamer_align_pair *items, const uint8_t *ops, uint64_t ops_bytes, uint64_t *pos_off)
{
    const kaamer_batch_top &r = bo->pub;
    const uint64_t n_ent = r.top_off[r.n_reported];
    kaamer_alignment zero;
    memset(&zero, 0, sizeof zero);
    bo->aln.assign((size_t)n_ent, zero);
    bo->has_aln = true;
    bo->has_text = f.rq.text;
    if (!f.rq.on) {   // "No matrix found": every hit keeps the empty AlignmentResult, in sortMapByValue order
        for (kaamer_alignment &a : bo->aln) a.status = 1;
        return KAAMER_OK;
    }
    uint32_t *pid = const_cast<uint32_t *>(r.top_pid), *km = const_cast<uint32_t *>(r.top_kmatch), *fp = const_cast<uint32_t *>(r.top_first_pos);
    std::vector<uint32_t> order;
    std::vector<kaamer_alignment> tmp_a;
    std::vector<uint32_t> tmp_u;
    std::vector<uint64_t> tmp_o;
    for (uint32_t i = 0; i < r.n_reported; i++) {
        const uint64_t a = r.top_off[i], b = r.top_off[i + 1];
        // Query.Sequence: the reported ORF's residues in the block, or the record in the staging copy of the batch input
        const uint8_t *qraw = f.nucl ? r.orf_aa + r.q[i].aa_off : f.h_in + r.q[i].aa_off;
        for (uint64_t e = a; e < b; e++) {
            const kaamer_align_pair &it = items[e];
            kaamer_alignment &al = bo->aln[(size_t)e];
            if (it.status != 0) { al.status = it.status; continue; }   // the empty AlignmentResult (BitScore 0)
            kaamer_align_ints ti;
            ti.n_ops = it.n_ops; ti.start_i = it.start_i; ti.start_j = it.start_j; ti.end_i = it.end_i; ti.end_j = it.end_j;
            ti.identical = it.identical; ti.similar = it.similar; ti.mismatches = it.mismatches; ti.gap_openings = it.gap_openings; ti.raw = it.raw;
            kaamer_align_finish(&al, &ti, it.query_len, f.number_of_aa, f.rq.lambda, f.rq.kk);
            if (f.rq.text) {
                al.aln_off = bo->aln_text.size();
                if (it.n_ops > 0) {
                    kaamer_protein_entry pe;
                    const int rc = kaamer_fetch_hits(f.table, &pid[e], 1, &pe);
                    if (rc) return rc;
                    if (!pe.found || it.off + (uint64_t)it.n_ops > ops_bytes) return kaamer_fail(KAAMER_E_FORMAT, "search_batch_top_aln: inconsistent result block");
                    bo->aln_text.resize(bo->aln_text.size() + 3 * (size_t)it.n_ops);
                    kaamer_align_rows(ops + it.off, it.n_ops, qraw, pe.sequence, it.start_i, it.start_j, f.matrix, f.rq.gap_open, f.rq.gap_extend,
                                      bo->aln_text.data() + al.aln_off, nullptr);
                }
            }
        }
        // sort.Slice by BitScore, descending (search.go:492); ties keep sortMapByValue's order
        const size_t n = (size_t)(b - a);
        order.resize(n);
        for (size_t k = 0; k < n; k++) order[k] = (uint32_t)k;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t u, uint32_t v) { return bo->aln[(size_t)a + u].bitscore > bo->aln[(size_t)a + v].bitscore; });
        bool same = true;
        for (size_t k = 0; k < n; k++) same = same && order[k] == k;
        if (same) continue;
        tmp_a.assign(bo->aln.begin() + (size_t)a, bo->aln.begin() + (size_t)b);
        for (size_t k = 0; k < n; k++) bo->aln[(size_t)a + k] = tmp_a[order[k]];
        for (uint32_t *arr : { pid, km, fp }) {
            tmp_u.assign(arr + a, arr + b);
            for (size_t k = 0; k < n; k++) arr[a + k] = tmp_u[order[k]];
        }
        if (pos_off) {
            tmp_o.assign(pos_off + a, pos_off + b);
            for (size_t k = 0; k < n; k++) pos_off[a + k] = tmp_o[order[k]];
        }
    }
    return KAAMER_OK;
}

// the floats and coordinates of ta_finish_rows on pair records the caller holds (read back from kaamer_topn_align_device, or
// built by hand): out[i] is what a result would carry for pairs[i]
int kaamer_align_finish_pairs(const kaamer_align_pair *pairs, uint64_t n, uint64_t number_of_aa, const char *sub_matrix, int32_t gap_open,
                              int32_t gap_extend, kaamer_alignment *out)
{
    if ((n && (!pairs || !out)) || !sub_matrix) return kaamer_fail(KAAMER_E_ARG, "align_finish_pairs: bad argument");
    double lambda = 0, kk = 0;
    const bool on = kaamer_align_options(sub_matrix, gap_open, gap_extend, &lambda, &kk);
    for (uint64_t e = 0; e < n; e++) {
        const kaamer_align_pair &it = pairs[e];
        kaamer_alignment &al = out[e];
        memset(&al, 0, sizeof al);
        if (!on) { al.status = 1; continue; }
        if (it.status != 0) { al.status = it.status; continue; }   // the empty AlignmentResult (BitScore 0)
        kaamer_align_ints ti;
        ti.n_ops = it.n_ops; ti.start_i = it.start_i; ti.start_j = it.start_j; ti.end_i = it.end_i; ti.end_j = it.end_j;
        ti.identical = it.identical; ti.similar = it.similar; ti.mismatches = it.mismatches; ti.gap_openings = it.gap_openings; ti.raw = it.raw;
        kaamer_align_finish(&al, &ti, it.query_len, number_of_aa, lambda, kk);
    }
    return KAAMER_OK;
}

// the finish of a one-device result (bo's block is complete; the slot is still the ticket's)
static int ta_finish_host(const kaamer_ticket *t, const TopSlot &h, batch_top_owner *bo)
{
    kaamer_index *ix = t->ix;
    TaFinish f;
    f.table = ix->aln_host; f.matrix = ix->aln_matrix; f.number_of_aa = ix->aln_number_of_aa;
    f.rq = t->aln; f.nucl = is_nucl(t->seq_type);
    f.h_in = h.h_in;
    const RepBlockHdr *hdr = reinterpret_cast<const RepBlockHdr *>(bo->block);
    const RepAlnExt *x = rep_aln_ext(hdr);
    const RepPosExt *px = rep_pos_ext(hdr);
    uint64_t *pos_off = bo->has_pos && px->off_pos_bits ? reinterpret_cast<uint64_t *>(bo->block + px->off_pos_off) : nullptr;
    return ta_finish_rows(f, bo, reinterpret_cast<const kaamer_align_pair *>(bo->block + x->off_items), bo->block + x->off_ops, x->ops_bytes, pos_off);
}

int kaamer_submit_batch_top_aln_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                     double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t want_positions,
                                     const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text, kaamer_ticket **ticket)
{
    if (!ix || !sub_matrix || !ticket) return kaamer_fail(KAAMER_E_ARG, "submit_batch_top_aln: bad argument");
    if (!ix->d_aln_raw) return kaamer_fail(KAAMER_E_ARG, "submit_batch_top_aln: no protein table is attached to the index (kaamer_index_attach_proteins)");
    kaamer_batch_in in;
    kaamer_topn_opts top;
    flat_in(&in, seqs, offsets, n_seqs, seq_type, want_positions ? 1 : 0);
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    const TopAlnRequest rq = top_aln_request(sub_matrix, gap_open, gap_extend, want_text);
    return top_submit(ix, &in, &top, true, ticket, want_positions != 0, &rq);
}

int kaamer_search_batch_top_aln_flat(kaamer_index *ix, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                     double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t want_positions,
                                     const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text, kaamer_batch_top **out)
{
    if (!out) return kaamer_fail(KAAMER_E_ARG, "search_batch_top_aln: bad argument");
    *out = nullptr;
    kaamer_ticket *t = nullptr;
    const int rc = kaamer_submit_batch_top_aln_flat(ix, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, want_positions,
                                                    sub_matrix, gap_open, gap_extend, want_text, &t);
    if (rc) return rc;
    return kaamer_wait_batch_top(t, out);
}

// kaamer_stream_* with the alignment of every reported hit (FastqSearch / ProteinSearch with -aln over chunks,
// search_fastq.go:60-136 + search.go:483-494): a push goes the way kaamer_submit_batch_top_aln_flat goes
int kaamer_stream_open_aln_flat(kaamer_index *ix, int32_t seq_type, double min_k_ratio, int64_t min_k_match, uint32_t max_results,
                                int32_t want_positions, const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text,
                                kaamer_stream **out)
{
    if (!ix || !sub_matrix || !out) return kaamer_fail(KAAMER_E_ARG, "stream_open_aln: bad argument");
    *out = nullptr;
    if (!ix->d_aln_raw) return kaamer_fail(KAAMER_E_ARG, "stream_open_aln: no protein table is attached to the index (kaamer_index_attach_proteins)");
    const int rc = kaamer_stream_open_flat(ix, seq_type, min_k_ratio, min_k_match, max_results, out);
    if (rc) return rc;
    (*out)->want_pos = want_positions != 0;
    (*out)->want_aln = true;
    (*out)->aln = top_aln_request(sub_matrix, gap_open, gap_extend, want_text);
    return KAAMER_OK;
}

int kaamer_batch_top_alignments(const kaamer_batch_top *out, const kaamer_alignment **items, const char **text)
{
    if (items) *items = nullptr;
    if (text) *text = nullptr;
    if (!out) return kaamer_fail(KAAMER_E_ARG, "batch_top_alignments: bad argument");
    const batch_top_owner *bo = reinterpret_cast<const batch_top_owner *>(out);  // pub is the first member
    if (!bo->has_aln) return KAAMER_OK;   // a call without alignments: both NULL
    static const kaamer_alignment none = {};
    if (items) *items = bo->aln.empty() ? &none : bo->aln.data();
    static const char no_text[1] = { 0 };
    if (text && bo->has_text) *text = bo->aln_text.empty() ? no_text : bo->aln_text.data();
    return KAAMER_OK;
}
