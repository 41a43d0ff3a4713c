// host_sharded_collect.hip.inc — the wait side of the one-process sharded driver (included by search.hip inside its
// extern "C" block, after host_sharded_submit.hip.inc): an attempt is waited for and checked, what it needed is kept for
// the next call, the W owners' results are interleaved into batch order; a bound that was too small grows and the batch
// runs again from the set's staging.

// the shards' work counters, summed: lookups, probes, postings are those of the shards' searches (every key is looked up by
// one shard); inputs and queries one shard's; n_hits is the caller's (those of the merged results)
static int sharded_sum_counters(std::vector<ShardState> &sh, kaamer_counters *c)
{
    memset(c, 0, sizeof *c);
    for (size_t d = 0; d < sh.size(); d++) {
        kaamer_counters sc;
        HIPCHK(hipSetDevice(sh[d].device));
        HIPCHK(hipMemcpy(&sc, sh[d].ws->d_counters, sizeof sc, hipMemcpyDeviceToHost));
        c->n_lookup += sc.n_lookup; c->n_probe += sc.n_probe; c->n_found += sc.n_found; c->n_post += sc.n_post;
        c->n_lists += sc.n_lists; c->n_list_ids += sc.n_list_ids; c->n_overflow += sc.n_overflow;
        if (d == 0) { c->n_in = sc.n_in; c->n_queries = sc.n_queries; }
    }
    return KAAMER_OK;
}

// Which bound: the first shard whose own search status word says what ran out there (*sst; sh.size(): none does).  Every
// shard's stream is waited for; a shard that failed may have left per-batch state behind.
static uint32_t sharded_failed_shard(std::vector<ShardState> &sh, uint32_t *sst)
{
    uint32_t bad = (uint32_t)sh.size();
    for (uint32_t s = 0; s < sh.size(); s++) {
        uint32_t st = 0;
        (void)hipSetDevice(sh[s].device);
        (void)hipStreamSynchronize(sh[s].stream);
        if (hipMemcpy(&st, sh[s].ws->d_status_out, 4, hipMemcpyDeviceToHost) != hipSuccess || !st) continue;
        sh[s].ws->clean = false;
        if (bad == sh.size()) { bad = s; *sst = st; }
    }
    return bad;
}

// what this batch's exchange blocks needed (every owner read the same W x W figures): sizes the next call's blocks
static void sharded_record_exchange_need(ShardSet *set)
{
    uint64_t st4[4];
    if (kaamer_exchange_stats(set->sh[0].mws, 0, st4) == KAAMER_OK) { set->need_queries = (uint32_t)st4[1]; set->need_entries = st4[2]; }
}

static inline const RepBlockHdr *owner_hdr(const ShardState &ow) { return reinterpret_cast<const RepBlockHdr *>(ow.h_block); }

// ---- a top call -------------------------------------------------------------------------------------------------------
// every owner's stream is waited for and its block's status read; the rest of a good block is fetched.  The first failed
// owner's error goes to *err with its text in `why`: the caller returns it once the batch's needs are recorded.
static int sharded_check_owners(kaamer_sharded_ticket *t, int *err, char *why, size_t why_n)
{
    std::vector<ShardState> &sh = t->set->sh;
    const uint32_t W = t->sx->n;
    t->pos_only = true;   // (read only on the KAAMER_E_CAPACITY path of kaamer_sharded_wait_batch_top: cleared by any other failure bit)
    t->cap_bits = 0; t->grow_sections = false;
    for (uint32_t d = 0; d < W; d++) {
        ShardState &ow = sh[d];
        HIPCHK(hipSetDevice(ow.device));
        HIPCHK(hipStreamSynchronize(ow.stream));
        const RepBlockHdr *hdr = owner_hdr(ow);
        const uint32_t status = hdr->status & 0x7FFFFFFFu;
        if (hdr->status & ~(uint32_t)(ST_POS_CAP | ST_IDS_CAP | ST_SEG_CAP)) t->pos_only = false;
        t->cap_bits |= hdr->status;
        if (status) { ow.mws->clean = false; ow.ws->clean = false; }
        int rc = status_to_error(status, ow.mws);
        if (!rc && (hdr->status & 0x80000000u)) rc = kaamer_fail(KAAMER_E_CAPACITY, "result block capacity exceeded");
        if (rc) {
            if (!*err) {
                // which bound: the owner's merge status says "a peer failed" or "a block overflowed"; the shards' own
                // search status words say what ran out there (ADVICE r3: a generic message hid a hit pool that never grew)
                uint32_t sst = 0;
                const uint32_t bad = sharded_failed_shard(sh, &sst);
                if (bad < W)
                    snprintf(why, why_n, "shard %u: search status 0x%x (%s%s%s)", bad, sst, (sst & ST_POOL_FULL) ? "hit pool " : "",
                             (sst & (ST_G_ARENA_FULL | ST_G_TABLE_FULL)) ? "G-tier arena " : "", (sst & (ST_QUERY_CAP | ST_AA_CAP)) ? "ORF capacity " : "");
                else
                    snprintf(why, why_n, "owner %u: merge status 0x%x (%s)", d, status,
                             (status & ST_SEG_CAP) ? "the reported hits' subjects exceed a segment" :
                             (status & ST_POS_CAP) ? "the reported hits' bitmaps exceed a segment" :
                             (status & ST_IDS_CAP) ? "the reported hits' ids exceed an ids block" :
                             (status & ST_EXCHANGE_CAP) ? "an exchange block overflowed" : "merge bounds");
                *err = rc;
            }
            continue;
        }
        rc = rep_block_fetch_rest(ow.d_block, &ow.guess, &ow.h_block, &ow.h_block_cap, &ow.copied, ow.stream);
        if (rc) return rc;
    }
    return KAAMER_OK;
}

// what the ids blocks and subject segments of this batch needed (the block headers and the holders' counts hold it,
// whatever became of the batch), and the figures of kaamer_sharded_align_info / _align_stage_info
static int sharded_record_needs(kaamer_sharded_ticket *t)
{
    ShardSet *set = t->set;
    std::vector<ShardState> &sh = set->sh;
    const uint32_t W = t->sx->n;
    sharded_record_exchange_need(set);
    if (tpos_or_aln(t)) {
        set->need_ids_rq = 0; set->need_ids_ent = 0;
        for (uint32_t d = 0; d < W; d++) {
            const RepBlockHdr *hdr = owner_hdr(sh[d]);
            if (hdr->n_rep > set->need_ids_rq) set->need_ids_rq = hdr->n_rep;
            if (hdr->n_ent > set->need_ids_ent) set->need_ids_ent = hdr->n_ent;
        }
    }
    if (!t->b.aln) return KAAMER_OK;
    // ... and the payload of the largest subject segment, as its holder counted it
    std::vector<unsigned long long> nd((size_t)2 * W);
    uint64_t need = 0;
    for (uint32_t s = 0; s < W; s++) {
        HIPCHK(hipSetDevice(sh[s].device));
        HIPCHK(hipMemcpy(nd.data(), sh[s].d_sa_need, nd.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t d = 0; d < W; d++) if (nd[2 * d] > need) need = nd[2 * d];
    }
    set->need_sa_bytes = need;
    set->sa_seen = true;
    set->sa_seg_bytes = tas_seg_bytes(sh[0].sa_wire);
    set->sa_need_seg = 16 + 8ull * ((uint64_t)set->need_ids_rq + 1) + 4ull * set->need_ids_ent + need;
    set->sa_attempts = (uint64_t)t->attempt + 1;
    set->sa_ids_bytes = 4ull * tps_ids_words(sh[0].ids_wire);
    for (int k = 0; k < 3; k++) { set->sa_us[k] = 0; set->sa_stage[k] = 0; }
    for (uint32_t d = 0; d < W; d++) {
        for (int k = 0; k < 3; k++) if (sh[d].sa_stage[k] > set->sa_stage[k]) set->sa_stage[k] = sh[d].sa_stage[k];
        if (!sh[d].timed) continue;
        const int from[3] = { 0, 2, 3 }, to[3] = { 1, 3, 4 };
        for (int k = 0; k < 3; k++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, sh[d].ev_t[from[k]], sh[d].ev_t[to[k]]) != hipSuccess) { (void)hipGetLastError(); continue; }
            const uint64_t us = (uint64_t)(ms * 1000.0f);
            if (us > set->sa_us[k]) set->sa_us[k] = us;
        }
    }
    return KAAMER_OK;
}

// ... and what a batch that passed says about the next one: the alignment sections of the owners' blocks (one that was
// too small: KAAMER_E_CAPACITY, the batch once more with what they needed), the bitmap segments
static int sharded_record_reported_needs(kaamer_sharded_ticket *t, const std::vector<const RepAlnExt *> &ax, const std::vector<const RepPosExt *> &px)
{
    ShardSet *set = t->set;
    std::vector<ShardState> &sh = set->sh;
    const uint32_t W = t->sx->n;
    if (t->b.aln) {
        uint64_t need = 0;
        bool small = false;
        for (uint32_t d = 0; d < W; d++) {
            sh[d].aln_guess = ax[d]->need_bytes + ax[d]->need_bytes / 4 + 4096;
            if (ax[d]->need_bytes > need) need = ax[d]->need_bytes;
            if (ax[d]->need_bytes > ax[d]->cap_bytes || !ax[d]->off_items) small = true;
        }
        if (small) {
            t->grow_sections = true;
            t->b.aln_cap = need + need / 4 + 65536;
            return kaamer_fail(KAAMER_E_CAPACITY, "sharded search: the alignment sections of a result block (%llu bytes needed)", (unsigned long long)need);
        }
    }
    if (t->b.tpos) {
        set->need_tp_words = 0;
        for (uint32_t d = 0; d < W; d++) {
            if (!px[d]->off_pos_bits) return kaamer_fail(KAAMER_E_HIP, "sharded search: owner %u returned a block without its bitmap sections", d);
            if (px[d]->n_pos_words > set->need_tp_words) set->need_tp_words = px[d]->n_pos_words;
        }
        set->tp_seen = true;
        set->tp_ids_bytes = 4ull * tps_ids_words(sh[0].ids_wire);
        set->tp_seg_bytes = 8ull * (sh[0].tp_wire + 1);
        set->tp_attempts = (uint64_t)t->attempt + 1;
    }
    return KAAMER_OK;
}

// the owners' pair records in batch order; their operations one owner behind the other, the records' offsets re-based
struct ShardedMergedAln {
    std::vector<kaamer_align_pair> items;
    std::vector<uint8_t> ops;
    uint64_t ops_bytes = 0;
    bool bad = false;              // a record points beyond its owner's operations
    uint64_t *pos_off = nullptr;   // the merged bitmaps' offsets (ta_finish_rows permutes them with the hits)
};

// ---- interleave the owners' reported queries back into batch order (query q is owned by shard q mod W): host memory
// only.  view[d], px[d], ax[d]: owner d's block and its two extensions; *out: the merged result, its counters left zero.
static int sharded_interleave(const std::vector<batch_top_owner> &view, const std::vector<const RepPosExt *> &px, const std::vector<const RepAlnExt *> &ax,
                              bool nucl, bool tpos, bool aln, bool aln_text, uint32_t max_results, batch_top_owner **out, ShardedMergedAln *am)
{
    const uint32_t W = (uint32_t)view.size();
    uint64_t n_rep = 0, n_ent = 0, n_aa = 0, nq = 0, n_words = 0;
    for (uint32_t d = 0; d < W; d++) {
        n_rep += view[d].pub.n_reported;
        n_ent += view[d].pub.top_off[view[d].pub.n_reported];
        nq += view[d].pub.n_queries;
        n_aa += reinterpret_cast<const RepBlockHdr *>(view[d].block)->n_aa;
        if (tpos) n_words += px[d]->n_pos_words;
    }
    const size_t o_rq = 0, o_trim = rep_align8(o_rq + 4 * n_rep), o_q = rep_align8(o_trim + 4 * n_rep),
                 o_off = rep_align8(o_q + sizeof(kaamer_query_meta) * n_rep), o_pid = o_off + 8 * (n_rep + 1), o_km = rep_align8(o_pid + 4 * n_ent),
                 o_fp = rep_align8(o_km + 4 * n_ent), o_aa = rep_align8(o_fp + 4 * n_ent), o_plen = rep_align8(o_aa + n_aa) + 8,
                 o_poff = rep_align8(o_plen + (tpos ? 4 * n_rep : 0)), o_pbits = o_poff + (tpos ? 8 * (n_ent + 1) : 0),
                 total = o_pbits + (tpos ? 8 * n_words : 0) + 8;
    batch_top_owner *bo = new (std::nothrow) batch_top_owner();
    uint8_t *blk = bo ? (uint8_t *)malloc(total) : nullptr;
    if (!bo || !blk) { delete bo; free(blk); return kaamer_fail(KAAMER_E_NOMEM, "merged result (%zu bytes)", total); }
    bo->block = blk; bo->block_cap = total; bo->pinned = false;
    uint32_t *rq = (uint32_t *)(blk + o_rq);
    int32_t *trim = (int32_t *)(blk + o_trim);
    kaamer_query_meta *qm = (kaamer_query_meta *)(blk + o_q);
    uint64_t *off = (uint64_t *)(blk + o_off);
    uint32_t *pid = (uint32_t *)(blk + o_pid), *km = (uint32_t *)(blk + o_km), *fp = (uint32_t *)(blk + o_fp);
    uint8_t *aa = blk + o_aa;
    int32_t *plen = (int32_t *)(blk + o_plen);
    uint64_t *poff = (uint64_t *)(blk + o_poff), *pbits = (uint64_t *)(blk + o_pbits);
    std::vector<uint64_t> ops_base(W + 1, 0);
    if (aln) {
        am->items.resize((size_t)n_ent);
        for (uint32_t d = 0; d < W; d++) ops_base[d + 1] = ops_base[d] + ax[d]->ops_bytes;
        am->ops.resize((size_t)ops_base[W] + 1);
        for (uint32_t d = 0; d < W; d++)
            if (ax[d]->ops_bytes) memcpy(am->ops.data() + ops_base[d], view[d].block + ax[d]->off_ops, (size_t)ax[d]->ops_bytes);
        am->ops_bytes = ops_base[W];
    }
    std::vector<uint32_t> cur(W, 0);
    uint64_t r = 0, e = 0, a = 0, w = 0;
    for (;;) {  // W-way merge by global query index (each owner's list ascends)
        uint32_t best = W;
        uint64_t best_q = ~0ull;
        for (uint32_t d = 0; d < W; d++)
            if (cur[d] < view[d].pub.n_reported) {
                const uint64_t gq = (uint64_t)d + (uint64_t)view[d].pub.rep_query[cur[d]] * W;
                if (gq < best_q) { best_q = gq; best = d; }
            }
        if (best == W) break;
        const kaamer_batch_top &v = view[best].pub;
        const uint32_t i = cur[best]++;
        const uint64_t b0 = v.top_off[i], b1 = v.top_off[i + 1];
        rq[r] = (uint32_t)best_q;
        trim[r] = v.trim[i];
        qm[r] = v.q[i];
        off[r] = e;
        memcpy(pid + e, v.top_pid + b0, (b1 - b0) * 4);
        memcpy(km + e, v.top_kmatch + b0, (b1 - b0) * 4);
        memcpy(fp + e, v.top_first_pos + b0, (b1 - b0) * 4);
        if (aln) {
            const kaamer_align_pair *src = reinterpret_cast<const kaamer_align_pair *>(view[best].block + ax[best]->off_items);
            for (uint64_t j = b0; j < b1; j++) {
                kaamer_align_pair it = src[j];
                if (it.status == 0 && it.n_ops > 0 && aln_text) {
                    if (it.off + (uint64_t)it.n_ops > ax[best]->ops_bytes) am->bad = true;
                    it.off += ops_base[best];
                }
                am->items[(size_t)(e + (j - b0))] = it;
            }
        }
        if (tpos) {   // the owner's bitmaps of the query are contiguous: re-based as a whole
            const uint8_t *ob = view[best].block;
            const uint64_t *v_off = reinterpret_cast<const uint64_t *>(ob + px[best]->off_pos_off);
            const uint64_t w0 = v_off[b0], w1 = v_off[b1];
            plen[r] = reinterpret_cast<const int32_t *>(ob + px[best]->off_pos_len)[i];
            for (uint64_t j = b0; j < b1; j++) poff[e + (j - b0)] = w + (v_off[j] - w0);
            memcpy(pbits + w, reinterpret_cast<const uint64_t *>(ob + px[best]->off_pos_bits) + w0, (w1 - w0) * 8);
            w += w1 - w0;
        }
        e += b1 - b0;
        if (nucl) {
            memcpy(aa + a, v.orf_aa + v.q[i].aa_off, v.q[i].aa_len);
            qm[r].aa_off = a;
            a += v.q[i].aa_len;
        }
        r++;
    }
    off[r] = e;
    if (tpos) {
        poff[e] = w;
        bo->has_pos = true;
        bo->m_pos_len = plen; bo->m_pos_off = poff; bo->m_pos_bits = pbits;
    }
    am->pos_off = tpos ? poff : nullptr;
    memset(&bo->pub, 0, sizeof bo->pub);
    bo->pub.n_queries = (uint32_t)nq;
    bo->pub.n_reported = (uint32_t)n_rep;
    bo->pub.max_results = max_results;
    bo->pub.rep_query = rq; bo->pub.trim = trim; bo->pub.q = qm; bo->pub.top_off = off;
    bo->pub.top_pid = pid; bo->pub.top_kmatch = km; bo->pub.top_first_pos = fp;
    bo->pub.orf_aa = nucl ? aa : nullptr;
    *out = bo;
    return KAAMER_OK;
}

// floats, rows and the sort by BitScore on the combined result: the one-device call's finish
static int sharded_finish_align(const kaamer_sharded_ticket *t, batch_top_owner *bo, const ShardedMergedAln &am)
{
    const kaamer_sharded_index *sx = t->sx;
    TaFinish f;
    f.table = sx->aln_host; f.matrix = sx->aln_matrix; f.number_of_aa = sx->aln_number_of_aa;
    f.rq = t->aln; f.nucl = is_nucl(t->seq_type);
    f.h_in = t->set->h_in;
    if (am.bad) return kaamer_fail(KAAMER_E_FORMAT, "sharded search: inconsistent alignment sections");
    return ta_finish_rows(f, bo, am.items.data(), am.ops.data(), am.ops_bytes, am.pos_off);
}

// waits for the attempt, checks it, fetches what the speculative copies missed and interleaves the owners' reported
// queries back into batch order.  KAAMER_E_CAPACITY: a bound was too small (the message says which, on which shard).
static int sharded_collect(kaamer_sharded_ticket *t, kaamer_batch_top **out)
{
    std::vector<ShardState> &sh = t->set->sh;
    const uint32_t W = t->sx->n;
    ShardSyncGuard guard{ t->set, true };
    int err = KAAMER_OK;
    char why[256] = "";
    int rc = sharded_check_owners(t, &err, why, sizeof why);
    if (rc) return rc;
    guard.armed = false;  // every stream has been waited for
    rc = sharded_record_needs(t);
    if (rc) return rc;
    if (err) return kaamer_fail(err, "sharded search: %s", why);
    std::vector<batch_top_owner> view(W);
    std::vector<const RepPosExt *> px(W);
    std::vector<const RepAlnExt *> ax(W);
    kaamer_counters c;
    for (uint32_t d = 0; d < W; d++) {
        view[d].block = sh[d].h_block;
        top_owner_fill(&view[d]);
        px[d] = rep_pos_ext(owner_hdr(sh[d]));
        ax[d] = rep_aln_ext(owner_hdr(sh[d]));
    }
    rc = sharded_record_reported_needs(t, ax, px);
    if (!rc) rc = sharded_sum_counters(sh, &c);
    if (rc) return rc;
    for (uint32_t d = 0; d < W; d++) c.n_hits += view[d].pub.counters.n_hits;
    batch_top_owner *bo = nullptr;
    ShardedMergedAln am;
    rc = sharded_interleave(view, px, ax, is_nucl(t->seq_type), t->b.tpos, t->b.aln, t->aln.text, t->top.max_results, &bo, &am);
    if (rc) return rc;
    bo->pub.counters = c;
    if (t->want_aln) rc = sharded_finish_align(t, bo, am);
    if (rc) { kaamer_batch_top_free(&bo->pub); return rc; }
    *out = &bo->pub;
    return KAAMER_OK;
}

// ---- a full call (kaamer_sharded_search_batch) --------------------------------------------------------------------------
// each owner's merged queries, CSR
struct OwnerCsr {
    uint32_t n = 0;
    std::vector<uint64_t> off, pos_base, pos_off, bits;
    std::vector<uint32_t> cnt, pid, km, fp;
};

// every owner's workspace is waited for and checked; the first failure's error is returned once the needs are recorded
static int sharded_check_owners_full(kaamer_sharded_ticket *t)
{
    std::vector<ShardState> &sh = t->set->sh;
    const uint32_t W = t->sx->n;
    ShardSyncGuard guard{ t->set, true };
    int err = KAAMER_OK;
    char why[256] = "";
    for (uint32_t d = 0; d < W; d++) {
        ShardState &ow = sh[d];
        const int rc = kaamer_workspace_finish(ow.mws, ow.stream, nullptr);
        if (rc && !err) {
            err = rc;
            snprintf(why, sizeof why, "owner %u: %s", d, kaamer_last_error());
            uint32_t sst = 0;
            const uint32_t bad = sharded_failed_shard(sh, &sst);   // which bound: a shard's own search status says what ran out there
            if (bad < W) snprintf(why, sizeof why, "shard %u: search status 0x%x", bad, sst);
        }
    }
    guard.armed = false;  // every owner's stream has been waited for (and with it every shard's packs)
    sharded_record_exchange_need(t->set);
    uint64_t sp[2] = { 0, 0 };
    if (kaamer_exchange_stats_positions(sh[0].mws, 0, sp) == KAAMER_OK) t->set->need_pos_words = sp[0];
    return err ? kaamer_fail(err, "sharded search: %s", why) : KAAMER_OK;
}

// each owner's merged CSR (bitmaps included) and the batch's queries as shard 0 translated them, to the host
static int sharded_fetch_full(kaamer_sharded_ticket *t, batch_out_owner *bo, std::vector<OwnerCsr> &oc, uint32_t *n_queries)
{
    std::vector<ShardState> &sh = t->set->sh;
    const uint32_t W = t->sx->n;
    const bool pos = t->b.pos;
    kaamer_workspace *q_ws = sh[0].ws;
    uint32_t nq = 0;
    hipError_t e = hipSetDevice(sh[0].device);
    if (e == hipSuccess) e = hipMemcpy(&nq, q_ws->d_nq, 4, hipMemcpyDeviceToHost);
    for (uint32_t d = 0; d < W && e == hipSuccess; d++) {
        ShardState &ow = sh[d];
        kaamer_workspace *m = ow.mws;
        OwnerCsr &o = oc[d];
        hipStream_t s = ow.stream;
        e = hipSetDevice(ow.device);
        if (e == hipSuccess) e = hipMemcpy(&o.n, m->d_nq, 4, hipMemcpyDeviceToHost);
        const uint32_t want = nq > d ? (nq - d + W - 1) / W : 0u;
        if (e == hipSuccess && o.n != want) return kaamer_fail(KAAMER_E_HIP, "sharded search: owner %u merged %u queries, expected %u", d, o.n, want);
        o.off.resize((size_t)o.n + 1); o.cnt.resize((size_t)o.n + 1);
        if (pos) o.pos_base.resize((size_t)o.n + 1);
        if (e == hipSuccess) e = hipMemcpyAsync(o.off.data(), m->d_csr_off, ((size_t)o.n + 1) * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && o.n) e = hipMemcpyAsync(o.cnt.data(), m->d_q_cnt, (size_t)o.n * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && pos) e = hipMemcpyAsync(o.pos_base.data(), m->d_pos_base, ((size_t)o.n + 1) * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) break;
        const uint64_t h = o.off[o.n], w = pos ? o.pos_base[o.n] : 0;
        o.pid.resize(h + 1); o.km.resize(h + 1); o.fp.resize(h + 1);
        if (pos) { o.pos_off.resize(h + 1); o.bits.resize(w + 1); }
        if (h) {
            e = hipMemcpyAsync(o.pid.data(), m->d_c_pid, h * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(o.km.data(), m->d_c_km, h * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(o.fp.data(), m->d_c_fp, h * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && pos) e = hipMemcpyAsync(o.pos_off.data(), m->d_pos_off, h * 8, hipMemcpyDeviceToHost, s);
        }
        if (e == hipSuccess && w) e = hipMemcpyAsync(o.bits.data(), m->d_pos_bits, w * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    // the batch's queries as shard 0 translated them
    uint64_t n_sa = 0;
    unsigned long long n_aa = 0;
    bo->q.resize(nq);
    if (e == hipSuccess) e = hipSetDevice(sh[0].device);
    if (e == hipSuccess && nq) e = hipMemcpy(bo->q.data(), q_ws->d_q, (size_t)nq * sizeof(kaamer_query_meta), hipMemcpyDeviceToHost);
    if (e == hipSuccess && q_ws->nucleotide) {
        const size_t cap6 = (size_t)q_ws->max_seqs * 6;
        e = hipMemcpy(&n_aa, q_ws->d_n_pos, sizeof n_aa, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(&n_sa, q_ws->d_off3 + 2 * (cap6 + 1) + (size_t)t->n_seqs * 6, sizeof n_sa, hipMemcpyDeviceToHost);
        bo->orf_aa.resize(n_aa + 1); bo->starts_alt.resize(n_sa + 1);
        if (e == hipSuccess && n_aa) e = hipMemcpy(bo->orf_aa.data(), q_ws->d_orf_aa, n_aa, hipMemcpyDeviceToHost);
        if (e == hipSuccess && n_sa) e = hipMemcpy(bo->starts_alt.data(), q_ws->d_starts_alt, n_sa * sizeof(int32_t), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return kaamer_fail(KAAMER_E_HIP, "D2H: %s", hipGetErrorString(e));
    *n_queries = nq;
    return KAAMER_OK;
}

// ---- interleave into batch order: host memory only
static int sharded_interleave_full(const std::vector<OwnerCsr> &oc, uint32_t nq, bool pos, batch_out_owner *bo)
{
    const uint32_t W = (uint32_t)oc.size();
    uint64_t n_hits = 0, n_words = 0;
    for (const OwnerCsr &o : oc) { n_hits += o.off[o.n]; n_words += pos ? o.pos_base[o.n] : 0; }
    bo->hit_off.resize((size_t)nq + 1); bo->hit_cnt.resize((size_t)nq + 1);
    if (!bo->pid.resize(n_hits) || !bo->km.resize(n_hits) || !bo->fp.resize(n_hits)) return kaamer_fail(KAAMER_E_NOMEM, "hit lists");
    if (pos) { bo->pos_off.resize(n_hits + 1); bo->pos_bits.resize(n_words + 1); }
    uint64_t hcur = 0, wcur = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const OwnerCsr &o = oc[q % W];
        const uint32_t i = q / W;
        const uint64_t a = o.off[i], n = o.cnt[i];
        bo->hit_off[q] = hcur;
        bo->hit_cnt[q] = (uint32_t)n;
        memcpy(bo->pid.data() + hcur, o.pid.data() + a, n * 4);
        memcpy(bo->km.data() + hcur, o.km.data() + a, n * 4);
        memcpy(bo->fp.data() + hcur, o.fp.data() + a, n * 4);
        if (pos) {
            const uint64_t b0 = o.pos_base[i], nw = o.pos_base[i + 1] - b0;
            memcpy(bo->pos_bits.data() + wcur, o.bits.data() + b0, nw * 8);
            for (uint64_t j = 0; j < n; j++) bo->pos_off[hcur + j] = wcur + (o.pos_off[a + j] - b0);
            wcur += nw;
        }
        hcur += n;
    }
    bo->hit_off[nq] = hcur;
    memset(&bo->pub, 0, sizeof bo->pub);
    bo->pub.n_queries = nq;
    bo->pub.q = bo->q.data();
    bo->pub.hit_off = bo->hit_off.data();
    bo->pub.hit_cnt = bo->hit_cnt.data();
    bo->pub.hit_pid = bo->pid.data();
    bo->pub.hit_kmatch = bo->km.data();
    bo->pub.hit_first_pos = bo->fp.data();
    if (pos) { bo->pub.pos_off = bo->pos_off.data(); bo->pub.pos_bits = bo->pos_bits.data(); }
    return KAAMER_OK;
}

// Waits for the attempt, checks every workspace and copies each owner's merged CSR (bitmaps included) to the host; then
// interleaves the owners' queries back into batch order (query q is owned by shard q mod W).  The query data (q, orf_aa,
// starts_alt) is shard 0's: every shard translates the batch alike.
static int sharded_collect_full(kaamer_sharded_ticket *t, kaamer_batch_out **out)
{
    std::vector<ShardState> &sh = t->set->sh;
    int rc = sharded_check_owners_full(t);
    if (rc) return rc;
    std::unique_ptr<batch_out_owner> bo(new (std::nothrow) batch_out_owner());
    if (!bo) return kaamer_fail(KAAMER_E_NOMEM, "batch_out");
    std::vector<OwnerCsr> oc(t->sx->n);
    uint32_t nq = 0;
    kaamer_counters c;
    rc = sharded_fetch_full(t, bo.get(), oc, &nq);
    if (!rc) rc = sharded_interleave_full(oc, nq, t->b.pos, bo.get());
    if (!rc) rc = sharded_sum_counters(sh, &c);
    if (rc) return rc;
    c.n_hits = bo->hit_off[nq];
    bo->pub.counters = c;
    if (sh[0].ws->nucleotide) { bo->pub.orf_aa = bo->orf_aa.data(); bo->pub.starts_alt = bo->starts_alt.data(); }
    *out = &bo.release()->pub;
    return KAAMER_OK;
}

// ---- wait: collect; a bound that was too small grows and the batch runs again; the set is given back --------------------
extern "C++" {
// collect(): sharded_collect / sharded_collect_full on the ticket; grow(): that call's rule for its bounds after
// KAAMER_E_CAPACITY (a non-OK return ends the loop with it)
template <class Collect, class Grow> static int sharded_wait(kaamer_sharded_ticket *t, Collect collect, Grow grow)
{
    int rc;
    for (;;) {
        rc = collect();
        if (rc != KAAMER_E_CAPACITY || t->attempt >= MAX_BOUND_RETRIES) break;
        t->attempt++;
        rc = grow();
        if (!rc) rc = sharded_enqueue(t);   // (an error here ends the loop, E_CAPACITY included: kept as it was)
        if (rc) break;
    }
    sharded_release(t->sx, t->set);
    return rc;
}

// search = submit, then wait
template <class Ticket, class Out, class Submit> static int sharded_search(Out **out, int (*wait)(Ticket *, Out **), Submit submit)
{
    if (out) *out = nullptr;
    Ticket *t = nullptr;
    const int rc = submit(&t);
    return rc ? rc : wait(t, out);
}
}  // extern "C++"

// the top call's rule: a subject segment, the alignment sections, the ids blocks and bitmap segments or every bound
static int sharded_grow_top(kaamer_sharded_ticket *t)
{
    if (t->cap_bits & ST_SEG_CAP) {   // a subject segment: its holder counted what it needs (also when sized from the previous call)
        const uint64_t need = t->set->need_sa_bytes + t->set->need_sa_bytes / 4 + 4096;
        if (need >= 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_CAPACITY, "sharded search: a subject segment of %llu bytes (the bound is 4 GiB)", (unsigned long long)need);
        if (need > t->b.sa_bytes) t->b.sa_bytes = need;
    }
    if (t->grow_sections) {
        // nothing but an owner's alignment sections was too small: t->b.aln_cap has grown, every other bound stays
    } else if (!t->adaptive) {
        // the bounds themselves were too small: enlarge them all (hit pool included: the unsharded call does the same),
        // or the ids blocks and segments alone when nothing else was exceeded
        if (t->pos_only) { if (t->cap_bits & (ST_POS_CAP | ST_IDS_CAP)) bounds_grow_positions(t->b.bb); }
        else { t->b.e_cap *= 4; bounds_grow(t->b.bb, t->seq_bytes, t->n_seqs, is_nucl(t->seq_type)); }
    }   // else: the blocks sized from the previous call were too small -- once more at the full capacity, same bounds
    return KAAMER_OK;
}

int kaamer_sharded_wait_batch_top(kaamer_sharded_ticket *t, kaamer_batch_top **out)
{
    if (!t || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_wait_batch_top: bad argument");
    *out = nullptr;
    const int rc = sharded_wait(t, [&] { return sharded_collect(t, out); }, [&] { return sharded_grow_top(t); });
    delete t;
    return rc;
}

int kaamer_sharded_wait_batch(kaamer_sharded_full_ticket *ft, kaamer_batch_out **out)
{
    if (!ft || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_wait_batch: bad argument");
    *out = nullptr;
    kaamer_sharded_ticket *t = &ft->t;
    const int rc = sharded_wait(t, [&] { return sharded_collect_full(t, out); }, [&] {
        if (!t->adaptive) {   // the bounds themselves were too small: enlarge them all, as kaamer_sharded_wait_batch_top does
            t->b.e_cap *= 4;
            t->b.p_cap *= 4;
            bounds_grow(t->b.bb, t->seq_bytes, t->n_seqs, is_nucl(t->seq_type));
        }   // else: the blocks sized from the previous call were too small -- once more at the full capacity, same bounds
        return KAAMER_OK;
    });
    delete ft;
    return rc;
}

// a ticket nobody waits for: its attempt runs out, the workspaces count as used, the set is given back
static void sharded_discard(kaamer_sharded_ticket *t)
{
    sharded_sync_all(t->set);
    for (ShardState &st : t->set->sh) { if (st.ws) st.ws->clean = false; if (st.mws) st.mws->clean = false; }
    sharded_release(t->sx, t->set);
}

void kaamer_sharded_ticket_discard(kaamer_sharded_ticket *t)
{
    if (!t) return;
    sharded_discard(t);
    delete t;
}

void kaamer_sharded_full_ticket_discard(kaamer_sharded_full_ticket *ft)
{
    if (!ft) return;
    sharded_discard(&ft->t);
    delete ft;
}

// ---- search = submit, then wait -------------------------------------------------------------------------------------------
int kaamer_sharded_search_batch_top(kaamer_sharded_index *sx, const kaamer_batch_in *in, const kaamer_topn_opts *top, kaamer_batch_top **out)
{
    return sharded_search(out, kaamer_sharded_wait_batch_top, [&](kaamer_sharded_ticket **t) { return kaamer_sharded_submit_batch_top(sx, in, top, t); });
}

int kaamer_sharded_search_batch_top_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                         double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    return sharded_search(out, kaamer_sharded_wait_batch_top, [&](kaamer_sharded_ticket **t) {
        return kaamer_sharded_submit_batch_top_flat(sx, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, t);
    });
}

int kaamer_sharded_search_batch_top_pos_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                             double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    return sharded_search(out, kaamer_sharded_wait_batch_top, [&](kaamer_sharded_ticket **t) {
        return kaamer_sharded_submit_batch_top_pos_flat(sx, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, t);
    });
}

int kaamer_sharded_search_batch_top_aln_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                             double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t want_positions,
                                             const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text, kaamer_batch_top **out)
{
    return sharded_search(out, kaamer_sharded_wait_batch_top, [&](kaamer_sharded_ticket **t) {
        return kaamer_sharded_submit_batch_top_aln_flat(sx, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, want_positions,
                                                        sub_matrix, gap_open, gap_extend, want_text, t);
    });
}

int kaamer_sharded_search_batch(kaamer_sharded_index *sx, const kaamer_batch_in *in, kaamer_batch_out **out)
{
    if (out) *out = nullptr;
    if (!sx || !in || !out || !in->offsets || (in->n_seqs && !in->seqs)) return kaamer_fail(KAAMER_E_ARG, "sharded_search_batch: bad argument");
    return kaamer_sharded_search_batch_flat(sx, in->seqs, in->offsets, in->n_seqs, in->seq_type, in->want_positions, out);
}

int kaamer_sharded_search_batch_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                     int32_t want_positions, kaamer_batch_out **out)
{
    return sharded_search(out, kaamer_sharded_wait_batch, [&](kaamer_sharded_full_ticket **t) {
        return kaamer_sharded_submit_batch_flat(sx, seqs, offsets, n_seqs, seq_type, want_positions, t);
    });
}
