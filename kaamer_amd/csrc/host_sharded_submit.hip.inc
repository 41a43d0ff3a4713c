// host_sharded_submit.hip.inc — the submit side of the one-process sharded driver (included by search.hip inside its
// extern "C" block, after host_sharded.hip.inc): what a set's shards hold for a call is made ready, the batch is enqueued
// on every shard's stream.  sharded_enqueue lists the phases of host_sharded.hip.inc's header comment in its order.

// workspaces, exchange buffers and staging of one shard for a batch of this size
struct ShardBounds {
    BatchBounds bb;      // of each shard's search workspace
    uint64_t e_cap;      // entries per (shard -> owner) block
    bool full, pos;      // a full call (hit lists to the host), with PositionHits bitmaps
    uint64_t p_cap;      // bitmap words per block (pos)
    bool tpos;           // a top call with the PositionHits of the reported hits (its bounds: bb.pos_scale x the rule)
    bool aln;            // a top call that aligns the reported hits
    uint64_t sa_bytes;   // payload bytes of one (holder -> owner) subject segment (aln)
    uint64_t aln_cap;    // bytes the alignment sections of an owner's result block may take (aln)
};

// one call in flight on a set: what submit leaves for wait
struct kaamer_sharded_ticket {
    kaamer_sharded_index *sx;
    ShardSet *set;
    uint32_t n_seqs;
    int32_t seq_type;
    uint64_t seq_bytes;
    kaamer_topn_opts top;
    ShardBounds b;
    bool adaptive;   // this attempt's exchange blocks were sized from the previous call's need, not the capacity
    bool pos_only;   // the attempt failed on the reported hits' ids blocks / bitmap segments alone (ST_IDS_CAP, ST_POS_CAP):
                     // only their bound (BatchBounds::pos_scale) grows, and only their buffers are made again
    int attempt;
    // the alignment of the reported hits (kaamer_sharded_submit_batch_top_aln_flat)
    bool want_aln;            // the result carries alignments; b.aln: the options name BLOSUM62 with a row, the exchange runs
    TopAlnRequest aln;
    uint32_t max_query_len;   // batch_max_query_len
    uint32_t cap_bits;        // the owners' status words of the attempt, OR-ed
    bool grow_sections;       // the attempt was fine but for an owner's alignment sections: they alone grow
};
// a full call (kaamer_sharded_search_batch): the same pipeline without the post-steps (t.b.full)
struct kaamer_sharded_full_ticket {
    kaamer_sharded_ticket t;
};

static inline bool tpos_or_aln(const kaamer_sharded_ticket *t) { return t->b.tpos || t->b.aln; }

static void sharded_sync_all(ShardSet *set)
{
    for (ShardState &st : set->sh)
        if (st.stream) { (void)hipSetDevice(st.device); (void)hipStreamSynchronize(st.stream); }
}

namespace {
struct ShardSyncGuard {   // every early return of its scope: nothing of the attempt is left running on any device
    ShardSet *set; bool armed;
    ~ShardSyncGuard() { if (armed) sharded_sync_all(set); }
};
}

static void sharded_release(kaamer_sharded_index *sx, ShardSet *set)
{
    { std::lock_guard<std::mutex> lock(sx->mu); set->busy = false; }
    sx->cv.notify_one();
}

// ---- the four device steps of the reported hits' bitmaps, as functions of (workspaces, buffers, stream) ------------------
// owner: the reported ids of the last kaamer_topn_device / topn_pack_block on `mws` into the ids block `d_ids`
static int tps_enqueue_ids_pack(kaamer_workspace *mws, const kaamer_topn_result *tr, uint8_t *d_block, size_t block_cap, uint32_t *d_ids,
                                const TpsIdsLayout &L, uint32_t owner, uint32_t W, uint32_t seq, hipStream_t s)
{
    TpsParams p;
    memset(&p, 0, sizeof p);
    p.world = W; p.owner = owner; p.seq = seq; p.ids_layout = L;
    p.m_nq = mws->d_nq; p.top_cnt = tr->d_top_cnt; p.top_pid = tr->d_top_pid; p.K = tr->max_results;
    p.rank = mws->d_rep_rank; p.eoff = mws->d_rep_eoff; p.aoff = mws->d_rep_aoff;
    p.m_status = mws->d_status_out;
    p.block = d_block; p.block_cap = block_cap;
    p.ids_out = d_ids;
    hipLaunchKernelGGL(tps_ids_pack_kernel, dim3(mws->n_cu * 8), dim3(256), 0, s, p);
    HIPCHK(hipGetLastError());
    return KAAMER_OK;
}

// what the shard-side steps share: the search workspace of the shard (kaamer_exchange_pack reads the hit lists and
// writes the send blocks, its own offsets and tile sums only: vals[], qinfo and the index's arena are as the search
// left them, which is what the unsharded path assumes after counting)
static TpsParams tps_shard_params(const kaamer_index *ix, const kaamer_workspace *ws, const uint32_t *d_ids, const TpsIdsLayout &L, uint32_t owner,
                                  uint32_t W, uint32_t seq, uint32_t K, uint32_t *d_n, uint32_t *d_words, const uint64_t *d_base)
{
    TpsParams p;
    memset(&p, 0, sizeof p);
    p.world = W; p.owner = owner; p.seq = seq; p.ids_layout = L; p.K = K;
    p.ids = d_ids;
    p.s_nq = ws->d_nq; p.qinfo = ws->d_qinfo; p.vals = ws->d_vals; p.arena = ix->d_arena; p.s_status = ws->d_status_out;
    p.n_out = d_n; p.words = d_words; p.base = d_base;
    return p;
}

// shard: the bitmap words of every reported query of `owner` and their scan (the same on every shard and on the owner)
static int tps_enqueue_words(const kaamer_index *ix, kaamer_workspace *ws, const uint32_t *d_ids, const TpsIdsLayout &L, uint32_t owner, uint32_t W,
                             uint32_t seq, uint32_t K, uint32_t *d_n, uint32_t *d_words, uint64_t *d_base, hipStream_t s)
{
    const TpsParams p = tps_shard_params(ix, ws, d_ids, L, owner, W, seq, K, d_n, d_words, d_base);
    uint32_t gb = (L.rq_cap + 255) / 256;
    if (gb > (uint32_t)ws->n_cu * 8) gb = (uint32_t)ws->n_cu * 8;
    if (gb < 1) gb = 1;
    hipLaunchKernelGGL(tps_words_kernel, dim3(gb), dim3(256), 0, s, p);
    // (an owner reports at most the batch's queries: the workspace's scan scratch, sized for q_cap, is enough)
    scan_u32_on(ws, d_words, d_n, L.rq_cap < ws->q_cap ? L.rq_cap : ws->q_cap, d_base, s);
    HIPCHK(hipGetLastError());
    return KAAMER_OK;
}

// shard: its partial bitmaps of the reported hits of `owner` into the segment `d_seg` (header word + seg_cap words)
static int tps_enqueue_bits(const kaamer_index *ix, kaamer_workspace *ws, const uint32_t *d_ids, const TpsIdsLayout &L, uint32_t owner, uint32_t W,
                            uint32_t seq, uint32_t K, uint32_t *d_n, const uint64_t *d_base, unsigned long long *d_seg, uint64_t seg_cap, hipStream_t s)
{
    TpsParams p = tps_shard_params(ix, ws, d_ids, L, owner, W, seq, K, d_n, nullptr, d_base);
    p.seg = d_seg; p.seg_cap = seg_cap;
    hipLaunchKernelGGL(tps_bits_kernel, dim3(ws->n_cu * 8), dim3(64 * TP_WAVES), 0, s, p);
    HIPCHK(hipGetLastError());
    return KAAMER_OK;
}

// owner: the W received segments (seg_stride u64 words apart) OR-ed into the bitmap sections of its packed block; `ws`,
// d_n and d_base: the owner's own shard and what it computed for this owner's ids block
static int tps_enqueue_or(const kaamer_index *ix, kaamer_workspace *mws, kaamer_workspace *ws, uint8_t *d_block, size_t block_cap, const uint32_t *d_ids,
                          const TpsIdsLayout &L, uint32_t owner, uint32_t W, uint32_t seq, uint32_t *d_n, const uint64_t *d_base,
                          unsigned long long *d_seg_recv, uint64_t seg_stride, uint64_t seg_cap, hipStream_t s)
{
    TpsParams p = tps_shard_params(ix, ws, d_ids, L, owner, W, seq, 0, d_n, nullptr, d_base);
    p.m_nq = mws->d_nq;
    p.rank = mws->d_rep_rank; p.eoff = mws->d_rep_eoff; p.aoff = mws->d_rep_aoff;
    p.block = d_block; p.block_cap = block_cap;
    p.seg = d_seg_recv; p.seg_stride = seg_stride; p.seg_cap = seg_cap;
    hipLaunchKernelGGL(tps_or_kernel, dim3(mws->n_cu * 8), dim3(256), 0, s, p);
    HIPCHK(hipGetLastError());
    return KAAMER_OK;
}


// ---- the two device steps of the reported hits' alignment (top_align_sharded.hip.inc) ----------------------------------
// holder `st` (device s): the stored bytes of the subjects it holds among owner d's reported ids, into segment d
static int tas_enqueue_gather(kaamer_sharded_index *sx, ShardState &st, uint32_t s, uint32_t d, uint32_t W, uint32_t seq, uint32_t K)
{
    const kaamer_sharded_index::AlnPart &part = (*sx->aln)[s];
    const size_t iw = (size_t)tps_ids_words(st.ids_wire), ab = (size_t)tas_seg_bytes(st.sa_wire);
    TasParams p;
    memset(&p, 0, sizeof p);
    p.world = W; p.owner = d; p.self = s; p.seq = seq; p.K = K;
    p.ids_layout = st.ids_wire; p.lay = st.sa_wire;
    p.ids = st.d_ids_recv + (size_t)d * iw;
    p.s_nq = st.ws->d_nq; p.s_status = st.ws->d_status_out;
    p.raw = part.d_raw; p.off = part.d_off; p.idmap = part.d_idmap; p.idmap_n = part.idmap_n;
    p.n_out = st.d_sa_n + 2 * d; p.qbytes = st.d_sa_qbytes;
    p.seg = st.d_sa_send + (size_t)d * ab;
    p.need_out = st.d_sa_need + 2 * d;
    uint32_t gb = (st.sa_wire.rq_cap + 3) / 4;   // a wave per reported query
    if (gb > (uint32_t)st.ws->n_cu * 8) gb = (uint32_t)st.ws->n_cu * 8;
    if (gb < 1) gb = 1;
    hipLaunchKernelGGL(tas_len_kernel, dim3(gb), dim3(256), 0, st.stream, p);
    // (an owner reports at most the batch's queries: the workspace's scan scratch, sized for q_cap, is enough)
    scan_u32_on(st.ws, st.d_sa_qbytes, st.d_sa_n + 2 * d, st.sa_wire.rq_cap < st.ws->q_cap ? st.sa_wire.rq_cap : st.ws->q_cap,
                reinterpret_cast<uint64_t *>(p.seg + tas_base_at()), st.stream);
    hipLaunchKernelGGL(tas_gather_kernel, dim3(gb), dim3(256), 0, st.stream, p);
    HIPCHK(hipGetLastError());
    return KAAMER_OK;
}

// owner `ow` (device d), its W segments pulled: the headers, then the stage of host_top_align.hip.inc fed the gathered
// subjects; pair records and operations go behind the packed block (and its bitmaps)
static int tas_enqueue_align(kaamer_sharded_index *sx, const kaamer_sharded_ticket *t, ShardState &ow, const kaamer_topn_result *tr, uint32_t d,
                             uint32_t W, uint32_t seq, uint64_t budget)
{
    const kaamer_sharded_index::AlnPart &part = (*sx->aln)[d];
    const size_t iw = (size_t)tps_ids_words(ow.ids_wire), ab = (size_t)tas_seg_bytes(ow.sa_wire);
    kaamer_workspace *mws = ow.mws, *ws = ow.ws;
    TasParams sp;
    memset(&sp, 0, sizeof sp);
    sp.world = W; sp.owner = d; sp.self = d; sp.seq = seq; sp.K = tr->max_results;
    sp.ids_layout = ow.ids_wire; sp.lay = ow.sa_wire;
    sp.ids = ow.d_ids_recv + (size_t)d * iw;
    sp.m_nq = mws->d_nq; sp.q = ws->d_q;
    sp.top_cnt = tr->d_top_cnt; sp.top_pid = tr->d_top_pid; sp.trim = tr->d_trim;
    sp.rank = mws->d_rep_rank; sp.eoff = mws->d_rep_eoff;
    sp.qraw = ws->nucleotide ? ws->d_orf_aa : ws->last_seqs;
    sp.segs = ow.d_sa_recv; sp.seg_stride = ab; sp.codes = ow.d_sa_codes; sp.pair_off = ow.d_sa_off;
    sp.block = ow.d_block;
    hipLaunchKernelGGL(tas_check_kernel, dim3(1), dim3(1), 0, ow.stream, sp);
    TaParams p;
    memset(&p, 0, sizeof p);
    p.d_nq = mws->d_nq; p.q = ws->d_q;
    p.top_cnt = tr->d_top_cnt; p.top_pid = tr->d_top_pid; p.trim = tr->d_trim; p.K = tr->max_results;
    p.eoff = mws->d_rep_eoff;
    p.qraw = sp.qraw;
    p.tab.raw = ow.d_sa_recv; p.tab.codes = ow.d_sa_codes; p.tab.off = ow.d_sa_off;   // (bad, idmap: ta_pairs_kernel's, not read here)
    p.matrix = part.d_matrix;
    p.gap_open = t->aln.gap_open; p.gap_extend = t->aln.gap_extend;
    p.block = ow.d_block; p.block_cap = ow.d_block.capacity(); p.aln_cap = t->b.aln_cap; p.want_text = t->aln.text ? 1 : 0;
    p.status = mws->d_status_out;
    return ta_stage(ws, p, budget, sx->aln_max_ns, t->max_query_len, &sp, ow.stream, ow.sa_stage, ow.timed ? ow.ev_t + 2 : nullptr);
}

// ---- what a shard holds for a call: each part is made again only when it no longer fits -------------------------------
// the two workspaces and the exchange buffers
static int shard_prepare_workspaces(ShardState &st, uint32_t W, uint32_t rank, uint64_t seq_bytes, uint32_t n_seqs, int32_t seq_type, const ShardBounds &b)
{
    const bool nucl = is_nucl(seq_type);
    const kaamer_workspace_opts &o = st.opts;
    const bool fits = st.ws && o.seq_type == seq_type && o.max_seq_bytes >= seq_bytes && o.max_seqs >= (n_seqs ? n_seqs : 1) &&
                      o.g_tier_slots >= b.bb.g_slots && o.max_queries >= b.bb.max_queries && st.e_cap >= b.e_cap &&
                      o.max_hits >= b.bb.max_hits && (b.bb.max_hits != 0 || o.max_hits == 0) &&
                      st.full == b.full && (o.want_positions != 0) == b.pos && (!b.pos || st.p_cap >= b.p_cap) &&
                      st.tpos == b.tpos;
    if (fits) return KAAMER_OK;
    HIPCHK(hipStreamSynchronize(st.stream));
    if (st.ws) kaamer_workspace_free(st.ws);
    if (st.mws) kaamer_workspace_free(st.mws);
    st.ws = st.mws = nullptr;
    kaamer_workspace_opts g;
    memset(&g, 0, sizeof g);
    g.max_seq_bytes = seq_bytes + seq_bytes / 4 + 4096;
    g.max_seqs = (n_seqs ? n_seqs : 1) + n_seqs / 4 + 16;
    g.seq_type = seq_type;
    // the exchange wants an explicit, equal setting on both workspaces; kaamer_batch_out always carries first positions
    g.first_pos = (nucl || b.full) ? 1u : 2u;
    g.want_positions = b.pos ? 1u : 0u;
    g.g_tier_slots = b.bb.g_slots;
    g.max_queries = b.bb.max_queries;
    g.max_hits = b.bb.max_hits;       // 0: the library's default for the input size (as the unsharded call starts)
    int rc = kaamer_workspace_create(st.ix, &g, &st.ws);
    if (rc) { st.ws = nullptr; return rc; }
    st.opts = g;
    st.e_cap = b.e_cap + b.e_cap / 4;
    st.full = b.full;
    st.p_cap = b.pos ? b.p_cap + b.p_cap / 4 : 0;
    if (b.pos) rc = kaamer_exchange_layout_init_positions(W, rank, st.ws->q_cap, st.e_cap, st.p_cap, &st.layout);
    else rc = kaamer_exchange_layout_init(W, rank, st.ws->q_cap, st.e_cap, &st.layout);
    if (rc) return rc;
    kaamer_workspace_opts m;
    memset(&m, 0, sizeof m);
    m.max_seq_bytes = 64;
    m.max_seqs = st.layout.q_cap;
    m.max_queries = st.layout.q_cap;
    m.seq_type = KAAMER_PROTEIN;
    m.first_pos = g.first_pos;
    m.max_hits = (uint64_t)W * st.layout.e_cap;
    m.g_tier_slots = b.bb.g_slots;
    m.want_positions = g.want_positions;
    m.max_pos_words = b.pos ? (uint64_t)W * x_p_cap(&st.layout) : 0;   // merged bitmaps <= the words received
    m.compact = b.full ? 1u : 0u;   // the full call copies CSR to the host
    rc = kaamer_workspace_create(st.ix, &m, &st.mws);
    if (rc) { st.mws = nullptr; return rc; }
    const size_t words = (size_t)W * st.layout.block_words;
    rc = reserve_group(st.stream, GROW_EXACT, { want(st.d_send, words), want(st.d_recv, words) });
    if (rc) return rc;
    shard_tps_free(st);   // (sized from the workspaces: shard_prepare_ids makes them again)
    st.tpos = b.tpos;
    st.tp_k = 0; st.tp_scale = 0;
    return KAAMER_OK;
}

// the reported hits' bitmaps: the unsharded rule (next to kaamer_topn_positions_device) divided over the owners,
// x pos_scale on a repeat, never beyond the hard bound; the ids block likewise (every owned query may report).  A
// repeat that grows pos_scale alone (or a larger MaxResults) makes these buffers and the result block again, nothing
// else: the workspaces and the exchange buffers stay.
static int shard_prepare_ids(ShardState &st, uint32_t W, bool nucl, const ShardBounds &b, uint32_t K)
{
    const uint32_t scale = b.bb.pos_scale ? b.bb.pos_scale : 1u;
    if (!((b.tpos || b.aln) && (st.tp_k < K || st.tp_scale < scale))) return KAAMER_OK;   // (the ids block serves both kinds; the rest is the bitmaps')
    HIPCHK(hipStreamSynchronize(st.stream));
    shard_tps_free(st);
    const uint64_t hard = tp_hard_words(st.ws, K);
    const uint64_t rule = tp_default_words(st.ws, K, scale), w = rule / W + 1024;
    st.tp_cap = (rule >= hard || w > hard) ? hard : w;   // (one owner may own all the long queries: the hard bound is not divided)
    const uint64_t oq = st.layout.q_cap, f = nucl ? 1u : (K < 16u ? K : 16u);
    const uint64_t e_hard = oq * K, e = oq * f > e_hard / scale ? e_hard : oq * f * scale;
    st.ids_cap.rq_cap = (uint32_t)oq;
    st.ids_cap.ent_cap = (e > e_hard ? e_hard : e) + 64;
    const size_t iw = (size_t)tps_ids_words(st.ids_cap), sw = (size_t)st.tp_cap + 1;
    int rc = reserve_group(st.stream, GROW_EXACT, { want(st.d_ids, iw), want(st.d_ids_recv, (size_t)W * iw) });
    if (!rc && b.tpos)
        rc = reserve_group(st.stream, GROW_EXACT, { want(st.d_seg_send, (size_t)W * sw), want(st.d_seg_recv, (size_t)W * sw), want(st.d_tps_words, (size_t)oq + 1),
                                                    want(st.d_tps_n, (size_t)2 * W), want(st.d_tps_base, (size_t)W * (oq + 1)) });
    if (rc) { shard_tps_free(st); st.tp_k = 0; st.tp_scale = 0; return rc; }
    st.tp_k = K; st.tp_scale = scale;
    return KAAMER_OK;
}

// the subject segments: what the ids block can describe, and the payload bound of this attempt.  They alone are made
// again when that bound grows.
static int shard_prepare_subjects(ShardState &st, uint32_t W, const ShardBounds &b)
{
    if (!(b.aln && (!st.d_sa_send || st.sa_cap.rq_cap < st.ids_cap.rq_cap || st.sa_cap.ent_cap < st.ids_cap.ent_cap || st.sa_cap.byte_cap < b.sa_bytes))) return KAAMER_OK;
    HIPCHK(hipStreamSynchronize(st.stream));
    TasLayout L;
    L.rq_cap = st.ids_cap.rq_cap; L.ent_cap = st.ids_cap.ent_cap;
    L.byte_cap = st.sa_cap.byte_cap > b.sa_bytes ? st.sa_cap.byte_cap : b.sa_bytes;
    shard_sa_free(st);
    const size_t sb = (size_t)tas_seg_bytes(L);
    const int rc = reserve_group(st.stream, GROW_EXACT, { want(st.d_sa_send, (size_t)W * sb), want(st.d_sa_recv, (size_t)W * sb), want(st.d_sa_codes, (size_t)W * sb),
                                                          want(st.d_sa_qbytes, (size_t)L.rq_cap + 1), want(st.d_sa_n, (size_t)2 * W),
                                                          want(st.d_sa_off, (size_t)L.ent_cap + 1), want(st.d_sa_need, (size_t)2 * W) });
    if (rc) return rc;
    st.sa_cap = L;
    return KAAMER_OK;
}

static int shard_prepare(ShardState &st, uint32_t W, uint32_t rank, uint64_t seq_bytes, uint32_t n_seqs, int32_t seq_type, const ShardBounds &b, uint32_t K)
{
    HIPCHK(hipSetDevice(st.device));
    seq_type = seq_base(seq_type);   // (the genetic code is the call's: every shard gets it with the batch, kaamer_search_device)
    int rc = shard_prepare_workspaces(st, W, rank, seq_bytes, n_seqs, seq_type, b);
    if (!rc) rc = shard_prepare_ids(st, W, is_nucl(seq_type), b, K);
    if (!rc) rc = shard_prepare_subjects(st, W, b);
    if (!rc) rc = reserve(st.d_seqs, (size_t)seq_bytes + 16, GROW_CALL, st.stream);
    if (!rc) rc = reserve(st.d_off, (size_t)n_seqs + 1, GROW_CALL, st.stream);
    if (!rc && !b.full) rc = reserve(st.d_block, rep_block_bound(st.mws, st.ws, K, b.tpos ? st.tp_cap : 0) + (b.aln ? (size_t)b.aln_cap + 64 : 0), GROW_CALL, st.stream);
    return rc;
}

// every shard of the set made ready for the call
static int sharded_prepare_all(kaamer_sharded_ticket *t)
{
    std::vector<ShardState> &sh = t->set->sh;
    for (uint32_t s = 0; s < t->sx->n; s++) {
        const int rc = shard_prepare(sh[s], t->sx->n, s, t->seq_bytes, t->n_seqs, t->seq_type, t->b, t->top.max_results);
        if (rc) {
            // some shards are prepared for this call and some are not: the ids blocks and segments have one layout on every
            // shard of a set, so all of them are sized again by the next call
            for (ShardState &x : sh) { x.tp_k = 0; x.tp_scale = 0; x.sa_cap = TasLayout(); }
            return rc;
        }
    }
    return KAAMER_OK;
}

// what the previous batch needed + a quarter + a floor, never beyond the capacity
static inline uint64_t wire_size(uint64_t need, uint64_t floor, uint64_t cap = ~0ull)
{
    const uint64_t n = need + need / 4 + floor;
    return n < cap ? n : cap;
}

// the blocks of this batch: what the previous batch on this set needed + a quarter (its W x W headers, read after the
// call), or the capacity for a first call and for a retry.  What the peer copies move is payload, not capacity.
static int sharded_size_wire(kaamer_sharded_ticket *t)
{
    const ShardSet *set = t->set;
    const bool nucl = is_nucl(t->seq_type);
    t->adaptive = t->attempt == 0 && set->need_entries != 0 && (!t->b.pos || set->need_pos_words != 0) && (!t->b.tpos || set->tp_seen) &&
                  (!t->b.aln || set->sa_seen);
    for (ShardState &st : t->set->sh) {
        st.wire = st.layout;
        if (t->adaptive) {   // (the layout's fit holds the three to the capacity itself)
            const uint32_t nq = (uint32_t)wire_size(set->need_queries, 64);
            const uint64_t ne = wire_size(set->need_entries, 1024);
            const int rc = t->b.pos ? kaamer_exchange_layout_fit_positions(&st.layout, nq, ne, wire_size(set->need_pos_words, 1024), &st.wire)
                                    : kaamer_exchange_layout_fit(&st.layout, nq, ne, (nucl || t->b.full) ? 1 : 0, &st.wire);
            if (rc) return rc;
        }
        if (tpos_or_aln(t)) {   // the ids blocks and segments of this batch (the round trip after top-N): sized the same way
            st.ids_wire = st.ids_cap;
            st.tp_wire = st.tp_cap;
            if (t->adaptive) {
                st.ids_wire.rq_cap = (uint32_t)wire_size(set->need_ids_rq, 64, st.ids_cap.rq_cap);
                st.ids_wire.ent_cap = wire_size(set->need_ids_ent, 1024, st.ids_cap.ent_cap);
                st.tp_wire = wire_size(set->need_tp_words, 1024, st.tp_cap);
            }
        }
        if (t->b.aln) {   // a subject segment describes what the previous batch reported + a quarter, and holds its payload + a quarter
            st.sa_wire = st.sa_cap;
            if (t->adaptive) {
                st.sa_wire.rq_cap = (uint32_t)wire_size(set->need_ids_rq, 16, st.sa_cap.rq_cap);
                st.sa_wire.ent_cap = wire_size(set->need_ids_ent, 64, st.sa_cap.ent_cap);
                st.sa_wire.byte_cap = wire_size(set->need_sa_bytes, 256, st.sa_cap.byte_cap);
            }
        }
    }
    return KAAMER_OK;
}

// a block of `bytes` from another shard's device (or this one) onto `s`, a stream of dst_device
static hipError_t peer_pull_async(void *dst, int dst_device, const void *src, int src_device, size_t bytes, hipStream_t s)
{
    return src_device == dst_device ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipMemcpyPeerAsync(dst, dst_device, src, src_device, bytes, s);
}

// shard `self` pulls its slice from every shard after that shard's event `ev` (its own work precedes on its own stream);
// copy(src, s) enqueues the copies from shard s on self's stream
extern "C++" {
template <class Copy> static int pull_from_all(std::vector<ShardState> &sh, uint32_t self, hipEvent_t ShardState::*ev, Copy copy)
{
    for (uint32_t s = 0; s < sh.size(); s++) {
        if (s != self) HIPCHK(hipStreamWaitEvent(sh[self].stream, sh[s].*ev, 0));
        HIPCHK(copy(sh[s], s));
    }
    return KAAMER_OK;
}
}  // extern "C++"

// the speculative copy of an owner's result block
static int sharded_copy_back(ShardState &ow)
{
    return rep_block_copy_guess(ow.d_block, ow.d_block.capacity(), ow.guess, &ow.h_block, &ow.h_block_cap, &ow.copied, ow.stream);
}

// ---- every shard: the whole batch against its keys, partial hit lists packed per owner
static int enqueue_search_pack(kaamer_sharded_ticket *t)
{
    const ShardSet *set = t->set;
    const uint64_t seq_bytes = t->seq_bytes;
    const size_t off_at = ((size_t)seq_bytes + 7) & ~(size_t)7;
    for (ShardState &st : t->set->sh) {
        HIPCHK(hipSetDevice(st.device));
        if (seq_bytes) HIPCHK(hipMemcpyAsync(st.d_seqs, set->h_in, (size_t)seq_bytes, hipMemcpyHostToDevice, st.stream));
        HIPCHK(hipMemcpyAsync(st.d_off, set->h_in + off_at, ((size_t)t->n_seqs + 1) * 8, hipMemcpyHostToDevice, st.stream));
        kaamer_device_result dr;
        int rc = kaamer_search_device(st.ix, st.ws, st.d_seqs, st.d_off, t->n_seqs, seq_bytes, t->seq_type, st.stream, &dr);
        if (!rc) rc = kaamer_exchange_pack(st.ws, &st.wire, st.d_send, st.stream);
        if (rc) return rc;
        HIPCHK(hipEventRecord(st.ev_packed, st.stream));
    }
    return KAAMER_OK;
}

// ---- every owner: pull its blocks, merge, post-steps, result block
static int enqueue_merge_topn(kaamer_sharded_ticket *t, uint32_t seq, std::vector<kaamer_topn_result> &trs)
{
    std::vector<ShardState> &sh = t->set->sh;
    const uint32_t W = t->sx->n;
    for (uint32_t d = 0; d < W; d++) {
        ShardState &ow = sh[d];
        HIPCHK(hipSetDevice(ow.device));
        const size_t bw = (size_t)ow.wire.block_words;
        int rc = pull_from_all(sh, d, &ShardState::ev_packed, [&](ShardState &src, uint32_t s) {
            return peer_pull_async(ow.d_recv + (size_t)s * bw, ow.device, src.d_send + (size_t)d * bw, src.device, bw * 4, ow.stream);
        });
        kaamer_device_result mr;
        if (!rc) rc = kaamer_exchange_merge(ow.mws, &ow.wire, ow.d_recv, ow.stream, &mr);
        if (rc) return rc;
        if (t->b.full) continue;   // the merged CSR (bitmaps included) stays on the owner until sharded_collect_full copies it
        kaamer_topn_opts tt = t->top;
        tt.best_start_codon = is_nucl(t->seq_type) ? 1u : 0u;
        tt.d_size_in_kmer = nullptr;
        tt.orf_source = ow.ws; tt.q_first = d; tt.q_stride = W;
        rc = kaamer_topn_device(ow.mws, &tt, ow.stream, &trs[d]);
        if (!rc) rc = topn_pack_block(ow.mws, ow.ws, d, W, &trs[d], ow.stream, ow.d_block, ow.d_block.capacity());
        if (rc) return rc;
        if (tpos_or_aln(t)) {   // the result block waits for its bitmaps and alignments (the second round trip)
            rc = tps_enqueue_ids_pack(ow.mws, &trs[d], ow.d_block, ow.d_block.capacity(), ow.d_ids, ow.ids_wire, d, W, seq, ow.stream);
            if (rc) return rc;
            HIPCHK(hipEventRecord(ow.ev_ids, ow.stream));
            continue;
        }
        rc = sharded_copy_back(ow);
        if (rc) return rc;
    }
    return KAAMER_OK;
}

// ---- every shard: pulls the W ids blocks; per owner, its partial bitmaps of the reported hits and the stored bytes
// of the reported subjects it holds, into segment d of the two send buffers
static int enqueue_ids_round_shards(kaamer_sharded_ticket *t, uint32_t seq, bool timing)
{
    std::vector<ShardState> &sh = t->set->sh;
    const uint32_t W = t->sx->n, K = t->top.max_results;
    const bool tpos = t->b.tpos, aln = t->b.aln;
    for (uint32_t s = 0; s < W; s++) {
        ShardState &st = sh[s];
        HIPCHK(hipSetDevice(st.device));
        const size_t iw = (size_t)tps_ids_words(st.ids_wire), sw = (size_t)st.tp_wire + 1, bw = (size_t)st.ids_wire.rq_cap + 1;
        int rc = pull_from_all(sh, s, &ShardState::ev_ids, [&](ShardState &ow, uint32_t d) {
            return peer_pull_async(st.d_ids_recv + (size_t)d * iw, st.device, ow.d_ids, ow.device, iw * 4, st.stream);
        });
        if (rc) return rc;
        st.timed = false;
        if (aln && timing) {   // (made on first use, on the shard's device)
            for (hipEvent_t &e : st.ev_t) if (!e) HIPCHK(hipEventCreate(&e));
            st.timed = true;
            HIPCHK(hipEventRecord(st.ev_t[0], st.stream));
        }
        for (uint32_t d = 0; d < W && aln; d++) {
            const int rc = tas_enqueue_gather(t->sx, st, s, d, W, seq, K);
            if (rc) return rc;
        }
        if (st.timed) HIPCHK(hipEventRecord(st.ev_t[1], st.stream));
        for (uint32_t d = 0; d < W && tpos; d++) {
            const uint32_t *ids = st.d_ids_recv + (size_t)d * iw;
            int rc = tps_enqueue_words(st.ix, st.ws, ids, st.ids_wire, d, W, seq, K, st.d_tps_n + 2 * d, st.d_tps_words, st.d_tps_base + (size_t)d * bw, st.stream);
            if (!rc) rc = tps_enqueue_bits(st.ix, st.ws, ids, st.ids_wire, d, W, seq, K, st.d_tps_n + 2 * d, st.d_tps_base + (size_t)d * bw,
                                           st.d_seg_send + (size_t)d * sw, st.tp_wire, st.stream);
            if (rc) return rc;
        }
        HIPCHK(hipEventRecord(st.ev_bits, st.stream));
    }
    return KAAMER_OK;
}

// ---- every owner: pulls segment d of every shard, ORs the bitmaps into its result block, aligns the pairs behind
// them, one D2H
static int enqueue_ids_round_owners(kaamer_sharded_ticket *t, uint32_t seq, const std::vector<kaamer_topn_result> &trs, uint64_t budget)
{
    std::vector<ShardState> &sh = t->set->sh;
    const uint32_t W = t->sx->n;
    const bool tpos = t->b.tpos, aln = t->b.aln;
    for (uint32_t d = 0; d < W; d++) {
        ShardState &ow = sh[d];
        HIPCHK(hipSetDevice(ow.device));
        const size_t iw = (size_t)tps_ids_words(ow.ids_wire), sw = (size_t)ow.tp_wire + 1, bw = (size_t)ow.ids_wire.rq_cap + 1;
        const size_t ab = aln ? (size_t)tas_seg_bytes(ow.sa_wire) : 0;
        int rc = pull_from_all(sh, d, &ShardState::ev_bits, [&](ShardState &src, uint32_t s) {
            hipError_t e = hipSuccess;
            if (tpos) e = peer_pull_async(ow.d_seg_recv + (size_t)s * sw, ow.device, src.d_seg_send + (size_t)d * sw, src.device, sw * 8, ow.stream);
            if (e == hipSuccess && aln) e = peer_pull_async(ow.d_sa_recv + (size_t)s * ab, ow.device, src.d_sa_send + (size_t)d * ab, src.device, ab, ow.stream);
            return e;
        });
        if (!rc && tpos) rc = tps_enqueue_or(ow.ix, ow.mws, ow.ws, ow.d_block, ow.d_block.capacity(), ow.d_ids_recv + (size_t)d * iw, ow.ids_wire, d, W, seq,
                                             ow.d_tps_n + 2 * d, ow.d_tps_base + (size_t)d * bw, ow.d_seg_recv, sw, ow.tp_wire, ow.stream);
        if (!rc && aln) rc = tas_enqueue_align(t->sx, t, ow, &trs[d], d, W, seq, budget);
        if (!rc) rc = sharded_copy_back(ow);
        if (rc) return rc;
    }
    return KAAMER_OK;
}

// the batch (in the set's pinned staging) onto every shard's stream: search, pack, peer copies, merge, post-steps, result
// block, one D2H per owner.  On a non-OK return everything enqueued so far has been waited for.
static int sharded_enqueue(kaamer_sharded_ticket *t)
{
    kaamer_sharded_index *sx = t->sx;
    ShardSyncGuard guard{ t->set, true };
    int rc = sharded_prepare_all(t);
    if (rc) return rc;
    const uint32_t seq = ++t->set->seq;
    std::vector<kaamer_topn_result> trs(sx->n);
    rc = sharded_size_wire(t);
    if (!rc) rc = enqueue_search_pack(t);
    if (!rc) rc = enqueue_merge_topn(t, seq, trs);
    if (!rc && tpos_or_aln(t)) {   // the round trip after top-N: the owners' ids blocks, the shards' segments
        uint64_t budget = 0;
        bool timing = false;
        if (t->b.aln) { std::lock_guard<std::mutex> lock(sx->mu); budget = sx->aln_budget ? sx->aln_budget : TA_DEFAULT_BUDGET; timing = sx->aln_timing; }
        rc = enqueue_ids_round_shards(t, seq, timing);
        if (!rc) rc = enqueue_ids_round_owners(t, seq, trs, budget);
    }
    if (rc) return rc;
    guard.armed = false;
    return KAAMER_OK;
}

// what the subject segments and the blocks' alignment sections may take on the first attempt on a set (a batch beyond
// either is repeated with what it needed; later calls start from the previous call's need plus a quarter).  Segments: the
// pairs a query reports (MaxResults, at most 16 as for the ids blocks) x the table's mean stored length, the batch's
// queries dealt over W owners and their subjects over W holders, doubled for skew.  Sections: ta_first_cap's rule per owner.
static void tas_first_caps(const kaamer_sharded_index *sx, kaamer_sharded_ticket *t)
{
    const uint64_t W = sx->n, K = t->top.max_results, f = K < 16 ? K : 16;
    const uint64_t mean = sx->aln_entries ? sx->aln_number_of_aa / sx->aln_entries + 1 : 1;
    const bool nucl = is_nucl(t->seq_type);
    const uint64_t queries = nucl ? t->seq_bytes / 300 + t->n_seqs : t->n_seqs;   // (an ORF that reports is about a read long)
    t->b.sa_bytes = 2 * (queries / W + 1) * f * mean / W + 65536;
    if (t->b.sa_bytes > (1ull << 30)) t->b.sa_bytes = 1ull << 30;   // (three buffers of W segments each: a batch beyond it says what it needs)
    uint64_t guess = 0;
    for (const ShardState &st : t->set->sh) if (st.aln_guess > guess) guess = st.aln_guess;
    if (guess) t->b.aln_cap = guess;
    else if (nucl) t->b.aln_cap = (1ull << 20) + t->seq_bytes / 4 / W;
    else t->b.aln_cap = ((uint64_t)t->n_seqs / W + 1) * K * sizeof(kaamer_align_pair) + (t->aln.text ? 2 * K * t->seq_bytes / W : 0) + 4096;
}

// The worker pool of search_protein.go:58-118 against ONE sharded handle: submit takes a free set of per-shard
// workspaces, buffers and streams (callers beyond the sets wait for one), copies the caller's buffers into the set's
// pinned staging and enqueues the whole batch on every device; wait collects it.  A ticket is waited for exactly once.
// top = NULL: a full call (kaamer_sharded_submit_batch_flat), `t` is then the caller's (a kaamer_sharded_full_ticket's).
// block = false: no waiting for a set (a stream must never wait for a set it holds itself): KAAMER_E_BUSY instead
static int sharded_submit(kaamer_sharded_index *sx, const kaamer_batch_in *in, const kaamer_topn_opts *top, kaamer_sharded_ticket *t,
                          bool top_pos, const TopAlnRequest *aln = nullptr, bool block = true)
{
    SEQ_TYPE_CHK(in->seq_type, "sharded_submit_batch");
    ShardSet *set = nullptr;
    {
        std::unique_lock<std::mutex> lock(sx->mu);
        for (;;) {
            for (int k = 0; k < KAAMER_SHARDED_SETS && !set; k++)
                if (!sx->sets[k].busy) set = &sx->sets[k];
            if (set) break;
            if (!block) return kaamer_fail(KAAMER_E_BUSY, "all %d sets of the handle are busy: wait for / pop an earlier batch first", KAAMER_SHARDED_SETS);
            sx->cv.wait(lock);
        }
        // an aligning call takes its set while the table is there: kaamer_sharded_index_attach_proteins refuses to replace
        // it from here on (same lock)
        if (aln && !sx->aln) return kaamer_fail(KAAMER_E_ARG, "sharded_submit_batch_top_aln: no protein table is attached to the handle (kaamer_sharded_index_attach_proteins)");
        set->busy = true;
    }
    memset(t, 0, sizeof *t);
    t->sx = sx; t->set = set; t->n_seqs = in->n_seqs; t->seq_type = in->seq_type; t->seq_bytes = in->offsets[in->n_seqs];
    if (top) t->top = *top;
    // entries one (shard -> owner) block can hold: data dependent; enlarged on KAAMER_E_CAPACITY like every bound
    t->b.e_cap = 2 * t->seq_bytes / sx->n + 65536;
    t->b.full = top == nullptr;
    t->b.pos = t->b.full && in->want_positions != 0;
    t->b.tpos = !t->b.full && top_pos;   // the bitmaps of the reported hits (kaamer_sharded_submit_batch_top_pos_flat)
    if (aln && !t->b.full) {
        t->want_aln = true; t->aln = *aln;
        t->b.aln = aln->on;   // (without a matrix row nothing is aligned and no exchange runs: the host marks every item)
        t->max_query_len = batch_max_query_len(in);
        if (t->b.aln) tas_first_caps(sx, t);
    }
    if (t->b.pos) {   // bitmap words per entry ~ 1 + SizeInKmer / 64 (ORFs: a third of the nucleotides)
        const bool nucl = is_nucl(in->seq_type);
        const uint64_t mean = t->seq_bytes / (in->n_seqs ? in->n_seqs : 1u) / (nucl ? 3u : 1u);
        t->b.p_cap = t->b.e_cap * (1 + mean / 64);
    }
    // the caller's buffers -> pinned staging, once; every device copies from there (and a retry runs from there)
    const size_t off_at = ((size_t)t->seq_bytes + 7) & ~(size_t)7;
    const size_t in_need = off_at + ((size_t)in->n_seqs + 1) * 8;
    int rc = reserve(set->h_in, in_need, GROW_SLOT, nullptr);   // (the set is this call's alone: nothing reads the old staging)
    if (!rc) {
        if (t->seq_bytes) memcpy(set->h_in, in->seqs, (size_t)t->seq_bytes);
        memcpy(set->h_in + off_at, in->offsets, ((size_t)in->n_seqs + 1) * 8);
        rc = sharded_enqueue(t);
    }
    if (rc) sharded_release(sx, set);
    return rc;
}

static int sharded_submit_top(kaamer_sharded_index *sx, const kaamer_batch_in *in, const kaamer_topn_opts *top, bool top_pos, kaamer_sharded_ticket **ticket,
                              const TopAlnRequest *aln = nullptr, bool block = true)
{
    if (!sx || !in || !top || !ticket || !in->offsets || (in->n_seqs && !in->seqs) || top->max_results < 1)
        return kaamer_fail(KAAMER_E_ARG, "sharded_submit_batch_top: bad argument");
    *ticket = nullptr;
    kaamer_sharded_ticket *t = new (std::nothrow) kaamer_sharded_ticket();
    if (!t) return kaamer_fail(KAAMER_E_NOMEM, "ticket");
    const int rc = sharded_submit(sx, in, top, t, top_pos, aln, block);
    if (rc) { delete t; return rc; }
    *ticket = t;
    return KAAMER_OK;
}

int kaamer_sharded_submit_batch_top(kaamer_sharded_index *sx, const kaamer_batch_in *in, const kaamer_topn_opts *top, kaamer_sharded_ticket **ticket)
{
    return sharded_submit_top(sx, in, top, false, ticket);
}

int kaamer_sharded_submit_batch_top_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                         double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_sharded_ticket **ticket)
{
    kaamer_batch_in in;
    kaamer_topn_opts top;
    flat_in(&in, seqs, offsets, n_seqs, seq_type, 0);
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    return kaamer_sharded_submit_batch_top(sx, &in, &top, ticket);
}

// ---- the same calls with the PositionHits bitmaps of the reported hits (search.go:442-452,520-522) ---------------------
int kaamer_sharded_submit_batch_top_pos_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                             double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_sharded_ticket **ticket)
{
    kaamer_batch_in in;
    kaamer_topn_opts top;
    flat_in(&in, seqs, offsets, n_seqs, seq_type, 1);
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    return sharded_submit_top(sx, &in, &top, true, ticket);
}

// ---- ... and with the alignment of the reported hits (search.go:483-494) ------------------------------------------------
int kaamer_sharded_submit_batch_top_aln_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                             double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t want_positions,
                                             const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text, kaamer_sharded_ticket **ticket)
{
    if (!sx || !sub_matrix || !ticket) return kaamer_fail(KAAMER_E_ARG, "sharded_submit_batch_top_aln: bad argument");
    kaamer_batch_in in;
    kaamer_topn_opts top;
    flat_in(&in, seqs, offsets, n_seqs, seq_type, want_positions ? 1 : 0);
    flat_top(&top, min_k_ratio, min_k_match, max_results);
    const TopAlnRequest rq = top_aln_request(sub_matrix, gap_open, gap_extend, want_text);
    return sharded_submit_top(sx, &in, &top, want_positions != 0, ticket, &rq);
}

// ---- full hit lists (kaamer_sharded_search_batch): the same pipeline without the post-steps -----------------------------
int kaamer_sharded_submit_batch_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                     int32_t want_positions, kaamer_sharded_full_ticket **ticket)
{
    if (!sx || !ticket || !offsets || (n_seqs && !seqs)) return kaamer_fail(KAAMER_E_ARG, "sharded_submit_batch: bad argument");
    *ticket = nullptr;
    kaamer_batch_in in;
    flat_in(&in, seqs, offsets, n_seqs, seq_type, want_positions);
    kaamer_sharded_full_ticket *ft = new (std::nothrow) kaamer_sharded_full_ticket();
    if (!ft) return kaamer_fail(KAAMER_E_NOMEM, "ticket");
    const int rc = sharded_submit(sx, &in, nullptr, &ft->t, false);
    if (rc) { delete ft; return rc; }
    *ticket = ft;
    return KAAMER_OK;
}
