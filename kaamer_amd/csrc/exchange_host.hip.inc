// exchange_host.hip.inc — the exchange step of the sharded index, host half (included by search.hip behind the merge; the
// block format, the kernels and the step's state XState are in exchange.hip.inc).  The include stands among the C entry
// points, hence the extern "C++" around its two templates.
//
//   layout calls           a block's size, and the cut of a capacity layout to one batch
//   kaamer_exchange_pack   check, grow, fill parameters, scans, copies
//   kaamer_exchange_merge  check, grow, fill parameters, scan, copy, bitmap scan and copy, statistics to the host, merge
//   stats calls            what the W headers of the last two merges said
//   kaamer_rccl_alltoall   the transport for hosts that own an RCCL communicator

// ---- layouts ------------------------------------------------------------------------------------------------------------
// blocks with bitmaps (arrays = 4): the section starts at the even word after the three entry arrays, and what is left of
// the block is its capacity: p_cap = (block_words - bits_off) / 2 u64 words
static uint64_t x_bits_off(const kaamer_exchange_layout *L) { return (X_HDR + 2ull * L->q_cap + 3ull * L->e_cap + 1) & ~1ull; }
static uint64_t x_p_cap(const kaamer_exchange_layout *L)
{
    const uint64_t o = x_bits_off(L);
    return L->arrays == 4 && L->block_words > o ? (L->block_words - o) / 2 : 0;
}
// words of a block with L's q_cap, e_cap and arrays, and (arrays = 4) room for pos_words u64 bitmap words
static uint64_t x_block_words(const kaamer_exchange_layout *L, uint64_t pos_words)
{
    if (L->arrays == 4) return (x_bits_off(L) + 2 * pos_words + 3) & ~3ull;
    return (X_HDR + (uint64_t)L->q_cap + (uint64_t)L->arrays * L->e_cap + 3) & ~3ull;
}
// q_cap and e_cap of a capacity layout cut to one batch
static void x_cut(kaamer_exchange_layout *L, uint32_t n_queries, uint64_t entries_per_block)
{
    const uint64_t q = ((uint64_t)n_queries + L->world - 1) / L->world + 1;
    if (q < L->q_cap) L->q_cap = (uint32_t)q;
    uint64_t e = (entries_per_block + 3) & ~3ull;
    if (e < 4) e = 4;
    if (e < L->e_cap) L->e_cap = e;
}

int kaamer_exchange_layout_init(uint32_t world, uint32_t rank, uint32_t max_queries, uint64_t max_entries_per_peer,
                                kaamer_exchange_layout *out)
{
    if (!out || world == 0 || world > 64 || rank >= world || max_entries_per_peer == 0 || max_entries_per_peer > 0xFFFFFFF0ull)
        return kaamer_fail(KAAMER_E_ARG, "exchange_layout_init: bad argument (1 <= world <= 64, rank < world, 0 < entries < 2^32)");
    memset(out, 0, sizeof *out);
    out->world = world;
    out->rank = rank;
    out->q_cap = (max_queries + world - 1) / world + 1;
    out->arrays = 3;
    out->e_cap = (max_entries_per_peer + 3) & ~3ull;
    out->block_words = x_block_words(out, 0);
    return KAAMER_OK;
}

int kaamer_exchange_layout_init_positions(uint32_t world, uint32_t rank, uint32_t max_queries, uint64_t max_entries_per_peer,
                                          uint64_t max_pos_words_per_peer, kaamer_exchange_layout *out)
{
    if (!out || max_pos_words_per_peer == 0 || max_pos_words_per_peer > 0xFFFFFFF0ull)
        return kaamer_fail(KAAMER_E_ARG, "exchange_layout_init_positions: bad argument (0 < pos words < 2^32)");
    const int rc = kaamer_exchange_layout_init(world, rank, max_queries, max_entries_per_peer, out);
    if (rc) return rc;
    out->arrays = 4;
    out->block_words = x_block_words(out, max_pos_words_per_peer);
    return KAAMER_OK;
}

int kaamer_exchange_layout_fit(const kaamer_exchange_layout *cap, uint32_t n_queries, uint64_t entries_per_block, int32_t with_first_pos,
                               kaamer_exchange_layout *out)
{
    if (!cap || !out || cap->world == 0) return kaamer_fail(KAAMER_E_ARG, "exchange_layout_fit: bad argument");
    kaamer_exchange_layout L = *cap;
    L.arrays = with_first_pos ? 3u : 2u;   // a protein search without -pos sends no first positions: no room for them either
    x_cut(&L, n_queries, entries_per_block);
    L.block_words = x_block_words(&L, 0);
    if (L.block_words > cap->block_words) L = *cap;   // never beyond what the buffers hold
    *out = L;
    return KAAMER_OK;
}

int kaamer_exchange_layout_fit_positions(const kaamer_exchange_layout *cap, uint32_t n_queries, uint64_t entries_per_block,
                                         uint64_t pos_words_per_block, kaamer_exchange_layout *out)
{
    if (!cap || !out || cap->world == 0 || cap->arrays != 4)
        return kaamer_fail(KAAMER_E_ARG, "exchange_layout_fit_positions: bad argument (a capacity layout of kaamer_exchange_layout_init_positions)");
    kaamer_exchange_layout L = *cap;
    x_cut(&L, n_queries, entries_per_block);
    uint64_t pw = pos_words_per_block < 2 ? 2 : pos_words_per_block;
    const uint64_t pc = x_p_cap(cap);
    if (pw > pc) pw = pc;
    L.block_words = x_block_words(&L, pw);
    if (L.block_words > cap->block_words) L = *cap;   // never beyond what the buffers hold
    *out = L;
    return KAAMER_OK;
}

// ---- steps that pack and merge share ------------------------------------------------------------------------------------
// what a layout asks of the workspace it is used with; `does` / `kind`: the words in which the two calls differ
static int x_check(const kaamer_workspace *ws, const kaamer_exchange_layout *L, const char *call, const char *does, const char *kind)
{
    if (L->arrays == 2 && ws->firstpos) return kaamer_fail(KAAMER_E_ARG, "%s: the layout has no room for the first positions this workspace %s", call, does);
    if (L->arrays == 4 && (!ws->want_positions || !ws->firstpos))
        return kaamer_fail(KAAMER_E_ARG, "%s: blocks with bitmaps need a %s workspace with want_positions = 1 and first_pos = 1", call, kind);
    if (L->arrays == 4 && x_p_cap(L) == 0) return kaamer_fail(KAAMER_E_ARG, "%s: the layout has no bitmap section", call);
    return KAAMER_OK;
}

// The growth rule of the step's buffers (reserve_group, GROW_EXACT): when one buffer of a group holds less than asked, the
// whole group is made again, every buffer exactly as large as asked (the capacity layout of a searcher does not change: a
// margin would only cost memory), once the stream is done with the old ones.

// the block geometry of a layout, and the tile sums its scans need: (world + 1) rows of n_tiles
static int x_params(kaamer_workspace *ws, const kaamer_exchange_layout *L, hipStream_t s, XParams *x)
{
    memset(x, 0, sizeof *x);
    x->world = L->world; x->rank = L->rank; x->q_cap = L->q_cap; x->e_cap = L->e_cap; x->block_words = L->block_words;
    x->ent_base = X_HDR + L->q_cap;
    if (L->arrays == 4) { x->ent_base += L->q_cap; x->bits_off = x_bits_off(L); x->p_cap = x_p_cap(L); }
    x->with_fp = ws->firstpos ? 1u : 0u;
    x->n_tiles = (uint32_t)(((uint64_t)L->q_cap + X_TILE - 1) / X_TILE);
    const int rc = reserve_group(s, GROW_EXACT, { want(ws->x.tiles, (size_t)(L->world + 1) * x->n_tiles) });
    x->tile_sum = ws->x.tiles;
    return rc;
}

// the scan of `rows` rows of per-query items (exchange.hip.inc): tile sums, their scan and the row totals' consequences,
// the items' offsets; the entry scans (modes 0, 1) of a few tiles per row in one launch instead
extern "C++" template <int MODE> static void x_enqueue_scan(const XParams &x, uint32_t rows, hipStream_t s)
{
    if constexpr (MODE < 2) {
        if (x.n_tiles <= X_SMALL_TILES) {
            hipLaunchKernelGGL(x_scan_small_kernel<MODE>, dim3(rows), dim3(X_BLOCK), 0, s, x);
            return;
        }
    }
    hipLaunchKernelGGL(x_scan_sums_kernel<MODE>, dim3(x.n_tiles, rows), dim3(X_BLOCK), 0, s, x);
    hipLaunchKernelGGL(x_scan_top_kernel<MODE>, dim3(1), dim3(X_BLOCK), 0, s, x);
    hipLaunchKernelGGL(x_scan_apply_kernel<MODE>, dim3(x.n_tiles, rows), dim3(X_BLOCK), 0, s, x);
}

// the copy kernels' form: a wave per query (few queries with long lists) while `form_queries` is at most X_WIDE_QUERIES,
// else 16 lanes per query; 4 / 16 queries of the n per workgroup, at most 8 workgroups per CU
struct XCopy { bool wide; uint32_t grid; };
static XCopy x_copy_form(const kaamer_workspace *ws, uint64_t form_queries, uint32_t n)
{
    XCopy c;
    c.wide = form_queries <= X_WIDE_QUERIES;
    c.grid = c.wide ? (n + 3) / 4 : (n + 15) / 16;
    if (c.grid > (uint32_t)ws->n_cu * 8) c.grid = (uint32_t)ws->n_cu * 8;
    if (c.grid < 1) c.grid = 1;
    return c;
}
#define X_LAUNCH_COPY(kernel, c, s, x)                                                                              \
    do {                                                                                                            \
        if ((c).wide) hipLaunchKernelGGL(kernel<X_GROUP_WIDE>, dim3((c).grid), dim3(X_COPY_BLOCK), 0, s, x);        \
        else hipLaunchKernelGGL(kernel<X_GROUP>, dim3((c).grid), dim3(X_COPY_BLOCK), 0, s, x);                      \
    } while (0)

// ---- pack ---------------------------------------------------------------------------------------------------------------
int kaamer_exchange_pack(kaamer_workspace *ws, const kaamer_exchange_layout *L, uint32_t *d_send, void *stream)
{
    if (!ws || !L || !d_send || L->world == 0) return kaamer_fail(KAAMER_E_ARG, "exchange_pack: bad argument");
    { const int rc = x_check(ws, L, "exchange_pack", "computes", "search"); if (rc) return rc; }
    // (a layout fitted to fewer queries than the batch turns out to have is an overflow like any other: flagged in the
    // block headers by the scan, reported by every owner)
    const bool pos = L->arrays == 4;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ws->device));
    { const int jrc = ws_join(ws, s); if (jrc) return jrc; }
    XState &xs = ws->x;
    const size_t per_query = (size_t)L->world * L->q_cap;
    int rc = reserve_group(s, GROW_EXACT, { want(xs.dst_off, per_query) });
    if (!rc && pos) rc = reserve_group(s, GROW_EXACT, { want(xs.dst_boff, per_query) });
    XParams x;
    if (!rc) rc = x_params(ws, L, s, &x);
    if (rc) return rc;
    const WsHits h = ws_hits(ws);
    x.d_nq = ws->d_nq;
    x.src_status = ws->d_status_out;  // written by the search's finalize step, earlier on this stream
    x.hit_off = h.off; x.hit_cnt = ws->d_q_cnt; x.pid = h.pid; x.km = h.km; x.fp = h.fp;
    x.send = d_send;
    x.dst_off = xs.dst_off;
    if (pos) {   // the bitmap sections: SizeInKmer per owned query, where each query's bitmaps start, header words [6], [7]
        x.qinfo = ws->d_qinfo;
        x.pos_off = ws->d_pos_off;
        x.pos_bits = ws->d_pos_bits;
        x.dst_boff = xs.dst_boff;
    }
    x_enqueue_scan<0>(x, L->world, s);
    if (pos) x_enqueue_scan<2>(x, L->world, s);
    const XCopy c = x_copy_form(ws, ws->q_cap, ws->q_cap);
    X_LAUNCH_COPY(x_pack_copy_kernel, c, s, x);
    if (pos) X_LAUNCH_COPY(x_pack_bits_kernel, c, s, x);
    HIPCHK(hipGetLastError());
    return KAAMER_OK;
}

// ---- merge --------------------------------------------------------------------------------------------------------------
// the unpack buffers for L: entries of all sources (m_cap), and with bitmaps their words (mb_cap); the statistics' slots
static int x_grow_unpack(XState &xs, const kaamer_exchange_layout *L, uint64_t m_cap, uint64_t mb_cap, hipStream_t s)
{
    int rc = reserve_group(s, GROW_EXACT, { want(xs.src_off, (size_t)L->world * L->q_cap), want(xs.nq_owned, 1), want(xs.ent_off, (size_t)L->q_cap + 1),
                         want(xs.pid, (size_t)m_cap), want(xs.km, (size_t)m_cap), want(xs.fp, (size_t)m_cap), want(xs.stats, 4) });
    const size_t pq = (size_t)L->world * L->q_cap + 1;   // per (source, owned query); also bounds the per-query arrays
    if (!rc && L->arrays == 4)
        rc = reserve_group(s, GROW_EXACT, { want(xs.src_boff, pq), want(xs.ent_boff, pq), want(xs.msize, pq), want(xs.mdst, (size_t)m_cap),
                         want(xs.gtab, 2 * (size_t)m_cap), want(xs.mbits, (size_t)mb_cap) });
    if (!rc) rc = reserve_group(s, GROW_EXACT, { want(xs.pstats, 2) });
    if (rc || xs.ev_stats[1]) return rc;   // (the statistics' pinned slots and their events are there)
    rc = reserve(xs.h_stats, 2, GROW_EXACT, s);
    if (rc) return rc;
    memset(xs.h_stats, 0, 2 * sizeof(XStatsSlot));
    for (DevEvent &e : xs.ev_stats) if (!e) HIPCHK(hipEventCreateWithFlags(&e.e, hipEventDisableTiming));
    return KAAMER_OK;
}

// what the W headers said, to the host: read by kaamer_exchange_stats without waiting for the merge itself
static int x_stats_to_host(XState &xs, hipStream_t s)
{
    const int i = (int)(xs.merge_seq & 1u);
    XStatsSlot &slot = xs.h_stats[i];
    HIPCHK(hipMemcpyAsync(slot.stats, xs.stats, sizeof slot.stats, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(slot.pstats, xs.pstats, sizeof slot.pstats, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(xs.ev_stats[i], s));
    xs.merge_seq++;
    return KAAMER_OK;
}

// behind the merge of blocks with bitmaps: the merged hits' bitmaps laid out (and zeroed), every received bitmap ORed in
static void x_enqueue_or_merge(kaamer_workspace *ws, XParams &x, uint32_t nq_bound, hipStream_t s)
{
    launch_pos_layout(ws, nq_bound, x.m_size, ws->d_list_counts + SLOT_STATUS, s);
    const WsHits h = ws_hits(ws);
    x.r_nq = ws->d_nq;
    x.r_cnt = ws->d_q_cnt;
    x.r_off = h.off;
    x.r_pid = h.pid;
    x.r_pos_off = ws->d_pos_off;
    x.r_pos_base = ws->d_pos_base;
    x.r_pos_bits = ws->d_pos_bits;
    x.r_bits_cap = ws->bits_cap;
    const uint32_t gb = nq_bound < (uint32_t)ws->n_cu * 16 ? nq_bound : (uint32_t)ws->n_cu * 16;
    hipLaunchKernelGGL(x_or_bits_kernel, dim3(gb ? gb : 1), dim3(64), 0, s, x);
}

int kaamer_exchange_merge(kaamer_workspace *ws, const kaamer_exchange_layout *L, const uint32_t *d_recv, void *stream,
                          kaamer_device_result *out)
{
    if (!ws || !L || !d_recv || !out || L->world == 0) return kaamer_fail(KAAMER_E_ARG, "exchange_merge: bad argument");
    { const int rc = x_check(ws, L, "exchange_merge", "wants", "merge"); if (rc) return rc; }
    if (L->q_cap > ws->q_cap) return kaamer_fail(KAAMER_E_CAPACITY, "exchange_merge: %u owned queries exceed the merge workspace (%u)", L->q_cap, ws->q_cap);
    const uint64_t m_cap = (uint64_t)L->world * L->e_cap;
    if (m_cap > ws->hit_cap) return kaamer_fail(KAAMER_E_CAPACITY, "exchange_merge: %llu entries exceed the merge workspace's max_hits (%llu)",
                                                 (unsigned long long)m_cap, (unsigned long long)ws->hit_cap);
    const bool pos = L->arrays == 4;
    const uint64_t mb_cap = pos ? (uint64_t)L->world * x_p_cap(L) : 0;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ws->device));
    XState &xs = ws->x;
    XParams x;
    int rc = x_grow_unpack(xs, L, m_cap, mb_cap, s);
    if (!rc) rc = x_params(ws, L, s, &x);
    if (!rc) rc = ws_reset_if_dirty(ws, s);   // the status word the unpack kernels may set must start from zero
    if (rc) return rc;
    ws->clean = true;
    x.recv = d_recv;
    x.src_off = xs.src_off;
    x.ent_off = xs.ent_off;
    x.d_nq_owned = xs.nq_owned;
    x.m_pid = xs.pid; x.m_km = xs.km; x.m_fp = xs.fp;
    x.m_cap = m_cap;
    x.stats = xs.stats;
    x.status = ws->d_list_counts + SLOT_STATUS;
    x_enqueue_scan<1>(x, L->world + 1, s);
    const XCopy c = x_copy_form(ws, (uint64_t)L->q_cap * L->world, L->q_cap);
    X_LAUNCH_COPY(x_unpack_copy_kernel, c, s, x);
    if (pos) {   // the bitmap sections: sizes checked alike in all blocks, offsets per source and per owned query, copy
        x.src_boff = xs.src_boff;
        x.ent_boff = xs.ent_boff;
        x.m_size = xs.msize;
        x.m_bits = xs.mbits;
        x.mb_cap = mb_cap;
        x.pstats = xs.pstats;
        x.m_dst = xs.mdst;
        x.g_tab = xs.gtab;
        x_enqueue_scan<3>(x, L->world + 1, s);
        X_LAUNCH_COPY(x_unpack_bits_kernel, c, s, x);
    } else {
        HIPCHK(hipMemsetAsync(xs.pstats, 0, 2 * sizeof(unsigned long long), s));
    }
    HIPCHK(hipGetLastError());
    rc = x_stats_to_host(xs, s);
    if (!rc) rc = merge_enqueue(ws, xs.ent_off, xs.pid, xs.km, xs.fp, L->q_cap, xs.nq_owned, m_cap, s);
    if (rc) return rc;
    if (pos) x_enqueue_or_merge(ws, x, L->q_cap, s);
    return merge_finish(ws, s, pos, out);
}

// ---- statistics -----------------------------------------------------------------------------------------------------------
// the pinned slot of the merge `back` calls ago, once its copy has arrived
static int x_stats_slot(kaamer_workspace *ws, const void *out, uint32_t back, const char *call, uint64_t *seq, const XStatsSlot **slot)
{
    if (!ws || !out || back > 1) return kaamer_fail(KAAMER_E_ARG, "%s: bad argument (back is 0 or 1)", call);
    if (ws->x.merge_seq <= back || !ws->x.h_stats) return kaamer_fail(KAAMER_E_ARG, "%s: no such merge yet", call);
    *seq = ws->x.merge_seq - 1 - back;
    HIPCHK(hipSetDevice(ws->device));
    HIPCHK(hipEventSynchronize(ws->x.ev_stats[*seq & 1u]));
    *slot = &ws->x.h_stats[*seq & 1u];
    return KAAMER_OK;
}

int kaamer_exchange_stats(kaamer_workspace *ws, uint32_t back, uint64_t out[4])
{
    uint64_t seq;
    const XStatsSlot *slot;
    const int rc = x_stats_slot(ws, out, back, "exchange_stats", &seq, &slot);
    if (rc) return rc;
    out[0] = seq;
    for (int i = 0; i < 3; i++) out[1 + i] = slot->stats[i];
    return KAAMER_OK;
}

int kaamer_exchange_stats_positions(kaamer_workspace *ws, uint32_t back, uint64_t out[2])
{
    uint64_t seq;
    const XStatsSlot *slot;
    const int rc = x_stats_slot(ws, out, back, "exchange_stats_positions", &seq, &slot);
    if (rc) return rc;
    for (int i = 0; i < 2; i++) out[i] = slot->pstats[i];
    return KAAMER_OK;
}

// ---- transport ------------------------------------------------------------------------------------------------------------
// grouped ncclSend / ncclRecv of equal blocks, for hosts that own an RCCL communicator and nothing else to drive it
// (the library does not link RCCL: the symbols are looked up in the process at first use)
int kaamer_rccl_alltoall(void *nccl_comm, const void *d_send, void *d_recv, uint64_t bytes_per_peer, uint32_t world, void *stream)
{
    typedef int (*grp_t)(void);
    typedef int (*send_t)(const void *, size_t, int, int, void *, void *);
    typedef int (*recv_t)(void *, size_t, int, int, void *, void *);
    static grp_t g_start = nullptr, g_end = nullptr;
    static send_t g_send = nullptr;
    static recv_t g_recv = nullptr;
    if (!nccl_comm || !d_send || !d_recv || world == 0) return kaamer_fail(KAAMER_E_ARG, "rccl_alltoall: bad argument");
    if (!g_send) {
        void *h = dlopen(nullptr, RTLD_NOW);
        void *sym = h ? dlsym(h, "ncclSend") : nullptr;
        if (!sym) { h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL); if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL); }
        if (!h) return kaamer_fail(KAAMER_E_HIP, "rccl_alltoall: librccl is not loaded and cannot be opened");
        g_start = (grp_t)dlsym(h, "ncclGroupStart"); g_end = (grp_t)dlsym(h, "ncclGroupEnd");
        g_recv = (recv_t)dlsym(h, "ncclRecv");
        g_send = (send_t)dlsym(h, "ncclSend");
        if (!g_start || !g_end || !g_send || !g_recv) { g_send = nullptr; return kaamer_fail(KAAMER_E_HIP, "rccl_alltoall: RCCL symbols not found"); }
    }
    const int nccl_uint8 = 1;  // ncclUint8 (nccl.h: ncclInt8 = 0, ncclUint8 = 1)
    int rc = g_start();
    for (uint32_t peer = 0; peer < world && rc == 0; peer++) {
        rc = g_send((const char *)d_send + (size_t)peer * bytes_per_peer, (size_t)bytes_per_peer, nccl_uint8, (int)peer, nccl_comm, stream);
        if (rc == 0) rc = g_recv((char *)d_recv + (size_t)peer * bytes_per_peer, (size_t)bytes_per_peer, nccl_uint8, (int)peer, nccl_comm, stream);
    }
    const int rc2 = g_end();
    if (rc || rc2) return kaamer_fail(KAAMER_E_HIP, "rccl_alltoall: RCCL error %d", rc ? rc : rc2);
    return KAAMER_OK;
}
