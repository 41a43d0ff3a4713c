// host_sharded.hip.inc — ONE process driving an index that is sharded over several devices (included by search.hip
// inside its extern "C" block, after host_top.hip.inc).
//
// The reference server is one process that opens its stores once and fans out goroutines (api/server.go:47-65,
// search_fastq.go:60-66).  kaamer_index_open_sharded gives that process one handle over W hash-prefix shards, each
// resident on its own device (SURVEY 8b: kaamer_index_open(path, devices[], n_devices)); a call drives all of them:
//
//   every shard s (its device, its stream):  H2D of the batch, kaamer_search_device, kaamer_exchange_pack
//   every owner d:  waits for the W pack events, pulls block (s -> d) of every shard with hipMemcpyPeerAsync
//                   (xGMI point to point: every owner pulls from every shard at once), kaamer_exchange_merge,
//                   kaamer_topn_device(orf_source = its own translation of the batch), the packed result block, one D2H
//   with PositionHits of the reported hits (kaamer_sharded_search_batch_top_pos_flat), one more round trip before the D2H
//   (top_positions_sharded.hip.inc), on the same streams and without a host synchronisation:
//   every owner d:  its reported ids as a compact ids block; every shard pulls all W of them
//   every shard s:  per owner, the partial bitmaps its own vals[] give, into segment d of a send buffer
//   every owner d:  pulls segment d of every shard and ORs them into the pos_bits section of its result block
//   with the alignment of the reported hits (kaamer_sharded_search_batch_top_aln_flat), the same round trip carries the
//   subjects (top_align_sharded.hip.inc): the Protein.Sequence table is partitioned over the devices by id mod W
//   every owner d:  the same ids block (packed and pulled once when positions are wanted too)
//   every holder s: per owner, the stored bytes of the reported subjects it holds, into segment d of a send buffer
//   every owner d:  pulls segment d of every holder, assembles the pairs and aligns them (ta_stage, host_top_align.hip.inc);
//                   pair records and operations are two more sections of its result block
//   host:  interleaves the W owners' reported queries back into batch order (query q is owned by shard q mod W)
// No external communicator, no second process.  (One process per GPU with RCCL is the other deployment:
// kaamer_exchange_pack / kaamer_rccl_alltoall / kaamer_exchange_merge, INTEGRATION.md 4b.)

struct ShardState {
    kaamer_index *ix = nullptr;
    int device = 0;
    kaamer_workspace *ws = nullptr, *mws = nullptr;
    kaamer_workspace_opts opts{};
    kaamer_exchange_layout layout{};   // capacity: what d_send / d_recv hold
    kaamer_exchange_layout wire{};     // the blocks of the batch in flight (<= capacity)
    uint64_t e_cap = 0;
    uint64_t p_cap = 0;                // bitmap words a block can hold (full calls with positions)
    bool full = false;                 // workspaces of a full call (kaamer_sharded_search_batch): first_pos = 1, CSR merge
    uint32_t *d_send = nullptr, *d_recv = nullptr;
    size_t x_words = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_packed = nullptr;
    uint8_t *d_seqs = nullptr;
    uint64_t *d_off = nullptr;
    size_t seq_cap = 0, off_cap = 0;
    uint8_t *d_block = nullptr, *h_block = nullptr;
    size_t d_block_cap = 0, h_block_cap = 0, guess = 1u << 16, copied = 0;
    // top calls with the PositionHits of the reported hits (top_positions_sharded.hip.inc)
    bool tpos = false;                 // workspaces and buffers of such a call
    uint32_t tp_k = 0, tp_scale = 0;   // MaxResults and BatchBounds::pos_scale the capacities below were made for
    TpsIdsLayout ids_cap{}, ids_wire{};   // the ids block: capacity, and as it travels for the batch in flight
    uint64_t tp_cap = 0, tp_wire = 0;     // bitmap words of one (shard -> owner) segment: capacity, as it travels
    uint32_t *d_ids = nullptr, *d_ids_recv = nullptr;                   // the owner's ids block; the W owners' blocks as pulled
    unsigned long long *d_seg_send = nullptr, *d_seg_recv = nullptr;    // W segments each (one header word + the bitmap words)
    uint32_t *d_tps_words = nullptr, *d_tps_n = nullptr;                // [rq_cap]; per owner {reported queries, status}
    uint64_t *d_tps_base = nullptr;                                     // [W][rq_cap + 1] word offsets per owner
    hipEvent_t ev_ids = nullptr, ev_bits = nullptr;   // the owner's ids block is packed; the shard's segments (bitmaps, subjects) are made
    // top calls that align the reported hits (top_align_sharded.hip.inc)
    TasLayout sa_cap{}, sa_wire{};     // a (holder -> owner) subject segment: capacity, and as it travels for the batch in flight
    uint8_t *d_sa_send = nullptr, *d_sa_recv = nullptr, *d_sa_codes = nullptr;   // W segments each; the letter codes of the received ones
    uint32_t *d_sa_qbytes = nullptr, *d_sa_n = nullptr;                          // [rq_cap + 1]; per owner {reported queries, status}
    uint64_t *d_sa_off = nullptr;                                                // owner: per pair, where its subject lies in d_sa_recv
    unsigned long long *d_sa_need = nullptr;                                     // holder: per owner {payload bytes needed, status}
    uint64_t aln_guess = 0;            // bytes the alignment sections of this owner's previous block needed, plus a quarter
    uint64_t sa_stage[3] = {0, 0, 0};  // the owner's last alignment stage: resident waves, slab bytes, long-subject waves
    hipEvent_t ev_t[5] = {};           // kaamer_sharded_index_set_align_timing: gather begin / end, assemble begin, alignment begin / end
    bool timed = false;                // ... recorded for the attempt in flight
};

// everything one call in flight needs on every shard (the indices themselves are shared by all sets)
struct ShardSet {
    std::vector<ShardState> sh;
    uint8_t *h_in = nullptr;
    size_t h_in_cap = 0;
    bool busy = false;
    uint64_t need_entries = 0;   // what the largest (shard -> owner) block of the previous batch on this set needed
    uint32_t need_queries = 0;   // its queries (ORFs)
    uint64_t need_pos_words = 0; // the bitmap words it needed (0: the previous batch carried no bitmaps)
    // the previous top call with positions on this set: what the largest ids block and bitmap segment needed
    bool tp_seen = false;
    uint32_t need_ids_rq = 0;
    uint64_t need_ids_ent = 0, need_tp_words = 0;
    uint64_t tp_ids_bytes = 0, tp_seg_bytes = 0, tp_attempts = 0;   // kaamer_sharded_positions_info
    uint32_t seq = 0;            // batch sequence of the ids blocks and segments
    // the previous aligning call on this set: payload bytes the largest subject segment needed; kaamer_sharded_align_info
    bool sa_seen = false;
    uint64_t need_sa_bytes = 0;
    uint64_t sa_seg_bytes = 0, sa_need_seg = 0, sa_attempts = 0;
    uint64_t sa_ids_bytes = 0;                  // one ids block as it travelled in that call
    uint64_t sa_us[3] = {0, 0, 0};              // its gather, assemble and alignment stages: the slowest device's, microseconds (timing on)
    uint64_t sa_stage[3] = {0, 0, 0};           // waves, slab bytes, long-subject waves: the largest over the owners
};
/* KAAMER_SHARDED_SETS (kaamer_hip.h): calls in flight per handle, the goroutines of search_fastq.go:60-66 against one handle */

struct kaamer_sharded_index {
    uint32_t n = 0;
    std::vector<kaamer_index *> *ix = nullptr;   // shard s, resident on device (*dev)[s]
    std::vector<int> *dev = nullptr;
    ShardSet *sets = nullptr;                    // KAAMER_SHARDED_SETS of them; a call takes a free one, callers beyond wait
    std::mutex mu;
    std::condition_variable cv;
    // kaamer_sharded_index_attach_proteins: the Protein.Sequence table, partitioned over the devices by id mod W
    struct AlnPart {
        uint8_t *d_raw = nullptr;      // the stored bytes of the entries this device holds
        uint64_t *d_off = nullptr;     // entries + 1
        uint32_t *d_idmap = nullptr;   // id / W -> entry, TA_NONE: no entry
        int *d_matrix = nullptr;
        uint32_t idmap_n = 0, entries = 0;
        uint64_t bytes = 0;
    };
    std::vector<AlnPart> *aln = nullptr;         // one per device once a table is attached
    const kaamer_proteins *aln_host = nullptr;   // borrowed: the rows of a result with text read the subjects from it
    int aln_matrix[26 * 26];
    uint32_t aln_entries = 0, aln_max_ns = 0;
    uint64_t aln_bytes = 0, aln_share = 0, aln_number_of_aa = 0;
    uint64_t aln_budget = 0;                     // kaamer_sharded_index_set_align_budget (0: the default)
    bool aln_timing = false;                     // kaamer_sharded_index_set_align_timing
};

static void shard_tps_free(ShardState &s)
{
    void *bufs[] = { s.d_ids, s.d_ids_recv, s.d_seg_send, s.d_seg_recv, s.d_tps_words, s.d_tps_n, s.d_tps_base };
    for (void *b : bufs) if (b) (void)hipFree(b);
    s.d_ids = s.d_ids_recv = nullptr; s.d_seg_send = s.d_seg_recv = nullptr;
    s.d_tps_words = s.d_tps_n = nullptr; s.d_tps_base = nullptr;
}

static void shard_sa_free(ShardState &s)
{
    void *bufs[] = { s.d_sa_send, s.d_sa_recv, s.d_sa_codes, s.d_sa_qbytes, s.d_sa_n, s.d_sa_off, s.d_sa_need };
    for (void *b : bufs) if (b) (void)hipFree(b);
    s.d_sa_send = s.d_sa_recv = s.d_sa_codes = nullptr; s.d_sa_qbytes = s.d_sa_n = nullptr; s.d_sa_off = nullptr; s.d_sa_need = nullptr;
    s.sa_cap = TasLayout();
}

static void sharded_aln_free(kaamer_sharded_index *sx)
{
    if (!sx->aln) return;
    for (uint32_t s = 0; s < sx->n; s++) {
        kaamer_sharded_index::AlnPart &a = (*sx->aln)[s];
        (void)hipSetDevice((*sx->dev)[s]);
        void *bufs[] = { a.d_raw, a.d_off, a.d_idmap, a.d_matrix };
        for (void *b : bufs) if (b) (void)hipFree(b);
    }
    delete sx->aln;
    sx->aln = nullptr; sx->aln_host = nullptr;
    sx->aln_entries = sx->aln_max_ns = 0; sx->aln_bytes = sx->aln_share = sx->aln_number_of_aa = 0;
}

static void shard_state_free(ShardState &s)
{
    (void)hipSetDevice(s.device);
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.ws) kaamer_workspace_free(s.ws);
    if (s.mws) kaamer_workspace_free(s.mws);
    void *bufs[] = { s.d_send, s.d_recv, s.d_seqs, s.d_off, s.d_block };
    for (void *b : bufs) if (b) (void)hipFree(b);
    shard_tps_free(s);
    shard_sa_free(s);
    if (s.h_block) pinned_put(s.h_block, s.h_block_cap);
    if (s.ev_packed) (void)hipEventDestroy(s.ev_packed);
    if (s.ev_ids) (void)hipEventDestroy(s.ev_ids);
    if (s.ev_bits) (void)hipEventDestroy(s.ev_bits);
    for (hipEvent_t e : s.ev_t) if (e) (void)hipEventDestroy(e);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = ShardState();   // (the index belongs to the handle)
}

void kaamer_sharded_index_close(kaamer_sharded_index *sx)
{
    if (!sx) return;
    if (sx->sets) {
        for (int k = 0; k < KAAMER_SHARDED_SETS; k++) {
            for (ShardState &s : sx->sets[k].sh) shard_state_free(s);
            if (sx->sets[k].h_in) (void)hipHostFree(sx->sets[k].h_in);
        }
        delete[] sx->sets;
    }
    if (sx->dev) sharded_aln_free(sx);
    if (sx->ix) {
        for (kaamer_index *ix : *sx->ix) if (ix) kaamer_index_close(ix);
        delete sx->ix;
    }
    delete sx->dev;
    delete sx;
}

static int sharded_open_common(uint32_t n, const int *devices, kaamer_sharded_index **out,
                               int (*open_one)(uint32_t, int, kaamer_index **, const void *), const void *ctx)
{
    if (!out || !devices || n == 0 || n > 64) return kaamer_fail(KAAMER_E_ARG, "index_open_sharded: bad argument");
    *out = nullptr;
    kaamer_sharded_index *sx = new (std::nothrow) kaamer_sharded_index();
    if (!sx) return kaamer_fail(KAAMER_E_NOMEM, "sharded index");
    sx->ix = new (std::nothrow) std::vector<kaamer_index *>(n, nullptr);
    sx->dev = new (std::nothrow) std::vector<int>(devices, devices + n);
    sx->sets = new (std::nothrow) ShardSet[KAAMER_SHARDED_SETS];
    if (!sx->ix || !sx->dev || !sx->sets) { kaamer_sharded_index_close(sx); return kaamer_fail(KAAMER_E_NOMEM, "sharded index"); }
    sx->n = n;
    for (int k = 0; k < KAAMER_SHARDED_SETS; k++) sx->sets[k].sh.resize(n);
    for (uint32_t s = 0; s < n; s++) {
        kaamer_index *&ix = (*sx->ix)[s];
        int rc = open_one(s, devices[s], &ix, ctx);
        if (!rc && (ix->hdr.n_shards != n || ix->hdr.shard != s))
            rc = kaamer_fail(KAAMER_E_FORMAT, "index_open_sharded: image %u is shard %u of %u, expected shard %u of %u", s, ix->hdr.shard,
                             ix->hdr.n_shards, s, n);
        for (int k = 0; k < KAAMER_SHARDED_SETS && !rc; k++) {
            ShardState &st = sx->sets[k].sh[s];
            st.device = devices[s];
            st.ix = ix;
            hipError_t e = hipSetDevice(devices[s]);
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&st.ev_packed, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&st.ev_ids, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&st.ev_bits, hipEventDisableTiming);
            if (e != hipSuccess) rc = kaamer_fail(KAAMER_E_HIP, "index_open_sharded: %s", hipGetErrorString(e));
        }
        if (rc) { kaamer_sharded_index_close(sx); return rc; }
    }
    // direct peer access where the devices allow it (the copies work without it, staged by the runtime)
    for (uint32_t a = 0; a < n; a++)
        for (uint32_t b = 0; b < n; b++) {
            if (devices[a] == devices[b]) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[a], devices[b]) == hipSuccess && can) {
                (void)hipSetDevice(devices[a]);
                (void)hipDeviceEnablePeerAccess(devices[b], 0);  // (already enabled: an error we ignore)
                (void)hipGetLastError();
            }
        }
    *out = sx;
    return KAAMER_OK;
}

static int open_one_path(uint32_t s, int device, kaamer_index **ix, const void *ctx)
{
    return kaamer_index_open(((const char *const *)ctx)[s], device, ix);
}
static int open_one_image(uint32_t s, int device, kaamer_index **ix, const void *ctx)
{
    return kaamer_index_open_image(((const kaamer_image *const *)ctx)[s], device, ix);
}

int kaamer_index_open_sharded(const char *const *paths, const int *devices, uint32_t n_shards, kaamer_sharded_index **out)
{
    if (!paths) return kaamer_fail(KAAMER_E_ARG, "index_open_sharded: bad argument");
    return sharded_open_common(n_shards, devices, out, open_one_path, paths);
}

int kaamer_index_open_sharded_images(const kaamer_image *const *images, const int *devices, uint32_t n_shards, kaamer_sharded_index **out)
{
    if (!images) return kaamer_fail(KAAMER_E_ARG, "index_open_sharded_images: bad argument");
    return sharded_open_common(n_shards, devices, out, open_one_image, images);
}

uint32_t kaamer_sharded_index_shards(const kaamer_sharded_index *sx) { return sx ? sx->n : 0u; }

extern "C++" {
template <class T> static int dev_grow(T **p, size_t *cap, size_t need)
{
    if (*cap >= need) return KAAMER_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    const size_t want = need + need / 4 + 64;
    const int rc = dev_alloc(p, want);
    if (!rc) *cap = want;
    return rc;
}
}  // extern "C++"

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
                             uint32_t W, uint32_t seq, uint64_t budget);

static int shard_prepare(ShardState &st, uint32_t W, uint32_t rank, uint64_t seq_bytes, uint32_t n_seqs, int32_t seq_type, const ShardBounds &b, uint32_t K)
{
    HIPCHK(hipSetDevice(st.device));
    seq_type = seq_base(seq_type);   // (the genetic code is the call's: every shard gets it with the batch, kaamer_search_device)
    const bool nucl = is_nucl(seq_type);
    const kaamer_workspace_opts &o = st.opts;
    const bool fits = st.ws && o.seq_type == seq_type && o.max_seq_bytes >= seq_bytes && o.max_seqs >= (n_seqs ? n_seqs : 1) &&
                      o.g_tier_slots >= b.bb.g_slots && o.max_queries >= b.bb.max_queries && st.e_cap >= b.e_cap &&
                      o.max_hits >= b.bb.max_hits && (b.bb.max_hits != 0 || o.max_hits == 0) &&
                      st.full == b.full && (o.want_positions != 0) == b.pos && (!b.pos || st.p_cap >= b.p_cap) &&
                      st.tpos == b.tpos;
    if (!fits) {
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
        if (st.x_words < words) {
            if (st.d_send) (void)hipFree(st.d_send);
            if (st.d_recv) (void)hipFree(st.d_recv);
            st.d_send = st.d_recv = nullptr; st.x_words = 0;
            rc = dev_alloc(&st.d_send, words);
            if (!rc) rc = dev_alloc(&st.d_recv, words);
            if (rc) return rc;
            st.x_words = words;
        }
        shard_tps_free(st);   // (sized from the workspaces: made again below)
        st.tpos = b.tpos;
        st.tp_k = 0; st.tp_scale = 0;
    }
    // the reported hits' bitmaps: the unsharded rule (next to kaamer_topn_positions_device) divided over the owners,
    // x pos_scale on a repeat, never beyond the hard bound; the ids block likewise (every owned query may report).  A
    // repeat that grows pos_scale alone (or a larger MaxResults) makes these buffers and the result block again, nothing
    // else: the workspaces and the exchange buffers stay.
    const uint32_t scale = b.bb.pos_scale ? b.bb.pos_scale : 1u;
    if ((b.tpos || b.aln) && (st.tp_k < K || st.tp_scale < scale)) {   // (the ids block serves both kinds; the rest is the bitmaps')
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
        int rc = dev_alloc(&st.d_ids, iw);
        if (!rc) rc = dev_alloc(&st.d_ids_recv, (size_t)W * iw);
        if (!rc && b.tpos) rc = dev_alloc(&st.d_seg_send, (size_t)W * sw);
        if (!rc && b.tpos) rc = dev_alloc(&st.d_seg_recv, (size_t)W * sw);
        if (!rc && b.tpos) rc = dev_alloc(&st.d_tps_words, (size_t)oq + 1);
        if (!rc && b.tpos) rc = dev_alloc(&st.d_tps_n, (size_t)2 * W);
        if (!rc && b.tpos) rc = dev_alloc(&st.d_tps_base, (size_t)W * (oq + 1));
        if (rc) { shard_tps_free(st); st.tp_k = 0; st.tp_scale = 0; return rc; }
        st.tp_k = K; st.tp_scale = scale;
    }
    // the subject segments: what the ids block can describe, and the payload bound of this attempt.  They alone are made
    // again when that bound grows.
    if (b.aln && (!st.d_sa_send || st.sa_cap.rq_cap < st.ids_cap.rq_cap || st.sa_cap.ent_cap < st.ids_cap.ent_cap || st.sa_cap.byte_cap < b.sa_bytes)) {
        HIPCHK(hipStreamSynchronize(st.stream));
        TasLayout L;
        L.rq_cap = st.ids_cap.rq_cap; L.ent_cap = st.ids_cap.ent_cap;
        L.byte_cap = st.sa_cap.byte_cap > b.sa_bytes ? st.sa_cap.byte_cap : b.sa_bytes;
        shard_sa_free(st);
        const size_t sb = (size_t)tas_seg_bytes(L);
        int rc = dev_alloc(&st.d_sa_send, (size_t)W * sb);
        if (!rc) rc = dev_alloc(&st.d_sa_recv, (size_t)W * sb);
        if (!rc) rc = dev_alloc(&st.d_sa_codes, (size_t)W * sb);
        if (!rc) rc = dev_alloc(&st.d_sa_qbytes, (size_t)L.rq_cap + 1);
        if (!rc) rc = dev_alloc(&st.d_sa_n, (size_t)2 * W);
        if (!rc) rc = dev_alloc(&st.d_sa_off, (size_t)L.ent_cap + 1);
        if (!rc) rc = dev_alloc(&st.d_sa_need, (size_t)2 * W);
        if (rc) { shard_sa_free(st); return rc; }
        st.sa_cap = L;
    }
    int rc = dev_grow(&st.d_seqs, &st.seq_cap, (size_t)seq_bytes + 16);
    if (!rc) rc = dev_grow(&st.d_off, &st.off_cap, (size_t)n_seqs + 1);
    if (!rc && !b.full) rc = dev_grow(&st.d_block, &st.d_block_cap, rep_block_bound(st.mws, st.ws, K, b.tpos ? st.tp_cap : 0) + (b.aln ? (size_t)b.aln_cap + 64 : 0));
    return rc;
}

struct kaamer_sharded_ticket;
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
    p.block = ow.d_block; p.block_cap = ow.d_block_cap; p.aln_cap = t->b.aln_cap; p.want_text = t->aln.text ? 1 : 0;
    p.status = mws->d_status_out;
    return ta_stage(ws, p, budget, sx->aln_max_ns, t->max_query_len, &sp, ow.stream, ow.sa_stage, ow.timed ? ow.ev_t + 2 : nullptr);
}

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

// a block of `bytes` from another shard's device (or this one) onto `s`, a stream of dst_device
static hipError_t peer_pull_async(void *dst, int dst_device, const void *src, int src_device, size_t bytes, hipStream_t s)
{
    return src_device == dst_device ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipMemcpyPeerAsync(dst, dst_device, src, src_device, bytes, s);
}

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

static void sharded_release(kaamer_sharded_index *sx, ShardSet *set)
{
    { std::lock_guard<std::mutex> lock(sx->mu); set->busy = false; }
    sx->cv.notify_one();
}

// the speculative copy of an owner's result block
static int sharded_copy_back(ShardState &ow)
{
    return rep_block_copy_guess(ow.d_block, ow.d_block_cap, ow.guess, &ow.h_block, &ow.h_block_cap, &ow.copied, ow.stream);
}

// the batch (in the set's pinned staging) onto every shard's stream: search, pack, peer copies, merge, post-steps, result
// block, one D2H per owner.  On a non-OK return everything enqueued so far has been waited for.
static int sharded_enqueue(kaamer_sharded_ticket *t)
{
    kaamer_sharded_index *sx_ = t->sx;
    ShardSet *sx = t->set;
    const uint32_t W = sx_->n;
    const uint64_t seq_bytes = t->seq_bytes;
    const bool nucl = is_nucl(t->seq_type);
    std::vector<ShardState> &sh = sx->sh;
    const size_t off_at = ((size_t)seq_bytes + 7) & ~(size_t)7;
    ShardSyncGuard guard{ sx, true };
    for (uint32_t s = 0; s < W; s++) {
        const int rc = shard_prepare(sh[s], W, s, seq_bytes, t->n_seqs, t->seq_type, t->b, t->top.max_results);
        if (rc) {
            // some shards are prepared for this call and some are not: the ids blocks and segments have one layout on every
            // shard of a set, so all of them are sized again by the next call
            for (ShardState &x : sh) { x.tp_k = 0; x.tp_scale = 0; x.sa_cap = TasLayout(); }
            return rc;
        }
    }
    // the blocks of this batch: what the previous batch on this set needed + a quarter (its W x W headers, read after the
    // call), or the capacity for a first call and for a retry.  What the peer copies move is payload, not capacity.
    t->adaptive = t->attempt == 0 && sx->need_entries != 0 && (!t->b.pos || sx->need_pos_words != 0) && (!t->b.tpos || sx->tp_seen) &&
                  (!t->b.aln || sx->sa_seen);
    const bool ids = t->b.tpos || t->b.aln;   // the round trip after top-N: the owners' ids blocks, the shards' segments
    const uint32_t seq = ++sx->seq;
    for (uint32_t s = 0; s < W; s++) {
        ShardState &st = sh[s];
        st.wire = st.layout;
        if (t->adaptive) {
            const uint32_t nq = sx->need_queries + sx->need_queries / 4 + 64;
            const uint64_t ne = sx->need_entries + sx->need_entries / 4 + 1024;
            const int rc = t->b.pos ? kaamer_exchange_layout_fit_positions(&st.layout, nq, ne, sx->need_pos_words + sx->need_pos_words / 4 + 1024, &st.wire)
                                    : kaamer_exchange_layout_fit(&st.layout, nq, ne, (nucl || t->b.full) ? 1 : 0, &st.wire);
            if (rc) return rc;
        }
        if (ids) {   // the ids blocks and segments of this batch: sized the same way
            st.ids_wire = st.ids_cap;
            st.tp_wire = st.tp_cap;
            if (t->adaptive) {
                const uint64_t rq = (uint64_t)sx->need_ids_rq + sx->need_ids_rq / 4 + 64, ne = sx->need_ids_ent + sx->need_ids_ent / 4 + 1024,
                               nw = sx->need_tp_words + sx->need_tp_words / 4 + 1024;
                if (rq < st.ids_cap.rq_cap) st.ids_wire.rq_cap = (uint32_t)rq;
                if (ne < st.ids_cap.ent_cap) st.ids_wire.ent_cap = ne;
                if (nw < st.tp_cap) st.tp_wire = nw;
            }
        }
        if (t->b.aln) {   // a subject segment describes what the previous batch reported + a quarter, and holds its payload + a quarter
            st.sa_wire = st.sa_cap;
            if (t->adaptive) {
                const uint64_t rq = (uint64_t)sx->need_ids_rq + sx->need_ids_rq / 4 + 16, ne = sx->need_ids_ent + sx->need_ids_ent / 4 + 64,
                               nb = sx->need_sa_bytes + sx->need_sa_bytes / 4 + 256;
                if (rq < st.sa_cap.rq_cap) st.sa_wire.rq_cap = (uint32_t)rq;
                if (ne < st.sa_cap.ent_cap) st.sa_wire.ent_cap = ne;
                if (nb < st.sa_cap.byte_cap) st.sa_wire.byte_cap = nb;
            }
        }
    }
    // ---- every shard: the whole batch against its keys, partial hit lists packed per owner
    for (uint32_t s = 0; s < W; s++) {
        ShardState &st = sh[s];
        HIPCHK(hipSetDevice(st.device));
        if (seq_bytes) HIPCHK(hipMemcpyAsync(st.d_seqs, sx->h_in, (size_t)seq_bytes, hipMemcpyHostToDevice, st.stream));
        HIPCHK(hipMemcpyAsync(st.d_off, sx->h_in + off_at, ((size_t)t->n_seqs + 1) * 8, hipMemcpyHostToDevice, st.stream));
        kaamer_device_result dr;
        int rc = kaamer_search_device(st.ix, st.ws, st.d_seqs, st.d_off, t->n_seqs, seq_bytes, t->seq_type, st.stream, &dr);
        if (!rc) rc = kaamer_exchange_pack(st.ws, &st.wire, st.d_send, st.stream);
        if (rc) return rc;
        HIPCHK(hipEventRecord(st.ev_packed, st.stream));
    }
    // ---- every owner: pull its blocks, merge, post-steps, result block
    std::vector<kaamer_topn_result> trs(W);
    for (uint32_t d = 0; d < W; d++) {
        ShardState &ow = sh[d];
        HIPCHK(hipSetDevice(ow.device));
        const size_t bw = (size_t)ow.wire.block_words;
        for (uint32_t s = 0; s < W; s++) {
            ShardState &src = sh[s];
            if (s != d) HIPCHK(hipStreamWaitEvent(ow.stream, src.ev_packed, 0));
            const uint32_t *from = src.d_send + (size_t)d * bw;
            uint32_t *to = ow.d_recv + (size_t)s * bw;
            HIPCHK(peer_pull_async(to, ow.device, from, src.device, bw * 4, ow.stream));
        }
        kaamer_device_result mr;
        if (t->b.full) {   // the merged CSR (bitmaps included) stays on the owner until sharded_collect_full copies it
            const int rc = kaamer_exchange_merge(ow.mws, &ow.wire, ow.d_recv, ow.stream, &mr);
            if (rc) return rc;
            continue;
        }
        kaamer_topn_result tr;
        kaamer_topn_opts tt = t->top;
        tt.best_start_codon = nucl ? 1u : 0u;
        tt.d_size_in_kmer = nullptr;
        tt.orf_source = ow.ws; tt.q_first = d; tt.q_stride = W;
        int rc = kaamer_exchange_merge(ow.mws, &ow.wire, ow.d_recv, ow.stream, &mr);
        if (!rc) rc = kaamer_topn_device(ow.mws, &tt, ow.stream, &tr);
        if (!rc) rc = topn_pack_block(ow.mws, ow.ws, d, W, &tr, ow.stream, ow.d_block, ow.d_block_cap);
        trs[d] = tr;
        if (!rc && ids) {   // the result block waits for its bitmaps and alignments (below)
            rc = tps_enqueue_ids_pack(ow.mws, &tr, ow.d_block, ow.d_block_cap, ow.d_ids, ow.ids_wire, d, W, seq, ow.stream);
            if (rc) return rc;
            HIPCHK(hipEventRecord(ow.ev_ids, ow.stream));
            continue;
        }
        if (rc) return rc;
        rc = sharded_copy_back(ow);
        if (rc) return rc;
    }
    if (ids) {
        const uint32_t K = t->top.max_results;
        const bool tpos = t->b.tpos, aln = t->b.aln;
        uint64_t budget = 0;
        bool timing = false;
        if (aln) { std::lock_guard<std::mutex> lock(sx_->mu); budget = sx_->aln_budget ? sx_->aln_budget : TA_DEFAULT_BUDGET; timing = sx_->aln_timing; }
        // ---- every shard: pulls the W ids blocks; per owner, its partial bitmaps of the reported hits and the stored bytes
        // of the reported subjects it holds, into segment d of the two send buffers
        for (uint32_t s = 0; s < W; s++) {
            ShardState &st = sh[s];
            HIPCHK(hipSetDevice(st.device));
            const size_t iw = (size_t)tps_ids_words(st.ids_wire), sw = (size_t)st.tp_wire + 1, bw = (size_t)st.ids_wire.rq_cap + 1;
            for (uint32_t d = 0; d < W; d++) {
                ShardState &ow = sh[d];
                if (d != s) HIPCHK(hipStreamWaitEvent(st.stream, ow.ev_ids, 0));
                uint32_t *to = st.d_ids_recv + (size_t)d * iw;
                HIPCHK(peer_pull_async(to, st.device, ow.d_ids, ow.device, iw * 4, st.stream));
            }
            st.timed = false;
            if (aln && timing) {   // (made on first use, on the shard's device)
                for (hipEvent_t &e : st.ev_t) if (!e) HIPCHK(hipEventCreate(&e));
                st.timed = true;
                HIPCHK(hipEventRecord(st.ev_t[0], st.stream));
            }
            for (uint32_t d = 0; d < W && aln; d++) {
                const int rc = tas_enqueue_gather(sx_, st, s, d, W, seq, K);
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
        // ---- every owner: pulls segment d of every shard, ORs the bitmaps into its result block, aligns the pairs behind
        // them, one D2H
        for (uint32_t d = 0; d < W; d++) {
            ShardState &ow = sh[d];
            HIPCHK(hipSetDevice(ow.device));
            const size_t iw = (size_t)tps_ids_words(ow.ids_wire), sw = (size_t)ow.tp_wire + 1, bw = (size_t)ow.ids_wire.rq_cap + 1;
            const size_t ab = aln ? (size_t)tas_seg_bytes(ow.sa_wire) : 0;
            for (uint32_t s = 0; s < W; s++) {
                ShardState &src = sh[s];
                if (s != d) HIPCHK(hipStreamWaitEvent(ow.stream, src.ev_bits, 0));
                if (tpos) {
                    const unsigned long long *from = src.d_seg_send + (size_t)d * sw;
                    unsigned long long *to = ow.d_seg_recv + (size_t)s * sw;
                    HIPCHK(peer_pull_async(to, ow.device, from, src.device, sw * 8, ow.stream));
                }
                if (aln) {
                    const uint8_t *from = src.d_sa_send + (size_t)d * ab;
                    uint8_t *to = ow.d_sa_recv + (size_t)s * ab;
                    HIPCHK(peer_pull_async(to, ow.device, from, src.device, ab, ow.stream));
                }
            }
            int rc = KAAMER_OK;
            if (tpos) rc = tps_enqueue_or(ow.ix, ow.mws, ow.ws, ow.d_block, ow.d_block_cap, ow.d_ids_recv + (size_t)d * iw, ow.ids_wire, d, W, seq,
                                          ow.d_tps_n + 2 * d, ow.d_tps_base + (size_t)d * bw, ow.d_seg_recv, sw, ow.tp_wire, ow.stream);
            if (!rc && aln) rc = tas_enqueue_align(sx_, t, ow, &trs[d], d, W, seq, budget);
            if (!rc) rc = sharded_copy_back(ow);
            if (rc) return rc;
        }
    }
    guard.armed = false;
    return KAAMER_OK;
}

// waits for the attempt, checks it, fetches what the speculative copies missed and interleaves the owners' reported
// queries back into batch order.  KAAMER_E_CAPACITY: a bound was too small (the message says which, on which shard).
static int sharded_collect(kaamer_sharded_ticket *t, kaamer_batch_top **out)
{
    kaamer_sharded_index *sx_ = t->sx;
    ShardSet *sx = t->set;
    const uint32_t W = sx_->n;
    const bool nucl = is_nucl(t->seq_type);
    std::vector<ShardState> &sh = sx->sh;
    ShardSyncGuard guard{ sx, true };
    int err = KAAMER_OK;
    char why[256] = "";
    t->pos_only = true;   // (read only on the KAAMER_E_CAPACITY path of kaamer_sharded_wait_batch_top: cleared by any other failure bit)
    t->cap_bits = 0; t->grow_sections = false;
    for (uint32_t d = 0; d < W; d++) {
        ShardState &ow = sh[d];
        HIPCHK(hipSetDevice(ow.device));
        HIPCHK(hipStreamSynchronize(ow.stream));
        const RepBlockHdr *hdr = reinterpret_cast<const RepBlockHdr *>(ow.h_block);
        const uint32_t status = hdr->status & 0x7FFFFFFFu;
        if (hdr->status & ~(uint32_t)(ST_POS_CAP | ST_IDS_CAP | ST_SEG_CAP)) t->pos_only = false;
        t->cap_bits |= hdr->status;
        if (status) { ow.mws->clean = false; ow.ws->clean = false; }
        int rc = status_to_error(status, ow.mws);
        if (!rc && (hdr->status & 0x80000000u)) rc = kaamer_fail(KAAMER_E_CAPACITY, "result block capacity exceeded");
        if (rc) {
            if (!err) {
                // which bound: the owner's merge status says "a peer failed" or "a block overflowed"; the shards' own
                // search status words say what ran out there (ADVICE r3: a generic message hid a hit pool that never grew)
                uint32_t sst = 0;
                const uint32_t bad = sharded_failed_shard(sh, &sst);
                if (bad < W)
                    snprintf(why, sizeof why, "shard %u: search status 0x%x (%s%s%s)", bad, sst, (sst & ST_POOL_FULL) ? "hit pool " : "",
                             (sst & (ST_G_ARENA_FULL | ST_G_TABLE_FULL)) ? "G-tier arena " : "", (sst & (ST_QUERY_CAP | ST_AA_CAP)) ? "ORF capacity " : "");
                else
                    snprintf(why, sizeof why, "owner %u: merge status 0x%x (%s)", d, status,
                             (status & ST_SEG_CAP) ? "the reported hits' subjects exceed a segment" :
                             (status & ST_POS_CAP) ? "the reported hits' bitmaps exceed a segment" :
                             (status & ST_IDS_CAP) ? "the reported hits' ids exceed an ids block" :
                             (status & ST_EXCHANGE_CAP) ? "an exchange block overflowed" : "merge bounds");
                err = rc;
            }
            continue;
        }
        rc = rep_block_fetch_rest(ow.d_block, &ow.guess, &ow.h_block, &ow.h_block_cap, &ow.copied, ow.stream);
        if (rc) return rc;
    }
    guard.armed = false;  // every stream has been waited for
    {   // what this batch's blocks needed (every owner read the same W x W figures): sizes the next call's blocks
        uint64_t st4[4];
        if (kaamer_exchange_stats(sh[0].mws, 0, st4) == KAAMER_OK) { sx->need_queries = (uint32_t)st4[1]; sx->need_entries = st4[2]; }
    }
    const bool aln = t->b.aln;
    if (tpos_or_aln(t)) {   // what the ids blocks of this batch needed (the block headers hold it, whatever became of the batch)
        sx->need_ids_rq = 0; sx->need_ids_ent = 0;
        for (uint32_t d = 0; d < W; d++) {
            const RepBlockHdr *hdr = reinterpret_cast<const RepBlockHdr *>(sh[d].h_block);
            if (hdr->n_rep > sx->need_ids_rq) sx->need_ids_rq = hdr->n_rep;
            if (hdr->n_ent > sx->need_ids_ent) sx->need_ids_ent = hdr->n_ent;
        }
    }
    if (aln) {   // ... and the payload of the largest subject segment, as its holder counted it
        std::vector<unsigned long long> nd((size_t)2 * W);
        uint64_t need = 0;
        for (uint32_t s = 0; s < W; s++) {
            HIPCHK(hipSetDevice(sh[s].device));
            HIPCHK(hipMemcpy(nd.data(), sh[s].d_sa_need, nd.size() * 8, hipMemcpyDeviceToHost));
            for (uint32_t d = 0; d < W; d++) if (nd[2 * d] > need) need = nd[2 * d];
        }
        sx->need_sa_bytes = need;
        sx->sa_seen = true;
        sx->sa_seg_bytes = tas_seg_bytes(sh[0].sa_wire);
        sx->sa_need_seg = 16 + 8ull * ((uint64_t)sx->need_ids_rq + 1) + 4ull * sx->need_ids_ent + need;
        sx->sa_attempts = (uint64_t)t->attempt + 1;
        sx->sa_ids_bytes = 4ull * tps_ids_words(sh[0].ids_wire);
        for (int k = 0; k < 3; k++) { sx->sa_us[k] = 0; sx->sa_stage[k] = 0; }
        for (uint32_t d = 0; d < W; d++) {
            for (int k = 0; k < 3; k++) if (sh[d].sa_stage[k] > sx->sa_stage[k]) sx->sa_stage[k] = sh[d].sa_stage[k];
            if (!sh[d].timed) continue;
            const int from[3] = { 0, 2, 3 }, to[3] = { 1, 3, 4 };
            for (int k = 0; k < 3; k++) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, sh[d].ev_t[from[k]], sh[d].ev_t[to[k]]) != hipSuccess) { (void)hipGetLastError(); continue; }
                const uint64_t us = (uint64_t)(ms * 1000.0f);
                if (us > sx->sa_us[k]) sx->sa_us[k] = us;
            }
        }
    }
    if (err) return kaamer_fail(err, "sharded search: %s", why);
    std::vector<const RepAlnExt *> ax(W, nullptr);
    if (aln) {   // an owner whose alignment sections were too small: the batch once more, with what they needed
        uint64_t need = 0;
        bool small = false;
        for (uint32_t d = 0; d < W; d++) {
            ax[d] = rep_aln_ext(reinterpret_cast<const RepBlockHdr *>(sh[d].h_block));
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
    // ---- interleave the owners' reported queries back into batch order
    const bool tpos = t->b.tpos;
    uint64_t n_rep = 0, n_ent = 0, n_aa = 0, nq = 0, n_words = 0;
    std::vector<batch_top_owner> view(W);
    std::vector<const RepPosExt *> px(W, nullptr);
    if (tpos) {   // what the bitmap segments of this batch needed: sizes the next call's
        sx->need_tp_words = 0;
        for (uint32_t d = 0; d < W; d++) {
            px[d] = rep_pos_ext(reinterpret_cast<const RepBlockHdr *>(sh[d].h_block));
            if (!px[d]->off_pos_bits) return kaamer_fail(KAAMER_E_HIP, "sharded search: owner %u returned a block without its bitmap sections", d);
            if (px[d]->n_pos_words > sx->need_tp_words) sx->need_tp_words = px[d]->n_pos_words;
            n_words += px[d]->n_pos_words;
        }
        sx->tp_seen = true;
        sx->tp_ids_bytes = 4ull * tps_ids_words(sh[0].ids_wire);
        sx->tp_seg_bytes = 8ull * (sh[0].tp_wire + 1);
        sx->tp_attempts = (uint64_t)t->attempt + 1;
    }
    for (uint32_t d = 0; d < W; d++) {
        view[d].block = sh[d].h_block;
        top_owner_fill(&view[d]);
        n_rep += view[d].pub.n_reported;
        n_ent += view[d].pub.top_off[view[d].pub.n_reported];
        nq += view[d].pub.n_queries;
        const RepBlockHdr *hdr = reinterpret_cast<const RepBlockHdr *>(sh[d].h_block);
        n_aa += hdr->n_aa;
    }
    kaamer_counters c;
    const int crc = sharded_sum_counters(sh, &c);
    if (crc) return crc;
    for (uint32_t d = 0; d < W; d++) c.n_hits += view[d].pub.counters.n_hits;
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
    // the owners' pair records in batch order; their operations one owner behind the other, the records' offsets re-based
    std::vector<kaamer_align_pair> items(aln ? (size_t)n_ent : 0);
    std::vector<uint64_t> ops_base(W + 1, 0);
    std::vector<uint8_t> ops;
    if (aln) {
        for (uint32_t d = 0; d < W; d++) ops_base[d + 1] = ops_base[d] + ax[d]->ops_bytes;
        ops.resize((size_t)ops_base[W] + 1);
        for (uint32_t d = 0; d < W; d++)
            if (ax[d]->ops_bytes) memcpy(ops.data() + ops_base[d], sh[d].h_block + ax[d]->off_ops, (size_t)ax[d]->ops_bytes);
    }
    bool aln_bad = false;
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
                if (it.status == 0 && it.n_ops > 0 && t->aln.text) {
                    if (it.off + (uint64_t)it.n_ops > ax[best]->ops_bytes) aln_bad = true;
                    it.off += ops_base[best];
                }
                items[(size_t)(e + (j - b0))] = it;
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
    memset(&bo->pub, 0, sizeof bo->pub);
    bo->pub.n_queries = (uint32_t)nq;
    bo->pub.n_reported = (uint32_t)n_rep;
    bo->pub.max_results = t->top.max_results;
    bo->pub.rep_query = rq; bo->pub.trim = trim; bo->pub.q = qm; bo->pub.top_off = off;
    bo->pub.top_pid = pid; bo->pub.top_kmatch = km; bo->pub.top_first_pos = fp;
    bo->pub.orf_aa = nucl ? aa : nullptr;
    bo->pub.counters = c;
    if (t->want_aln) {   // floats, rows and the sort by BitScore on the combined result: the one-device call's finish
        TaFinish f;
        f.table = sx_->aln_host; f.matrix = sx_->aln_matrix; f.number_of_aa = sx_->aln_number_of_aa;
        f.rq = t->aln; f.nucl = nucl;
        f.h_in = sx->h_in;
        int rc = aln_bad ? kaamer_fail(KAAMER_E_FORMAT, "sharded search: inconsistent alignment sections") : KAAMER_OK;
        if (!rc) rc = ta_finish_rows(f, bo, items.data(), ops.data(), ops_base[W], tpos ? poff : nullptr);
        if (rc) { kaamer_batch_top_free(&bo->pub); return rc; }
    }
    *out = &bo->pub;
    return KAAMER_OK;
}

// The worker pool of search_protein.go:58-118 against ONE sharded handle: submit takes a free set of per-shard
// workspaces, buffers and streams (callers beyond the sets wait for one), copies the caller's buffers into the set's
// pinned staging and enqueues the whole batch on every device; wait collects it.  A ticket is waited for exactly once.
// top = NULL: a full call (kaamer_sharded_submit_batch_flat), `t` is then the caller's (a kaamer_sharded_full_ticket's)
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
    int rc = KAAMER_OK;
    if (set->h_in_cap < in_need) {
        if (set->h_in) (void)hipHostFree(set->h_in);
        set->h_in = nullptr; set->h_in_cap = 0;
        const size_t cap = in_need + in_need / 4 + 4096;
        if (hipHostMalloc((void **)&set->h_in, cap, hipHostMallocPortable) != hipSuccess) rc = kaamer_fail(KAAMER_E_NOMEM, "pinned input staging (%zu bytes)", cap);
        else set->h_in_cap = cap;
    }
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

int kaamer_sharded_wait_batch_top(kaamer_sharded_ticket *t, kaamer_batch_top **out)
{
    if (!t || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_wait_batch_top: bad argument");
    *out = nullptr;
    int rc;
    for (;;) {
        rc = sharded_collect(t, out);
        if (rc != KAAMER_E_CAPACITY || t->attempt >= MAX_BOUND_RETRIES) break;
        t->attempt++;
        if (t->cap_bits & ST_SEG_CAP) {   // a subject segment: its holder counted what it needs (also when sized from the previous call)
            const uint64_t need = t->set->need_sa_bytes + t->set->need_sa_bytes / 4 + 4096;
            if (need >= 0xFFFFFFFFull) { rc = kaamer_fail(KAAMER_E_CAPACITY, "sharded search: a subject segment of %llu bytes (the bound is 4 GiB)", (unsigned long long)need); break; }
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
        rc = sharded_enqueue(t);   // (an error here ends the loop, E_CAPACITY included: kept as it was)
        if (rc) break;
    }
    sharded_release(t->sx, t->set);
    delete t;
    return rc;
}

void kaamer_sharded_ticket_discard(kaamer_sharded_ticket *t)
{
    if (!t) return;
    sharded_sync_all(t->set);
    for (ShardState &st : t->set->sh) { if (st.ws) st.ws->clean = false; if (st.mws) st.mws->clean = false; }
    sharded_release(t->sx, t->set);
    delete t;
}

int kaamer_sharded_search_batch_top(kaamer_sharded_index *sx, const kaamer_batch_in *in, const kaamer_topn_opts *top, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_sharded_ticket *t = nullptr;
    const int rc = kaamer_sharded_submit_batch_top(sx, in, top, &t);
    if (rc) return rc;
    return kaamer_sharded_wait_batch_top(t, out);
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

int kaamer_sharded_search_batch_top_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                         double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_sharded_ticket *t = nullptr;
    const int rc = kaamer_sharded_submit_batch_top_flat(sx, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, &t);
    if (rc) return rc;
    return kaamer_sharded_wait_batch_top(t, out);
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

int kaamer_sharded_search_batch_top_pos_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                             double min_k_ratio, int64_t min_k_match, uint32_t max_results, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_sharded_ticket *t = nullptr;
    const int rc = kaamer_sharded_submit_batch_top_pos_flat(sx, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, &t);
    if (rc) return rc;
    return kaamer_sharded_wait_batch_top(t, out);
}

// ---- ... and with the alignment of the reported hits (search.go:483-494) ------------------------------------------------
int kaamer_sharded_index_attach_proteins(kaamer_sharded_index *sx, const kaamer_proteins *p)
{
    if (!sx || !p) return kaamer_fail(KAAMER_E_ARG, "sharded_index_attach_proteins: bad argument");
    const uint32_t W = sx->n;
    std::vector<uint32_t> uniq;
    std::vector<kaamer_protein_entry> ent;
    int rc = proteins_distinct(p, uniq, ent);
    if (rc) return rc;
    const uint32_t n = (uint32_t)uniq.size();
    const uint64_t map_n = n ? (uint64_t)uniq.back() / W + 1 : 0;   // of a device's local map, indexed by id / W
    if (map_n > (1ull << 31)) return kaamer_fail(KAAMER_E_ARG, "sharded_index_attach_proteins: protein ids up to %llu: the id maps are dense", (unsigned long long)uniq.back());
    uint64_t st[3] = {0, 0, 0};
    kaamer_proteins_stats(p, st);
    std::unique_lock<std::mutex> lock(sx->mu);   // held to the end: no call starts on a half-made table
    for (int k = 0; k < KAAMER_SHARDED_SETS; k++)
        if (sx->sets[k].busy) return kaamer_fail(KAAMER_E_BUSY, "sharded_index_attach_proteins: calls are in flight on the handle");
    for (uint32_t s = 0; s < W; s++) { HIPCHK(hipSetDevice((*sx->dev)[s])); HIPCHK(hipDeviceSynchronize()); }
    const uint64_t budget = sx->aln_budget;
    sharded_aln_free(sx);   // a second attach replaces the first
    sx->aln_budget = budget;
    sx->aln = new (std::nothrow) std::vector<kaamer_sharded_index::AlnPart>(W);
    if (!sx->aln) return kaamer_fail(KAAMER_E_NOMEM, "protein table");
    kaamer_align_matrix(sx->aln_matrix);
    uint32_t max_ns = 0;
    uint64_t total = 0, share = 0;
    std::vector<uint64_t> off;
    std::vector<uint8_t> raw;
    std::vector<uint32_t> idmap;
    for (uint32_t s = 0; s < W && !rc; s++) {   // device s: the entries whose id mod W == s, in id order
        kaamer_sharded_index::AlnPart &a = (*sx->aln)[s];
        off.assign(1, 0); raw.clear();
        idmap.assign((size_t)map_n + 1, TA_NONE);
        for (uint32_t i = 0; i < n; i++) {
            if (uniq[i] % W != s) continue;
            idmap[uniq[i] / W] = (uint32_t)off.size() - 1;
            raw.insert(raw.end(), ent[i].sequence, ent[i].sequence + ent[i].sequence_len);
            off.push_back(raw.size());
            if (ent[i].sequence_len > max_ns) max_ns = ent[i].sequence_len;
        }
        raw.resize(raw.size() + 16, 0);
        hipError_t e = hipSetDevice((*sx->dev)[s]);
        if (e != hipSuccess) { rc = kaamer_fail(KAAMER_E_HIP, "hipSetDevice: %s", hipGetErrorString(e)); break; }
        rc = dev_alloc(&a.d_raw, raw.size());
        if (!rc) rc = dev_alloc(&a.d_off, off.size());
        if (!rc) rc = dev_alloc(&a.d_idmap, idmap.size());
        if (!rc) rc = dev_alloc(&a.d_matrix, (size_t)ALN_NL * ALN_NL);
        if (rc) break;
        e = hipMemcpy(a.d_raw, raw.data(), raw.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(a.d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(a.d_idmap, idmap.data(), idmap.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(a.d_matrix, sx->aln_matrix, sizeof sx->aln_matrix, hipMemcpyHostToDevice);
        if (e != hipSuccess) { rc = kaamer_fail(KAAMER_E_HIP, "protein table upload: %s", hipGetErrorString(e)); break; }
        a.idmap_n = (uint32_t)map_n; a.entries = (uint32_t)off.size() - 1;
        a.bytes = raw.size() + off.size() * 8 + idmap.size() * 4 + sizeof sx->aln_matrix;
        total += a.bytes;
        if (a.bytes > share) share = a.bytes;
    }
    if (rc) { sharded_aln_free(sx); return rc; }
    sx->aln_host = p;
    sx->aln_entries = n; sx->aln_max_ns = max_ns; sx->aln_number_of_aa = st[1];
    sx->aln_bytes = total; sx->aln_share = share;
    for (int k = 0; k < KAAMER_SHARDED_SETS; k++) {   // what earlier calls needed was measured on another table
        sx->sets[k].sa_seen = false; sx->sets[k].need_sa_bytes = 0;
        for (ShardState &sh : sx->sets[k].sh) sh.aln_guess = 0;
    }
    return KAAMER_OK;
}

int kaamer_sharded_index_set_align_budget(kaamer_sharded_index *sx, uint64_t bytes)
{
    if (!sx) return kaamer_fail(KAAMER_E_ARG, "sharded_index_set_align_budget: bad argument");
    std::lock_guard<std::mutex> lock(sx->mu);
    sx->aln_budget = bytes;
    return KAAMER_OK;
}

int kaamer_sharded_align_info(kaamer_sharded_index *sx, uint64_t out[8])
{
    if (!sx || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_align_info: bad argument");
    std::lock_guard<std::mutex> lock(sx->mu);
    const ShardSet &set = sx->sets[0];
    out[0] = sx->aln_bytes; out[1] = sx->aln_share; out[2] = sx->aln_entries; out[3] = sx->aln_max_ns; out[4] = sx->aln_number_of_aa;
    out[5] = set.sa_seg_bytes; out[6] = set.sa_need_seg; out[7] = set.sa_attempts;
    return KAAMER_OK;
}

int kaamer_sharded_index_set_align_timing(kaamer_sharded_index *sx, int32_t on)
{
    if (!sx) return kaamer_fail(KAAMER_E_ARG, "sharded_index_set_align_timing: bad argument");
    std::lock_guard<std::mutex> lock(sx->mu);
    sx->aln_timing = on != 0;
    return KAAMER_OK;
}

int kaamer_sharded_align_stage_info(kaamer_sharded_index *sx, uint64_t out[8])
{
    if (!sx || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_align_stage_info: bad argument");
    std::lock_guard<std::mutex> lock(sx->mu);
    const ShardSet &set = sx->sets[0];
    out[0] = sx->aln_timing ? 1 : 0;
    out[1] = set.sa_us[0]; out[2] = set.sa_us[1]; out[3] = set.sa_us[2];
    out[4] = set.sa_ids_bytes;
    out[5] = set.sa_stage[0]; out[6] = set.sa_stage[1]; out[7] = set.sa_stage[2];
    return KAAMER_OK;
}

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

int kaamer_sharded_search_batch_top_aln_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                             double min_k_ratio, int64_t min_k_match, uint32_t max_results, int32_t want_positions,
                                             const char *sub_matrix, int32_t gap_open, int32_t gap_extend, int32_t want_text, kaamer_batch_top **out)
{
    if (out) *out = nullptr;
    kaamer_sharded_ticket *t = nullptr;
    const int rc = kaamer_sharded_submit_batch_top_aln_flat(sx, seqs, offsets, n_seqs, seq_type, min_k_ratio, min_k_match, max_results, want_positions,
                                                            sub_matrix, gap_open, gap_extend, want_text, &t);
    if (rc) return rc;
    return kaamer_sharded_wait_batch_top(t, out);
}

// the ids blocks and bitmap segments of the last finished call with positions on the handle's first set (tests, bench):
// out = { bytes of one ids block as it travelled, bytes of one (shard -> owner) bitmap segment as it travelled, bitmap
// words the largest segment needed, attempts the call took }
int kaamer_sharded_positions_info(kaamer_sharded_index *sx, uint64_t out[4])
{
    if (!sx || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_positions_info: bad argument");
    std::lock_guard<std::mutex> lock(sx->mu);
    const ShardSet &set = sx->sets[0];
    if (!set.tp_seen) return kaamer_fail(KAAMER_E_ARG, "sharded_positions_info: no call with positions yet");
    out[0] = set.tp_ids_bytes;
    out[1] = set.tp_seg_bytes;
    out[2] = set.need_tp_words;
    out[3] = set.tp_attempts;
    return KAAMER_OK;
}

// ---- full hit lists (kaamer_sharded_search_batch) ----------------------------------------------------------------------
// Waits for the attempt, checks every workspace and copies each owner's merged CSR (bitmaps included) to the host; then
// interleaves the owners' queries back into batch order (query q is owned by shard q mod W).  The query data (q, orf_aa,
// starts_alt) is shard 0's: every shard translates the batch alike.
static int sharded_collect_full(kaamer_sharded_ticket *t, kaamer_batch_out **out)
{
    ShardSet *sx = t->set;
    const uint32_t W = t->sx->n;
    const bool pos = t->b.pos;
    std::vector<ShardState> &sh = sx->sh;
    ShardSyncGuard guard{ sx, true };
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
    {   // what this batch's blocks needed (every owner read the same W x W figures): sizes the next call's blocks
        uint64_t st4[4], sp[2] = { 0, 0 };
        if (kaamer_exchange_stats(sh[0].mws, 0, st4) == KAAMER_OK) { sx->need_queries = (uint32_t)st4[1]; sx->need_entries = st4[2]; }
        if (kaamer_exchange_stats_positions(sh[0].mws, 0, sp) == KAAMER_OK) sx->need_pos_words = sp[0];
    }
    if (err) return kaamer_fail(err, "sharded search: %s", why);

    kaamer_workspace *q_ws = sh[0].ws;
    batch_out_owner *bo = new (std::nothrow) batch_out_owner();
    if (!bo) return kaamer_fail(KAAMER_E_NOMEM, "batch_out");
    std::unique_ptr<batch_out_owner> own(bo);
    uint32_t nq = 0;
    hipError_t e = hipSetDevice(sh[0].device);
    if (e == hipSuccess) e = hipMemcpy(&nq, q_ws->d_nq, 4, hipMemcpyDeviceToHost);
    // each owner's merged queries, CSR
    struct OwnerCsr {
        uint32_t n = 0;
        std::vector<uint64_t> off, pos_base, pos_off, bits;
        std::vector<uint32_t> cnt, pid, km, fp;
    };
    std::vector<OwnerCsr> oc(W);
    uint64_t n_hits = 0, n_words = 0;
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
        n_hits += h; n_words += w;
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

    // ---- interleave into batch order
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
    kaamer_counters c;
    const int crc = sharded_sum_counters(sh, &c);
    if (crc) return crc;
    c.n_hits = n_hits;
    memset(&bo->pub, 0, sizeof bo->pub);
    bo->pub.n_queries = nq;
    bo->pub.q = bo->q.data();
    bo->pub.hit_off = bo->hit_off.data();
    bo->pub.hit_cnt = bo->hit_cnt.data();
    bo->pub.hit_pid = bo->pid.data();
    bo->pub.hit_kmatch = bo->km.data();
    bo->pub.hit_first_pos = bo->fp.data();
    if (q_ws->nucleotide) { bo->pub.orf_aa = bo->orf_aa.data(); bo->pub.starts_alt = bo->starts_alt.data(); }
    if (pos) { bo->pub.pos_off = bo->pos_off.data(); bo->pub.pos_bits = bo->pos_bits.data(); }
    bo->pub.counters = c;
    *out = &own.release()->pub;
    return KAAMER_OK;
}

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

int kaamer_sharded_wait_batch(kaamer_sharded_full_ticket *ft, kaamer_batch_out **out)
{
    if (!ft || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_wait_batch: bad argument");
    *out = nullptr;
    kaamer_sharded_ticket *t = &ft->t;
    int rc;
    for (;;) {
        rc = sharded_collect_full(t, out);
        if (rc != KAAMER_E_CAPACITY || t->attempt >= MAX_BOUND_RETRIES) break;
        t->attempt++;
        if (!t->adaptive) {   // the bounds themselves were too small: enlarge them all, as kaamer_sharded_wait_batch_top does
            t->b.e_cap *= 4;
            t->b.p_cap *= 4;
            bounds_grow(t->b.bb, t->seq_bytes, t->n_seqs, is_nucl(t->seq_type));
        }   // else: the blocks sized from the previous call were too small -- once more at the full capacity, same bounds
        rc = sharded_enqueue(t);   // (an error here ends the loop, E_CAPACITY included: kept as it was)
        if (rc) break;
    }
    sharded_release(t->sx, t->set);
    delete ft;
    return rc;
}

void kaamer_sharded_full_ticket_discard(kaamer_sharded_full_ticket *ft)
{
    if (!ft) return;
    kaamer_sharded_ticket *t = &ft->t;
    sharded_sync_all(t->set);
    for (ShardState &st : t->set->sh) { if (st.ws) st.ws->clean = false; if (st.mws) st.mws->clean = false; }
    sharded_release(t->sx, t->set);
    delete ft;
}

int kaamer_sharded_search_batch(kaamer_sharded_index *sx, const kaamer_batch_in *in, kaamer_batch_out **out)
{
    if (out) *out = nullptr;
    if (!sx || !in || !out || !in->offsets || (in->n_seqs && !in->seqs)) return kaamer_fail(KAAMER_E_ARG, "sharded_search_batch: bad argument");
    kaamer_sharded_full_ticket *t = nullptr;
    const int rc = kaamer_sharded_submit_batch_flat(sx, in->seqs, in->offsets, in->n_seqs, in->seq_type, in->want_positions, &t);
    if (rc) return rc;
    return kaamer_sharded_wait_batch(t, out);
}

int kaamer_sharded_search_batch_flat(kaamer_sharded_index *sx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_seqs, int32_t seq_type,
                                     int32_t want_positions, kaamer_batch_out **out)
{
    if (out) *out = nullptr;
    kaamer_sharded_full_ticket *t = nullptr;
    const int rc = kaamer_sharded_submit_batch_flat(sx, seqs, offsets, n_seqs, seq_type, want_positions, &t);
    if (rc) return rc;
    return kaamer_sharded_wait_batch(t, out);
}

// bytes the last call's exchange moved between devices per owner and what its blocks carried (tests, bench):
// out = { wire bytes per (shard -> owner) block, entries the largest block needed, queries of the batch, 1 if adaptive }
int kaamer_sharded_exchange_info(kaamer_sharded_index *sx, uint64_t out[4])
{
    if (!sx || !out) return kaamer_fail(KAAMER_E_ARG, "sharded_exchange_info: bad argument");
    std::lock_guard<std::mutex> lock(sx->mu);
    const ShardSet &set = sx->sets[0];
    if (set.sh.empty() || !set.sh[0].ws) return kaamer_fail(KAAMER_E_ARG, "sharded_exchange_info: no call yet");
    out[0] = 4ull * set.sh[0].wire.block_words;
    out[1] = set.need_entries;
    out[2] = set.need_queries;
    out[3] = set.sh[0].wire.e_cap < set.sh[0].layout.e_cap ? 1u : 0u;
    return KAAMER_OK;
}
