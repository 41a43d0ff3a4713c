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
//
// This file: the handle and what a set of it holds, open and close, the protein table, the *_info and set_* calls.
// host_sharded_submit.hip.inc: a set made ready and the phases above enqueued (sharded_enqueue).
// host_sharded_collect.hip.inc: the attempt waited for, checked and interleaved (sharded_collect), the retry, discard.

// top calls with the PositionHits of the reported hits (top_positions_sharded.hip.inc): a shard's buffers
struct ShardTps {
    DevBuf<uint32_t> d_ids, d_ids_recv;                   // the owner's ids block; the W owners' blocks as pulled
    DevBuf<unsigned long long> d_seg_send, d_seg_recv;    // W segments each (one header word + the bitmap words)
    DevBuf<uint32_t> d_tps_words, d_tps_n;                // [rq_cap]; per owner {reported queries, status}
    DevBuf<uint64_t> d_tps_base;                          // [W][rq_cap + 1] word offsets per owner
};
// top calls that align the reported hits (top_align_sharded.hip.inc): a shard's buffers and what they hold
struct ShardSa {
    TasLayout sa_cap{};                                   // a (holder -> owner) subject segment: capacity
    DevBuf<uint8_t> d_sa_send, d_sa_recv, d_sa_codes;     // W segments each; the letter codes of the received ones
    DevBuf<uint32_t> d_sa_qbytes, d_sa_n;                 // [rq_cap + 1]; per owner {reported queries, status}
    DevBuf<uint64_t> d_sa_off;                            // owner: per pair, where its subject lies in d_sa_recv
    DevBuf<unsigned long long> d_sa_need;                 // holder: per owner {payload bytes needed, status}
};

struct ShardState : ShardTps, ShardSa {
    kaamer_index *ix = nullptr;
    int device = 0;
    kaamer_workspace *ws = nullptr, *mws = nullptr;
    kaamer_workspace_opts opts{};
    kaamer_exchange_layout layout{};   // capacity: what d_send / d_recv hold
    kaamer_exchange_layout wire{};     // the blocks of the batch in flight (<= capacity)
    uint64_t e_cap = 0;
    uint64_t p_cap = 0;                // bitmap words a block can hold (full calls with positions)
    bool full = false;                 // workspaces of a full call (kaamer_sharded_search_batch): first_pos = 1, CSR merge
    DevBuf<uint32_t> d_send, d_recv;
    hipStream_t stream = nullptr;
    hipEvent_t ev_packed = nullptr;
    DevBuf<uint8_t> d_seqs;
    DevBuf<uint64_t> d_off;
    DevBuf<uint8_t> d_block;
    uint8_t *h_block = nullptr;        // a block of the pinned cache (pinned_get)
    size_t h_block_cap = 0, guess = 1u << 16, copied = 0;
    // top calls with the PositionHits of the reported hits (ShardTps)
    bool tpos = false;                 // workspaces and buffers of such a call
    uint32_t tp_k = 0, tp_scale = 0;   // MaxResults and BatchBounds::pos_scale the capacities below were made for
    TpsIdsLayout ids_cap{}, ids_wire{};   // the ids block: capacity, and as it travels for the batch in flight
    uint64_t tp_cap = 0, tp_wire = 0;     // bitmap words of one (shard -> owner) segment: capacity, as it travels
    hipEvent_t ev_ids = nullptr, ev_bits = nullptr;   // the owner's ids block is packed; the shard's segments (bitmaps, subjects) are made
    // top calls that align the reported hits (ShardSa)
    TasLayout sa_wire{};               // a subject segment as it travels for the batch in flight (<= sa_cap)
    uint64_t aln_guess = 0;            // bytes the alignment sections of this owner's previous block needed, plus a quarter
    uint64_t sa_stage[3] = {0, 0, 0};  // the owner's last alignment stage: resident waves, slab bytes, long-subject waves
    hipEvent_t ev_t[5] = {};           // kaamer_sharded_index_set_align_timing: gather begin / end, assemble begin, alignment begin / end
    bool timed = false;                // ... recorded for the attempt in flight
};

// everything one call in flight needs on every shard (the indices themselves are shared by all sets)
struct ShardSet {
    std::vector<ShardState> sh;
    Buf<uint8_t, Mem::PINNED_PORTABLE> h_in;   // the caller's batch: every device copies from it
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
        DevBuf<uint8_t> d_raw;         // the stored bytes of the entries this device holds
        DevBuf<uint64_t> d_off;        // entries + 1
        DevBuf<uint32_t> d_idmap;      // id / W -> entry, TA_NONE: no entry
        DevBuf<int> d_matrix;
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

// (the shard's device is selected)
static void shard_tps_free(ShardState &s) { static_cast<ShardTps &>(s) = ShardTps(); }
static void shard_sa_free(ShardState &s) { static_cast<ShardSa &>(s) = ShardSa(); }

static void sharded_aln_free(kaamer_sharded_index *sx)
{
    if (!sx->aln) return;
    for (uint32_t s = 0; s < sx->n; s++) {
        (void)hipSetDevice((*sx->dev)[s]);
        (*sx->aln)[s] = kaamer_sharded_index::AlnPart();
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
    if (s.h_block) pinned_put(s.h_block, s.h_block_cap);
    if (s.ev_packed) (void)hipEventDestroy(s.ev_packed);
    if (s.ev_ids) (void)hipEventDestroy(s.ev_ids);
    if (s.ev_bits) (void)hipEventDestroy(s.ev_bits);
    for (hipEvent_t e : s.ev_t) if (e) (void)hipEventDestroy(e);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = ShardState();   // its buffers go here, on its device (the index belongs to the handle)
}

void kaamer_sharded_index_close(kaamer_sharded_index *sx)
{
    if (!sx) return;
    if (sx->sets) {
        for (int k = 0; k < KAAMER_SHARDED_SETS; k++) {
            for (ShardState &s : sx->sets[k].sh) shard_state_free(s);
        }
        delete[] sx->sets;   // (with each set's pinned staging)
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
        rc = reserve_group(nullptr, GROW_EXACT, { want(a.d_raw, raw.size()), want(a.d_off, off.size()), want(a.d_idmap, idmap.size()),
                                                  want(a.d_matrix, (size_t)ALN_NL * ALN_NL) });
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
