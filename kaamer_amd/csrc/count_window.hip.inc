// count_window.hip.inc — the steps that turn one window of 64 query positions into table adds (included by search.hip
// before count_group.hip.inc and count_pack.hip.inc; both LDS counting kernels call these, each from its own pipeline).
//
//   1. flat position -> (query, position in the query)        window_pos
//   2. the list head of a position                            issue_head, head_of
//   3. the ids beyond the first of every lane, flattened      flatten_begin / flatten_round / flatten_end, flatten_tail
//   4. runs of equal (query, id) in adjacent lanes, once      add_runs
//   5. the add into the query's LDS table                     table_probe, table_add_packed, table_add
//
// Every function is inlined into its kernel and takes the LDS arrays it touches as arguments: after inlining the
// compiler sees the __shared__ array behind each pointer and the accesses stay ds_* (a pointer that loses its address
// space on the way -- stored, selected, made volatile -- turns every access into a FLAT one).  None of them knows which
// kernel calls it; where callers differ, the difference is a template argument with a meaning of its own.

// inclusive scan of a wave with DPP row shifts (VALU, ~10 cycles a step) instead of six dependent
// ds_bpermute round trips (~100 cycles each); rows of 16 lanes, then row_bcast:15 / row_bcast:31
// carry the row totals (gfx9 DPP controls).
__device__ __forceinline__ uint32_t wave_inclusive_scan_dpp(uint32_t v)
{
#define KH_DPP_ADD(ctrl, rmask) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, 0xf, false)
    KH_DPP_ADD(0x111, 0xf);  // row_shr:1
    KH_DPP_ADD(0x112, 0xf);  // row_shr:2
    KH_DPP_ADD(0x114, 0xf);  // row_shr:4
    KH_DPP_ADD(0x118, 0xf);  // row_shr:8
    KH_DPP_ADD(0x142, 0xa);  // row_bcast:15 -> rows 1 and 3
    KH_DPP_ADD(0x143, 0xc);  // row_bcast:31 -> rows 2 and 3
#undef KH_DPP_ADD
    return v;
}

// inclusive max-scan over the wave, same DPP steps (0 is the identity: lanes without a source read 0)
__device__ __forceinline__ uint32_t wave_inclusive_max_dpp(uint32_t v)
{
#define KH_DPP_MAX(ctrl, rmask) { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, 0xf, false); v = v > t_ ? v : t_; }
    KH_DPP_MAX(0x111, 0xf);  // row_shr:1
    KH_DPP_MAX(0x112, 0xf);  // row_shr:2
    KH_DPP_MAX(0x114, 0xf);  // row_shr:4
    KH_DPP_MAX(0x118, 0xf);  // row_shr:8
    KH_DPP_MAX(0x142, 0xa);  // row_bcast:15 -> rows 1 and 3
    KH_DPP_MAX(0x143, 0xc);  // row_bcast:31 -> rows 2 and 3
#undef KH_DPP_MAX
    return v;
}

#define GRP_MAX_PROBES 96u   /* slots one table add may inspect before the query is handed to the G tier */

// ---- 1. the window's query -----------------------------------------------------------------------------------------
// largest j < nq with g_pref[j] <= i (g_pref: first flat position of every query; QMAX: a power of two >= nq)
template <uint32_t QMAX>
__device__ __forceinline__ uint32_t prefix_search(const uint32_t *g_pref, uint32_t nq, uint32_t i)
{
    uint32_t j = 0;
#pragma unroll
    for (uint32_t sft = QMAX / 2; sft > 0; sft >>= 1)
        if (j + sft < nq && g_pref[j + sft] <= i) j += sft;
    return j;
}

// flat position i of window w -> (query, position in the query); an idle lane (!valid) gets (0, 0).  The first n_hint
// windows know the query of their first position (wq): the lane's query is that one or shortly after it; later windows
// (a group made of one very long query) search the prefix.  LDS only.
struct WinPos { uint32_t j, ps; };
template <uint32_t QMAX>
__device__ __forceinline__ WinPos window_pos(uint32_t w, uint32_t i, bool valid, const uint8_t *wq, uint32_t n_hint, const uint32_t *g_pref, uint32_t nq)
{
    WinPos r;
    uint32_t j = 0;
    if (valid) {
        if (w < n_hint) {
            j = wq[w];
            while (j + 1 < nq && g_pref[j + 1] <= i) j++;
        } else {
            j = prefix_search<QMAX>(g_pref, nq, i);
        }
    }
    r.j = j;
    r.ps = valid ? i - g_pref[j] : 0u;
    return r;
}

// ---- 2. the list head ----------------------------------------------------------------------------------------------
// ISSUES the load of the list head {count, id0, id1, id2} of probe result v, unconditionally: v == 0 (key absent, idle
// lane) and a single inline id read word 0 -- the arena's first 16 bytes are zero: "no list"
__device__ __forceinline__ uint4 issue_head(const uint32_t *arena, uint32_t v)
{
    return reinterpret_cast<const uint4 *>(arena)[(v & KH_INLINE_BIT) ? 0u : v];
}

// the head as the counting sees it: the inline id folded in by arithmetic on the raw load (a select would let the
// compiler sink the load into a branch again)
__device__ __forceinline__ uint4 head_of(uint32_t v, const uint4 &hv)
{
    const uint32_t inl = (v & KH_INLINE_BIT) ? 0xFFFFFFFFu : 0u;
    return make_uint4(hv.x | (inl & 1u), hv.y | (inl & v & ~KH_INLINE_BIT), hv.z, hv.w);
}

// what the lane's list asks of the counting: its first id (KH_EMPTY_PID: none) and how many ids follow it.  A postings
// list longer than the query's table can never fit it: the query goes to the G tier at once (expanding the list first,
// 64 ids at a time, only to find the table full was 60 us per window), and a query already on its way there is only
// counted, not expanded.
struct LaneList { uint32_t first_id, extra; };
template <class TabT, class OvfT>
__device__ __forceinline__ LaneList lane_list(const uint4 &h, uint32_t j, const TabT *g_cap, OvfT *g_ovf)
{
    const uint32_t lcnt = h.x;
    if (lcnt > g_cap[j] && lcnt != 0u) g_ovf[j] = 1u;
    const bool dead = lcnt != 0u && g_ovf[j] != 0u;
    LaneList r;
    r.first_id = (lcnt > 0 && !dead) ? h.y : KH_EMPTY_PID;
    r.extra = (lcnt > 1u && !dead) ? lcnt - 1u : 0u;
    return r;
}

// work counters of a wave (lane-private partial sums): postings, lists read from the arena, their ids
struct WorkCount {
    uint32_t post = 0, lists = 0, lids = 0;
    __device__ __forceinline__ void list(uint32_t v, uint32_t lcnt)
    {
        if (lcnt != 0u) {
            post += lcnt;
            if (!(v & KH_INLINE_BIT)) { lists++; lids += lcnt; }
        }
    }
};

// ---- 5. the table add ----------------------------------------------------------------------------------------------
// home slot of id pid in a table of cap slots (any capacity: no power of two needed)
__device__ __forceinline__ uint32_t table_home(uint32_t pid, uint32_t cap)
{
    return (uint32_t)(((uint64_t)(pid * 0x9E3779B1u) * cap) >> 32);
}

// Finds or claims the slot of id pid in table j (slots [g_tab[j], g_tab[j] + g_cap[j]) of the arena) and calls
// hit(slot); a table with no slot left within GRP_MAX_PROBES sets g_ovf[j]: the query goes to the G tier.  A table that
// crowded is as good as full, and walking all of a full 4096-slot table for every further id of the query (a query that
// meets a postings list of thousands of proteins) cost 170 us per add -- 0.4 s per batch on a skewed database.
template <class TabT, class OvfT, class Hit>
__device__ __forceinline__ void table_probe(uint32_t *a_keys, const TabT *g_tab, const TabT *g_cap, OvfT *g_ovf, uint32_t j, uint32_t pid, Hit hit)
{
    const uint32_t base = g_tab[j], cap = g_cap[j];
    uint32_t hh = table_home(pid, cap);
    const uint32_t tmax = cap < GRP_MAX_PROBES ? cap : GRP_MAX_PROBES;
    for (uint32_t t = 0; t < tmax; t++) {
        // ONE LDS round trip per slot inspected: the compare-and-swap is issued whatever the slot holds (it returns
        // the occupant of a taken slot).  Reading first and swapping only an empty slot is two dependent round trips
        // whenever any lane of the wave meets an empty slot -- nearly every iteration.
        const uint32_t old = atomicCAS(&a_keys[base + hh], KH_EMPTY_PID, pid);
        const uint32_t kk = old == KH_EMPTY_PID ? pid : old;
        if (kk == pid) {
            hit(base + hh);
            return;
        }
        hh = (hh + 1u == cap) ? 0u : hh + 1u;
    }
    g_ovf[j] = 1;
}

// packed: count (low 16 bits) += n and lowest position (high 16 bits) = min(., pos) share one word of a_cnt.  The
// position is lowered rarely (windows are taken in order): a CAS loop, started from a fresh read of the word -- starting
// it from the add's own return value (a returning LDS atomic) measured 2-4 % slower in both kernels
// (profiles/r12_count_window.md).
template <class TabT, class OvfT>
__device__ __forceinline__ void table_add_packed(uint32_t *a_keys, uint32_t *a_cnt, const TabT *g_tab, const TabT *g_cap, OvfT *g_ovf,
                                                 uint32_t j, uint32_t pid, uint32_t pos, uint32_t n)
{
    table_probe(a_keys, g_tab, g_cap, g_ovf, j, pid, [&](uint32_t slot) {
        atomicAdd(&a_cnt[slot], n);
        uint32_t old = __hip_atomic_load(&a_cnt[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        while (pos < (old >> 16)) {
            const uint32_t seen = atomicCAS(&a_cnt[slot], old, (old & 0xFFFFu) | (pos << 16));
            if (seen == old) break;
            old = seen;
        }
    });
}

// unpacked: a_cnt += n; MINPOS: a_min = min(a_min, pos), a table of its own
template <bool MINPOS, class TabT, class OvfT>
__device__ __forceinline__ void table_add(uint32_t *a_keys, uint32_t *a_cnt, uint32_t *a_min, const TabT *g_tab, const TabT *g_cap, OvfT *g_ovf,
                                          uint32_t j, uint32_t pid, uint32_t pos, uint32_t n)
{
    table_probe(a_keys, g_tab, g_cap, g_ovf, j, pid, [&](uint32_t slot) {
        atomicAdd(&a_cnt[slot], n);
        if (MINPOS) atomicMin(&a_min[slot], pos);
    });
}

// ---- 4. the run add ------------------------------------------------------------------------------------------------
// runs of equal (query, id) in adjacent lanes are added once, with their length: add(j, x, pos, len) by the run's first lane
template <class Add>
__device__ __forceinline__ void add_runs(uint32_t lane, uint32_t j, uint32_t x, uint32_t pos, Add add)
{
    const uint32_t px = __shfl_up(x, 1, 64), pj = __shfl_up(j, 1, 64);
    const bool change = (lane == 0) || px != x || pj != j;
    const unsigned long long cm = __ballot(change);
    if (change && x != KH_EMPTY_PID) {
        const unsigned long long above = (lane == 63) ? 0ull : (cm >> (lane + 1));
        const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : 64u - lane;
        add(j, x, pos, len);
    }
}

// ---- 3. the flatten ------------------------------------------------------------------------------------------------
// The first id of every lane is added directly.  All further ids of the window (about as many again, held by a minority
// of the lanes) are FLATTENED over the wave: item t belongs to the lane whose exclusive prefix of `extra` is the highest
// at or before t, so the adds run with dense lanes instead of once per list slot with a few lanes each.  Ids 1 and 2 of
// a list come with its head, the rest are loaded from the arena.
//
// what the flatten reads of every lane of the window: probe result (the list's offset in the arena), ids 1 and 2 of its
// head, query and position
struct XWin { uint32_t v, z, w, j, ps; };
// the same of lane lo, in every lane (executed by all lanes: the owner may be a lane that is idle in this round)
__device__ __forceinline__ XWin xwin_of(const XWin &x, uint32_t lo)
{
    XWin o;
    o.v = __shfl(x.v, (int)lo, 64);
    o.z = __shfl(x.z, (int)lo, 64); o.w = __shfl(x.w, (int)lo, 64);
    o.j = __shfl(x.j, (int)lo, 64);
    o.ps = __shfl(x.ps, (int)lo, 64);
    return o;
}
// the owner of item t < xtotal: the last lane whose prefix is <= t (lanes without further ids share their successor's)
__device__ __forceinline__ uint32_t flatten_owner(const uint32_t *pref, uint32_t t)
{
    uint32_t lo = 0;
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1)
        if (pref[lo + sft] <= t) lo += sft;
    return lo;
}

// begin: pref[lane] = exclusive prefix of extra; -> the window's number of further ids.  Every owner marks its FIRST item
// (of the first XIT * 64) with its lane number + 1 -- an item's owner is the highest mark at or before it (owners ascend
// with the items): one LDS store per owner and a max-scan per 64 items instead of a store per item in a divergent loop as
// long as the longest list of the window.  own[] is clean on entry and left clean by the rounds.
template <int XIT>
__device__ __forceinline__ uint32_t flatten_begin(uint32_t lane, uint32_t extra, uint32_t *pref, uint8_t *own)
{
    const uint32_t inc = wave_inclusive_scan_dpp(extra);
    const uint32_t xtotal = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    pref[lane] = inc - extra;
    if (extra != 0u && inc - extra < XIT * 64u) own[inc - extra] = (uint8_t)(lane + 1u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return xtotal;
}

// one round: items [64 it, 64 it + 64).  The id of the lane's item is (ld & m) | (id & ~m) -- xround_id -- arithmetic on
// the raw arena load ld, so that a caller may carry ld to a later pipeline stage before it waits for it.  (Scalars, not
// arrays indexed by the round: a select between two array elements became a scratch access by address.)
// ALWAYS_LOAD: the arena load is issued unconditionally (lanes without an id there read word 0) and the compiler's
// s_waitcnt vmcnt(N) counts exactly; without it the load sits in a branch and the round waits for it there.
struct XRound { uint32_t id = KH_EMPTY_PID, ld = 0, j = 0, ps = 0, m = 0; };
__device__ __forceinline__ uint32_t xround_id(const XRound &r) { return (r.ld & r.m) | (r.id & ~r.m); }
template <bool ALWAYS_LOAD>
__device__ __forceinline__ XRound flatten_round(uint32_t lane, uint32_t it, uint32_t xtotal, uint32_t &carry, const XWin &x,
                                                const uint32_t *pref, uint8_t *own, const uint32_t *arena)
{
    XRound r;
    const uint32_t t = it * 64u + lane;
    const bool act = t < xtotal;
    uint32_t mk = own[t];
    own[t] = 0;  // the marks are left clean for the next window
    mk = wave_inclusive_max_dpp(mk > carry ? mk : carry);
    carry = (uint32_t)__builtin_amdgcn_readlane((int)mk, 63);
    const uint32_t lo = act ? mk - 1u : 0u;
    const XWin o = xwin_of(x, lo);
    r.j = o.j;
    r.ps = o.ps;
    const uint32_t k = act ? t - pref[lo] : 0u;  // item k of the owner = id k+1 of its list
    const bool from_arena = act && k >= 2u;
    r.m = from_arena ? 0xFFFFFFFFu : 0u;
    if (ALWAYS_LOAD) r.ld = arena[from_arena ? (uint64_t)o.v * 4 + 2 + k : 0ull];
    else if (from_arena) r.ld = arena[(uint64_t)o.v * 4 + 2 + k];
    r.id = !act ? KH_EMPTY_PID : k == 0u ? o.z : o.w;
    return r;
}

// very many ids in one window: items [from, xtotal), 64 at a time, each chunk searched, loaded and added at once:
// add(j, id, pos).  (A table that has just filled up is not walked again for every further id.)
template <class OvfT, class Add>
__device__ __forceinline__ void flatten_tail(uint32_t lane, uint32_t from, uint32_t xtotal, const XWin &x, const uint32_t *pref,
                                             const OvfT *g_ovf, const uint32_t *arena, Add add)
{
    for (uint32_t t0 = from; t0 < xtotal; t0 += 64) {
        const uint32_t t = t0 + lane;
        const bool act = t < xtotal;
        const uint32_t lo = act ? flatten_owner(pref, t) : 0u;
        const XWin o = xwin_of(x, lo);
        if (act && !g_ovf[o.j]) {
            const uint32_t k = t - pref[lo];
            add(o.j, k == 0u ? o.z : k == 1u ? o.w : arena[(uint64_t)o.v * 4 + 2 + k], o.ps);
        }
    }
}

// end: pref is rewritten by the next window's begin
__device__ __forceinline__ void flatten_end()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
