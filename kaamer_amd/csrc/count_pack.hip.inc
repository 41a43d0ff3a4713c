// count_pack.hip.inc — the counting kernel of an ORF batch (included by search.hip after count_group.hip.inc).
//
// Replaces, for a whole batch, the per-id loop of KmerSearch (search.go:431-436): Counter[id]++ (and the lowest
// matching position, what SetBestStartCodon reads from PositionHits) for every id of every found k-mer.
//
// Why not the group kernel (count_group.hip.inc: protein batches, the PositionHits pass and the merge of a sharded
// index): with eight waves sharing a group of tables every group costs four workgroup barriers, a ticket on one
// global word, and a software pipeline that never fills (2-3 windows per wave); 78 % of its wave cycles were waits
// (profiles/r02_sq_protein.txt) and the skeleton alone -- no counting at all -- took 53 of its 97 us.
//
// Here a workgroup is ONE wave and owns everything it touches: a PACK of consecutive queries (the tables that
// start in one window of `budget` slots of the table layout E), an arena of PK_ARENA table slots in LDS, its own
// scratch.  No workgroup barrier.  Packs are handed out by ticket, but not from one word (one L2 word serialises at
// ~90 atomics/us): the packs are cut into PK_TICKETS contiguous ranges with a counter each, a wave draws from the
// counter blockIdx.x mod PK_TICKETS, and the ticket is taken two packs ahead of its use.  (Dealing the packs out
// statically, longest first and boustrophedon, left the average wave idle for half of the kernel: a pack's cost is
// its postings, not its table size, and 3.5 packs per wave do not average out.)  The descriptors of the next pack are
// fetched while this one is counted, and inside a pack the windows run through a four-stage pipeline (probe results
// -> list heads -> further ids -> table adds) in which every load was issued an iteration before it is waited for.
// A table larger than the arena allows (PK_ARENA - budget + 64 slots) is counted in that many slots all the same: a
// table is sized for the worst case (1.5 slots per position) and a query has ~0.5 distinct hits per position, so it
// nearly always fits; if it does not, the query goes to the G tier like any query whose table fills up.
// PK_ARENA (template parameter): table slots per wave.  640 (5 KB of keys + counts, 24 waves per CU) for ORFs of reads,
// whose tables are 64-128 slots; 1024 for longer ORFs (search.hip: PK_ARENA_ORF_LONG).  Counts and lowest positions
// are always kept: the ORFs of nucleotide input carry PositionHits in the reference (search.go:416).
// The steps of a window (its query, the list head, the flatten, the run add, the packed table add) are
// count_window.hip.inc's, shared with the group kernel; the four-stage pipeline that runs them is this kernel's own.
#define PK_QMAX 32u      /* queries of a pack: budget / 64 at most */
#define PK_WHINT 64u     /* windows with a start hint (the rest search the prefix) */
#define PK_TICKETS 64u   /* ticket counters (ranges of packs) */

template <uint32_t PK_ARENA>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void count_pack_kernel(CountParams p)
{
    constexpr int XIT = 2;
    __shared__ uint32_t a_keys[PK_ARENA];
    __shared__ uint32_t a_cnt[PK_ARENA];  // count (low 16 bits) and lowest position (high 16 bits) share one word
    __shared__ uint32_t g_q[PK_QMAX], g_size[PK_QMAX], g_tab[PK_QMAX], g_cap[PK_QMAX], g_ovf[PK_QMAX], g_eoff[PK_QMAX];
    __shared__ uint32_t g_pref[PK_QMAX + 1];
    __shared__ uint64_t g_aa[PK_QMAX];
    __shared__ uint32_t pref[64];
    __shared__ uint8_t own[XIT * 64];
    __shared__ uint8_t s_wq[PK_WHINT];

    const uint32_t lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t n_groups = *p.d_n_groups;
    const uint32_t nq_total = *p.d_nq;
    const uint32_t bshift = p.pack_shift;                       // budget = 1 << bshift slots
    const uint32_t max_table = PK_ARENA - (1u << bshift) + 64u; // a table that starts in the last 64 slots of the window still fits
    for (uint32_t i = lane; i < XIT * 64; i += 64) own[i] = 0;  // owner marks: clean between windows

    // ---- packs by ticket: range c = blockIdx.x mod PK_TICKETS of the packs, its own counter
    const uint32_t n_packs = n_groups;
    const uint32_t chunk = (n_packs + PK_TICKETS - 1u) / PK_TICKETS;
    const uint32_t tc = blockIdx.x % PK_TICKETS;
    const uint32_t r_begin = tc * chunk, r_end = (r_begin + chunk < n_packs) ? r_begin + chunk : n_packs;
    uint32_t *const tcount = p.pack_tickets + tc;
    auto take = [&]() { uint32_t t = 0; if (lane == 0) t = atomicAdd(tcount, 1u); return t; };  // the value lands in lane 0
    auto pack_entry = [&](uint32_t traw) {  // ticket -> (pack, its first query); past the end of the range: no pack
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)traw);
        const uint32_t g = r_begin + t;
        if (t >= chunk || g >= r_end) return make_uint2(0xFFFFFFFFu, GRP_NONE);
        return make_uint2(g, p.group_first[g]);
    };
    auto fetch_desc = [&](uint32_t first, QInfo &qi, uint64_t &e) {
        qi.size = 0; qi.slots = 0; qi.aa_off = 0; e = 0;
        if (first != GRP_NONE && (uint64_t)first + lane < nq_total) { qi = p.qinfo[first + lane]; e = p.slot_off[first + lane]; }
    };
    uint32_t tk_a = take(), tk_b = take();
    uint2 e_cur = pack_entry(tk_a);
    uint2 e_nxt = pack_entry(tk_b);
    uint32_t tk_c = take();  // in flight: the pack after e_nxt
    QInfo pre_qi;
    uint64_t pre_e;
    fetch_desc(e_cur.y, pre_qi, pre_e);

    // work counters of this wave (lane-private partial sums; totals at the end)
    WorkCount work;
    uint32_t c_hits = 0, c_q = 0, c_ovf = 0, c_big = 0;
    unsigned long long c_in = 0;

    while (e_cur.x != 0xFFFFFFFFu) {  // (tickets of one counter ascend: after the first one past the range, all are)
        const uint32_t gid = e_cur.x, first = e_cur.y;
        // the pack after next: its ticket was taken an iteration ago, its entry is in flight while this pack is counted
        const uint2 e_nn = pack_entry(tk_c);
        tk_c = take();
        if (first == GRP_NONE) {  // no table starts in this window of the layout (identity schedule only)
            e_cur = e_nxt; e_nxt = e_nn;
            fetch_desc(e_cur.y, pre_qi, pre_e);
            continue;
        }
        // ---- 1. the pack's queries
        const uint64_t e_first = __shfl(pre_e, 0, 64);
        uint32_t nq = 0, tab_run = 0;
        {
            uint64_t q0 = first;
            bool done = false;
            while (!done) {
                const uint64_t q = q0 + lane;
                const bool in_range = q < nq_total;
                QInfo qi;
                qi.size = 0; qi.slots = 0; qi.aa_off = 0;
                uint64_t e = 0;
                if (q0 == first) { qi = pre_qi; e = pre_e; }
                else if (in_range) { qi = p.qinfo[q]; e = p.slot_off[q]; }
                const bool searched = in_range && qi.slots != 0;
                const bool beyond = !in_range || (searched && (e >> bshift) > gid);
                const unsigned long long bm = __ballot(beyond);
                const uint32_t cutoff = bm ? (uint32_t)__ffsll((long long)bm) - 1 : 64u;
                const bool here = searched && lane < cutoff;
                // a table larger than the arena allows: the G tier counts that query (a workgroup-wide LDS table).
                // (Counting it here in fewer slots was tried: at 0.9 slots per distinct hit the probe sequences of the
                // few large queries made the whole kernel three times slower.)
                const bool big = here && qi.slots > max_table;
                if (big) {
                    const uint32_t slot = atomicAdd(p.ovf_count, 1u);
                    WorkItem wi;
                    wi.q = (uint32_t)q; wi.size = -qi.size; wi.aa_off = qi.aa_off;  // negative: nothing of this query has been counted yet
                    if (slot < p.list_cap) p.ovf_list[slot] = wi;
                    else atomicOr(p.status, (uint32_t)ST_LIST_FULL);
                    c_q++; c_big++; c_in += (unsigned long long)(uint32_t)qi.size + 6ull;
                }
                const bool mine = here && !big;
                const unsigned long long mm = __ballot(mine);
                // tables are placed one after the other in the wave's arena
                const uint32_t capu = mine ? qi.slots : 0u;
                const uint32_t cinc = wave_inclusive_scan_dpp(capu);
                if (mine) {
                    const uint32_t idx = nq + (uint32_t)__popcll(mm & below);
                    if (idx < PK_QMAX) {
                        g_q[idx] = (uint32_t)q;
                        g_size[idx] = (uint32_t)qi.size;
                        g_aa[idx] = qi.aa_off;
                        g_eoff[idx] = (uint32_t)(e - e_first);
                        g_tab[idx] = tab_run + cinc - capu;
                        g_cap[idx] = capu;
                        g_ovf[idx] = qi.size >= 65535 ? 1u : 0u;  // 16-bit counts and positions
                    }
                }
                tab_run += (uint32_t)__builtin_amdgcn_readlane((int)cinc, 63);
                nq += (uint32_t)__popcll(mm);
                done = bm != 0;
                q0 += 64;
            }
            if (nq > PK_QMAX) nq = PK_QMAX;  // cannot happen: >= 64 slots per searched query, budget <= 64 * PK_QMAX
        }
        // the next pack's descriptors: issued now, used at the top of the next iteration
        fetch_desc(e_nxt.y, pre_qi, pre_e);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t n_posn, n_slots;
        {
            const uint32_t sz = lane < nq ? g_size[lane] : 0u;
            const uint32_t inc = wave_inclusive_scan_dpp(sz);
            if (lane < nq) g_pref[lane] = inc - sz;
            n_posn = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            if (lane == 0) g_pref[nq] = n_posn;
            n_slots = tab_run;
            if (n_slots > PK_ARENA) n_slots = PK_ARENA;  // cannot happen (max_table)
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t n_win = (n_posn + 63u) >> 6;
        if (lane < PK_WHINT && (lane << 6) < n_posn) {  // the query that holds position 64 w, for the first windows
            s_wq[lane] = (uint8_t)prefix_search<PK_QMAX>(g_pref, nq, lane << 6);
        }
        // ---- 2. clear the tables in use
        for (uint32_t i = lane; i < n_slots; i += 64) {
            a_keys[i] = KH_EMPTY_PID;
            a_cnt[i] = 0xFFFF0000u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // ---- 3. count.  Window w = flat positions [64 w, 64 w + 64) of the pack's queries laid end to end.
        // Every global load of the window loop is issued UNCONDITIONALLY (idle lanes read word 0 of their array; the
        // arena's first 16 bytes are zero: "no list") and its result is consumed an ITERATION LATER, as a raw loop-carried
        // register: the compiler's s_waitcnt vmcnt(N) then counts exactly and a stage waits only for the load it needs.
        // One load inside a branch, or one select on a load's result in the iteration that issued it, makes every wait of
        // the loop a vmcnt(0) -- three exposed round trips per window (measured: 185 us for a 10 000-query batch).
        auto is_valid = [&](uint32_t w) { return ((w << 6) + lane) < n_posn; };
        struct WinA { uint32_t vraw, j, ps; };
        auto stage_a = [&](uint32_t w) {  // flat position -> (query, position in the query); ISSUES the load of its probe result
            WinA r;
            const uint32_t i = (w << 6) + lane;
            const bool valid = i < n_posn;
            const WinPos wp = window_pos<PK_QMAX>(w, i, valid, s_wq, PK_WHINT, g_pref, nq);
            r.j = wp.j;
            r.ps = wp.ps;
            r.vraw = p.vals[valid ? g_aa[wp.j] + wp.ps : 0ull];
            return r;
        };
        // stage B ISSUES the load of the list head (issue_head); stage C reads it (head_of)
        auto add_n = [&](uint32_t j, uint32_t pid, uint32_t pos, uint32_t n) { table_add_packed(a_keys, a_cnt, g_tab, g_cap, g_ovf, j, pid, pos, n); };
        auto add_one = [&](uint32_t j, uint32_t pid, uint32_t pos) { add_n(j, pid, pos, 1u); };
        // stage C: the ids beyond the first of every lane are flattened over the lanes; the arena loads of the rounds are
        // ISSUED here and read by stage D an iteration later (XRound.ld: raw)
        struct WinX { XRound r0, r1; uint32_t first_id; };
        static_assert(XIT == 2, "two flattened rounds per window are written out");
        auto stage_c = [&](uint32_t v, uint32_t wj, uint32_t wps, const uint4 &h) {
            WinX x;
            const LaneList ll = lane_list(h, wj, g_cap, g_ovf);
            x.first_id = ll.first_id;
            work.list(v, h.x);
            const XWin xw = {v, h.z, h.w, wj, wps};
            const uint32_t xtotal = flatten_begin<XIT>(lane, ll.extra, pref, own);
            uint32_t carry = 0;
            x.r0 = flatten_round<true>(lane, 0u, xtotal, carry, xw, pref, own, p.arena);
            x.r1 = flatten_round<true>(lane, 1u, xtotal, carry, xw, pref, own, p.arena);
            flatten_tail(lane, XIT * 64u, xtotal, xw, pref, g_ovf, p.arena, add_one);  // (rare)
            flatten_end();
            return x;
        };
        auto stage_d = [&](uint32_t wj, uint32_t wps, const WinX &x) {  // the table adds of one window
            add_runs(lane, wj, x.first_id, wps, add_n);
            const uint32_t id0 = xround_id(x.r0);
            if (id0 != KH_EMPTY_PID) add_one(x.r0.j, id0, x.r0.ps);
            const uint32_t id1 = xround_id(x.r1);
            if (id1 != KH_EMPTY_PID) add_one(x.r1.j, id1, x.r1.ps);
        };
        {
            // iteration w: A(w+3) issued; B(w+2) issued on A(w+2)'s result; C(w+1) on B(w+1)'s; D(w) on C(w)'s -- every
            // load is read one iteration after it was issued
            WinA a1 = stage_a(0), a2 = stage_a(1), a3 = stage_a(2);
            uint32_t v1 = is_valid(0) ? a1.vraw : 0u;
            uint4 hv1 = issue_head(p.arena, v1);
            uint32_t v2 = is_valid(1) ? a2.vraw : 0u;
            uint4 hv2 = issue_head(p.arena, v2);
            uint32_t j0 = a1.j, ps0 = a1.ps;
            WinX x0 = stage_c(v1, a1.j, a1.ps, head_of(v1, hv1));
            // from here on: window w is (j0, ps0, x0); w+1 is (v2, a2, hv2); w+2 is a3 (raw)
            for (uint32_t w = 0; w < n_win; w++) {
                const WinA a4 = stage_a(w + 3);
                const uint32_t v3 = is_valid(w + 2) ? a3.vraw : 0u;
                const uint4 hv3 = issue_head(p.arena, v3);
                const WinX x1 = stage_c(v2, a2.j, a2.ps, head_of(v2, hv2));
                stage_d(j0, ps0, x0);
                j0 = a2.j; ps0 = a2.ps; x0 = x1;
                a2 = a3; v2 = v3; hv2 = hv3;
                a3 = a4;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // ---- 4. every table is packed into its query's hit list at E[q] (a table never holds more distinct ids than
        // its capacity: nothing is allocated, nothing counted first)
        for (uint32_t j = 0; j < nq; j++) {
            const uint32_t q = g_q[j], base_slot = g_tab[j], cap = g_cap[j];
            c_q += lane == 0 ? 1u : 0u;
            c_in += lane == 0 ? (unsigned long long)g_size[j] + 6ull : 0ull;
            if (g_ovf[j]) {
                if (lane == 0) {
                    c_ovf++;
                    const uint32_t slot = atomicAdd(p.ovf_count, 1u);
                    WorkItem wi;
                    wi.q = q; wi.size = (int32_t)g_size[j]; wi.aa_off = g_aa[j];
                    if (slot < p.list_cap) p.ovf_list[slot] = wi;
                    else atomicOr(p.status, (uint32_t)ST_LIST_FULL);
                    p.q_cnt[q] = 0;
                    p.hit_off[q] = 0;
                }
                continue;
            }
            const unsigned long long base = e_first + g_eoff[j];  // = E[q]: the list's place in the hit arrays
            const bool have = base + cap <= p.hit_cap;
            if (!have && lane == 0) atomicOr(p.status, (uint32_t)ST_POOL_FULL);
            uint32_t running = 0;
            if (have) {
                for (uint32_t i0 = 0; i0 < cap; i0 += 64) {
                    const uint32_t k = a_keys[base_slot + i0 + lane];
                    const bool has = k != KH_EMPTY_PID;
                    const unsigned long long bm = __ballot(has);
                    if (has) {
                        const uint32_t idx = running + (uint32_t)__popcll(bm & below);
                        p.hit_pid[base + idx] = k;
                        const uint32_t cw = a_cnt[base_slot + i0 + lane];
                        p.hit_km[base + idx] = cw & 0xFFFFu;
                        p.hit_fp[base + idx] = cw >> 16;
                    }
                    running += (uint32_t)__popcll(bm);
                }
            }
            if (lane == 0) { p.q_cnt[q] = running; p.hit_off[q] = have ? base : 0; c_hits += running; }
        }
        e_cur = e_nxt; e_nxt = e_nn;
    }
    // ---- totals of the wave -> the batch's counters (one replica per wave index)
    {
        const uint32_t a = wave_total(work.post), b = wave_total(work.lists), c = wave_total(work.lids), d = wave_total(c_q), big = wave_total(c_big);
        unsigned long long in = c_in;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) in += __shfl_xor(in, o, 64);
        if (lane == 0) {
            const uint32_t rep = blockIdx.x;
            add_counter(p.counters, rep, CTR_IN, in);
            add_counter(p.counters, rep, CTR_QUERIES, d);
            add_counter(p.counters, rep, CTR_POST, a);
            add_counter(p.counters, rep, CTR_HITS, c_hits);
            add_counter(p.counters, rep, CTR_OVERFLOW, c_ovf + big);
            add_counter(p.counters, rep, CTR_LISTS, b);
            add_counter(p.counters, rep, CTR_LIST_IDS, c);
        }
    }
}
