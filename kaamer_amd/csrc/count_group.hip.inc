// count_group.hip.inc — the counting kernel (included by search.hip).
//
// Replaces, for a whole batch, the per-id loop of KmerSearch (search.go:431-436):
// Counter[id]++ and PositionHits[id][pos] for every id of every found k-mer.
//
// Per-query costs (descriptor fetch, table clear, compaction, pool allocation) dominated
// a one-wave-per-query design, so queries are packed into GROUPS: prep gives every query
// an LDS table capacity (1.5 x SizeInKmer rounded up to 64 slots, 64..4096), an exclusive
// scan of the capacities lays the tables out, and group g owns the queries whose table
// starts in [g*GRP_BUDGET, (g+1)*GRP_BUDGET) slots.  One 8-wave workgroup takes one group:
// its positions are processed FLAT (lane <-> position of the concatenated queries, the
// owning query found by binary search in LDS), so every lane is busy whatever the query
// lengths are, all memory round trips of a group overlap, and one compaction pass serves
// up to 32 queries.  Counts are exact integers; a table that fills up sends its query to
// the G tier (count_global_kernel), never a partial result.
// The steps that turn one window of 64 positions into table adds (the window's query, the list head, the flatten, the run
// add, the table add) are count_window.hip.inc's, shared with the ORF kernel (count_pack.hip.inc); what is here is the
// group's own: layout, schedule, descriptors, the window pipelines of the three modes, compaction.

#ifndef GRP_WAVES
#define GRP_WAVES 8
#endif
#ifndef GRP_BUDGET
#define GRP_BUDGET 2048u     /* slots of tables that may START in one group */
#endif
#define GRP_SHIFT 11u         /* log2(GRP_BUDGET): the layout kernels take the window as a shift */
static_assert((1u << GRP_SHIFT) == GRP_BUDGET, "GRP_BUDGET must be 1 << GRP_SHIFT");
#define GRP_MAX_TABLE 4096u  /* largest single table */
#define GRP_MIN_TABLE 64u
#define GRP_ARENA (GRP_BUDGET + GRP_MAX_TABLE)
#define GRP_QMAX (GRP_BUDGET / GRP_MIN_TABLE)
// count_group_kernel takes the window of a group from its parameters: GRP_SHIFT, or GRP_SHIFT + 1 -- a UNIT of two windows,
// counted in one barrier cycle when its tables fit the arena (nearly always: the arena is sized for the worst overhang of
// one window) and in two when they do not.  Twice the windows per cycle: the fixed part of a cycle (descriptors,
// barriers, the first two loads, packing: half of a group's time) is paid once, and the waves' unequal shares even out.
// slots of the arena a cycle can use: tables start at multiples of 64 within a window, none is larger than GRP_MAX_TABLE
#define GRP_FIT (GRP_BUDGET - 64u + GRP_MAX_TABLE)
#define GRP_NONE 0xFFFFFFFFu
#ifndef GRP_LONG_UNROLL
#define GRP_LONG_UNROLL 4u  /* chunks of 64 ids per round of the long-list path (registers: the kernel must stay at <= 80) */
#endif

// what prep leaves per query for the counting kernel (one 16-byte load)
struct alignas(16) QInfo {
    int32_t size;     // SizeInKmer; <= 0: not searched
    uint32_t slots;   // LDS table capacity (0: not searched)
    uint64_t aa_off;  // first residue position
};

// scale_q4 (sixteenths, >= 16): how many distinct proteins a k-mer of the previous batch hit on average, with a margin
// (finalize_body).  1 on a database like DB-SP; on a database where most k-mers meet several proteins by chance
// (DB-UR-lite: 2.2 per k-mer on one device) a table of 1.5 x SizeInKmer slots overflows for a third of the ORFs.
#define SLOT_SCALE_ONE 16u
#ifndef TABLE_FACTOR_Q4
#define TABLE_FACTOR_Q4 24u   /* 1.5 slots per k-mer, in sixteenths */
#endif
__device__ __forceinline__ uint32_t table_slots_for(int32_t size, uint32_t scale_q4 = SLOT_SCALE_ONE)
{
    if (size <= 0) return 0u;
    // 1.5 x SizeInKmer (x scale), a multiple of 64 (the compaction walks 64-slot stripes); the slot of an
    // id is (hash * capacity) >> 32, so the capacity need not be a power of two
    uint64_t want = ((((uint64_t)(uint32_t)size * TABLE_FACTOR_Q4) >> 4) * scale_q4) >> 4;
    want = (want + 63) & ~63ull;
    if (want < GRP_MIN_TABLE) want = GRP_MIN_TABLE;
    if (want > GRP_MAX_TABLE) want = GRP_MAX_TABLE;
    return (uint32_t)want;
}

// The scale this batch's tables get: what the previous batch asked for, but never more than THIS batch's positions
// leave room for in the hit arrays (tables <= 1.5 x scale x positions, + up to 128 per query of rounding and minimum
// size).  The workspace is provisioned for its largest batch at scale 1; a batch below that size -- ORFs are 40 % of
// the 2 amino acids per nucleotide the arrays are sized for -- leaves the rest to larger tables.
__device__ __forceinline__ uint32_t fit_table_scale(uint32_t want_q4, unsigned long long n_pos, uint32_t nq, unsigned long long room_slots)
{
    if (want_q4 <= SLOT_SCALE_ONE) return SLOT_SCALE_ONE;   // (the usual case costs no division)
    const unsigned long long fixed = 128ull * nq;
    if (room_slots <= fixed) return SLOT_SCALE_ONE;
    const unsigned long long fit = (room_slots - fixed) * 256ull / ((unsigned long long)TABLE_FACTOR_Q4 * (n_pos ? n_pos : 1ull));
    if (fit <= SLOT_SCALE_ONE) return SLOT_SCALE_ONE;
    return want_q4 < fit ? want_q4 : (uint32_t)fit;
}

// ---- table layout: exclusive scan E of the table capacities + first query of every group,
// in ONE pass (tiles chained by decoupled look-back; tile work is uniform, so the chain is short).
// Group g owns the tables that START in [g*BUDGET, (g+1)*BUDGET).  Tables tile [0, total) without
// gaps, so for every boundary g*BUDGET <= total exactly one searched query q has
// E[q] < g*BUDGET <= E[q] + slots[q]: the table after it starts at E[q+1], in group
// floor(E[q+1] / BUDGET); groups strictly between have no start.  That query writes those
// entries, so every group_first[g], g < n_groups, is written exactly once per batch (nothing to
// clean); the group kernel skips unsearched queries after `first` and accepts an empty group.
#define LAY_THREADS 256
#define LAY_ITEMS 8
#define LAY_TILE (LAY_THREADS * LAY_ITEMS)
#define CHAIN_VAL_BITS 38
#define CHAIN_VAL_MASK ((1ull << CHAIN_VAL_BITS) - 1ull)

__device__ __forceinline__ unsigned long long chain_pack(uint32_t epoch, uint32_t flag, unsigned long long v)
{
    return ((unsigned long long)epoch << (CHAIN_VAL_BITS + 2)) | ((unsigned long long)flag << CHAIN_VAL_BITS) | (v & CHAIN_VAL_MASK);
}

__global__ __launch_bounds__(LAY_THREADS) void layout_kernel(const uint32_t *slots, const uint32_t *d_nq, uint64_t *E,
                                                            uint32_t *group_first, uint64_t *group_start, uint32_t *d_n_groups, uint32_t groups_cap,
                                                            unsigned long long *chain, uint32_t epoch, uint32_t *status, uint32_t bshift)
{
    __shared__ uint64_t s_w[LAY_THREADS / 64];
    __shared__ uint64_t s_prefix;
    const uint32_t nq = *d_nq;
    const uint64_t base = (uint64_t)blockIdx.x * LAY_TILE;
    if (base > nq) return;  // nobody waits for a tile past the end
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t v[LAY_ITEMS];
    uint64_t sum = 0;
    const uint64_t i0 = base + (uint64_t)tid * LAY_ITEMS;
#pragma unroll
    for (int i = 0; i < LAY_ITEMS; i++) {
        v[i] = i0 + i < nq ? slots[i0 + i] : 0u;
        sum += v[i];
    }
    uint64_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint64_t woff = 0, tile_total = 0;
#pragma unroll
    for (int i = 0; i < LAY_THREADS / 64; i++) {
        if (i < (int)wv) woff += s_w[i];
        tile_total += s_w[i];
    }
    if (wv == 0) {
        unsigned long long prefix = 0;
        if (blockIdx.x > 0) {
            if (lane == 0)
                __hip_atomic_store(&chain[blockIdx.x], chain_pack(epoch, 1u, tile_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            long long j = (long long)blockIdx.x - 1;  // nearest predecessor still to be added
            uint32_t spins = 0;
            bool done = false;
            while (!done) {
                const long long idx = j - (long long)lane;
                unsigned long long w = chain_pack(epoch, 2u, 0ull);  // before tile 0: inclusive prefix 0
                if (idx >= 0) w = __hip_atomic_load(&chain[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t flag = (uint32_t)(w >> (CHAIN_VAL_BITS + 2)) == epoch ? (uint32_t)(w >> CHAIN_VAL_BITS) & 3u : 0u;
                const unsigned long long m_inc = __ballot(flag == 2u), m_inv = __ballot(flag == 0u);
                const uint32_t first_inc = m_inc ? (uint32_t)__ffsll((long long)m_inc) - 1u : 64u;
                const unsigned long long need = first_inc >= 63u ? ~0ull : ((2ull << first_inc) - 1ull);
                if (m_inv & need) {  // a predecessor has not published yet
                    if (++spins > (1u << 20)) { if (lane == 0) atomicOr(status, (uint32_t)ST_CHAIN_TIMEOUT); break; }
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                unsigned long long part = lane <= first_inc ? (w & CHAIN_VAL_MASK) : 0ull;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
                prefix += part;
                done = first_inc < 64u;
                j -= 64;
            }
        }
        if (lane == 0) {
            __hip_atomic_store(&chain[blockIdx.x], chain_pack(epoch, 2u, prefix + tile_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_prefix = prefix;
        }
    }
    __syncthreads();
    uint64_t ex = s_prefix + woff + inc - sum;
    if (i0 == 0 && nq > 0 && groups_cap > 0) { group_first[0] = 0u; group_start[0] = 0; }
#pragma unroll
    for (int i = 0; i < LAY_ITEMS; i++) {
        const uint64_t idx = i0 + i;
        if (idx <= nq) E[idx] = ex;
        if (idx == nq) {  // ex = total
            uint64_t ng = ex ? ((ex - 1) >> bshift) + 1 : 0;
            if (ng > groups_cap) { atomicOr(status, (uint32_t)ST_LIST_FULL); ng = 0; }
            *d_n_groups = (uint32_t)ng;
        }
        if (idx < nq && v[i]) {
            const uint64_t g = ex >> bshift, g_hi = (ex + v[i]) >> bshift;
            for (uint64_t gg = g + 1; gg <= g_hi && gg < groups_cap; gg++) {
                group_first[gg] = gg == g_hi ? (uint32_t)(idx + 1) : GRP_NONE;
                group_start[gg] = ex + v[i];  // slot of the next table start: the schedule's weights are differences of these
            }
        }
        ex += v[i];
    }
}

// Order in which the groups are handed out: longest first.  Group sizes vary 0..3x (a group takes
// every table that STARTS in its slot window, whatever its length), the counting kernel runs only
// ~3.5 groups per workgroup on a 10 000-query batch, and with groups in index order the stragglers
// of the last round cost ~15 % of the kernel (list scheduling vs longest-processing-time-first).
// Weight = slots of the group's tables, in 16 classes; a counting sort by class, one workgroup.
#define SCHED_MAX_GROUPS 32768u
__global__ __launch_bounds__(1024) void schedule_kernel(const uint32_t *group_first, const uint64_t *group_start, const uint64_t *E,
                                                        const uint32_t *d_n_groups, const uint32_t *d_nq, uint2 *sched, uint32_t *d_n_sched,
                                                        uint32_t cshift)
{
    __shared__ uint32_t s_hist[16], s_base[16], s_cur[16];
    __shared__ uint8_t s_cls[SCHED_MAX_GROUPS];
    const uint32_t ng = *d_n_groups, tid = threadIdx.x;
    if (ng > SCHED_MAX_GROUPS) {  // many groups per workgroup: the tail is negligible, index order (top bit = identity)
        if (tid == 0) *d_n_sched = ng | 0x80000000u;
        return;
    }
    const uint64_t total = E[*d_nq];
    if (tid < 16) { s_hist[tid] = 0; s_cur[tid] = 0; }
    __syncthreads();
    for (uint32_t g = tid; g < ng; g += 1024) {
        uint32_t c = 0xFFu;  // no table starts in the group: not scheduled
        if (group_first[g] != GRP_NONE) {
            const uint64_t ext = (g + 1 < ng ? group_start[g + 1] : total) - group_start[g];  // slots up to the next group's first table
            c = (uint32_t)(ext >> cshift);
            c = c > 15u ? 15u : c;
            atomicAdd(&s_hist[c], 1u);
        }
        s_cls[g] = (uint8_t)c;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int c = 15; c >= 0; c--) { s_base[c] = run; run += s_hist[c]; }
        *d_n_sched = run;
    }
    __syncthreads();
    for (uint32_t g = tid; g < ng; g += 1024) {
        const uint32_t c = s_cls[g];
        if (c != 0xFFu) sched[s_base[c] + atomicAdd(&s_cur[c], 1u)] = make_uint2(g, group_first[g]);
    }
}

// Protein batches: prep (search.go:286-296, search_protein.go:70-76), table layout and group schedule
// in ONE launch.  The three steps are tiny (~5 us each, mostly launch floor) and were three kernels in
// a row ahead of the probe.  Tiles of 2048 queries as in layout_kernel; the tile that finishes last
// builds the schedule, reading the other tiles' outputs with device-scope atomic loads (they are
// stored with device-scope atomic stores: no agent fence).
struct PrepLayoutParams {
    const uint8_t *seqs;
    const uint64_t *offsets;
    uint32_t n_seqs;
    uint64_t pos_bound;  // bytes of the batch as the caller gave them (<= the workspace's max_seq_bytes, checked on the host)
    kaamer_query_meta *q;
    uint32_t *d_nq;
    unsigned long long *d_n_pos;
    unsigned long long *invalid;
    QInfo *qinfo;
    uint64_t *hit_off;
    uint32_t *q_cnt;
    uint64_t *E;
    uint32_t *group_first;
    uint64_t *group_start;
    uint32_t *d_n_groups;
    uint32_t groups_cap;
    unsigned long long *chain;
    uint32_t epoch;
    uint32_t *status;
    uint2 *sched;
    uint32_t *d_n_sched;
    uint32_t *slots;              // table capacity per query (a later layout pass -- the PositionHits pass -- reads it)
    uint32_t bshift;              // a group / pack = the tables that start in one window of (1 << bshift) slots of the layout
    uint32_t cshift;              // schedule classes: slots of the group >> cshift (16 classes, longest first)
    uint32_t no_sched;            // 1: no group schedule is wanted (the pack kernel takes packs by ticket, in layout order)
    uint32_t *tiles_done;         // zero between batches (the last tile resets it)
    unsigned long long *d_total;  // total slots, for the schedule
    const uint32_t *slot_scale;   // table capacity scale left by the previous batch's finalize step (sixteenths)
    unsigned long long room_slots;   // slots of the hit arrays the tables may take (fit_table_scale)
};

#define PL_ITEMS 1   /* one query per thread: the prep part is a chain of dependent loads per query */
#define PL_TILE (LAY_THREADS * PL_ITEMS)
__global__ __launch_bounds__(LAY_THREADS) void prep_layout_schedule_kernel(PrepLayoutParams p)
{
    __shared__ uint64_t s_w[LAY_THREADS / 64];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_slots[PL_TILE];
    __shared__ uint32_t s_last;
    const uint32_t nq = p.n_seqs;
    const uint64_t base = (uint64_t)blockIdx.x * PL_TILE;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    // the offsets live in device memory and size every later access (vals, bitmap): offsets that do not agree with the
    // batch size the buffers were sized for make the whole batch an error, and nothing of it is searched
    const bool batch_bad = p.offsets[nq] > p.pos_bound;
    const uint32_t slot_scale = p.slot_scale ? fit_table_scale(*p.slot_scale, batch_bad ? 0ull : p.offsets[nq], nq, p.room_slots) : SLOT_SCALE_ONE;
    if (blockIdx.x == 0 && tid == 0) {
        const uint64_t n_pos = batch_bad ? 0 : p.offsets[nq];
        if (batch_bad) atomicOr(p.status, (uint32_t)ST_AA_CAP);
        *p.d_nq = nq;
        *p.d_n_pos = n_pos;
        mark_invalid_range(p.invalid, n_pos, (n_pos + 63) & ~63ull);  // bits past the end, in the last word the probe reads
    }
    // ---- prep: one query per thread and round (coalesced), its table capacity into LDS
#pragma unroll
    for (int r = 0; r < PL_ITEMS; r++) {
        const uint64_t i = base + (uint64_t)r * LAY_THREADS + tid;
        uint32_t slots = 0;
        if (i < nq) {
            uint64_t b = p.offsets[i], e = p.offsets[i + 1];
            if (batch_bad || e < b || e > p.pos_bound) {  // (not ascending: the same error)
                if (!batch_bad) atomicOr(p.status, (uint32_t)ST_AA_CAP);
                b = e = 0;
            }
            const int64_t len = (int64_t)(e - b);
            int32_t size = (int32_t)(len - KAAMER_KMER_SIZE + 1);       // search.go:290
            if (len > 0 && p.seqs[e - 1] == '*') size--;                // search.go:291-293
            kaamer_query_meta m;
            m.src_seq = (uint32_t)i;
            m.size_in_kmer = size;
            m.start_position = 1;                                       // search.go:225,303
            m.end_position = (int32_t)len;                              // search.go:294
            m.plus_strand = 1;
            m.aa_len = (uint32_t)len;
            m.aa_off = b;
            m.sa_off = 0;
            m.sa_len = 0;
            p.q[i] = m;
            p.q_cnt[i] = 0;
            p.hit_off[i] = 0;
            QInfo qi;
            qi.size = size;
            qi.aa_off = b;
            if (size >= 7) {                                            // search_protein.go:74-76
                qi.slots = table_slots_for(size, slot_scale);
                mark_invalid_range(p.invalid, b + (uint64_t)size, e);    // positions >= SizeInKmer start no k-mer
            } else {
                qi.slots = 0;
                mark_invalid_range(p.invalid, b, e);                     // the whole query is dropped
            }
            p.qinfo[i] = qi;
            p.slots[i] = qi.slots;
            slots = qi.slots;
        }
        s_slots[r * LAY_THREADS + tid] = slots;
    }
    __syncthreads();
    // ---- layout: as layout_kernel
    uint32_t v[PL_ITEMS];
    uint64_t sum = 0;
    const uint64_t i0 = base + (uint64_t)tid * PL_ITEMS;
#pragma unroll
    for (int i = 0; i < PL_ITEMS; i++) {
        v[i] = s_slots[tid * PL_ITEMS + i];
        sum += v[i];
    }
    uint64_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint64_t woff = 0, tile_total = 0;
#pragma unroll
    for (int i = 0; i < LAY_THREADS / 64; i++) {
        if (i < (int)wv) woff += s_w[i];
        tile_total += s_w[i];
    }
    if (wv == 0) {
        unsigned long long prefix = 0;
        if (blockIdx.x > 0) {
            if (lane == 0)
                __hip_atomic_store(&p.chain[blockIdx.x], chain_pack(p.epoch, 1u, tile_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            long long j = (long long)blockIdx.x - 1;
            uint32_t spins = 0;
            bool done = false;
            while (!done) {
                const long long idx = j - (long long)lane;
                unsigned long long w = chain_pack(p.epoch, 2u, 0ull);
                if (idx >= 0) w = __hip_atomic_load(&p.chain[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t flag = (uint32_t)(w >> (CHAIN_VAL_BITS + 2)) == p.epoch ? (uint32_t)(w >> CHAIN_VAL_BITS) & 3u : 0u;
                const unsigned long long m_inc = __ballot(flag == 2u), m_inv = __ballot(flag == 0u);
                const uint32_t first_inc = m_inc ? (uint32_t)__ffsll((long long)m_inc) - 1u : 64u;
                const unsigned long long need = first_inc >= 63u ? ~0ull : ((2ull << first_inc) - 1ull);
                if (m_inv & need) {
                    if (++spins > (1u << 20)) { if (lane == 0) atomicOr(p.status, (uint32_t)ST_CHAIN_TIMEOUT); break; }
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                unsigned long long part = lane <= first_inc ? (w & CHAIN_VAL_MASK) : 0ull;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
                prefix += part;
                done = first_inc < 64u;
                j -= 64;
            }
        }
        if (lane == 0) {
            __hip_atomic_store(&p.chain[blockIdx.x], chain_pack(p.epoch, 2u, prefix + tile_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_prefix = prefix;
        }
    }
    __syncthreads();
    uint64_t ex = s_prefix + woff + inc - sum;
    if (i0 == 0 && nq > 0 && p.groups_cap > 0) {
        __hip_atomic_store(&p.group_first[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&p.group_start[0], (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int i = 0; i < PL_ITEMS; i++) {
        const uint64_t idx = i0 + i;
        if (idx <= nq) p.E[idx] = ex;
        if (idx == nq) {  // ex = total
            uint64_t ng = ex ? ((ex - 1) >> p.bshift) + 1 : 0;
            if (ng > p.groups_cap) { atomicOr(p.status, (uint32_t)ST_LIST_FULL); ng = 0; }
            __hip_atomic_store(p.d_n_groups, (uint32_t)ng, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.d_total, (unsigned long long)ex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p.no_sched) *p.d_n_sched = (uint32_t)ng | 0x80000000u;  // groups in index order (top bit: identity)
        }
        if (idx < nq && v[i]) {
            const uint64_t g = ex >> p.bshift, g_hi = (ex + v[i]) >> p.bshift;
            for (uint64_t gg = g + 1; gg <= g_hi && gg < p.groups_cap; gg++) {
                __hip_atomic_store(&p.group_first[gg], gg == g_hi ? (uint32_t)(idx + 1) : GRP_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&p.group_start[gg], (uint64_t)(ex + v[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        ex += v[i];
    }
    // ---- the last tile to get here builds the schedule
    if (p.no_sched) return;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's atomic stores are done
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(p.tiles_done, 1u) == gridDim.x - 1u;
    __syncthreads();
    if (!s_last) return;
    if (tid == 0) __hip_atomic_store(p.tiles_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t *s_hist = s_slots, *s_base = s_slots + 16, *s_cur = s_slots + 32;  // the tile's slots are dead
    __shared__ uint8_t s_cls[SCHED_MAX_GROUPS];
    const uint32_t ng = __hip_atomic_load(p.d_n_groups, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ng > SCHED_MAX_GROUPS) {
        if (tid == 0) *p.d_n_sched = ng | 0x80000000u;
        return;
    }
    const uint64_t total = __hip_atomic_load(p.d_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 16) { s_hist[tid] = 0; s_cur[tid] = 0; }
    __syncthreads();
    for (uint32_t g = tid; g < ng; g += LAY_THREADS) {
        uint32_t c = 0xFFu;
        if (__hip_atomic_load(&p.group_first[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != GRP_NONE) {
            const uint64_t nxt = g + 1 < ng ? __hip_atomic_load(&p.group_start[g + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : total;
            const uint64_t ext = nxt - __hip_atomic_load(&p.group_start[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            c = (uint32_t)(ext >> p.cshift);
            c = c > 15u ? 15u : c;
            atomicAdd(&s_hist[c], 1u);
        }
        s_cls[g] = (uint8_t)c;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int c = 15; c >= 0; c--) { s_base[c] = run; run += s_hist[c]; }
        *p.d_n_sched = run;
    }
    __syncthreads();
    for (uint32_t g = tid; g < ng; g += LAY_THREADS) {
        const uint32_t c = s_cls[g];
        if (c != 0xFFu)
            p.sched[s_base[c] + atomicAdd(&s_cur[c], 1u)] =
                make_uint2(g, __hip_atomic_load(&p.group_first[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
}

#ifdef KAAMER_PHASE_CLOCK  /* measurement build only (tools/phase_clock.sh): where a group's time goes, in 10 ns ticks */
__device__ unsigned long long g_phase_clock[2048][16];  // per workgroup: summed on the host (global atomics would serialise)
#define PHASE_T() wall_clock64()
#define PHASE_ADD(i, v) pc_acc[i] += (unsigned long long)(v)
#endif
// MODE 0: count (Counter increments).  MODE 1: PositionHits (search.go:442-452): the hit
// lists are final; every table maps protein id -> index in the query's hit list and each
// (id, position) sets one bit of that hit's bitmap in HBM.  MODE 2: merge of partial hit
// lists (sharded index, SURVEY 8e): a "position" is one partial entry (id, count, first
// position) received from a shard; counts add, first positions take the minimum.
// A unit of two group windows whose tables exceed the arena (sized for ONE window's worst overhang, so that three workgroups
// fit a CU) is counted in two parts.
template <bool FIRSTPOS, int MODE = 0>
__global__ __launch_bounds__(64 * GRP_WAVES) void count_group_kernel(CountParams p)
{
    constexpr int WAVES = GRP_WAVES;
    constexpr uint32_t UQMAX = 2u * GRP_QMAX;   // queries of a unit
    constexpr uint32_t FIT = GRP_FIT;           // slots of the arena
    static_assert(UQMAX <= 256 && FIT <= 65535u, "query indices are bytes, table offsets 16-bit");
    constexpr int XIT = 2;
    __shared__ uint32_t a_keys[FIT];
    __shared__ uint32_t a_cnt[FIT];
    // MODE 0 with first positions: count (low 16 bits) and lowest position (high 16 bits) share one
    // word, so the tables cost the same LDS as without positions (3 workgroups per CU instead of 2);
    // queries of 65 535 k-mers or more go to the G tier.  The merge (MODE 2) keeps a separate array.
    constexpr bool PACKED = FIRSTPOS && MODE == 0;
    __shared__ uint32_t a_min[(FIRSTPOS && !PACKED) ? FIT : 1];
    __shared__ uint32_t g_q[UQMAX];
    __shared__ uint32_t g_size[MODE == 1 ? UQMAX : 1];   // (MODE 1: words of a hit's bitmap; the other modes read qinfo again when a query leaves)
    __shared__ uint16_t g_tab[UQMAX], g_cap[UQMAX];   // (slots of the arena)
    __shared__ uint8_t g_ovf[UQMAX];
    __shared__ uint32_t g_pref[UQMAX + 1];
    __shared__ unsigned long long g_base[MODE == 1 ? UQMAX : 1];  // MODE 1: first bitmap word of the query
    __shared__ uint64_t g_aa[UQMAX];
    __shared__ uint32_t s_splitq;   // the unit's tables do not fit the arena: the first query of its second part (GRP_NONE: none)
    constexpr bool FLATTENS = MODE != 2;   // (the merge adds one entry per position)
    __shared__ uint32_t s_pref[FLATTENS ? WAVES : 1][FLATTENS ? 64 : 1];
    __shared__ uint8_t s_own[FLATTENS ? WAVES : 1][FLATTENS ? XIT * 64 : 1];
    __shared__ uint32_t s_nq, s_slots, s_win;
    __shared__ uint8_t s_wq[2 * 64];  // query of the first position of every window
    __shared__ uint8_t s_sq[FIT / 64];  // query whose table holds 64-slot stripe s of the arena
    __shared__ uint32_t g_hits[UQMAX];    // distinct ids packed so far, per query (stripes are packed by any wave)
    // the tables start clean and every compaction leaves the stripes it packs clean again: no clear phase (and no barrier
    // after it) per group.  The positions pass does not compact: it clears the tables it fills.
    constexpr bool TABLES_LEFT_CLEAN = MODE != 1;
    __shared__ unsigned long long s_efirst;  // E of the group's first table = first hit-list entry of the group
    __shared__ unsigned long long s_tot[8];
    enum { T_IN = 0, T_Q, T_POST, T_HITS, T_OVF, T_LISTS, T_LIDS };

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
#ifdef KAAMER_PHASE_CLOCK
    const unsigned long long pc_start = PHASE_T();
    unsigned long long pc_t = pc_start;
    bool pc_first = true;
    unsigned long long pc_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    __shared__ unsigned long long pc_loop_all;
    if (tid == 0) pc_loop_all = 0;
#endif
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t n_groups = *p.d_n_groups;
    const uint32_t nq_total = *p.d_nq;
    if (tid < 8) s_tot[tid] = 0;
    if (FLATTENS)
        for (uint32_t i = tid; i < WAVES * XIT * 64; i += 64 * WAVES) (&s_own[0][0])[i] = 0;  // owner marks: clean between windows

    if (TABLES_LEFT_CLEAN) {
        for (uint32_t i = tid; i < FIT; i += 64 * WAVES) {
            a_keys[i] = KH_EMPTY_PID;
            a_cnt[i] = PACKED ? 0xFFFF0000u : 0u;
            if (FIRSTPOS && !PACKED) a_min[i] = 0xFFFFFFFFu;
        }
    }
    bool have_prev = false;  // a group has been packed whose per-query results (counts, list offsets) are still in LDS
    // what the stripes of the finished group added up to, per query: wave 0, before the descriptors are overwritten
    auto epilogue = [&]() {
        const uint32_t nqp = s_nq;
        for (uint32_t j = lane; j < nqp; j += 64) {
            const uint32_t q = g_q[j];
            if (g_ovf[j]) {
                if (MODE == 0) atomicAdd(&s_tot[T_OVF], 1ull);
                const uint32_t slot = atomicAdd(p.ovf_count, 1u);
                WorkItem wi;
                wi.q = q; wi.size = p.qinfo[q].size; wi.aa_off = g_aa[j];
                if (slot < p.list_cap) p.ovf_list[slot] = wi;
                else atomicOr(p.status, (uint32_t)ST_LIST_FULL);
                p.q_cnt[q] = 0;
                p.hit_off[q] = 0;
            } else {
                const unsigned long long base = s_efirst + g_tab[j];
                const bool have = base + g_cap[j] <= p.hit_cap;
                if (!have) atomicOr(p.status, (uint32_t)ST_POOL_FULL);
                p.q_cnt[q] = have ? g_hits[j] : 0u;   // (hits are added to the batch's counter by the stripes themselves)
                p.hit_off[q] = have ? base : 0;
            }
        }
    };
    // Groups are handed out dynamically (their sizes vary 0..4000 positions): a workgroup starts
    // with group blockIdx.x and then takes tickets from one counter.  Everything about the
    // following groups is fetched ahead so that no round trip is exposed: the ticket for the
    // group after next is taken at the top of a group, its first query is loaded during the
    // compaction, and the first 64 descriptors of the next group (wave 0) after the counting loop.
    __shared__ uint32_t s_ticket;
    const uint32_t n_sched_raw = *p.d_n_sched;
    const uint32_t n_sched = n_sched_raw & 0x7FFFFFFFu;
    const bool sched_identity = (n_sched_raw >> 31) != 0u;
    // ticket t -> (group, its first query) in the schedule (longest groups first); past the end: no group
    auto sched_entry = [&](uint32_t t) {
        if (t >= n_sched) return make_uint2(0xFFFFFFFFu, GRP_NONE);
        return sched_identity ? make_uint2(t, p.group_first[t]) : p.sched[t];
    };
    if (tid == 0) s_ticket = atomicAdd(p.group_queue, 1u) + gridDim.x;
    const uint2 e0 = sched_entry(blockIdx.x);
    uint32_t gid = e0.x, first = e0.y;
    __syncthreads();
    const uint2 e1 = sched_entry(s_ticket);
    uint32_t gid1 = e1.x, first1 = e1.y;
    QInfo pre_qi;
    pre_qi.size = 0; pre_qi.slots = 0; pre_qi.aa_off = 0;
    uint64_t pre_e = 0;
    if (wv == 0 && first != GRP_NONE && (uint64_t)first + lane < nq_total) { pre_qi = p.qinfo[first + lane]; pre_e = p.slot_off[first + lane]; }

    const uint32_t gshift = p.pack_shift ? p.pack_shift : GRP_SHIFT;   // window of a unit (the layout kernels were given the same)
    bool part_b = false;        // this cycle is the second part of the unit of the cycle before
    uint32_t split_from = 0;
    uint32_t ticket = 0;        // (thread 0) the ticket taken at the top of the unit's first cycle

    while (gid < n_groups) {
        __syncthreads();  // previous group's LDS state is dead (and s_ticket has been read)
#ifdef KAAMER_PHASE_CLOCK
        if (MODE == 0 && tid == 0) {
            const unsigned long long t = PHASE_T();
            if (pc_first) { PHASE_ADD(8, t - pc_start); pc_first = false; } else PHASE_ADD(5, t - pc_t);
            PHASE_ADD(0, 1);
            pc_t = t;
        }
#endif
        if (TABLES_LEFT_CLEAN && have_prev) {
            if (wv == 0) epilogue();
            have_prev = false;
        }
        if (tid == 0 && !part_b) ticket = atomicAdd(p.group_queue, 1u);  // in flight until after the counting loop
        if (first == GRP_NONE && !part_b) {  // a group without table starts (rare): advance, paying the round trips
            if (tid == 0) s_ticket = ticket + gridDim.x;
            __syncthreads();
            gid = gid1; first = first1;
            const uint2 en = sched_entry(s_ticket);
            gid1 = en.x; first1 = en.y;
            pre_qi.size = 0; pre_qi.slots = 0; pre_qi.aa_off = 0; pre_e = 0;
            if (wv == 0 && first != GRP_NONE && (uint64_t)first + lane < nq_total) { pre_qi = p.qinfo[first + lane]; pre_e = p.slot_off[first + lane]; }
            continue;
        }

        // ---- 1. descriptors of the unit's queries (wave 0)
        if (wv == 0) {
            // ONE pass, everything from registers: the flat position prefix is a DPP scan over the lanes' own sizes (no LDS
            // round trip through g_size, no six-step ds_bpermute scan), and every query marks the windows whose first position
            // falls inside it and the 64-slot stripes its table covers (stores only: the binary search per window that stood
            // here was ten dependent LDS reads).  The workgroup's other seven waves wait at the barrier below for this.
            // Queries from q_from on whose tables start below e_hi; -> (queries, positions, slots, first query left out)
            struct Desc { uint32_t nq, npos, slots, q_next; };
            auto describe = [&](uint32_t q_from, uint64_t e_hi, bool from_pre) {
                uint64_t e_first = __shfl(pre_e, 0, 64);
                if (!from_pre) e_first = p.slot_off[q_from];
                if (lane == 0) s_efirst = e_first;
                uint32_t nq = 0, pos_carry = 0, slots_end = 0, q_next = GRP_NONE;
                uint64_t q0 = q_from;
                bool done = false;
                while (!done) {
                    const uint64_t q = q0 + lane;
                    const bool in_range = q < nq_total;
                    QInfo qi;
                    qi.size = 0; qi.slots = 0; qi.aa_off = 0;
                    uint64_t e = 0;
                    if (from_pre && q0 == q_from) { qi = pre_qi; e = pre_e; }
                    else if (in_range) { qi = p.qinfo[q]; e = p.slot_off[q]; }
                    const bool searched = in_range && qi.slots != 0;
                    const bool beyond = !in_range || (searched && e >= e_hi);
                    const unsigned long long bm = __ballot(beyond);
                    const uint32_t cutoff = bm ? (uint32_t)__ffsll((long long)bm) - 1 : 64u;
                    const bool mine = searched && lane < cutoff;
                    const unsigned long long mm = __ballot(mine);
                    const uint32_t szm = mine ? (uint32_t)qi.size : 0u;
                    const uint32_t inc = wave_inclusive_scan_dpp(szm);
                    const uint32_t tab = (uint32_t)(e - e_first);
                    if (mine) {
                        const uint32_t idx = nq + (uint32_t)__popcll(mm & below);
                        if (idx < UQMAX && tab + qi.slots <= FIT) {   // (a table past the arena: the caller counts the unit in two parts)
                            const uint32_t lo = pos_carry + inc - szm, hi = pos_carry + inc;
                            g_q[idx] = (uint32_t)q;
                            if (MODE == 1) g_size[idx] = (uint32_t)qi.size;
                            g_aa[idx] = qi.aa_off;
                            g_tab[idx] = (uint16_t)tab;
                            g_cap[idx] = (uint16_t)qi.slots;
                            g_ovf[idx] = (PACKED && qi.size >= 65535) ? 1u : 0u;  // 16-bit counts and positions
                            g_pref[idx] = lo;
                            for (uint32_t w = (lo + 63u) >> 6; (w << 6) < hi && w < 128u; w++) s_wq[w] = (uint8_t)idx;
                            if (TABLES_LEFT_CLEAN) {
                                g_hits[idx] = 0u;
                                for (uint32_t st = tab >> 6; st < ((tab + qi.slots) >> 6) && st < FIT / 64; st++) s_sq[st] = (uint8_t)idx;
                            }
                        }
                    }
                    if (mm) {
                        const int last = 63 - __builtin_clzll(mm);
                        slots_end = (uint32_t)__builtin_amdgcn_readlane((int)(tab + qi.slots), last);
                    }
                    pos_carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
                    nq += (uint32_t)__popcll(mm);
                    done = bm != 0;
                    if (done && cutoff < 64u && q0 + cutoff < nq_total) q_next = (uint32_t)(q0 + cutoff);
                    q0 += 64;
                }
                Desc d;
                d.nq = nq > UQMAX ? UQMAX : nq;  // (cannot exceed it: >= 64 slots per searched query)
                d.npos = pos_carry; d.slots = slots_end; d.q_next = q_next;
                return d;
            };
            const uint64_t win_lo = (uint64_t)gid << gshift, win_hi = win_lo + (1ull << gshift);
            Desc d;
            uint32_t splitq = GRP_NONE;
            if (part_b) {
                d = describe(split_from, win_hi, false);          // the unit's second part (rare: the round trips are paid)
            } else {
                d = describe(first, win_hi, true);
                if (d.slots > FIT) {   // the unit's tables do not fit the arena: the tables that start in its first half now
                    d = describe(first, win_lo + (1ull << (gshift - 1u)), true);
                    splitq = d.q_next;
                }
            }
            if (lane == 0) {
                g_pref[d.nq] = d.npos;
                s_win = 0;
                s_nq = d.nq;
                s_slots = d.slots;
                s_splitq = splitq;
                if (TABLES_LEFT_CLEAN && MODE == 0) { s_tot[T_Q] += d.nq; s_tot[T_IN] += (unsigned long long)d.npos + 6ull * d.nq; }  // (only this lane writes these two)
            }
        }
        __syncthreads();
#ifdef KAAMER_PHASE_CLOCK
        if (MODE == 0 && tid == 0) { const unsigned long long t = PHASE_T(); PHASE_ADD(1, t - pc_t); pc_t = t; }
#endif
        const uint32_t nq = s_nq;
        const uint32_t split_now = s_splitq;   // != GRP_NONE: this cycle counts the unit's first part, the next one the rest
        const uint32_t n_slots = s_slots < FIT ? s_slots : FIT;
        const uint32_t n_posn = g_pref[nq];

        // ---- 2. clear the tables in use
        if (!TABLES_LEFT_CLEAN) {
            for (uint32_t i = tid; i < n_slots; i += 64 * WAVES) {
                a_keys[i] = KH_EMPTY_PID;
                a_cnt[i] = PACKED ? 0xFFFF0000u : 0u;
                if (FIRSTPOS && !PACKED) a_min[i] = 0xFFFFFFFFu;
            }
            __syncthreads();
        }
#ifdef KAAMER_PHASE_CLOCK
        unsigned long long pc_loop0 = 0;
        if (MODE == 0 && lane == 0) { pc_loop0 = PHASE_T(); if (tid == 0) { PHASE_ADD(2, pc_loop0 - pc_t); pc_t = pc_loop0; } }
#endif

        if (MODE == 1) {
            for (uint32_t j = wv; j < nq; j += WAVES) {
                const uint32_t q = g_q[j], base_slot = g_tab[j], cap = g_cap[j];
                const uint32_t cnt = p.q_cnt[q];
                const uint64_t off = p.hit_off[q];
                if (lane == 0) g_base[j] = p.pos_base[q];
                bool ok = true;
                for (uint32_t i = lane; i < cnt; i += 64) {
                    const uint32_t pid = p.hit_pid[off + i];
                    uint32_t hh = table_home(pid, cap);
                    bool placed = false;
                    for (uint32_t t = 0; t < cap && !placed; t++) {
                        if (atomicCAS(&a_keys[base_slot + hh], KH_EMPTY_PID, pid) == KH_EMPTY_PID) { a_cnt[base_slot + hh] = i; placed = true; }
                        else hh = (hh + 1u == cap) ? 0u : hh + 1u;
                    }
                    ok = ok && placed;
                }
                // a hit list that does not fit the table came from the G tier: positions_global_kernel
                // sets its bits (what this pass sets for the ids that did fit is the same bits)
                if (!__all(ok) && lane == 0) g_ovf[j] = 1;
            }
            __syncthreads();
        }

        // ---- 3. count: windows of 64 flat positions, software-pipelined per wave (the steps of a window:
        // count_window.hip.inc).  A window needs three dependent loads: its probe results (vals), the 16-byte list
        // heads, the ids beyond the three in a head.  Stage A(w+2), B(w+1) and the leftovers of w are issued in the same
        // iteration, so one memory round trip per iteration is exposed instead of three.
        // Windows are taken from an LDS counter: a window costs anything from an empty bitmap word to a few hundred ids,
        // and static striding left waves waiting at the barrier for a fifth of the kernel.  The first two windows of a
        // wave are static (no round trip).
        WorkCount work;
        const uint32_t n_win = (n_posn + 63u) >> 6;
        auto valid_at = [&](uint32_t w) { return w < n_win && ((w << 6) + lane) < n_posn; };
        auto pos_of = [&](uint32_t w) { return window_pos<UQMAX>(w, (w << 6) + lane, valid_at(w), s_wq, 128u, g_pref, nq); };
        uint32_t w0 = wv, w1 = wv + WAVES;
        uint32_t tk = 0;  // ticket in flight for the window after w1
        if (lane == 0) tk = atomicAdd(&s_win, 1u);

        if constexpr (MODE == 0) {
            // The search's counting pass.  Every global load of the loop is issued UNCONDITIONALLY (idle lanes read
            // word 0 of their array; the arena's first 16 bytes are zero: "no list") and the probe results and list heads
            // are consumed an ITERATION AFTER they were issued, as raw loop-carried registers: the compiler's
            // s_waitcnt vmcnt(N) then counts exactly.  With the loads inside branches (as MODE 1 / 2 below still have
            // them) every wait of the loop was a vmcnt(0): a window's three dependent loads cost three exposed round
            // trips.  The ids beyond a head's three are loaded before the first ids are added and read after.
            uint32_t *const pref = s_pref[wv];  // LDS accesses stay ds_* (a generic/volatile pointer becomes FLAT)
            uint8_t *const own = s_own[wv];
            auto add_n = [&](uint32_t j, uint32_t pid, uint32_t pos, uint32_t n) {
                if constexpr (PACKED) table_add_packed(a_keys, a_cnt, g_tab, g_cap, g_ovf, j, pid, pos, n);
                else table_add<FIRSTPOS>(a_keys, a_cnt, a_min, g_tab, g_cap, g_ovf, j, pid, pos, n);
            };
            struct RawA { uint32_t vraw, j, ps; };
            auto issue_a = [&](uint32_t w) {
                RawA r;
                const WinPos wp = pos_of(w);
                r.j = wp.j;
                r.ps = wp.ps;
                r.vraw = p.vals[valid_at(w) ? g_aa[wp.j] + wp.ps : 0ull];
                return r;
            };
            auto count_window = [&](uint32_t v, uint32_t wj, uint32_t wps, const uint4 &hv) {
                const uint4 h = head_of(v, hv);
                const LaneList ll = lane_list(h, wj, g_cap, g_ovf);
                work.list(v, h.x);
                const XWin xw = {v, h.z, h.w, wj, wps};
                const uint32_t xtotal = flatten_begin<XIT>(lane, ll.extra, pref, own);
                uint32_t carry = 0;
                XRound x[XIT];
#pragma unroll
                for (int it = 0; it < XIT; it++) x[it] = flatten_round<true>(lane, (uint32_t)it, xtotal, carry, xw, pref, own, p.arena);
                // the first ids are added while the loads above are in flight
                add_runs(lane, wj, ll.first_id, wps, add_n);
#pragma unroll
                for (int it = 0; it < XIT; it++) {
                    const uint32_t id = xround_id(x[it]);
                    if (id != KH_EMPTY_PID) add_n(x[it].j, id, x[it].ps, 1u);
                }
                if (xtotal > XIT * 64u) {
                    // very many ids in one window (a database with long postings lists: hundreds of ids behind one
                    // position): GRP_LONG_UNROLL chunks of 64 ids per round, their arena loads issued together
                    // (unconditionally, at clamped addresses) before the first add -- one dependent search -> load -> add
                    // chain per chunk (flatten_tail) made this path 5 x the cost of the rest on a database with lists of ~1 000
                    for (uint32_t t0 = XIT * 64u; t0 < xtotal; t0 += GRP_LONG_UNROLL * 64u) {
                        uint32_t lid[GRP_LONG_UNROLL], lj[GRP_LONG_UNROLL], lp[GRP_LONG_UNROLL];
#pragma unroll
                        for (int u = 0; u < (int)GRP_LONG_UNROLL; u++) {
                            const uint32_t t = t0 + (uint32_t)u * 64u + lane;
                            const bool act = t < xtotal;
                            const uint32_t tt = act ? t : xtotal - 1u;
                            const uint32_t lo = flatten_owner(pref, tt);
                            const XWin o = xwin_of(xw, lo);
                            lj[u] = o.j;
                            lp[u] = o.ps;
                            const uint32_t k = tt - pref[lo];
                            const uint32_t ld = p.arena[k >= 2u ? (uint64_t)o.v * 4 + 2 + k : 0ull];
                            const uint32_t m = k >= 2u ? 0xFFFFFFFFu : 0u;
                            const uint32_t idr = k == 0u ? o.z : o.w;
                            lid[u] = act ? ((ld & m) | (idr & ~m)) : KH_EMPTY_PID;
                        }
#pragma unroll
                        for (int u = 0; u < (int)GRP_LONG_UNROLL; u++)
                            if (lid[u] != KH_EMPTY_PID && !g_ovf[lj[u]]) add_n(lj[u], lid[u], lp[u], 1u);
                    }
                }
                flatten_end();
            };
            RawA a0 = issue_a(w0), a1 = issue_a(w1);
            uint32_t v0 = valid_at(w0) ? a0.vraw : 0u;
            uint4 hv0 = issue_head(p.arena, v0);
            while (w0 < n_win) {
                const uint32_t w2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)tk) + 2 * WAVES;
                if (lane == 0) tk = atomicAdd(&s_win, 1u);
                const RawA a2 = issue_a(w2);
                const uint32_t v1 = valid_at(w1) ? a1.vraw : 0u;
                const uint4 hv1 = issue_head(p.arena, v1);
                count_window(v0, a0.j, a0.ps, hv0);
                a0 = a1; v0 = v1; hv0 = hv1; a1 = a2;
                w0 = w1; w1 = w2;
            }
        } else {
            // MODE 1 and MODE 2: the same loop over their own three steps (loads inside branches: neither is the hot kernel)
            struct WinA { uint32_t v, j, ps; uint64_t a; };   // v: the lane has a position (MODE 1: its probe result)
            auto locate = [&](uint32_t w) {  // flat position -> (query, position in the query, index in the batch's arrays)
                WinA r;
                const WinPos wp = pos_of(w);
                r.v = valid_at(w) ? 1u : 0u;
                r.j = wp.j;
                r.ps = wp.ps;
                r.a = r.v ? g_aa[wp.j] + wp.ps : 0ull;
                return r;
            };
            auto window_loop = [&](auto stage_a, auto stage_b, auto step) {
                WinA a0 = stage_a(w0), a1 = stage_a(w1);
                uint4 h0 = stage_b(a0);
                while (w0 < n_win) {
                    const uint32_t w2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)tk) + 2 * WAVES;
                    if (lane == 0) tk = atomicAdd(&s_win, 1u);
                    const WinA a2 = stage_a(w2);
                    const uint4 h1 = stage_b(a1);
                    step(a0, h0);
                    a0 = a1; h0 = h1; a1 = a2;
                    w0 = w1; w1 = w2;
                }
            };
            if constexpr (MODE == 1) {
                // The positions pass: the ids of a window, flattened as in the count, each set the bits of their positions
                uint32_t *const pref = s_pref[wv];  // LDS accesses stay ds_* (a generic/volatile pointer becomes FLAT)
                uint8_t *const own = s_own[wv];
                auto stage_a = [&](uint32_t w) {
                    WinA r = locate(w);
                    if (r.v) r.v = p.vals[r.a];
                    return r;
                };
                // inline single id, or the list head {count, id0, id1, id2} from the arena
                auto stage_b = [&](const WinA &w) {
                    uint4 h = make_uint4(0, 0, 0, 0);
                    if (w.v & KH_INLINE_BIT) h = make_uint4(1u, w.v & ~KH_INLINE_BIT, 0, 0);
                    else if (w.v != 0u) h = reinterpret_cast<const uint4 *>(p.arena)[w.v];
                    return h;
                };
                // positions pos .. pos+n-1 (n <= 64: at most two words) of query j in the bitmap of its hit pid
                auto set_bits = [&](uint32_t j, uint32_t pid, uint32_t pos, uint32_t n) {
                    if (g_ovf[j]) return;
                    const uint32_t base = g_tab[j], cap = g_cap[j];
                    uint32_t hh = table_home(pid, cap);
                    for (uint32_t t = 0; t < cap; t++) {
                        const uint32_t kk = __hip_atomic_load(&a_keys[base + hh], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (kk == pid) {
                            const uint32_t words = (g_size[j] + 63u) >> 6;
                            unsigned long long *bm = p.pos_bits + g_base[j] + (unsigned long long)a_cnt[base + hh] * words;
                            const uint32_t w0 = pos >> 6, b0 = pos & 63u;
                            const uint32_t n0 = n < 64u - b0 ? n : 64u - b0;
                            atomicOr(&bm[w0], (n0 == 64u ? ~0ull : ((1ull << n0) - 1ull)) << b0);
                            if (n > n0) atomicOr(&bm[w0 + 1], (1ull << (n - n0)) - 1ull);
                            return;
                        }
                        if (kk == KH_EMPTY_PID) return;  // not a hit of this query (cannot happen)
                        hh = (hh + 1u == cap) ? 0u : hh + 1u;
                    }
                };
                auto set_bit = [&](uint32_t j, uint32_t pid, uint32_t pos) { set_bits(j, pid, pos, 1u); };
                auto step = [&](const WinA &w, const uint4 &h) {
                    const uint32_t lcnt = h.x;
                    const bool dead = lcnt != 0u && g_ovf[w.j] != 0u;  // (its hit list came from the G tier, and so do its bits)
                    const XWin xw = {w.v, h.z, h.w, w.j, w.ps};
                    const uint32_t xtotal = flatten_begin<XIT>(lane, (lcnt > 1u && !dead) ? lcnt - 1u : 0u, pref, own);
                    uint32_t carry = 0;
                    XRound x[XIT];
#pragma unroll
                    for (int it = 0; it < XIT; it++)
                        if ((uint32_t)it * 64u < xtotal)  // wave-uniform
                            x[it] = flatten_round<false>(lane, (uint32_t)it, xtotal, carry, xw, pref, own, p.arena);
                    add_runs(lane, w.j, (lcnt > 0 && !dead) ? h.y : KH_EMPTY_PID, w.ps, set_bits);
                    if (xtotal) {  // wave-uniform
#pragma unroll
                        for (int it = 0; it < XIT; it++) {
                            const uint32_t id = xround_id(x[it]);
                            if (id != KH_EMPTY_PID) set_bit(x[it].j, id, x[it].ps);
                        }
                        flatten_tail(lane, XIT * 64u, xtotal, xw, pref, g_ovf, p.arena, set_bit);
                        flatten_end();
                    }
                };
                window_loop(stage_a, stage_b, step);
            } else {
                // The merge: a "position" is one partial entry (id, count, first position), and a window is one add per
                // entry -- no list head, no flatten
                auto stage_b = [&](const WinA &w) {
                    return w.v ? make_uint4(1u, p.m_pid[w.a], p.m_km[w.a], FIRSTPOS ? p.m_fp[w.a] : 0u) : make_uint4(0, 0, 0, 0);
                };
                auto step = [&](const WinA &w, const uint4 &h) {
                    if (h.x != 0u) table_add<FIRSTPOS>(a_keys, a_cnt, a_min, g_tab, g_cap, g_ovf, w.j, h.y, h.w, h.z);  // (id, first position, count)
                };
                window_loop(locate, stage_b, step);
            }
        }
#ifdef KAAMER_PHASE_CLOCK
        if (MODE == 0 && lane == 0) { const unsigned long long t = PHASE_T(); atomicAdd(&pc_loop_all, t - pc_loop0); if (tid == 0) { PHASE_ADD(3, t - pc_t); pc_t = t; } }
#endif
        // prefetch the next group's descriptors (used at the top of the next iteration; a unit's second part loads its own)
        if (split_now == GRP_NONE) {
            pre_qi.size = 0; pre_qi.slots = 0; pre_qi.aa_off = 0; pre_e = 0;
            if (wv == 0 && first1 != GRP_NONE && (uint64_t)first1 + lane < nq_total) { pre_qi = p.qinfo[first1 + lane]; pre_e = p.slot_off[first1 + lane]; }
        }
        if (tid == 0) s_ticket = ticket + gridDim.x;
        if (MODE == 0) {
            const uint32_t a = wave_total(work.post), b = wave_total(work.lists), c = wave_total(work.lids);
            if (lane == 0) {
                atomicAdd(&s_tot[T_POST], (unsigned long long)a);
                atomicAdd(&s_tot[T_LISTS], (unsigned long long)b);
                atomicAdd(&s_tot[T_LIDS], (unsigned long long)c);
            }
        }
        __syncthreads();
#ifdef KAAMER_PHASE_CLOCK
        if (MODE == 0 && tid == 0) { const unsigned long long t = PHASE_T(); PHASE_ADD(4, t - pc_t); pc_t = t; }
#endif
        if (split_now != GRP_NONE) {   // the same unit again: its second part
            part_b = true; split_from = split_now;
        } else {
            const uint2 e2 = sched_entry(s_ticket);  // lands during the compaction
            gid = gid1; first = first1;
            gid1 = e2.x; first1 = e2.y;
            part_b = false;
        }
        if (MODE == 1) continue;  // bitmaps are written; nothing to compact (the loop top synchronises)

        // ---- 4. compaction: one wave per query packs its table into the query's hit list.
        // The list of query q lives at [E[q], E[q] + hits) of the hit arrays -- E is the table
        // layout, a table holds at most its capacity of distinct ids -- so nothing is allocated
        // and no pass has to count first.
        // a 64-slot stripe per wave and round, whatever query it belongs to (tables are multiples of 64 slots): all
        // eight waves pack -- a wave per QUERY left half of them idle on a group of three or four queries and the
        // longest table set the time; the position inside the query's list comes from a counter per query in LDS
        // (the order of a hit list is free).  The stripe is left clean for the next group.
        const uint32_t n_str = n_slots >> 6;
        for (uint32_t st = wv; st < n_str; st += WAVES) {
            const uint32_t slot = (st << 6) + lane;
            const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_sq[st]);
            const uint32_t k = a_keys[slot];
            const uint32_t w = a_cnt[slot];
            uint32_t mn = 0;
            if (FIRSTPOS && !PACKED) { mn = a_min[slot]; a_min[slot] = 0xFFFFFFFFu; }
            a_keys[slot] = KH_EMPTY_PID;
            a_cnt[slot] = PACKED ? 0xFFFF0000u : 0u;
            const unsigned long long base = s_efirst + g_tab[j];
            const bool usable = g_ovf[j] == 0u && base + g_cap[j] <= p.hit_cap;
            const bool has = usable && k != KH_EMPTY_PID;
            const unsigned long long bm = __ballot(has);
            if (bm) {  // wave-uniform
                uint32_t off = 0;
                if (lane == 0) {
                    off = atomicAdd(&g_hits[j], (uint32_t)__popcll(bm));
                    atomicAdd(&s_tot[T_HITS], (unsigned long long)__popcll(bm));
                }
                off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off);
                if (has) {
                    const unsigned long long idx = base + off + (uint32_t)__popcll(bm & below);
                    p.hit_pid[idx] = k;
                    p.hit_km[idx] = PACKED ? (w & 0xFFFFu) : w;
                    if (FIRSTPOS) p.hit_fp[idx] = PACKED ? (w >> 16) : mn;
                }
            }
        }
        have_prev = true;
    }
    __syncthreads();
    if (TABLES_LEFT_CLEAN && have_prev) {
        if (wv == 0) epilogue();
        __syncthreads();
    }
#ifdef KAAMER_PHASE_CLOCK
    if (MODE == 0 && tid == 0) { const unsigned long long t = PHASE_T(); if (!pc_first) PHASE_ADD(5, t - pc_t); PHASE_ADD(7, t - pc_start); PHASE_ADD(9, 1); pc_acc[6] = pc_loop_all;
        if (blockIdx.x < 2048) for (int i = 0; i < 10; i++) g_phase_clock[blockIdx.x][i] += pc_acc[i]; }
#endif
    if (tid == 0 && MODE == 2) add_counter(p.counters, blockIdx.x, CTR_HITS, s_tot[T_HITS]);
    if (tid == 0 && MODE == 0) {
        const uint32_t rep = blockIdx.x;
        add_counter(p.counters, rep, CTR_IN, s_tot[T_IN]);
        add_counter(p.counters, rep, CTR_QUERIES, s_tot[T_Q]);
        add_counter(p.counters, rep, CTR_POST, s_tot[T_POST]);
        add_counter(p.counters, rep, CTR_HITS, s_tot[T_HITS]);
        add_counter(p.counters, rep, CTR_OVERFLOW, s_tot[T_OVF]);
        add_counter(p.counters, rep, CTR_LISTS, s_tot[T_LISTS]);
        add_counter(p.counters, rep, CTR_LIST_IDS, s_tot[T_LIDS]);
    }
}

// ---- PositionHits bitmaps: layout helpers ---------------------------------------------------------
// words of one hit's bitmap = ceil(SizeInKmer / 64); a query's bitmaps are contiguous, in the
// order of its hit list.
// sizes: NULL = QInfo.size (a search); after an exchange merge, the owned queries' SizeInKmer (QInfo.size then holds
// their entry counts)
__global__ void pos_words_kernel(const QInfo *qinfo, const int32_t *sizes, const uint32_t *q_cnt, const uint32_t *d_nq, uint32_t *words)
{
    const uint32_t nq = *d_nq;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * blockDim.x) {
        const int32_t size = sizes ? sizes[q] : qinfo[q].size;
        const uint64_t w = size > 0 ? (uint64_t)q_cnt[q] * (((uint32_t)size + 63u) >> 6) : 0;
        words[q] = w > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)w;
    }
}

__global__ void pos_layout_kernel(const QInfo *qinfo, const int32_t *sizes, const uint32_t *q_cnt, const uint64_t *hit_off, const uint64_t *pos_base,
                                  const uint32_t *d_nq, uint64_t *pos_off, unsigned long long *pos_bits, uint64_t bits_cap,
                                  uint32_t *status)
{
    const uint32_t nq = *d_nq;
    const uint64_t total = pos_base[nq];
    if (total > bits_cap) { if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, (uint32_t)ST_POS_CAP); return; }
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = gtid; i < total; i += gsz) pos_bits[i] = 0ull;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t q = gtid >> 6; q < nq; q += gsz >> 6) {
        const uint32_t cnt = q_cnt[q];
        const int32_t size = sizes ? sizes[q] : qinfo[q].size;
        const uint64_t w = size > 0 ? (((uint32_t)size + 63u) >> 6) : 0;
        for (uint32_t i = lane; i < cnt; i += 64) pos_off[hit_off[q] + i] = pos_base[q] + (uint64_t)i * w;
    }
}

// ---- merge of partial hit lists (sharded index) ----------------------------------------------------
__global__ void prep_merge_kernel(const uint64_t *ent_off, uint32_t n_queries, const uint32_t *d_n_queries, QInfo *qinfo, uint32_t *slots,
                                  uint32_t *d_nq, uint64_t *hit_off, uint32_t *q_cnt)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (d_n_queries) n_queries = *d_n_queries < n_queries ? *d_n_queries : n_queries;  // the actual number (n_queries: a bound)
    if (i == 0) *d_nq = n_queries;
    if (i >= n_queries) return;
    const uint64_t b = ent_off[i], e = ent_off[i + 1];
    QInfo qi;
    qi.size = (int32_t)(e - b);
    qi.aa_off = b;
    qi.slots = (e - b) > (GRP_MAX_TABLE / 3) * 2 ? GRP_MAX_TABLE : table_slots_for(qi.size);
    qinfo[i] = qi;
    slots[i] = qi.slots;
    q_cnt[i] = 0;
    hit_off[i] = 0;
}

// queries whose partial entries exceed an LDS table: exact-size table in HBM (2 x entries)
__global__ __launch_bounds__(256) void merge_global_kernel(CountParams p)
{
    __shared__ uint32_t s_nd, s_cursor;
    __shared__ unsigned long long s_off, s_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t n_items = *p.list_count < p.list_cap ? *p.list_count : p.list_cap;
    unsigned long long tot_hits = 0;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const WorkItem wi = p.list[item];
        const uint32_t q = wi.q, n = (uint32_t)wi.size;
        uint32_t log2cap = 10;
        while ((1ull << log2cap) < 2ull * n && log2cap < 31) log2cap++;
        const unsigned long long cap = 1ull << log2cap;
        if (tid == 0) {
            s_nd = 0; s_cursor = 0;
            const unsigned long long off = atomicAdd(p.g_cursor, cap);
            if (off + cap > p.g_slots) { atomicOr(p.status, (uint32_t)ST_G_ARENA_FULL); s_off = ~0ull; }
            else s_off = off;
        }
        __syncthreads();
        const unsigned long long off = s_off;
        if (off == ~0ull) { if (tid == 0) { p.q_cnt[q] = 0; p.hit_off[q] = 0; } __syncthreads(); continue; }
        GlobalTable gt;
        gt.slots = p.g_keys + 4ull * off; gt.nd = &s_nd; gt.log2cap = log2cap;
        for (unsigned long long i = tid; i < cap; i += blockDim.x)
            reinterpret_cast<uint4 *>(gt.slots)[i] = make_uint4(KH_EMPTY_PID, 0u, 0xFFFFFFFFu, 0u);
        __syncthreads();
        uint32_t nnew = 0;
        for (uint32_t i = tid; i < n; i += blockDim.x) gt.add_n(p.m_pid[wi.aa_off + i], p.merge_fp ? p.m_fp[wi.aa_off + i] : 0u, p.m_km[wi.aa_off + i], nnew);
        {
            const uint32_t wn = wave_total(nnew);
            if (lane == 0 && wn) atomicAdd(&s_nd, wn);
        }
        __syncthreads();
        const uint32_t total = s_nd;
        if (tid == 0) {
            if (total == 0) s_base = 0;
            else s_base = tail_alloc(p, total);
        }
        __syncthreads();
        const unsigned long long base = s_base;
        if (base != ~0ull && total > 0) {
            for (unsigned long long i0 = (unsigned long long)(tid & ~63u); i0 < cap; i0 += blockDim.x) {
                const uint4 sv = reinterpret_cast<const uint4 *>(gt.slots)[i0 + lane];
                const uint32_t k = sv.x;
                const bool has = k != KH_EMPTY_PID;
                const unsigned long long bm = __ballot(has);
                uint32_t wbase = 0;
                if (lane == 0 && bm) wbase = atomicAdd(&s_cursor, (uint32_t)__popcll(bm));
                wbase = __shfl(wbase, 0, 64);
                if (has) {
                    const uint32_t idx = wbase + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
                    p.hit_pid[base + idx] = k;
                    p.hit_km[base + idx] = sv.y;
                    p.hit_fp[base + idx] = sv.z;
                }
            }
            if (tid == 0) tot_hits += total;
        }
        if (tid == 0) { p.q_cnt[q] = (base != ~0ull) ? total : 0u; p.hit_off[q] = base == ~0ull ? 0 : base; }
        __syncthreads();
    }
    if (tid == 0) add_counter(p.counters, blockIdx.x, CTR_HITS, tot_hits);
}
