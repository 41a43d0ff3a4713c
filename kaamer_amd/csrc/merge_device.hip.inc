// merge_device.hip.inc — kaamer_image_merge (builder.cpp) on the device: the same image, byte for byte.
// Included by builder_device.hip, inside its namespace: the merge supplies the two things a build takes from its
// proteins -- the pairs and, per key, the index of its first pair -- and bd_build_from_pairs does the rest.
//
//   merge(img_0 .. img_{n-1}) := kaamer_image_build_pairs(E(img_0) ++ .. ++ E(img_{n-1}))
//   E(img): the keys whose slot holds a list offset by (offset, key) ascending, each as (key, id) for its ids in stored
//           order, then the keys with an inline id by key ascending.
//
// Pairs.  The builder sorts them, so they are written in the order of the slots and not of E: a count pass over every slot
// of an input (0 for an empty slot, 1 for an inline id, arena[4 val] for a list), an exclusive scan, an emit pass.  Both
// passes read a slot through md_slot_count, so they agree; the scan's total is held against the host's own count of the
// input's pairs.  A list whose 16-byte units fill one 16-byte read of a whole wave (MD_WAVE_UNITS units = 64 lanes, so
// 252 ids and more) is copied by the wave, unit u by lane u mod 64, coalesced; a shorter one by the lane that owns its slot,
// in 16-byte reads as well: below that length a wave-wide read would have idle lanes, whatever the list.
// Ranks.  (offset, key) is 63 bits and leaves no room for the number of the input, so each input is ranked on its own:
// its non-empty slots become words  offset << 32 | key  (lists) and  1 << 63 | key  (inline ids), a radix sort puts them
// in the order of E, an exclusive scan of their counts gives the index of every key's first pair inside E(img), and the
// input's base (the pairs of the inputs before it) is added when the word is folded into the merged key array: the
// directory lookup of the build (key_index) and a 64-bit atomicMin per (input, key), at most n per word.
// Every arena access is bounded by the input's arena_words, here as in kaamer_merge_check on the host.
// Memory: the two 8-byte pair buffers of a build over the same number of pairs; next to the first of them one input at a
// time (buckets, arena, 4 bytes per slot for the counts and their scan) and 12 bytes per key of every input for the ranks.

#define MD_WAVE_UNITS 64u   // 16-byte units one read of a wave covers: lists of that many units and more go to the wave

__device__ inline uint32_t md_units(uint32_t c) { return (1u + c + 3u) / 4u; }

// pairs of slot s: 0 (empty), 1 (inline id) or the length of its list; a reference outside the arena counts 0 and is reported
__device__ inline uint32_t md_slot_count(const kh_slot *__restrict__ slots, uint64_t s, const uint32_t *__restrict__ arena, uint64_t aw,
                                         uint32_t &key, uint32_t &val, BuildStats *st)
{
    const kh_slot sl = slots[s];
    key = sl.key;
    val = sl.val;
    if (sl.key == KH_EMPTY_KEY) return 0;
    if (sl.val & KH_INLINE_BIT) return 1;
    const uint64_t off = (uint64_t)sl.val * 4;
    if (sl.val == 0 || off + 1 > aw) { st->bad = 1; return 0; }
    const uint32_t c = arena[off];
    if (off + 1 + c > aw) { st->bad = 1; return 0; }
    return c;
}

__global__ __launch_bounds__(256) void md_count_kernel(const kh_slot *__restrict__ slots, uint64_t n_slots, const uint32_t *__restrict__ arena,
                                                       uint64_t aw, uint32_t *__restrict__ cnt, BuildStats *st)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s >= n_slots) return;
    uint32_t key, val;
    cnt[s] = md_slot_count(slots, s, arena, aw, key, val, st);
}

// unit u of a list of c ids (word 0 of unit 0 is the count) -> its pairs
__device__ inline void md_emit_unit(const uint32_t *__restrict__ list, uint32_t u, uint32_t c, uint32_t key, uint64_t *__restrict__ dst)
{
    const uint4 w = *(const uint4 *)(list + (uint64_t)u * 4);
    const uint32_t v[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
    for (uint32_t t = 0; t < 4; t++) {
        const uint32_t word = u * 4 + t;   // id number word - 1
        if (word >= 1 && word <= c) dst[word - 1] = ((uint64_t)key << 32) | v[t];
    }
}

// arena: the device copy has 32 bytes of slack behind arena_words, so the last 16-byte read of a list that ends at the
// arena's last word stays inside the allocation whatever arena_words is
__global__ __launch_bounds__(256) void md_emit_kernel(const kh_slot *__restrict__ slots, uint64_t n_slots, const uint32_t *__restrict__ arena,
                                                      uint64_t aw, const uint32_t *__restrict__ off, uint64_t base, uint64_t *__restrict__ pairs,
                                                      uint64_t cap, BuildStats *st)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t key = 0, val = 0, c = 0;
    unsigned long long at = 0;
    if (s < n_slots) {
        c = md_slot_count(slots, s, arena, aw, key, val, st);
        at = base + off[s];
    }
    if (c && at + c > cap) { st->bad = 1; c = 0; }
    const bool is_list = c && !(val & KH_INLINE_BIT);
    const bool wide = is_list && md_units(c) >= MD_WAVE_UNITS;
    if (c && !is_list) pairs[at] = ((uint64_t)key << 32) | (val & ~KH_INLINE_BIT);
    else if (is_list && !wide) {
        const uint32_t *list = arena + (uint64_t)val * 4;
        for (uint32_t u = 0; u < md_units(c); u++) md_emit_unit(list, u, c, key, pairs + at);
    }
    // the long lists of this wave's slots, one after the other, each by all 64 lanes
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t w_val = __shfl(val, src, 64), w_c = __shfl(c, src, 64), w_key = __shfl(key, src, 64);
        const unsigned long long w_at = __shfl(at, src, 64);
        const uint32_t *list = arena + (uint64_t)w_val * 4;
        for (uint32_t u = lane; u < md_units(w_c); u += 64u) md_emit_unit(list, u, w_c, w_key, pairs + w_at);
    }
}

// ---- ranks: the order of E(img) ---------------------------------------------------------------------------------
#define MD_NO_WORD 0xFFFFFFFFFFFFFFFFull

struct SlotWord {   // slot -> its sort word (see the header)
    const kh_slot *slots;
    __device__ unsigned long long operator()(unsigned long long s) const
    {
        const kh_slot sl = slots[s];
        if (sl.key == KH_EMPTY_KEY) return MD_NO_WORD;
        if (sl.val & KH_INLINE_BIT) return (1ull << 63) | sl.key;
        return ((unsigned long long)sl.val << 32) | sl.key;
    }
};
struct IsWord {
    __device__ bool operator()(unsigned long long w) const { return w != MD_NO_WORD; }
};
struct OneIfWord {   // (the sum's type is that of its terms: 64 bits)
    __device__ unsigned long long operator()(unsigned long long w) const { return w != MD_NO_WORD ? 1ull : 0ull; }
};
struct WordCount {   // sorted word j -> the pairs its key contributes
    const unsigned long long *words;
    const uint32_t *arena;
    uint64_t aw;
    __device__ uint32_t operator()(uint32_t j) const
    {
        const unsigned long long w = words[j];
        if (w >> 63) return 1u;
        const uint64_t off = (w >> 32) * 4;
        return off + 1 <= aw ? arena[off] : 0u;
    }
};

// first[j] = index of the first pair of word j's key inside E(img); + base = inside the whole enumeration
__global__ __launch_bounds__(256) void md_rank_kernel(const unsigned long long *__restrict__ words, const uint32_t *__restrict__ first, uint32_t n,
                                                      unsigned long long base, FirstWindow fw, BuildStats *st)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t key = (uint32_t)words[j];
    const uint32_t ki = key_index(fw, key);
    if (ki >= fw.n_keys || fw.keys[ki] != key) { st->bad = 1; return; }   // (every enumerated key is a key of the merged pairs)
    atomicMin(fw.min_pos + ki, base + first[j]);
}

struct MergeRanks {   // what is kept of an input after its pairs are out
    DevMem words, first;   // [n_keys] in the order of E(img)
    uint32_t n_keys = 0;
    unsigned long long base = 0;
};

inline hipError_t md_grow(DevMem &d_tmp, size_t &have, size_t need)
{
    if (need <= have) return hipSuccess;
    have = need;
    return d_tmp.alloc(need);
}

// The whole merge; on success *out owns two device allocations (hipFree).  The inputs passed kaamer_merge_check, which
// counted n_pairs[i] and their sum `total` (< 2^32 - 1).
int md_merge_on_device(const kaamer_image *const *imgs, uint32_t n, const uint64_t *n_pairs, uint64_t total, double load, int device,
                       kaamer_device_image *out)
{
    out->d_buckets = nullptr;
    out->d_arena = nullptr;
    BD_HIP(hipSetDevice(device));
    Trace tr;
    DevMem d_st;
    BD_HIP(d_st.alloc(sizeof(BuildStats)));
    BD_HIP(hipMemset(d_st.p, 0, sizeof(BuildStats)));
    BuildStats *st = d_st.as<BuildStats>();
    BuildStats hs;

    DevMem d_pairs, d_pairs_alt, d_tmp;
    size_t tmp_bytes = 0;
    if (total) BD_HIP(d_pairs.alloc(total * 8));
    std::unique_ptr<MergeRanks[]> ranks(new (std::nothrow) MergeRanks[n]);
    if (!ranks) return kaamer_fail(KAAMER_E_NOMEM, "image_merge_device");
    unsigned long long base = 0;
    for (uint32_t i = 0; i < n; i++) {
        const kaamer_image *img = imgs[i];
        const uint64_t nb = img->hdr.n_buckets, aw = img->hdr.arena_words, n_slots = nb * KH_SLOTS_PER_BUCKET;
        MergeRanks &r = ranks[i];
        r.base = base;
        // ---- upload ------------------------------------------------------------------------------------------
        DevMem d_slots, d_arena, d_cnt, d_off;
        BD_HIP(d_slots.alloc((size_t)nb * sizeof(kh_bucket)));
        BD_HIP(d_arena.alloc((size_t)aw * 4 + 32));
        BD_HIP(hipMemcpy(d_slots.p, img->buckets, (size_t)nb * sizeof(kh_bucket), hipMemcpyHostToDevice));
        BD_HIP(hipMemcpy(d_arena.p, img->arena, (size_t)aw * 4, hipMemcpyHostToDevice));
        BD_HIP(hipMemset((char *)d_arena.p + (size_t)aw * 4, 0, 32));
        tr.lap("merge: upload", nb * 64 + aw * 4);
        const kh_slot *slots = d_slots.as<kh_slot>();
        const uint32_t *arena = d_arena.as<uint32_t>();
        // ---- pairs: count, scan, emit --------------------------------------------------------------------------
        BD_HIP(d_cnt.alloc((size_t)n_slots * 4));
        BD_HIP(d_off.alloc((size_t)n_slots * 4));
        const unsigned sb = blocks_for(n_slots, 256);
        hipLaunchKernelGGL(md_count_kernel, dim3(sb), dim3(256), 0, 0, slots, n_slots, arena, aw, d_cnt.as<uint32_t>(), st);
        {
            size_t need = 0;
            BD_HIP(rocprim::exclusive_scan(nullptr, need, d_cnt.as<uint32_t>(), d_off.as<uint32_t>(), 0u, (size_t)n_slots, rocprim::plus<uint32_t>()));
            BD_HIP(md_grow(d_tmp, tmp_bytes, need));
            BD_HIP(rocprim::exclusive_scan(d_tmp.p, need, d_cnt.as<uint32_t>(), d_off.as<uint32_t>(), 0u, (size_t)n_slots, rocprim::plus<uint32_t>()));
        }
        uint32_t last_off = 0, last_cnt = 0;
        BD_HIP(hipMemcpy(&last_off, d_off.as<uint32_t>() + (n_slots - 1), 4, hipMemcpyDeviceToHost));
        BD_HIP(hipMemcpy(&last_cnt, d_cnt.as<uint32_t>() + (n_slots - 1), 4, hipMemcpyDeviceToHost));
        BD_HIP(hipMemcpy(&hs, st, sizeof hs, hipMemcpyDeviceToHost));
        if (hs.bad || (uint64_t)last_off + last_cnt != n_pairs[i])
            return kaamer_fail(KAAMER_E_HIP, "device merge: the count pass over input %u disagrees with the host's", i);
        hipLaunchKernelGGL(md_emit_kernel, dim3(sb), dim3(256), 0, 0, slots, n_slots, arena, aw, d_off.as<uint32_t>(), (uint64_t)base,
                           d_pairs.as<uint64_t>(), total, st);
        BD_HIP(hipMemcpy(&hs, st, sizeof hs, hipMemcpyDeviceToHost));
        if (hs.bad) return kaamer_fail(KAAMER_E_HIP, "device merge: the emit pass over input %u disagrees with the count pass", i);
        d_cnt.release(); d_off.release();
        tr.lap("merge: expand", n_pairs[i]);
        // ---- ranks: the non-empty slots in the order of E(img), and the index of every key's first pair ----------------
        DevMem d_words, d_words_alt, d_count;
        BD_HIP(d_count.alloc(8));
        {
            auto words = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned long long>(0), SlotWord{ slots });
            // every non-empty slot is selected: the output is sized by the slots the input really fills, not by its header
            unsigned long long filled = 0;
            {
                auto ones = rocprim::make_transform_iterator(words, OneIfWord());
                size_t need = 0;
                BD_HIP(rocprim::reduce(nullptr, need, ones, d_count.as<unsigned long long>(), 0ull, (size_t)n_slots, rocprim::plus<unsigned long long>()));
                BD_HIP(md_grow(d_tmp, tmp_bytes, need));
                BD_HIP(rocprim::reduce(d_tmp.p, need, ones, d_count.as<unsigned long long>(), 0ull, (size_t)n_slots, rocprim::plus<unsigned long long>()));
                BD_HIP(hipMemcpy(&filled, d_count.p, sizeof filled, hipMemcpyDeviceToHost));
            }
            if (filled >= 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_CAPACITY, "device merge: input %u holds too many keys", i);
            BD_HIP(d_words.alloc(filled * 8));
            BD_HIP(d_words_alt.alloc(filled * 8));
            size_t need = 0;
            BD_HIP(rocprim::select(nullptr, need, words, d_words.as<unsigned long long>(), d_count.as<size_t>(), (size_t)n_slots, IsWord()));
            BD_HIP(md_grow(d_tmp, tmp_bytes, need));
            BD_HIP(rocprim::select(d_tmp.p, need, words, d_words.as<unsigned long long>(), d_count.as<size_t>(), (size_t)n_slots, IsWord()));
            r.n_keys = (uint32_t)filled;
        }
        if (r.n_keys) {
            rocprim::double_buffer<unsigned long long> wb(d_words.as<unsigned long long>(), d_words_alt.as<unsigned long long>());
            size_t need = 0;
            BD_HIP(rocprim::radix_sort_keys(nullptr, need, wb, (size_t)r.n_keys, 0u, 64u));
            BD_HIP(md_grow(d_tmp, tmp_bytes, need));
            BD_HIP(rocprim::radix_sort_keys(d_tmp.p, need, wb, (size_t)r.n_keys, 0u, 64u));
            if (wb.current() == d_words.as<unsigned long long>()) { r.words.p = d_words.take(); d_words_alt.release(); }
            else { r.words.p = d_words_alt.take(); d_words.release(); }
            BD_HIP(r.first.alloc((size_t)r.n_keys * 4));
            auto counts = rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0), WordCount{ r.words.as<unsigned long long>(), arena, aw });
            need = 0;
            BD_HIP(rocprim::exclusive_scan(nullptr, need, counts, r.first.as<uint32_t>(), 0u, (size_t)r.n_keys, rocprim::plus<uint32_t>()));
            BD_HIP(md_grow(d_tmp, tmp_bytes, need));
            BD_HIP(rocprim::exclusive_scan(d_tmp.p, need, counts, r.first.as<uint32_t>(), 0u, (size_t)r.n_keys, rocprim::plus<uint32_t>()));
        }
        BD_HIP(hipDeviceSynchronize());   // (the input's buffers go out of scope here)
        tr.lap("merge: order of E", r.n_keys);
        base += n_pairs[i];
    }
    d_tmp.release();
    if (total) BD_HIP(d_pairs_alt.alloc(total * 8));
    BD_HIP(hipMemset(st, 0, sizeof(BuildStats)));

    const RankSource by_enumeration = [&](const FirstWindow &fw) {
        for (uint32_t i = 0; i < n; i++) {
            MergeRanks &r = ranks[i];
            if (!r.n_keys) continue;
            hipLaunchKernelGGL(md_rank_kernel, dim3(blocks_for(r.n_keys, 256)), dim3(256), 0, 0, r.words.as<unsigned long long>(),
                               r.first.as<uint32_t>(), r.n_keys, r.base, fw, st);
        }
        BD_HIP(hipGetLastError());
        for (uint32_t i = 0; i < n; i++) { ranks[i].words.release(); ranks[i].first.release(); }   // (hipFree waits for the kernels)
        return (int)KAAMER_OK;
    };
    return bd_build_from_pairs(d_pairs, d_pairs_alt, total, imgs[0]->hdr.shard, imgs[0]->hdr.n_shards, load, st, tr, total, by_enumeration, out);
}
