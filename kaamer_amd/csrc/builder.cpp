// builder.cpp — host-side emitter of the GPU hash-table layout (kaamer_layout.h).
//
// Semantics follow the reference's offline side:
//   emit   : pkg/makedb/inputFASTA.go:245-248, inputTSV.go:236-239 (every 7-mer
//            window of every protein with len >= 7 -> (key, proteinId))
//   collapse: pkg/indexdb/indexdb.go:68-132 (KeyToList gathers all versions of a
//            key) + pkg/kvstore/kv_store.go:284-305 (RemoveDuplicatesFromSlice)
//            => key -> set<proteinId>
//   sharing: pkg/kvstore/kcomb_store.go:42-85 (identical sets stored once)
// The LSM stores themselves are replaced by the bucketised table.
#include "kaamer_internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

namespace {

unsigned n_threads()
{
    unsigned n = std::thread::hardware_concurrency();
    if (const char *e = getenv("KAAMER_BUILD_THREADS")) n = (unsigned)atoi(e);
    if (n < 1) n = 1;
    if (n > 64) n = 64;
    return n;
}

template <class F> void parallel_for(size_t n, unsigned nt, F f)
{
    if (nt <= 1 || n < 2) { f(0, n, 0); return; }
    std::vector<std::thread> th;
    size_t per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        size_t b = std::min(n, per * t), e = std::min(n, per * (t + 1));
        if (b >= e) break;
        th.emplace_back([=] { f(b, e, t); });
    }
    for (auto &x : th) x.join();
}

// sort u64 ascending: partition on the top 11 bits, then std::sort the parts in parallel
void sort_u64(uint64_t *a, size_t n)
{
    unsigned nt = n_threads();
    if (n < (1u << 16) || nt == 1) { std::sort(a, a + n); return; }
    const int B = 11, NB = 1 << B;
    std::vector<size_t> cnt(NB + 1, 0);
    for (size_t i = 0; i < n; i++) cnt[(a[i] >> (64 - B)) + 1]++;
    for (int i = 0; i < NB; i++) cnt[i + 1] += cnt[i];
    uint64_t *tmp = (uint64_t *)malloc(n * sizeof(uint64_t));
    if (!tmp) { std::sort(a, a + n); return; }
    {
        std::vector<size_t> pos(cnt.begin(), cnt.end() - 1);
        for (size_t i = 0; i < n; i++) tmp[pos[a[i] >> (64 - B)]++] = a[i];
    }
    std::atomic<int> next(0);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&] {
            for (;;) {
                int b = next.fetch_add(1);
                if (b >= NB) break;
                std::sort(tmp + cnt[b], tmp + cnt[b + 1]);
            }
        });
    for (auto &x : th) x.join();
    memcpy(a, tmp, n * sizeof(uint64_t));
    free(tmp);
}

// KAAMER_BUILD_TRACE=1: phase times of a build on stderr
struct Trace {
    bool on = getenv("KAAMER_BUILD_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what, uint64_t n)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[kaamer build] %-22s %8.2f s  (%llu)\n", what, std::chrono::duration<double>(now - t).count(), (unsigned long long)n);
        t = now;
    }
};

uint64_t hash_list(const uint32_t *ids, uint32_t n)
{
    uint64_t h = 0x9E3779B97F4A7C15ull ^ n;
    for (uint32_t i = 0; i < n; i++) {
        h ^= ids[i] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h *= 0xff51afd7ed558ccdull;
        h ^= h >> 33;
    }
    return h ? h : 1;
}

// The sorted distinct keys of a build behind a directory on their top bits: key -> index in a few steps.
struct KeyIndex {
    const uint32_t *keys;
    uint64_t n;
    int shift;
    std::vector<uint32_t> dir;   // dir[d] = first index whose key >> shift is >= d
    KeyIndex(const uint32_t *k, uint64_t n_keys) : keys(k), n(n_keys)
    {
        int bits = 4;
        while (bits < 22 && (8ull << bits) < n) bits++;
        shift = 32 - bits;
        dir.assign(((size_t)1 << bits) + 1, (uint32_t)n);
        for (uint64_t i = n; i-- > 0;) dir[keys[i] >> shift] = (uint32_t)i;
        for (size_t d = dir.size() - 1; d-- > 0;) dir[d] = std::min(dir[d], dir[d + 1]);
    }
    uint64_t find(uint32_t key) const   // the key is one of keys[]
    {
        uint64_t lo = dir[key >> shift], hi = dir[(key >> shift) + 1];
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] <= key) lo = mid; else hi = mid;
        }
        return lo;
    }
};

inline void atomic_min(std::atomic<uint64_t> &a, uint64_t v)
{
    uint64_t c = a.load(std::memory_order_relaxed);
    while (v < c && !a.compare_exchange_weak(c, v, std::memory_order_relaxed)) {}
}

// fills rank[k], preset to ~0, with the smallest window index that refers to key k (see build_from_sorted_input)
using RankFill = std::function<void(const KeyIndex &, std::atomic<uint64_t> *)>;

struct RankedList { uint64_t rank; uint32_t list; };

// ascending rank (ranks are distinct and <= max_rank): partition on the top 11 bits, std::sort the parts in parallel
void sort_ranked(std::vector<RankedList> &a, uint64_t max_rank)
{
    const size_t n = a.size();
    const auto less = [](const RankedList &x, const RankedList &y) { return x.rank < y.rank; };
    unsigned nt = n_threads();
    if (n < (1u << 16) || nt == 1) { std::sort(a.begin(), a.end(), less); return; }
    const int B = 11, NB = 1 << B;
    int shift = 0;
    while ((max_rank >> shift) >= (uint64_t)NB) shift++;
    std::vector<size_t> cnt(NB + 1, 0);
    for (size_t i = 0; i < n; i++) cnt[(a[i].rank >> shift) + 1]++;
    for (int i = 0; i < NB; i++) cnt[i + 1] += cnt[i];
    std::vector<RankedList> tmp(n);
    {
        std::vector<size_t> pos(cnt.begin(), cnt.end() - 1);
        for (size_t i = 0; i < n; i++) tmp[pos[a[i].rank >> shift]++] = a[i];
    }
    std::atomic<int> next(0);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&] {
            for (;;) {
                int b = next.fetch_add(1);
                if (b >= NB) break;
                std::sort(tmp.begin() + cnt[b], tmp.begin() + cnt[b + 1], less);
            }
        });
    for (auto &x : th) x.join();
    a.swap(tmp);
}

}  // namespace

int kaamer_image_alloc(kaamer_image *img, uint64_t n_buckets, uint64_t arena_words)
{
    img->buckets = nullptr;
    img->arena = nullptr;
    if (posix_memalign((void **)&img->buckets, 4096, (size_t)n_buckets * sizeof(kh_bucket)) != 0)
        return KAAMER_E_NOMEM;
    if (posix_memalign((void **)&img->arena, 4096, (size_t)std::max<uint64_t>(arena_words, 4) * 4) != 0)
        return KAAMER_E_NOMEM;
    img->hdr.n_buckets = n_buckets;
    img->hdr.arena_words = arena_words;
    return KAAMER_OK;
}

// pairs64: key<<32|id, any order, possibly with duplicates; consumed (sorted in place)
//
// Order of the arena.  The rank of a stored postings list is the smallest window index that refers to it, over every
// key that shares the list; rank_of_keys supplies it per key (build_proteins: the absolute residue position of the
// window, so proteins in input order and positions ascending; build_pairs: the index of the pair in the input).  Lists
// are laid out in ascending rank from unit 1: the lists behind consecutive windows of a protein are consecutive 16-byte
// units, four heads to a 64-byte sector, and a query that resembles the protein reads them coalesced.  The rank is a
// minimum and not "the order a walk meets them", so builder_device.hip computes it in parallel and lands on the same bytes.
static int build_from_sorted_input(uint64_t *pairs64, uint64_t n, uint32_t shard, uint32_t n_shards,
                                   double load, const RankFill &rank_of_keys, kaamer_image **out)
{
    if (!(load > 0.05 && load <= 0.95)) load = 0.5;
    Trace tr;
    sort_u64(pairs64, n);
    tr.lap("sort pairs", n);
    n = (uint64_t)(std::unique(pairs64, pairs64 + n) - pairs64);
    tr.lap("unique", n);

    // distinct keys
    uint64_t n_keys = 0;
    for (uint64_t i = 0; i < n; i++)
        if (i == 0 || (pairs64[i] >> 32) != (pairs64[i - 1] >> 32)) n_keys++;
    std::vector<uint64_t> kstart((size_t)n_keys + 1);
    std::vector<uint32_t> keys((size_t)n_keys);
    {
        uint64_t k = 0;
        for (uint64_t i = 0; i < n; i++)
            if (i == 0 || (pairs64[i] >> 32) != (pairs64[i - 1] >> 32)) { kstart[k] = i; keys[k++] = (uint32_t)(pairs64[i] >> 32); }
        kstart[n_keys] = n;
    }

    kaamer_image *img = new (std::nothrow) kaamer_image();
    if (!img) return kaamer_fail(KAAMER_E_NOMEM, "image alloc");
    img->buckets = nullptr;
    img->arena = nullptr;
    memset(&img->hdr, 0, sizeof img->hdr);
    img->hdr.magic = KH_IMAGE_MAGIC;
    img->hdr.version = KH_IMAGE_VERSION;
    img->hdr.kmer_size = KAAMER_KMER_SIZE;
    img->hdr.shard = shard;
    img->hdr.n_shards = n_shards;
    img->hdr.load_factor = load;
    img->hdr.n_pairs = n;
    img->hdr.n_keys = n_keys;

    uint64_t n_buckets = (uint64_t)((double)n_keys / (KH_SLOTS_PER_BUCKET * load)) + 1;
    if (n_buckets >= (1ull << 32)) { delete img; return kaamer_fail(KAAMER_E_ARG, "too many buckets"); }

    // ---- rank of every key: its first window -------------------------------
    std::unique_ptr<std::atomic<uint64_t>[]> rank(new (std::nothrow) std::atomic<uint64_t>[(size_t)n_keys + 1]);
    if (!rank) { delete img; return kaamer_fail(KAAMER_E_NOMEM, "rank buffer"); }
    for (uint64_t k = 0; k < n_keys; k++) rank[k].store(~0ull, std::memory_order_relaxed);
    if (n_keys) {
        const KeyIndex ki(keys.data(), n_keys);
        rank_of_keys(ki, rank.get());
    }
    tr.lap("first windows", n_keys);

    // ---- postings sets with sharing ----------------------------------------
    // a set is stored once: keys are matched through an open-addressed table on the 64-bit content hash of their set
    // and verified against the pairs of the set's first key; the set's rank is the minimum over its keys
    auto is_inline = [&](uint64_t k) { return kstart[k + 1] - kstart[k] == 1 && (uint32_t)pairs64[kstart[k]] < KH_INLINE_BIT; };
    uint64_t n_lists_ub = 0, ub_words = 4;   // offset 0 is reserved (val 0 never used)
    for (uint64_t k = 0; k < n_keys; k++)
        if (!is_inline(k)) { n_lists_ub++; ub_words += ((1 + (kstart[k + 1] - kstart[k]) + 3) / 4) * 4; }
    if (ub_words / 4 >= KH_INLINE_BIT) { delete img; return kaamer_fail(KAAMER_E_ARG, "arena exceeds 32 GiB per shard"); }
    uint64_t dcap = 16;
    while (dcap < n_lists_ub * 2) dcap <<= 1;
    std::vector<uint64_t> dh(dcap, 0);
    std::vector<uint32_t> dlist(dcap, 0);
    std::vector<uint32_t> list_of((size_t)n_keys, 0);   // list index of a key, later its slot value
    std::vector<uint32_t> lkey;                         // first key of a list
    std::vector<RankedList> order;

    uint64_t n_inline = 0, max_list = 0, n_displaced = 0, max_rank = 0;
    uint32_t max_pid = 0;
    std::vector<uint32_t> tmp;
    for (uint64_t k = 0; k < n_keys; k++) {
        const uint64_t i = kstart[k];
        const uint32_t c = (uint32_t)(kstart[k + 1] - i);
        max_pid = std::max(max_pid, (uint32_t)pairs64[i + c - 1]);
        if (is_inline(k)) { n_inline++; continue; }
        tmp.resize(c);
        for (uint32_t t = 0; t < c; t++) tmp[t] = (uint32_t)pairs64[i + t];  // ascending
        const uint64_t h = hash_list(tmp.data(), c);
        const uint64_t r = rank[k].load(std::memory_order_relaxed);
        uint64_t s = h & (dcap - 1);
        bool found = false;
        for (;;) {
            if (dh[s] == 0) break;
            if (dh[s] == h) {
                const uint64_t ri = kstart[lkey[dlist[s]]];
                bool same = kstart[lkey[dlist[s]] + 1] - ri == c;
                for (uint32_t t = 0; same && t < c; t++) same = (uint32_t)pairs64[ri + t] == tmp[t];
                if (same) { found = true; break; }
            }
            s = (s + 1) & (dcap - 1);
        }
        if (found) {
            list_of[k] = dlist[s];
            order[dlist[s]].rank = std::min(order[dlist[s]].rank, r);
        } else {
            dh[s] = h;
            dlist[s] = list_of[k] = (uint32_t)lkey.size();
            lkey.push_back((uint32_t)k);
            order.push_back(RankedList{ r, (uint32_t)order.size() });
            max_list = std::max<uint64_t>(max_list, c);
        }
    }
    const uint64_t n_lists = lkey.size();
    for (const RankedList &o : order) max_rank = std::max(max_rank, o.rank);
    std::vector<uint64_t>().swap(dh);
    std::vector<uint32_t>().swap(dlist);
    rank.reset();
    tr.lap("share lists", n_lists);

    // ---- arena in ascending rank -------------------------------------------
    sort_ranked(order, max_rank);
    std::vector<uint32_t> loff((size_t)n_lists);   // list -> offset in 16-byte units
    uint64_t words = 4;
    for (const RankedList &o : order) {
        loff[o.list] = (uint32_t)(words / 4);
        const uint64_t k = lkey[o.list];
        words += ((1 + (kstart[k + 1] - kstart[k]) + 3) / 4) * 4;
    }
    std::vector<RankedList>().swap(order);
    int rc = kaamer_image_alloc(img, n_buckets, words);
    if (rc) { kaamer_image_free(img); return kaamer_fail(rc, "image buffers"); }
    memset(img->buckets, 0xFF, (size_t)n_buckets * sizeof(kh_bucket));
    memset(img->arena, 0, 16);
    parallel_for((size_t)n_lists, n_threads(), [&](size_t b, size_t e, unsigned) {
        for (size_t li = b; li < e; li++) {
            const uint64_t i = kstart[lkey[li]];
            const uint32_t c = (uint32_t)(kstart[lkey[li] + 1] - i);
            uint32_t *l = img->arena + (uint64_t)loff[li] * 4;
            l[0] = c;
            for (uint32_t t = 0; t < c; t++) l[1 + t] = (uint32_t)pairs64[i + t];
            const uint64_t used = 1 + (uint64_t)c, padded = ((used + 3) / 4) * 4;
            for (uint64_t p = used; p < padded; p++) l[p] = KH_EMPTY_PID;
        }
    });
    tr.lap("arena", words);

    // ---- the bucket table, keys in ascending order ---------------------------
    for (uint64_t k = 0; k < n_keys; k++) {
        const uint32_t key = keys[k];
        const uint32_t val = is_inline(k) ? (KH_INLINE_BIT | (uint32_t)pairs64[kstart[k]]) : loff[list_of[k]];
        uint64_t b = kh_home_bucket(key, n_shards, n_buckets);
        bool placed = false, home = true;
        for (uint64_t tries = 0; tries < n_buckets && !placed; tries++) {
            kh_bucket &bk = img->buckets[b];
            for (int sidx = 0; sidx < KH_SLOTS_PER_BUCKET; sidx++) {
                if (bk.s[sidx].key == KH_EMPTY_KEY) {
                    bk.s[sidx].key = key;
                    bk.s[sidx].val = val;
                    placed = true;
                    break;
                }
            }
            if (!placed) { b = (b + 1 == n_buckets) ? 0 : b + 1; home = false; }
        }
        if (!placed) { kaamer_image_free(img); return kaamer_fail(KAAMER_E_CAPACITY, "table full"); }
        if (!home) n_displaced++;
    }
    tr.lap("placement", n_keys);
    img->hdr.arena_words = words;
    img->hdr.n_inline = n_inline;
    img->hdr.n_lists = n_lists;
    img->hdr.max_list = max_list;
    img->hdr.n_displaced = n_displaced;
    img->hdr.max_protein_id = max_pid;
    *out = img;
    return KAAMER_OK;
}

extern "C" {

uint32_t kaamer_shard_of(uint32_t key, uint32_t n_shards)
{
    return n_shards <= 1 ? 0 : kh_shard_of(key, n_shards);
}

uint32_t kaamer_encode_kmer(const uint8_t kmer[KAAMER_KMER_SIZE])
{
    return kh_key_from_codes(kh_residue_code(kmer[0]), kh_residue_code(kmer[1]), kh_residue_code(kmer[2]),
                             kh_residue_code(kmer[3]), kh_residue_code(kmer[4]), kh_residue_code(kmer[5]),
                             kh_residue_code(kmer[6]));
}

int kaamer_image_build_pairs(const kaamer_pair *pairs, uint64_t n, uint32_t shard, uint32_t n_shards,
                             double load_factor, kaamer_image **out)
{
    if (!out || (!pairs && n) || n_shards == 0 || shard >= n_shards) return kaamer_fail(KAAMER_E_ARG, "build_pairs: bad argument");
    *out = nullptr;
    uint64_t *p64 = (uint64_t *)malloc((n ? n : 1) * sizeof(uint64_t));
    if (!p64) return kaamer_fail(KAAMER_E_NOMEM, "pairs buffer");
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (pairs[i].key == KH_EMPTY_KEY || pairs[i].protein_id == KH_EMPTY_PID) {
            free(p64);
            return kaamer_fail(KAAMER_E_ARG, "key/id 0xFFFFFFFF is reserved");
        }
        if (n_shards > 1 && kh_shard_of(pairs[i].key, n_shards) != shard) continue;
        p64[m++] = ((uint64_t)pairs[i].key << 32) | pairs[i].protein_id;
    }
    // a pair stands for a window; the windows' order is the order of the pairs
    const RankFill by_input_order = [&](const KeyIndex &ki, std::atomic<uint64_t> *rank) {
        parallel_for(n, n_threads(), [&](size_t b, size_t e, unsigned) {
            for (size_t i = b; i < e; i++) {
                if (n_shards > 1 && kh_shard_of(pairs[i].key, n_shards) != shard) continue;
                atomic_min(rank[ki.find(pairs[i].key)], i);
            }
        });
    };
    int rc = build_from_sorted_input(p64, m, shard, n_shards, load_factor, by_input_order, out);
    free(p64);
    return rc;
}

int kaamer_image_build_proteins(const uint8_t *seqs, const uint64_t *offsets, const uint32_t *ids,
                                uint32_t n_proteins, uint32_t shard, uint32_t n_shards,
                                double load_factor, kaamer_image **out)
{
    if (!out || !offsets || (!seqs && n_proteins) || n_shards == 0 || shard >= n_shards)
        return kaamer_fail(KAAMER_E_ARG, "build_proteins: bad argument");
    *out = nullptr;
    // Two passes over the proteins, both parallel: (1) windows per protein that belong to THIS shard,
    // (2) emit exactly those.  The pair buffer is therefore O(shard), not O(database): a database of
    // W windows in S shards needs 8 W / S bytes here (+ the same again inside the sort).
    auto for_windows = [&](size_t p, auto &&f) {
        const uint8_t *s = seqs + offsets[p];
        const uint64_t len = offsets[p + 1] - offsets[p];
        if (len < KAAMER_KMER_SIZE) return;                                  // inputFASTA.go:228, inputTSV.go:139
        const uint64_t nw = len - KAAMER_KMER_SIZE + 1;                      // inputFASTA.go:245, inputTSV.go:236
        uint32_t c[7];
        for (int t = 0; t < 6; t++) c[t + 1] = kh_residue_code(s[t]);
        for (uint64_t i = 0; i < nw; i++) {
            for (int t = 0; t < 6; t++) c[t] = c[t + 1];
            c[6] = kh_residue_code(s[i + 6]);
            const uint32_t key = kh_key_from_codes(c[0], c[1], c[2], c[3], c[4], c[5], c[6]);
            if (n_shards > 1 && kh_shard_of(key, n_shards) != shard) continue;
            f(key, i);
        }
    };
    std::vector<uint64_t> woff((size_t)n_proteins + 1, 0);
    std::atomic<int> bad(0);
    parallel_for(n_proteins, n_threads(), [&](size_t b, size_t e, unsigned) {
        for (size_t p = b; p < e; p++) {
            const uint32_t id = ids ? ids[p] : (uint32_t)p;  // inputTSV.go:141-142
            if (id == KH_EMPTY_PID) { bad = 1; continue; }
            if (n_shards == 1) {
                const uint64_t len = offsets[p + 1] - offsets[p];
                woff[p + 1] = len >= KAAMER_KMER_SIZE ? len - KAAMER_KMER_SIZE + 1 : 0;
            } else {
                uint64_t k = 0;
                for_windows(p, [&](uint32_t, uint64_t) { k++; });
                woff[p + 1] = k;
            }
        }
    });
    if (bad) return kaamer_fail(KAAMER_E_ARG, "protein id 0xFFFFFFFF is reserved");
    for (uint32_t p = 0; p < n_proteins; p++) woff[p + 1] += woff[p];
    const uint64_t total = woff[n_proteins];
    uint64_t *p64 = (uint64_t *)malloc((total ? total : 1) * sizeof(uint64_t));
    if (!p64) return kaamer_fail(KAAMER_E_NOMEM, "pairs buffer (%llu pairs)", (unsigned long long)total);
    parallel_for(n_proteins, n_threads(), [&](size_t b, size_t e, unsigned) {
        for (size_t p = b; p < e; p++) {
            const uint32_t id = ids ? ids[p] : (uint32_t)p;
            uint64_t *w = p64 + woff[p];
            for_windows(p, [&](uint32_t key, uint64_t) { *w++ = ((uint64_t)key << 32) | id; });
        }
    });
    // window index = absolute residue position of the window: proteins in input order, positions ascending
    const RankFill by_walk = [&](const KeyIndex &ki, std::atomic<uint64_t> *rank) {
        parallel_for(n_proteins, n_threads(), [&](size_t b, size_t e, unsigned) {
            for (size_t p = b; p < e; p++) {
                const uint64_t at = offsets[p];
                for_windows(p, [&](uint32_t key, uint64_t i) { atomic_min(rank[ki.find(key)], at + i); });
            }
        });
    };
    int rc = build_from_sorted_input(p64, total, shard, n_shards, load_factor, by_walk, out);
    free(p64);
    return rc;
}

}  // extern "C"

// What both merge forms check before anything is dereferenced: the inputs agree on shard, n_shards, kmer_size and version,
// and every list reference stays inside its image's arena.  n_pairs[i] = the number of pairs image i enumerates.
int kaamer_merge_check(const kaamer_image *const *imgs, uint32_t n, uint64_t *n_pairs)
{
    if (!imgs || n == 0) return kaamer_fail(KAAMER_E_ARG, "image_merge: no input");
    for (uint32_t i = 0; i < n; i++) {
        if (!imgs[i] || !imgs[i]->buckets || !imgs[i]->arena) return kaamer_fail(KAAMER_E_ARG, "image_merge: input %u is null", i);
        const kh_image_header &h = imgs[i]->hdr, &h0 = imgs[0]->hdr;
        if (h.version != KH_IMAGE_VERSION || h.kmer_size != KAAMER_KMER_SIZE || h.n_shards == 0 || h.shard >= h.n_shards ||
            h.n_buckets == 0 || h.n_buckets >= (1ull << 32) || h.arena_words < 4)
            return kaamer_fail(KAAMER_E_ARG, "image_merge: input %u is not an image of this layout", i);
        if (h.shard != h0.shard || h.n_shards != h0.n_shards || h.kmer_size != h0.kmer_size || h.version != h0.version)
            return kaamer_fail(KAAMER_E_ARG, "image_merge: input %u is shard %u of %u, input 0 is shard %u of %u", i, h.shard, h.n_shards,
                               h0.shard, h0.n_shards);
        const uint64_t nb = h.n_buckets, aw = h.arena_words;
        const unsigned nt = n_threads();
        std::vector<uint64_t> part(nt, 0);
        std::atomic<int> bad_ref(0);
        parallel_for((size_t)nb, nt, [&](size_t b0, size_t b1, unsigned t) {
            uint64_t c = 0;
            for (size_t b = b0; b < b1; b++)
                for (int s = 0; s < KH_SLOTS_PER_BUCKET; s++) {
                    const kh_slot &sl = imgs[i]->buckets[b].s[s];
                    if (sl.key == KH_EMPTY_KEY) continue;
                    if (sl.val & KH_INLINE_BIT) { c++; continue; }
                    const uint64_t off = (uint64_t)sl.val * 4;
                    if (sl.val == 0 || off + 1 > aw || off + 1 + imgs[i]->arena[off] > aw) { bad_ref = 1; continue; }
                    c += imgs[i]->arena[off];
                }
            part[t] += c;
        });
        if (bad_ref) return kaamer_fail(KAAMER_E_ARG, "image_merge: input %u: postings reference out of range", i);
        n_pairs[i] = 0;
        for (uint64_t c : part) n_pairs[i] += c;
    }
    return KAAMER_OK;
}

extern "C" {

// mergedb.go:42-135 (kmer_store leg) + indexdb.go:68-132 over the union.  The merged image is
// kaamer_image_build_pairs(E(img_0) ++ E(img_1) ++ ...): E(img) lists the keys that own a list by (offset, key) ascending,
// each with its ids in stored order, then the keys with an inline id by key ascending.  An image does not record which
// window first referred to a list, so the order of its arena is the only order a merge can keep.
int kaamer_image_merge(const kaamer_image *const *imgs, uint32_t n, double load_factor, kaamer_image **out)
{
    if (!out) return kaamer_fail(KAAMER_E_ARG, "image_merge: bad argument");
    *out = nullptr;
    std::vector<uint64_t> n_pairs(n ? n : 1, 0);
    int rc = kaamer_merge_check(imgs, n, n_pairs.data());
    if (rc) return rc;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += n_pairs[i];
    if (total >= 0xFFFFFFFFull) return kaamer_fail(KAAMER_E_CAPACITY, "image_merge: %llu pairs in one shard; use more shards", (unsigned long long)total);
    uint64_t *p64 = (uint64_t *)malloc((total ? total : 1) * sizeof(uint64_t));
    if (!p64) return kaamer_fail(KAAMER_E_NOMEM, "pairs buffer");
    struct First { uint32_t key; uint64_t at; };   // a key of one input and the index of its first pair in the enumeration
    std::vector<First> firsts;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const kaamer_image *img = imgs[i];
        std::vector<uint64_t> lists, inl;   // offset << 32 | key;  key << 32 | id
        for (uint64_t b = 0; b < img->hdr.n_buckets; b++)
            for (int s = 0; s < KH_SLOTS_PER_BUCKET; s++) {
                const kh_slot &sl = img->buckets[b].s[s];
                if (sl.key == KH_EMPTY_KEY) continue;
                if (sl.val & KH_INLINE_BIT) inl.push_back(((uint64_t)sl.key << 32) | (sl.val & ~KH_INLINE_BIT));
                else lists.push_back(((uint64_t)sl.val << 32) | sl.key);
            }
        sort_u64(lists.data(), lists.size());
        sort_u64(inl.data(), inl.size());
        for (uint64_t w : lists) {
            const uint32_t key = (uint32_t)w, *l = img->arena + (w >> 32) * 4;
            firsts.push_back(First{ key, at });
            for (uint32_t t = 0; t < l[0]; t++) p64[at++] = ((uint64_t)key << 32) | l[1 + t];
        }
        for (uint64_t w : inl) {
            firsts.push_back(First{ (uint32_t)(w >> 32), at });
            p64[at++] = w;
        }
    }
    const RankFill by_enumeration = [&](const KeyIndex &ki, std::atomic<uint64_t> *rank) {
        parallel_for(firsts.size(), n_threads(), [&](size_t b, size_t e, unsigned) {
            for (size_t i = b; i < e; i++) atomic_min(rank[ki.find(firsts[i].key)], firsts[i].at);
        });
    };
    rc = build_from_sorted_input(p64, total, imgs[0]->hdr.shard, imgs[0]->hdr.n_shards, load_factor, by_enumeration, out);
    free(p64);
    return rc;
}

double kaamer_image_load_factor(const kaamer_image *img) { return img ? img->hdr.load_factor : 0.0; }

int kaamer_image_save(const kaamer_image *img, const char *path)
{
    if (!img || !path) return kaamer_fail(KAAMER_E_ARG, "image_save: bad argument");
    FILE *f = fopen(path, "wb");
    if (!f) return kaamer_fail(KAAMER_E_IO, "cannot open for writing");
    bool ok = fwrite(&img->hdr, sizeof img->hdr, 1, f) == 1;
    ok = ok && fwrite(img->buckets, sizeof(kh_bucket), (size_t)img->hdr.n_buckets, f) == img->hdr.n_buckets;
    ok = ok && fwrite(img->arena, 4, (size_t)img->hdr.arena_words, f) == img->hdr.arena_words;
    ok = (fclose(f) == 0) && ok;
    return ok ? KAAMER_OK : kaamer_fail(KAAMER_E_IO, "short write");
}

int kaamer_image_load(const char *path, kaamer_image **out)
{
    if (!path || !out) return kaamer_fail(KAAMER_E_ARG, "image_load: bad argument");
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) return kaamer_fail(KAAMER_E_IO, "cannot open index image");
    kaamer_image *img = new (std::nothrow) kaamer_image();
    if (!img) { fclose(f); return kaamer_fail(KAAMER_E_NOMEM, "image alloc"); }
    img->buckets = nullptr;
    img->arena = nullptr;
    if (fread(&img->hdr, sizeof img->hdr, 1, f) != 1) { fclose(f); delete img; return kaamer_fail(KAAMER_E_IO, "short header"); }
    if (img->hdr.magic != KH_IMAGE_MAGIC || img->hdr.version != KH_IMAGE_VERSION || img->hdr.kmer_size != KAAMER_KMER_SIZE) {
        fclose(f); delete img;
        return kaamer_fail(KAAMER_E_FORMAT, "not a kaamer GPU index image (magic/version)");
    }
    uint64_t nb = img->hdr.n_buckets, aw = img->hdr.arena_words;
    // the header drives allocations and device-side indexing: validate it against the file
    {
        const long here = ftell(f);
        bool sane = nb >= 1 && nb < (1ull << 32) && aw >= 4 && aw / 4 < KH_INLINE_BIT && img->hdr.n_shards >= 1 &&
                    img->hdr.shard < img->hdr.n_shards && here == (long)sizeof img->hdr;
        if (sane && fseek(f, 0, SEEK_END) == 0) {
            const long long size = ftell(f);
            sane = size == (long long)(sizeof img->hdr + nb * sizeof(kh_bucket) + aw * 4);
            fseek(f, here, SEEK_SET);
        } else sane = false;
        if (!sane) { fclose(f); delete img; return kaamer_fail(KAAMER_E_FORMAT, "index image header does not match the file"); }
    }
    int rc = kaamer_image_alloc(img, nb, aw);
    if (rc) { fclose(f); kaamer_image_free(img); return kaamer_fail(rc, "image buffers"); }
    bool ok = fread(img->buckets, sizeof(kh_bucket), (size_t)nb, f) == nb;
    ok = ok && fread(img->arena, 4, (size_t)aw, f) == aw;
    fclose(f);
    if (!ok) { kaamer_image_free(img); return kaamer_fail(KAAMER_E_IO, "short read"); }
    // every list reference must stay inside the arena (a corrupted image must not make the kernels read
    // outside the device allocation)
    {
        std::atomic<int> bad_ref(0);
        parallel_for((size_t)nb, n_threads(), [&](size_t b0, size_t b1, unsigned) {
            for (size_t b = b0; b < b1; b++)
                for (int c = 0; c < KH_SLOTS_PER_BUCKET; c++) {
                    const kh_slot &sl = img->buckets[b].s[c];
                    if (sl.key == KH_EMPTY_KEY || (sl.val & KH_INLINE_BIT)) continue;
                    const uint64_t off = (uint64_t)sl.val * 4;
                    if (sl.val == 0 || off + 1 > aw || off + 1 + img->arena[off] > aw) bad_ref = 1;
                }
        });
        if (bad_ref) { kaamer_image_free(img); return kaamer_fail(KAAMER_E_FORMAT, "index image: postings reference out of range"); }
    }
    *out = img;
    return KAAMER_OK;
}

static void fill_stats(const kh_image_header &h, kaamer_image_stats *s)
{
    memset(s, 0, sizeof *s);
    s->n_pairs = h.n_pairs; s->n_keys = h.n_keys; s->n_buckets = h.n_buckets;
    s->arena_words = h.arena_words; s->n_inline = h.n_inline; s->n_lists = h.n_lists;
    s->max_list = h.max_list; s->n_displaced = h.n_displaced; s->shard = h.shard;
    s->n_shards = h.n_shards; s->max_protein_id = h.max_protein_id;
}

int kaamer_image_get_stats(const kaamer_image *img, kaamer_image_stats *out)
{
    if (!img || !out) return kaamer_fail(KAAMER_E_ARG, "image_get_stats: bad argument");
    fill_stats(img->hdr, out);
    return KAAMER_OK;
}

void kaamer_stats_from_header(const kh_image_header *h, kaamer_image_stats *out) { fill_stats(*h, out); }

void kaamer_image_free(kaamer_image *img)
{
    if (!img) return;
    free(img->buckets);
    free(img->arena);
    delete img;
}

uint32_t kaamer_image_get(const kaamer_image *img, uint32_t key, uint32_t *ids, uint32_t cap)
{
    if (!img || img->hdr.n_buckets == 0) return 0;
    if (img->hdr.n_shards > 1 && kh_shard_of(key, img->hdr.n_shards) != img->hdr.shard) return 0;
    uint64_t nb = img->hdr.n_buckets, b = kh_home_bucket(key, img->hdr.n_shards, nb);
    for (uint64_t tries = 0; tries < nb; tries++) {
        const kh_bucket &bk = img->buckets[b];
        bool has_empty = false;
        for (int s = 0; s < KH_SLOTS_PER_BUCKET; s++) {
            if (bk.s[s].key == key) {
                uint32_t v = bk.s[s].val;
                if (v & KH_INLINE_BIT) { if (ids && cap) ids[0] = v & ~KH_INLINE_BIT; return 1; }
                const uint32_t *l = img->arena + (uint64_t)v * 4;
                for (uint32_t t = 0; t < l[0] && t < cap && ids; t++) ids[t] = l[1 + t];
                return l[0];
            }
            if (bk.s[s].key == KH_EMPTY_KEY) has_empty = true;
        }
        if (has_empty) return 0;
        b = (b + 1 == nb) ? 0 : b + 1;
    }
    return 0;
}

// Re-lays the postings lists of `img` in the order in which a walk over the proteins (input order) and their windows
// (ascending position) first meets them: the order both builders produce, so on an image they built from these proteins
// it reproduces the image.  On an image file of an older build (lists in ascending-key order, same format) it gives the
// new order.  bench.py calls it under KAAMER_EXP_ARENA_ORDER=2; not declared in the public header.
int kaamer_exp_relayout_first_touch(kaamer_image *img, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_proteins)
{
    if (!img || !offsets || (!seqs && n_proteins)) return kaamer_fail(KAAMER_E_ARG, "exp_relayout: bad argument");
    const uint64_t units = img->hdr.arena_words / 4;
    std::vector<uint32_t> new_off((size_t)units + 1, 0u);
    std::vector<uint32_t> out((size_t)img->hdr.arena_words, 0u);
    uint32_t cur = 1;
    const uint64_t nb = img->hdr.n_buckets;
    auto place = [&](uint32_t old) {
        if (new_off[old]) return;
        const uint32_t cnt = img->arena[(uint64_t)old * 4], u = (1u + cnt + 3u) / 4u;
        memcpy(&out[(size_t)cur * 4], &img->arena[(size_t)old * 4], (size_t)u * 16);
        new_off[old] = cur;
        cur += u;
    };
    for (uint32_t p = 0; p < n_proteins; p++) {
        const uint8_t *s = seqs + offsets[p];
        const uint64_t len = offsets[p + 1] - offsets[p];
        for (uint64_t i = 0; i + KAAMER_KMER_SIZE <= len; i++) {
            const uint32_t key = kaamer_encode_kmer(s + i);
            if (img->hdr.n_shards > 1 && kh_shard_of(key, img->hdr.n_shards) != img->hdr.shard) continue;
            uint64_t b = kh_home_bucket(key, img->hdr.n_shards, nb);
            for (uint64_t tries = 0; tries < nb; tries++) {
                const kh_bucket &bk = img->buckets[b];
                bool done = false, has_empty = false;
                for (int t = 0; t < KH_SLOTS_PER_BUCKET; t++) {
                    if (bk.s[t].key == key) { if (!(bk.s[t].val & KH_INLINE_BIT) && bk.s[t].val) place(bk.s[t].val); done = true; break; }
                    if (bk.s[t].key == KH_EMPTY_KEY) has_empty = true;
                }
                if (done || has_empty) break;
                b = (b + 1 == nb) ? 0 : b + 1;
            }
        }
    }
    for (uint64_t b = 0; b < nb; b++)   // (lists no window reached: none, every key came from a window; kept for safety)
        for (int t = 0; t < KH_SLOTS_PER_BUCKET; t++) {
            kh_slot &sl = img->buckets[b].s[t];
            if (sl.key != KH_EMPTY_KEY && !(sl.val & KH_INLINE_BIT) && sl.val) { place(sl.val); sl.val = new_off[sl.val]; }
        }
    memcpy(img->arena, out.data(), (size_t)img->hdr.arena_words * 4);
    return KAAMER_OK;
}

}  // extern "C"
