// Host test of kaamer_amd/csrc/devbuf.h against a counting fake of the HIP calls it makes: the growth rules' capacities,
// the all-or-nothing group, move / reset / scope-exit frees and the stream wait.  No HIP runtime, no library.
// Built with -fsanitize=address,undefined and run by tests/test_devbuf_host.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <utility>
#include <vector>

// ---- the fake runtime -------------------------------------------------------------------------------------------------------
typedef int hipError_t;
typedef struct FakeStream *hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum { hipHostMallocDefault = 0, hipHostMallocPortable = 1 };

struct Fake {
    std::map<void *, std::pair<size_t, int>> live;   // pointer -> (bytes, kind: 0 device, 1 pinned, 2 pinned portable)
    std::vector<size_t> sizes;                       // bytes of every allocation asked for, in order
    std::vector<hipStream_t> waits;                  // the stream of every wait
    long n_alloc = 0, fail_at = -1;                  // fail_at: the allocation call (counted from 0) that is refused
    long n_free = 0, bad_free = 0;
} g;

static hipError_t fake_alloc(void **p, size_t bytes, int kind)
{
    g.sizes.push_back(bytes);
    if (g.n_alloc++ == g.fail_at) { *p = (void *)0x1; return hipErrorOutOfMemory; }   // (garbage: the header must not keep it)
    *p = malloc(1);   // a distinct address; 2^32 + 1 elements are asked for, never touched
    g.live[*p] = { bytes, kind };
    return hipSuccess;
}
static hipError_t fake_free(void *p, bool pinned)
{
    auto it = g.live.find(p);
    if (it == g.live.end() || (it->second.second != 0) != pinned) { g.bad_free++; return hipSuccess; }
    g.live.erase(it);
    g.n_free++;
    free(p);
    return hipSuccess;
}
static hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(p, bytes, 0); }
static hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) { return fake_alloc(p, bytes, flags == hipHostMallocPortable ? 2 : 1); }
static hipError_t hipFree(void *p) { return fake_free(p, false); }
static hipError_t hipHostFree(void *p) { return fake_free(p, true); }
static hipError_t hipStreamSynchronize(hipStream_t s) { g.waits.push_back(s); return hipSuccess; }
static int devbuf_fail(hipError_t e, size_t bytes) { (void)bytes; return 1000 + e; }

#include "../kaamer_amd/csrc/devbuf.h"

static int n_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { n_failed++; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static hipStream_t const S1 = (hipStream_t)0x10, S2 = (hipStream_t)0x20;
static const size_t NEEDS[] = { 0, 1, 63, 64, 4095, 4096, ((size_t)1 << 32) + 1 };

// (a) one fresh buffer of T by `rule` for `need`: the capacity and the bytes the old helper allocated, or nothing at all
template <class T, Mem MEM> static void fresh(GrowRule rule, size_t need, bool allocates, size_t cap, size_t bytes)
{
    const size_t before = g.sizes.size();
    {
        Buf<T, MEM> b;
        CHECK(reserve(b, need, rule, S1) == 0);
        CHECK(b.capacity() == cap);
        CHECK((b.get() != nullptr) == allocates);
        CHECK(g.sizes.size() == before + (allocates ? 1 : 0));
        if (allocates) {
            CHECK(g.sizes.back() == bytes);
            CHECK(g.live[b.get()].second == (MEM == Mem::DEVICE ? 0 : MEM == Mem::PINNED ? 1 : 2));
        }
        // (b) at or below the capacity nothing is allocated
        const size_t n = g.sizes.size();
        T *const p = b;
        CHECK(reserve(b, need, rule, S1) == 0);
        if (cap >= rule.pad) CHECK(reserve(b, cap - rule.pad, rule, S1) == 0);
        if (need) CHECK(reserve(b, need - 1, rule, S1) == 0);
        CHECK(g.sizes.size() == n && b.get() == p && b.capacity() == cap);
    }
    CHECK(g.live.empty());
    CHECK(g.waits.empty());   // nothing was there before: no wait
}

static void test_rules()
{
    for (size_t need : NEEDS) {
        // dev_grow: made when cap < need, for need + need / 4 + 64
        fresh<uint64_t, Mem::DEVICE>(grow_quarter(64), need, need > 0, need > 0 ? need + need / 4 + 64 : 0, (need + need / 4 + 64) * 8);
        // slot_grow_dev without pad: made when cap < need, for need + need / 4 + 4096
        fresh<uint8_t, Mem::DEVICE>(grow_quarter(4096), need, need > 0, need > 0 ? need + need / 4 + 4096 : 0, need + need / 4 + 4096);
        // slot_grow_dev with pad 16 (the sequences of a slot): made when cap < need + 16
        fresh<uint8_t, Mem::DEVICE>(grow_quarter(4096, 16), need, true, need + need / 4 + 4096, need + need / 4 + 4096);
        // slot_grow_pinned: bytes, made when cap < need
        fresh<uint8_t, Mem::PINNED>(grow_quarter(4096), need, need > 0, need > 0 ? need + need / 4 + 4096 : 0, need + need / 4 + 4096);
        // the sharded set's staging: the same rule, portable
        fresh<uint8_t, Mem::PINNED_PORTABLE>(grow_quarter(4096), need, need > 0, need > 0 ? need + need / 4 + 4096 : 0, need + need / 4 + 4096);
        // the offsets of a slot: made when cap < n + 1, for n + n / 4 + 16
        fresh<uint64_t, Mem::DEVICE>(grow_quarter(16, 1), need, true, need + need / 4 + 16, (need + need / 4 + 16) * 8);
        // ta_grow, x_grow, dev_alloc: made when missing or cap < need, for exactly need (one element when need is 0)
        fresh<uint32_t, Mem::DEVICE>(GROW_EXACT, need, true, need, (need ? need : 1) * 4);
        fresh<uint64_t, Mem::PINNED>(GROW_EXACT, need, true, need, (need ? need : 1) * 8);
    }
}

struct Five {
    DevBuf<uint32_t> a, b;
    DevBuf<uint64_t> c, d, e;
    int reserve_all(hipStream_t s, size_t n) { return reserve_group(s, GROW_EXACT, { want(a, n), want(b, n), want(c, n + 1), want(d, n + 1), want(e, n + 1) }); }
    bool all_null() const { return !a && !b && !c && !d && !e && !a.capacity() && !b.capacity() && !c.capacity() && !d.capacity() && !e.capacity(); }
    bool all_set(size_t n) const { return a && b && c && d && e && a.capacity() == n && b.capacity() == n && c.capacity() == n + 1 && d.capacity() == n + 1 && e.capacity() == n + 1; }
};

// (c) a group of five with allocation k refused, from nothing and from a smaller group
static void test_group_failure()
{
    for (int from_full = 0; from_full < 2; from_full++)
        for (long k = 0; k < 5; k++) {
            Five f;
            if (from_full) { CHECK(f.reserve_all(S1, 10) == 0); CHECK(f.all_set(10)); }
            g.fail_at = g.n_alloc + k;
            CHECK(f.reserve_all(S1, 100) == 1000 + hipErrorOutOfMemory);
            g.fail_at = -1;
            CHECK(f.all_null());
            CHECK(g.live.empty());
            CHECK(f.reserve_all(S1, 100) == 0);   // the retry fills all five
            CHECK(f.all_set(100));
            CHECK(g.live.size() == 5);
        }
    CHECK(g.live.empty());
    g.waits.clear();
}

// (d) every way a buffer goes frees it exactly once
struct Slot {
    DevBuf<uint8_t> d;
    PinnedBuf<uint8_t> h;
    size_t n = 7;
};
static void test_ownership()
{
    const long f0 = g.n_free;
    {
        DevBuf<uint32_t> a;
        CHECK(reserve(a, 10, GROW_EXACT, S1) == 0);
        uint32_t *const pa = a;
        DevBuf<uint32_t> b(std::move(a));                   // move-construct: nothing freed, the source is empty
        CHECK(!a && a.capacity() == 0 && b.get() == pa && b.capacity() == 10 && g.n_free == f0);
        DevBuf<uint32_t> c;
        CHECK(reserve(c, 20, GROW_EXACT, S1) == 0);
        c = std::move(b);                                   // move-assign onto a full buffer: the old one is freed, once
        CHECK(g.n_free == f0 + 1 && c.get() == pa && c.capacity() == 10 && !b && g.live.size() == 1);
        c = std::move(c);                                   // (onto itself: nothing)
        CHECK(c.get() == pa && g.n_free == f0 + 1);
        uint32_t *const raw = c.release();                  // release: the caller's from here on
        CHECK(raw == pa && !c && c.capacity() == 0 && g.n_free == f0 + 1 && g.live.size() == 1);
        CHECK(hipFree(raw) == hipSuccess);
    }
    CHECK(g.n_free == f0 + 2 && g.live.empty());
    {
        Slot s;
        CHECK(reserve(s.d, 100, grow_quarter(4096, 16), S1) == 0);
        CHECK(reserve(s.h, 100, grow_quarter(4096), S1) == 0);
        s.n = 9;
        s = Slot();                                         // a struct reset frees both, once each
        CHECK(g.n_free == f0 + 4 && g.live.empty() && !s.d && !s.h && s.n == 7);
        CHECK(reserve(s.d, 1, GROW_EXACT, S1) == 0);
    }                                                       // scope exit
    CHECK(g.n_free == f0 + 5 && g.live.empty() && g.bad_free == 0);
    CHECK(g.waits.empty());
}

// (e) a regrow waits for the stream once per group, and only when something was there
static void test_waits()
{
    Five f;
    CHECK(f.reserve_all(S1, 10) == 0);
    CHECK(g.waits.empty());                                 // first use
    CHECK(f.reserve_all(S1, 10) == 0 && f.reserve_all(S1, 3) == 0);
    CHECK(g.waits.empty());                                 // fits
    CHECK(f.reserve_all(S2, 11) == 0);                      // one member short: the group is made again, one wait
    CHECK(g.waits.size() == 1 && g.waits[0] == S2 && g.live.size() == 5 && f.all_set(11));
    DevBuf<uint8_t> one;
    CHECK(reserve(one, 5, grow_quarter(64), S1) == 0);
    CHECK(g.waits.size() == 1);
    CHECK(reserve(one, 500, grow_quarter(64), S1) == 0);
    CHECK(g.waits.size() == 2 && g.waits[1] == S1 && one.capacity() == 500 + 125 + 64);
    // a group of which one member alone is there: still one wait
    DevBuf<uint8_t> x, y;
    CHECK(reserve(x, 5, GROW_EXACT, S1) == 0);
    CHECK(reserve_group(S2, GROW_EXACT, { want(x, 5), want(y, 5) }) == 0);
    CHECK(g.waits.size() == 3 && g.waits[2] == S2 && x.capacity() == 5 && y.capacity() == 5);
    g.waits.clear();
}

int main()
{
    test_rules();
    test_group_failure();
    test_ownership();
    test_waits();
    CHECK(g.live.empty());
    CHECK(g.bad_free == 0);
    if (n_failed) { fprintf(stderr, "devbuf_host: %d checks failed\n", n_failed); return 1; }
    printf("devbuf_host ok: %ld allocations, %ld frees\n", g.n_alloc, g.n_free);
    return 0;
}
