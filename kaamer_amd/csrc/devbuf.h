// devbuf.h — the buffers the search side owns on the device and in pinned host memory: one owning type, one growth
// function, one all-or-nothing group.  The including file provides the HIP runtime (hipMalloc, hipFree, hipHostMalloc,
// hipHostFree, hipStreamSynchronize, hipError_t, hipStream_t) and
//     int devbuf_fail(hipError_t e, size_t bytes);   // the nonzero code of a refused allocation (bytes = 0: a failed wait)
// before this header: the library includes <hip/hip_runtime.h>, the host test a counting fake.
#pragma once
#include <stddef.h>

#include <initializer_list>

// pointer and capacity (in elements) of one allocation; what the typed buffers below own
struct BufBase {
    void *p = nullptr;
    size_t cap = 0;
};

// where a buffer lives: device memory, or pinned host memory (PINNED_PORTABLE: pinned for every device's copies)
enum class Mem { DEVICE, PINNED, PINNED_PORTABLE };
static inline void mem_free_(Mem m, void *p)
{
    if (m == Mem::DEVICE) (void)hipFree(p);
    else (void)hipHostFree(p);
}

// A typed, move-only buffer: the destructor frees, release() hands the pointer on.  It converts to T *, so parameter
// structs and kernel launches keep taking raw pointers.
template <class T, Mem MEM> class Buf : private BufBase {
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept { p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { reset(); }
    operator T *() const { return (T *)p; }
    T *get() const { return (T *)p; }
    size_t capacity() const { return cap; }
    void reset()
    {
        if (p) mem_free_(MEM, p);
        p = nullptr; cap = 0;
    }
    T *release() { T *r = (T *)p; p = nullptr; cap = 0; return r; }
    BufBase &base() { return *this; }
};
template <class T> using DevBuf = Buf<T, Mem::DEVICE>;
template <class T> using PinnedBuf = Buf<T, Mem::PINNED>;

// When a buffer is made again and how large.  EXACT: whenever it is missing or holds fewer than `need` elements, for
// exactly `need`.  grow_quarter(extra, pad): when it holds fewer than need + pad, for need + need / 4 + extra (a buffer
// that is missing stays missing while need + pad is 0).
struct GrowRule { bool quarter; size_t extra, pad; };
static constexpr GrowRule GROW_EXACT = { false, 0, 0 };
static constexpr GrowRule grow_quarter(size_t extra, size_t pad = 0) { return { true, extra, pad }; }
static inline size_t grow_capacity(GrowRule r, size_t need) { return r.quarter ? need + need / 4 + r.extra : need; }

// one member of a group: the buffer, the elements asked for, the element size
struct BufWant { BufBase *b; size_t n, elem; Mem mem; };
template <class T, Mem MEM> static inline BufWant want(Buf<T, MEM> &b, size_t n) { return { &b.base(), n, sizeof(T), MEM }; }

static inline void buf_drop_(const BufWant &w)
{
    if (w.b->p) mem_free_(w.mem, w.b->p);
    w.b->p = nullptr; w.b->cap = 0;
}

// The buffers of `group` by one rule.  When each of them passes the rule's test nothing happens.  Otherwise the whole group
// is made again, once `s` is done with the old ones (one wait, and none when there were no old ones).  Either all end up
// at least as large as asked, or -- the wait or an allocation refused -- the error is returned and all of them are null
// with capacity 0 (after a refused wait: left as they were).
static inline int reserve_group(hipStream_t s, GrowRule rule, std::initializer_list<BufWant> group)
{
    bool fits = true, used = false;
    for (const BufWant &w : group) {
        fits = fits && (w.b->p || rule.quarter) && w.b->cap >= w.n + rule.pad;
        used = used || w.b->p;
    }
    if (fits) return 0;
    if (used) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return devbuf_fail(e, 0);
    }
    for (const BufWant &w : group) buf_drop_(w);
    for (const BufWant &w : group) {
        const size_t n = grow_capacity(rule, w.n), bytes = (n ? n : 1) * w.elem;
        const hipError_t e = w.mem == Mem::DEVICE ? hipMalloc(&w.b->p, bytes)
                                                  : hipHostMalloc(&w.b->p, bytes, w.mem == Mem::PINNED ? hipHostMallocDefault : hipHostMallocPortable);
        if (e != hipSuccess) {
            w.b->p = nullptr;
            for (const BufWant &v : group) buf_drop_(v);
            return devbuf_fail(e, bytes);
        }
        w.b->cap = n;
    }
    return 0;
}

// one buffer: a group of one
template <class T, Mem MEM> static inline int reserve(Buf<T, MEM> &b, size_t need, GrowRule rule, hipStream_t s)
{
    return reserve_group(s, rule, { want(b, need) });
}
