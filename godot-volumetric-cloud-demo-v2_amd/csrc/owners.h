// owners.h -- the one place that knows how a GPU resource of the host layer dies: four move-only owners of a device buffer, a pinned host
// buffer, an event and a stream.  Each converts implicitly to the raw handle, so call sites read as they did with raw pointers; each releases
// its handle in its destructor, ignoring the result, and makes no HIP call when it is empty.  The caller has the owning device current and has
// waited for the work that may still use the resource (csky_destroy, csky_multi_destroy) before an owner dies.  Errors go through fail().
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include "../../include/cloudsky_internal.h"

struct csky_ctx;

namespace csky {

// writes the error text into c->err (g_err when c is NULL) and returns `code` (api.cpp)
int fail(csky_ctx* c, int code, const char* fmt, ...);
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail((c), CSKY_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

// Memory: a T* and its element count, which is the one capacity a grow-only buffer has.  DevBuf<T> is device memory; PinnedBuf is page-locked host
// memory (a device-to-host copy into it is a real asynchronous DMA), counted in bytes.
template <class T, bool PINNED> class Buf {
    T* p_ = nullptr; size_t n_ = 0;
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf& operator=(Buf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
    ~Buf() { reset(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }                              // for reinterpret_cast, which looks through no conversion
    size_t count() const { return n_; }
    void reset() { if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; n_ = 0; }
    // exactly n elements.  The old buffer goes BEFORE the new one is asked for: the largest buffers (the exact cells, ~150 MB) must not exist twice.
    // A failure leaves the owner empty.
    int alloc(csky_ctx* c, size_t n) {
        reset();
        void* q = nullptr;
        if (PINNED) HIPCHK(c, hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault));
        else HIPCHK(c, hipMalloc(&q, n * sizeof(T)));
        p_ = static_cast<T*>(q); n_ = n;
        return CSKY_OK;
    }
    int grow(csky_ctx* c, size_t n) { return (p_ && n_ >= n) ? CSKY_OK : alloc(c, n); }
};
template <class T> using DevBuf = Buf<T, false>;
using PinnedBuf = Buf<unsigned char, true>;

class Event {
    hipEvent_t ev_ = nullptr;
public:
    Event() = default;
    Event(Event&& o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); ev_ = o.ev_; o.ev_ = nullptr; } return *this; }
    ~Event() { reset(); }
    operator hipEvent_t() const { return ev_; }
    void reset() { if (ev_) (void)hipEventDestroy(ev_); ev_ = nullptr; }
    int create(csky_ctx* c, unsigned flags) {                  // hipEventDefault: a timing event
        reset();
        if (flags == hipEventDefault) HIPCHK(c, hipEventCreate(&ev_));
        else HIPCHK(c, hipEventCreateWithFlags(&ev_, flags));
        return CSKY_OK;
    }
};

class Stream {
    hipStream_t s_ = nullptr;
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
    ~Stream() { reset(); }
    operator hipStream_t() const { return s_; }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    int create(csky_ctx* c, unsigned flags) {
        reset();
        HIPCHK(c, hipStreamCreateWithFlags(&s_, flags));
        return CSKY_OK;
    }
};

}  // namespace csky
