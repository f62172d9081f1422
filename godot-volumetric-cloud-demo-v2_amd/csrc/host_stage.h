// host_stage.h -- the device memory the blocking host forms work in, and the one way through it.  A blocking form uploads the caller's arrays,
// enqueues what its _device form enqueues, copies the result out and waits, all on the context's stream.  It owns its scratch only until it returns,
// so every such form shares ONE grow-only buffer (csky_ctx::stage): a context holds the largest call's bytes, not the sum over the features it has
// used.  A call names the sizes of its regions once (HostCall's constructor: stage_layout, then one grow), then: up() its inputs, step() with the
// internal launch its _device form makes, down() the result, return finish().  Every step after the first error is skipped, and finish() waits for
// the stream whenever this call has enqueued anything, whatever failed: a caller that gets an error back may free its arrays at once.
#pragma once
#include <cstdint>
#include <initializer_list>
#include "owners.h"

namespace csky {

constexpr size_t STAGE_ALIGN = 256;       // what hipMalloc guarantees: a region is aligned at least as well as the allocation it replaces
constexpr int STAGE_MAX_REGIONS = 5;      // four input images and the output (the compositor, the radiance cubemap)

// Offsets of n regions of bytes[i] bytes, in order, each on a STAGE_ALIGN boundary, and total = off[n - 1] + bytes[n - 1].  A region of 0 bytes takes
// nothing: the next one begins where it does.  Pure (no HIP call or type).  CSKY_ERR_INVALID: n out of range, or the sum does not fit in size_t.
inline int stage_layout(const size_t* bytes, int n, size_t* off, size_t& total) {
    total = 0;
    if (n < 1 || n > STAGE_MAX_REGIONS) return CSKY_ERR_INVALID;
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        const size_t pad = (STAGE_ALIGN - at % STAGE_ALIGN) % STAGE_ALIGN;
        if (pad > SIZE_MAX - at || bytes[i] > SIZE_MAX - at - pad) return CSKY_ERR_INVALID;
        off[i] = at + pad; at = off[i] + bytes[i];
    }
    total = at;
    return CSKY_OK;
}

// The owner: grow-only, exactly the largest total asked for so far.  What lies where in it is the business of the call that is using it.
struct HostStage { DevBuf<uint8_t> d; };

// One blocking call `fn` with regions of `bytes` on stream s (the context's).  rc is the first error; a step that finds one set does nothing.
struct HostCall {
    csky_ctx* c; HostStage& st; hipStream_t s; int rc; bool enqueued = false; size_t off[STAGE_MAX_REGIONS] = {};
    HostCall(csky_ctx* c_, HostStage& st_, hipStream_t s_, const char* fn, std::initializer_list<size_t> bytes) : c(c_), st(st_), s(s_) {
        size_t total;
        if (stage_layout(bytes.begin(), (int)bytes.size(), off, total)) rc = fail(c, CSKY_ERR_INVALID, "%s: the sizes of the call's buffers overflow size_t", fn);
        else rc = total ? st.d.grow(c, total) : CSKY_OK;
    }
    template <class T> T* at(int region) const { return reinterpret_cast<T*>(st.d.get() + off[region]); }
    // host memory -> a region, and a region -> host memory, from the region's start.  0 bytes: nothing (the radiance form's optional inputs)
    int up(int region, const void* src, size_t bytes) { return (rc || !bytes) ? rc : (rc = copy(at<uint8_t>(region), src, bytes, hipMemcpyHostToDevice)); }
    int down(void* dst, int region, size_t bytes) { return (rc || !bytes) ? rc : (rc = copy(dst, at<uint8_t>(region), bytes, hipMemcpyDeviceToHost)); }
    // what the _device form enqueues, given this call's stream: returns a CSKY code with the context's error text set.  It may have enqueued part of
    // its work before it failed, so it counts as enqueued either way.
    template <class F> int step(F enqueue) { if (rc) return rc; enqueued = true; return rc = enqueue(); }
    // the wait every blocking form ends with, and the first error.  An error of the wait itself never replaces an earlier one's text.
    int finish() {
        if (!enqueued) return rc;
        const hipError_t e = hipStreamSynchronize(s);
        if (rc == CSKY_OK && e != hipSuccess) rc = fail(c, CSKY_ERR_HIP, "hipStreamSynchronize(c->stream) failed: %s", hipGetErrorString(e));
        return rc;
    }
private:
    int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, kind, s)); enqueued = true; return CSKY_OK; }
};

}  // namespace csky
