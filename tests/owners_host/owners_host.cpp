// TEST TOOL ONLY: the owner types of csrc/owners.h and the destruction of a real csky_ctx (csrc/context.h), run on the CPU.
// The HIP entry points the owners use are defined HERE as counting stubs: they hand out distinct fake handles (never dereferenced), refuse a release
// of a handle that is not live, and log every release in order.  No GPU call is made and the HIP runtime is not linked.
// Two pieces of the frame ring's and the timing pool's own code (context.h) run over the same stubs: the growth of the order tables and a pool growth
// that fails part-way.  So does the blocking host forms' staging (host_stage.h): its layout function, and a HostCall's way through the stage.
// Prints one "name value" line per figure and "FAIL: ..." per broken expectation; exit status 1 if any.  tests/test_owners_host.py checks both.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/context.h"

namespace {

enum Kind { DEV, PINNED, EVENT, STREAM, KINDS };                     // in g_calls a release is its kind + KINDS
// entries of g_calls ONLY, no kinds -- never an index of the arrays below: hipDeviceSynchronize; hipMemcpyAsync to and from the device,
// hipStreamSynchronize, and the mark a HostCall's enqueue step leaves when the test's own step runs
const Kind DEVICE_SYNC = static_cast<Kind>(2 * KINDS), COPY_UP = static_cast<Kind>(2 * KINDS + 1), COPY_DOWN = static_cast<Kind>(2 * KINDS + 2),
           STREAM_SYNC = static_cast<Kind>(2 * KINDS + 3), STEP = static_cast<Kind>(2 * KINDS + 4);
const char* const kind_name[KINDS] = {"dev", "pinned", "event", "stream"};
struct Release { Kind kind; void* handle; };

uintptr_t g_next = 0;
std::set<void*> g_live[KINDS];
std::vector<Release> g_log;            // every release, in order
std::vector<Kind> g_calls;             // every acquire (its kind) and release (its kind + KINDS), in order
long g_made[KINDS] = {}, g_bad_release = 0, g_last_error_calls = 0;
int g_fail_next_malloc = 0;
int g_fail_event_in = 0;                 // n > 0: the n-th event creation from here on fails
int g_fail_copy_in = 0;                  // n > 0: the n-th hipMemcpyAsync from here on fails
struct Copy { void* dst; const void* src; size_t bytes; hipStream_t s; };
std::vector<Copy> g_copies;            // every hipMemcpyAsync that succeeded, in order
hipStream_t g_synced = nullptr;        // the stream of the last hipStreamSynchronize
std::vector<size_t> g_malloc_bytes;    // of every hipMalloc that succeeded, in order
long g_device_syncs = 0;
int g_failures = 0;

hipError_t acquire(Kind k, void** out) {
    g_calls.push_back(k);
    void* h = reinterpret_cast<void*>(++g_next * 0x1000);
    g_live[k].insert(h); g_made[k]++;
    *out = h;
    return hipSuccess;
}
hipError_t release(Kind k, void* h) {
    g_calls.push_back(static_cast<Kind>(k + KINDS));
    if (!g_live[k].erase(h)) { g_bad_release++; return hipErrorInvalidValue; }   // never handed out, of another kind, or released before
    g_log.push_back({k, h});
    return hipSuccess;
}

void expect(bool ok, const char* fmt, ...) {
    if (ok) return;
    g_failures++;
    printf("FAIL: ");
    va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap);
    printf("\n");
}
long live_total() { long n = 0; for (auto& s : g_live) n += (long)s.size(); return n; }
long released(Kind k, size_t from = 0) { long n = 0; for (size_t i = from; i < g_log.size(); i++) n += g_log[i].kind == k; return n; }

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_next_malloc) { g_fail_next_malloc = 0; g_calls.push_back(DEV); *p = nullptr; return hipErrorOutOfMemory; }
    g_malloc_bytes.push_back(bytes);
    return acquire(DEV, p);
}
hipError_t hipDeviceSynchronize(void) { g_calls.push_back(DEVICE_SYNC); g_device_syncs++; return hipSuccess; }
hipError_t hipFree(void* p) { return release(DEV, p); }
hipError_t hipHostMalloc(void** p, size_t, unsigned int) { return acquire(PINNED, p); }
hipError_t hipHostFree(void* p) { return release(PINNED, p); }
hipError_t hipEventCreate(hipEvent_t* e) {
    if (g_fail_event_in && --g_fail_event_in == 0) { g_calls.push_back(EVENT); *e = nullptr; return hipErrorOutOfMemory; }
    return acquire(EVENT, reinterpret_cast<void**>(e));
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return acquire(EVENT, reinterpret_cast<void**>(e)); }
hipError_t hipEventDestroy(hipEvent_t e) { return release(EVENT, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return acquire(STREAM, reinterpret_cast<void**>(s)); }
hipError_t hipStreamDestroy(hipStream_t s) { return release(STREAM, s); }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    g_calls.push_back(kind == hipMemcpyHostToDevice ? COPY_UP : COPY_DOWN);
    if (g_fail_copy_in && --g_fail_copy_in == 0) return hipErrorInvalidValue;
    g_copies.push_back({dst, src, bytes, s});
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { g_calls.push_back(STREAM_SYNC); g_synced = s; return hipSuccess; }
hipError_t hipGetLastError(void) { g_last_error_calls++; return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory (stub)" : "error (stub)"; }
}

namespace csky {
thread_local char g_err[512];
int fail(csky_ctx* c, int code, const char* fmt, ...) {       // as api.cpp's
    char* dst = c ? c->err : g_err;
    va_list ap; va_start(ap, fmt); vsnprintf(dst, 512, fmt, ap); va_end(ap);
    if (code == CSKY_ERR_HIP) (void)hipGetLastError();
    return code;
}
}  // namespace csky

using namespace csky;

namespace {

// 1. each owner type: one release, none after being moved from (by construction or by assignment), none when empty
template <class Owner, class Make> void once(Kind k, const char* what, Make make) {
    const size_t log0 = g_log.size(); const long bad0 = g_bad_release;
    { Owner empty; }
    expect(g_log.size() == log0, "%s: an empty owner made a release call", what);
    {
        Owner a; make(a);
        void* const h = *g_live[k].rbegin();
        Owner b(std::move(a));
        expect(!a, "%s: still holds its handle after being moved from", what);
        Owner c; make(c);                                      // c's own handle must go when it is assigned over
        c = std::move(b);
        expect(!b, "%s: still holds its handle after being move-assigned from", what);
        expect(released(k, log0) == 1, "%s: move assignment released %ld handles, not the one it overwrote", what, released(k, log0));
        expect(g_live[k].count(h) == 1, "%s: the moved handle died on the way", what);
        c.reset();
        expect(!c && g_live[k].count(h) == 0, "%s: reset() did not release", what);
        c.reset();
    }
    expect(released(k, log0) == 2 && g_log.size() == log0 + 2, "%s: 2 handles made, %ld released", what, released(k, log0));
    expect(g_bad_release == bad0, "%s: a handle was released twice", what);
    printf("owner_%s_made 2\nowner_%s_released %ld\n", kind_name[k], kind_name[k], released(k, log0));
}

void test_owners(csky_ctx* c) {
    once<DevBuf<float>>(DEV, "DevBuf", [&](DevBuf<float>& b) { expect(b.alloc(c, 16) == CSKY_OK && b.count() == 16, "DevBuf::alloc"); });
    once<PinnedBuf>(PINNED, "PinnedBuf", [&](PinnedBuf& b) { expect(b.alloc(c, 64) == CSKY_OK && b.count() == 64, "PinnedBuf::alloc"); });
    once<Event>(EVENT, "Event", [&](Event& e) { expect(e.create(c, hipEventDisableTiming) == CSKY_OK, "Event::create"); });
    once<Event>(EVENT, "Event (timing)", [&](Event& e) { expect(e.create(c, hipEventDefault) == CSKY_OK, "Event::create"); });
    once<Stream>(STREAM, "Stream", [&](Stream& s) { expect(s.create(c, hipStreamNonBlocking) == CSKY_OK, "Stream::create"); });

    // 2. alloc releases the old buffer BEFORE it asks for the new one;  3. grow makes no call when the buffer is large enough
    {
        DevBuf<uint2> b;
        expect(b.grow(c, 100) == CSKY_OK && b.count() == 100, "grow of an empty buffer");
        uint2* const first = b;
        size_t calls0 = g_calls.size();
        expect(b.grow(c, 100) == CSKY_OK && b.grow(c, 1) == CSKY_OK && b.grow(c, 0) == CSKY_OK, "grow within the capacity");
        expect(g_calls.size() == calls0 && b == first && b.count() == 100, "grow within the capacity made %zu HIP calls", g_calls.size() - calls0);
        printf("grow_within_capacity_calls %zu\n", g_calls.size() - calls0);
        calls0 = g_calls.size();
        expect(b.grow(c, 101) == CSKY_OK && b.count() == 101, "grow beyond the capacity");
        expect(g_calls.size() == calls0 + 2 && g_calls[calls0] == DEV + KINDS && g_calls[calls0 + 1] == DEV, "grow beyond the capacity: not hipFree then hipMalloc");
        calls0 = g_calls.size();
        expect(b.alloc(c, 7) == CSKY_OK && b.count() == 7, "alloc allocates exactly what it is asked for");
        expect(g_calls.size() == calls0 + 2 && g_calls[calls0] == DEV + KINDS && g_calls[calls0 + 1] == DEV, "alloc: not hipFree then hipMalloc");
        printf("alloc_order_free_then_malloc %d\n", g_calls[calls0] == DEV + KINDS && g_calls[calls0 + 1] == DEV);

        // 4. a failed hipMalloc: the owner is empty with count 0 (the old buffer is gone: it went first), the context has the text
        c->err[0] = 0;
        const long le0 = g_last_error_calls, live0 = (long)g_live[DEV].size();
        g_fail_next_malloc = 1;
        const int rc = b.grow(c, 1000);
        expect(rc == CSKY_ERR_HIP, "failed hipMalloc: return code %d", rc);
        expect(!b && b.count() == 0, "failed hipMalloc: the owner is not empty");
        expect((long)g_live[DEV].size() == live0 - 1, "failed hipMalloc: the old buffer was not released");
        expect(c->err[0] != 0, "failed hipMalloc: no error text in the context");
        expect(g_last_error_calls == le0 + 1, "failed hipMalloc: the runtime's sticky error was not cleared");
        printf("failed_malloc_error_text %s\n", c->err);
    }
    expect(live_total() == 0, "owner tests: %ld handles left alive", live_total());
}

// 5. / 6. a real csky_ctx with every owning member populated, then deleted
void test_context() {
    const long made0[KINDS] = {g_made[DEV], g_made[PINNED], g_made[EVENT], g_made[STREAM]};
    const size_t log0 = g_log.size(); const long bad0 = g_bad_release;
    Event foreign; foreign.create(nullptr, hipEventDisableTiming);      // what csky_multi owns and lut.writers only views
    csky_ctx* c = new csky_ctx();
    int rc = 0;
    // in an order unlike the declaration order on purpose: what dies when is the struct's business
    for (auto& hs : c->hring) { rc |= hs.h.alloc(c, 4096); rc |= hs.d.alloc(c, 512); rc |= hs.done.create(c, hipEventDisableTiming); rc |= hs.s.create(c, hipStreamNonBlocking); }
    c->kt.ev.resize(2); for (Event& e : c->kt.ev) rc |= e.create(c, hipEventDefault);
    rc |= c->kt.grow(c, 70);   // a grown pool: the vector moved its events
    expect(c->kt.ev.size() == 70, "the timing pool did not grow to 70 events");
    for (csky_ctx::RadSet* r : {&c->rad_pf, &c->rad}) { rc |= r->out_cones.alloc(c, 6); rc |= r->src_cones.alloc(c, 6); rc |= r->tab.alloc(c, 12); }
    rc |= c->ev_rad.create(c, hipEventDisableTiming); rc |= c->stage.d.alloc(c, 64);
    rc |= c->ev_rays.create(c, hipEventDisableTiming); rc |= c->d_rays_fc.alloc(c, 1); rc |= c->ev_aerial.create(c, hipEventDisableTiming);
    for (Event& e : c->rows_cache.ev_read) rc |= e.create(c, hipEventDisableTiming);
    rc |= c->rows_cache.ev_fill.create(c, hipEventDisableTiming); rc |= c->rows_cache.d.alloc(c, 16);
    rc |= c->ring.d_heads.alloc(c, RING * 16); rc |= c->ring.d_sort_scratch.alloc(c, 8); rc |= c->ring.d_feedback_order.alloc(c, 8); rc |= c->ring.d_cost.alloc(c, 8);
    for (FrameSlot& k : c->ring.slot) { rc |= k.order.alloc(c, 8); rc |= k.ev_clouds.create(c, hipEventDisableTiming); rc |= k.ev_setup.create(c, hipEventDisableTiming); rc |= k.fc.alloc(c, 1); }
    rc |= c->d_frame.alloc(c, 64); rc |= c->d_stats.alloc(c, 130);
    for (int k = 0; k < 2; k++) { rc |= c->lut.ring_f[k].alloc(c, 8); rc |= c->lut.ring_h[k].alloc(c, 32); }
    rc |= c->d_trans_f.alloc(c, 8); rc |= c->d_trans_h.alloc(c, 32);
    rc |= c->noise.d_weather32.alloc(c, 8); rc |= c->noise.d_detail32.alloc(c, 8); rc |= c->noise.d_shape32.alloc(c, 8); rc |= c->noise.d_brick.alloc(c, 8);
    rc |= c->noise.d_detail_h.alloc(c, 8); rc |= c->noise.d_weather.alloc(c, 8); rc |= c->noise.d_detail.alloc(c, 8); rc |= c->noise.d_shape.alloc(c, 8);
    rc |= c->noise.d_bake_meta.alloc(c, 32); rc |= c->noise.d_raw_weather.alloc(c, 8); rc |= c->noise.d_raw_small.alloc(c, 8); rc |= c->noise.d_raw_large.alloc(c, 8);
    rc |= c->ev_copy.create(c, hipEventDisableTiming); rc |= c->ev1.create(c, hipEventDefault); rc |= c->ev0.create(c, hipEventDefault);
    rc |= c->stream.create(c, hipStreamNonBlocking);
    // the views: copies of somebody else's events.  None of them may be released by the context.
    c->ring.cur = 3; c->lut.writers.push_back(foreign);
    expect(c->ring.fc() == c->ring.slot[3].fc.get(), "the ring's frame constants are not the current slot's");
    expect(rc == 0, "populating the context failed");
    void* const main_stream = static_cast<hipStream_t>(c->stream);
    const long made[KINDS] = {g_made[DEV] - made0[DEV], g_made[PINNED] - made0[PINNED], g_made[EVENT] - made0[EVENT] - 1, g_made[STREAM] - made0[STREAM]};
    // the owning members of context.h, counted by hand, in its order.
    // device buffers: the stage 1, the noise set 12, the transmittance LUT 2, the sky LUT's ring 4, the rows cache 1, the frame ring RING frame
    //   constants + RING order tables + 4 shared, d_stats and d_frame 2, the two radiance sets 3 each, d_rays_fc 1, one per host slot
    // events: ev0 ev1 ev_copy 3, the rows cache 1 + RING, two per frame slot, the timing pool 70, ev_rad ev_aerial ev_rays 3, one per host slot
    const long want[KINDS] = {1 + 12 + 2 + 4 + 1 + RING + RING + 4 + 2 + 6 + 1 + HOST_RING, HOST_RING, 3 + 1 + RING + 2 * RING + 70 + 3 + HOST_RING, 1 + HOST_RING};
    for (int k = 0; k < KINDS; k++) expect(made[k] == want[k], "context: %ld %s handles made, %ld expected", made[k], kind_name[k], want[k]);

    delete c;

    for (int k = 0; k < KINDS; k++) {
        printf("context_%s_made %ld\ncontext_%s_released %ld\n", kind_name[k], made[k], kind_name[k], released((Kind)k, log0));
        expect(released((Kind)k, log0) == made[k], "context: %ld of %ld %s handles released", released((Kind)k, log0), made[k], kind_name[k]);
    }
    expect(g_bad_release == bad0, "context: %ld releases of a handle that was not live (double release)", g_bad_release - bad0);
    expect(live_total() == 1 && g_live[EVENT].count(static_cast<hipEvent_t>(foreign)) == 1, "context: a viewed event was released, or something is left (%ld live)", live_total());
    // 6. the context's stream is the last stream destroyed, and after every event
    size_t last_stream = 0, last_event = 0; void* last_stream_h = nullptr;
    for (size_t i = log0; i < g_log.size(); i++) {
        if (g_log[i].kind == STREAM) { last_stream = i; last_stream_h = g_log[i].handle; }
        if (g_log[i].kind == EVENT) last_event = i;
    }
    expect(last_stream_h == main_stream, "context: its stream is not the last stream destroyed");
    expect(last_stream > last_event, "context: an event was destroyed after the context's stream");
    printf("context_stream_destroyed_last %d\ncontext_stream_after_every_event %d\n", last_stream_h == main_stream, last_stream > last_event);
    // a host slot's stream goes after the rest of its slot
    for (size_t i = log0; i + 1 < g_log.size(); i++)
        if (g_log[i].kind == STREAM && g_log[i].handle != main_stream && i >= 3)
            expect(g_log[i - 1].kind == EVENT && g_log[i - 2].kind == DEV && g_log[i - 3].kind == PINNED, "host slot: its stream was not destroyed after its event and buffers");
}

// 7. an empty context makes no release call
void test_empty_context() {
    const size_t calls0 = g_calls.size();
    delete new csky_ctx();
    printf("empty_context_calls %zu\n", g_calls.size() - calls0);
    expect(g_calls.size() == calls0, "an empty context made %zu HIP calls when deleted", g_calls.size() - calls0);
}

// 8. the order tables grow together (FrameRing::grow_order_tables): one device-wide wait, then every table that is too small is re-allocated at exactly
// the grid asked for, its free before its malloc, and forgets its key; a table that is large enough keeps its memory and its key
void test_order_table_growth() {
    csky_ctx* c = new csky_ctx();
    FrameRing& r = c->ring;
    const size_t caps[RING] = {8, 8, 64, 8, 8, 8, 8, 8};
    int rc = 0;
    for (int k = 0; k < RING; k++) { rc |= r.slot[k].order.alloc(c, caps[k]); r.slot[k].order_st.written(order_key(k + 1, 1, 1, 8)); }
    expect(rc == 0, "order-table growth: populating the ring failed");
    uint32_t* const large = r.slot[2].order;
    const size_t calls0 = g_calls.size(), mallocs0 = g_malloc_bytes.size(); const long syncs0 = g_device_syncs;
    expect(r.grow_order_tables(c, 32) == CSKY_OK, "order-table growth failed");
    const size_t ncalls = g_calls.size() - calls0;
    bool order_ok = ncalls == 15 && g_calls[calls0] == DEVICE_SYNC;
    for (size_t i = 1; order_ok && i < ncalls; i += 2) order_ok = g_calls[calls0 + i] == DEV + KINDS && g_calls[calls0 + i + 1] == DEV;
    expect(order_ok, "order-table growth: not one device-wide wait followed by seven times hipFree then hipMalloc (%zu calls)", ncalls);
    long of_32 = 0, forgotten = 0;
    for (size_t i = mallocs0; i < g_malloc_bytes.size(); i++) of_32 += g_malloc_bytes[i] == 32 * sizeof(uint32_t);
    for (int k = 0; k < RING; k++) {
        forgotten += !r.slot[k].order_st.key.valid;
        if (k != 2) expect(r.slot[k].order.count() == 32 && !r.slot[k].order_st.key.valid, "order-table growth: slot %d is not a 32-entry table without a key", k);
    }
    const bool kept = r.slot[2].order == large && r.slot[2].order.count() == 64 && r.slot[2].order_st.hit(true, order_key(3, 1, 1, 8));
    expect(kept, "order-table growth: the 64-entry table lost its memory or its key");
    expect(of_32 == 7 && g_malloc_bytes.size() - mallocs0 == 7 && forgotten == 7, "order-table growth: %ld allocations of 32 entries, %ld keys forgotten", of_32, forgotten);
    printf("order_growth_device_syncs %ld\norder_growth_calls_in_order %d\norder_growth_allocations_of_32 %ld\norder_growth_keys_forgotten %ld\norder_growth_large_table_kept %d\n",
           g_device_syncs - syncs0, order_ok, of_32, forgotten, kept);
    // a second growth to a size every table has: the wait, and nothing else
    const size_t calls1 = g_calls.size();
    expect(r.grow_order_tables(c, 32) == CSKY_OK && g_calls.size() == calls1 + 1, "order-table growth within every table's capacity allocated something");
    delete c;
    expect(live_total() == 0, "order-table growth: %ld handles left alive", live_total());
}

// 9. the timing pool (TimingPool): a growth that cannot make one of its events returns the error, keeps the old size and releases the events it had made;
// the pool of a timed launch starts at 512 events and doubles when the next pair does not fit
void test_timing_pool() {
    csky_ctx* c = new csky_ctx();
    TimingPool& p = c->kt;
    expect(p.grow(c, 4) == CSKY_OK && p.ev.size() == 4, "timing pool: growth to 4 events");
    const long made0 = g_made[EVENT], live0 = (long)g_live[EVENT].size(); const size_t log0 = g_log.size();
    c->err[0] = 0;
    g_fail_event_in = 3;
    const int rc = p.grow(c, 10);
    expect(rc == CSKY_ERR_HIP && g_fail_event_in == 0, "timing pool: a failed growth returned %d", rc);
    expect(p.ev.size() == 4 && p.ev[0] && p.ev[3], "timing pool: a failed growth left %zu events", p.ev.size());
    expect(g_made[EVENT] - made0 == 2 && released(EVENT, log0) == 2 && (long)g_live[EVENT].size() == live0, "timing pool: a failed growth made %ld events and released %ld",
           g_made[EVENT] - made0, released(EVENT, log0));
    printf("pool_growth_failure_is_error %d\npool_growth_failure_size %zu\npool_growth_failure_events_made %ld\npool_growth_failure_events_released %ld\npool_growth_failure_error_text %s\n",
           rc == CSKY_ERR_HIP, p.ev.size(), g_made[EVENT] - made0, released(EVENT, log0), c->err);
    expect(p.grow(c, 10) == CSKY_OK && p.ev.size() == 10, "timing pool: the growth after a failed one");
    delete c;

    c = new csky_ctx();
    TimingPool& q = c->kt;
    const Event* pair = nullptr; size_t after_256 = 0;
    for (int i = 0; i < 257; i++) {
        expect(q.next_pair(c, pair) == CSKY_OK && pair == &q.ev[(size_t)i * 2] && pair[0] && pair[1], "timing pool: pair %d", i);
        if (i == 255) after_256 = q.ev.size();
    }
    expect(after_256 == 512 && q.ev.size() == 1024 && q.count == 257, "timing pool: %zu events after 256 pairs, %zu after 257", after_256, q.ev.size());
    printf("pool_events_after_256_pairs %zu\npool_events_after_257_pairs %zu\n", after_256, q.ev.size());
    delete c;
    expect(live_total() == 0, "timing pool: %ld handles left alive", live_total());
}

// 10. the layout of a blocking call's regions (host_stage.h stage_layout): pure arithmetic, no HIP call
void test_stage_layout() {
    const size_t calls0 = g_calls.size();
    const size_t A = STAGE_ALIGN;
    auto check = [&](const char* what, std::vector<size_t> bytes) {
        size_t off[STAGE_MAX_REGIONS], total = 0;
        const int n = (int)bytes.size();
        bool ok = stage_layout(bytes.data(), n, off, total) == CSKY_OK && off[0] == 0 && total == off[n - 1] + bytes[n - 1];
        for (int i = 0; ok && i < n; i++) ok = off[i] % A == 0;
        // in order and apart: a region begins at or after the end of the one before it, less than one alignment step after it
        for (int i = 1; ok && i < n; i++) ok = off[i] >= off[i - 1] + bytes[i - 1] && off[i] - (off[i - 1] + bytes[i - 1]) < A;
        // a region of no bytes costs nothing: the next region begins where it does
        for (int i = 0; ok && i + 1 < n; i++) if (bytes[i] == 0) ok = off[i + 1] == off[i];
        expect(ok, "stage layout: %s", what);
        return ok ? total : (size_t)0;
    };
    const size_t image = (size_t)8192 * 8192 * 8, volume = (size_t)512 * 512 * 256 * 8, map = (size_t)8192 * 8192 * 2;
    const size_t t_image = check("an 8192 x 8192 RGBA16F image", {image});
    const size_t t_shafts = check("an 8192 x 8192 R16F map and a 512 x 512 x 256 volume", {map, volume});
    const size_t t_ragged = check("ragged sizes", {1, 255, 256, 257, 2});
    const size_t t_zero = check("regions of no bytes between others", {0, 33 * 9 * 8, 0, 0, 7});
    const size_t t_view = check("no directions, then the image (the direct march of a view)", {0, 33 * 9 * 8});
    check("all regions empty", {0, 0, 0});
    expect(t_image == image && t_shafts == map + volume, "stage layout: aligned sizes at the forms' limits leave no gaps (%zu, %zu)", t_image, t_shafts);
    expect(t_ragged == 5 * A + 2 && t_zero == 2560 + 7 && t_view == 33 * 9 * 8, "stage layout: totals %zu %zu %zu", t_ragged, t_zero, t_view);
    printf("stage_layout_image_total %zu\nstage_layout_shafts_total %zu\nstage_layout_ragged_total %zu\nstage_layout_zero_regions_total %zu\n", t_image, t_shafts, t_ragged, t_zero);

    // sums that do not fit in size_t, in the addition and in the rounding up; region counts out of range
    size_t off[STAGE_MAX_REGIONS + 1], total = 1;
    const size_t over_add[] = {SIZE_MAX - 100, 200}, over_pad[] = {SIZE_MAX - 3, 0}, fits[] = {SIZE_MAX - A, 0}, six[STAGE_MAX_REGIONS + 1] = {};
    const bool refused = stage_layout(over_add, 2, off, total) == CSKY_ERR_INVALID && total == 0 && stage_layout(over_pad, 2, off, total) == CSKY_ERR_INVALID &&
                         stage_layout(six, STAGE_MAX_REGIONS + 1, off, total) == CSKY_ERR_INVALID && stage_layout(six, 0, off, total) == CSKY_ERR_INVALID;
    expect(refused, "stage layout: an overflowing sum or a bad region count was not refused");
    expect(stage_layout(fits, 2, off, total) == CSKY_OK && total == SIZE_MAX - A + 1, "stage layout: a sum that just fits was refused");
    // ... and reserve nothing: the stage keeps what it has, makes no call and names the caller
    csky_ctx* c = new csky_ctx();
    c->err[0] = 0;
    HostCall over = host_call(c, "some_entry_point", {SIZE_MAX - 100, 200});
    over.up(0, &total, sizeof total);
    over.step([] { g_calls.push_back(STEP); return (int)CSKY_OK; });
    const int rc = over.finish();
    expect(rc == CSKY_ERR_INVALID && !c->stage.d && c->stage.d.count() == 0, "stage: an overflowing reservation returned %d or reserved something", rc);
    printf("stage_overflow_refused %d\nstage_overflow_is_invalid %d\nstage_overflow_error_text %s\n", refused, rc == CSKY_ERR_INVALID, c->err);
    delete c;
    expect(g_calls.size() == calls0, "stage layout: %zu HIP calls made", g_calls.size() - calls0);
    printf("stage_layout_hip_calls %zu\n", g_calls.size() - calls0);
}

// 11. a blocking call's way through the stage (host_stage.h HostCall): reserve, uploads, the step, the download, ONE wait -- and the wait whenever
// something was enqueued, whatever failed
void test_host_call() {
    csky_ctx* c = new csky_ctx();
    expect(c->stream.create(c, hipStreamNonBlocking) == CSKY_OK, "host call: the context's stream");
    const hipStream_t s = c->stream;
    char in0[300] = {}, in1[40] = {}, out[64] = {};
    auto since = [](size_t from) { return std::vector<Kind>(g_calls.begin() + (long)from, g_calls.end()); };
    auto step_ok = [&] { g_calls.push_back(STEP); return (int)CSKY_OK; };

    // a call that succeeds, on an empty stage: one allocation of exactly the total, then uploads, step, download, wait
    size_t calls0 = g_calls.size(), copies0 = g_copies.size(), mallocs0 = g_malloc_bytes.size();
    HostCall a = host_call(c, "first", {sizeof in0, 0, sizeof in1, sizeof out});
    a.up(0, in0, sizeof in0); a.up(1, in0, 0); a.up(2, in1, sizeof in1);
    a.step(step_ok);
    a.down(out, 3, sizeof out);
    int rc = a.finish();
    const bool first_ok = rc == CSKY_OK && since(calls0) == std::vector<Kind>{DEV, COPY_UP, COPY_UP, STEP, COPY_DOWN, STREAM_SYNC};
    expect(first_ok, "host call: a successful call made %zu calls, not malloc, 2 uploads, the step, the download and one wait", g_calls.size() - calls0);
    uint8_t* const base = c->stage.d;
    expect(g_malloc_bytes.size() == mallocs0 + 1 && g_malloc_bytes.back() == 512 + 256 + sizeof out && c->stage.d.count() == 512 + 256 + sizeof out, "host call: the stage is not the call's total");
    bool copies_ok = g_copies.size() == copies0 + 3 && g_synced == s;
    if (copies_ok) {
        const Copy& u0 = g_copies[copies0]; const Copy& u1 = g_copies[copies0 + 1]; const Copy& d0 = g_copies[copies0 + 2];
        copies_ok = u0.dst == base && u0.src == in0 && u0.bytes == sizeof in0 && u0.s == s && u1.dst == base + 512 && u1.src == in1 && u1.bytes == sizeof in1 && u1.s == s &&
                    d0.dst == out && d0.src == base + 768 && d0.bytes == sizeof out && d0.s == s && a.at<char>(1) == (char*)base + 512 && a.at<uint2>(3) == (uint2*)(base + 768);
    }
    expect(copies_ok, "host call: a copy has the wrong region, size or stream, or the wait is not for the context's stream");
    printf("host_call_success_in_order %d\nhost_call_copies_in_their_regions %d\n", first_ok, copies_ok);

    // a second call that needs less: no allocation call, the same memory
    calls0 = g_calls.size();
    HostCall b = host_call(c, "second", {16});
    b.step(step_ok);
    b.down(out, 0, 16);
    rc = b.finish();
    const bool smaller_ok = rc == CSKY_OK && since(calls0) == std::vector<Kind>{STEP, COPY_DOWN, STREAM_SYNC} && c->stage.d == base;
    expect(smaller_ok, "host call: a call within the stage's size allocated, or made %zu calls", g_calls.size() - calls0);
    // a third that needs more: the old buffer goes before the new one is asked for
    calls0 = g_calls.size();
    HostCall g = host_call(c, "third", {4096, 4096});
    g.step(step_ok);
    rc = g.finish();
    const bool larger_ok = rc == CSKY_OK && since(calls0) == std::vector<Kind>{static_cast<Kind>(DEV + KINDS), DEV, STEP, STREAM_SYNC} && c->stage.d.count() == 8192;
    expect(larger_ok, "host call: a call beyond the stage's size did not free, then allocate");
    printf("host_call_smaller_allocates_nothing %d\nhost_call_larger_frees_then_allocates %d\n", smaller_ok, larger_ok);

    // the step fails: no download, one wait, the step's code and text
    calls0 = g_calls.size(); c->err[0] = 0;
    HostCall f = host_call(c, "fourth", {sizeof in0, sizeof out});
    f.up(0, in0, sizeof in0);
    f.step([&] { g_calls.push_back(STEP); return fail(c, CSKY_ERR_STATE, "the step's own text"); });
    f.down(out, 1, sizeof out);
    rc = f.finish();
    const bool step_fail_ok = rc == CSKY_ERR_STATE && since(calls0) == std::vector<Kind>{COPY_UP, STEP, STREAM_SYNC};
    expect(step_fail_ok, "host call: a failed step returned %d after %zu calls", rc, g_calls.size() - calls0);
    printf("host_call_step_failure_waits_once %d\nhost_call_step_failure_error_text %s\n", step_fail_ok, c->err);

    // the first upload fails: nothing was enqueued, so no step, no download and no wait
    calls0 = g_calls.size(); c->err[0] = 0; g_fail_copy_in = 1;
    HostCall h = host_call(c, "fifth", {sizeof in0, sizeof in1, sizeof out});
    h.up(0, in0, sizeof in0); h.up(1, in1, sizeof in1);
    h.step(step_ok);
    h.down(out, 2, sizeof out);
    rc = h.finish();
    const bool up0_fail_ok = rc == CSKY_ERR_HIP && since(calls0) == std::vector<Kind>{COPY_UP};
    expect(up0_fail_ok, "host call: a failed first upload returned %d after %zu calls", rc, g_calls.size() - calls0);
    printf("host_call_first_upload_failure_waits_never %d\nhost_call_upload_failure_error_text %s\n", up0_fail_ok, c->err);
    // the second upload fails: the first is in flight from the caller's memory, so one wait; still no step and no download
    calls0 = g_calls.size(); g_fail_copy_in = 2;
    HostCall k = host_call(c, "sixth", {sizeof in0, sizeof in1, sizeof out});
    k.up(0, in0, sizeof in0); k.up(1, in1, sizeof in1);
    k.step(step_ok);
    k.down(out, 2, sizeof out);
    rc = k.finish();
    const bool up1_fail_ok = rc == CSKY_ERR_HIP && since(calls0) == std::vector<Kind>{COPY_UP, COPY_UP, STREAM_SYNC};
    expect(up1_fail_ok, "host call: a failed second upload returned %d after %zu calls", rc, g_calls.size() - calls0);
    printf("host_call_second_upload_failure_waits_once %d\n", up1_fail_ok);
    // a reservation that fails: nothing else happens
    calls0 = g_calls.size(); g_fail_next_malloc = 1;
    HostCall m = host_call(c, "seventh", {1 << 20});
    m.up(0, in0, sizeof in0);
    m.step(step_ok);
    m.down(out, 0, sizeof out);
    rc = m.finish();
    const bool reserve_fail_ok = rc == CSKY_ERR_HIP && since(calls0) == std::vector<Kind>{static_cast<Kind>(DEV + KINDS), DEV} && !c->stage.d;
    expect(reserve_fail_ok, "host call: a failed reservation returned %d after %zu calls", rc, g_calls.size() - calls0);
    printf("host_call_reserve_failure_enqueues_nothing %d\n", reserve_fail_ok);
    delete c;
    expect(live_total() == 0, "host call: %ld handles left alive", live_total());
}

}  // namespace

int main() {
    {
        csky_ctx* c = new csky_ctx();
        test_owners(c);
        delete c;
    }
    test_context();
    test_empty_context();
    test_order_table_growth();
    test_timing_pool();
    test_stage_layout();
    test_host_call();
    printf("double_releases %ld\nlive_handles_at_exit %ld\nfailures %d\n", g_bad_release, live_total(), g_failures);
    return g_failures ? 1 : 0;
}
