// context.h -- the context of libcloudsky (csky_ctx) and the host helpers its C ABI sources share.  Internal to libcloudsky:
// api.cpp (lifecycle, textures, cloud entry points, host ring), api_lut.cpp (the transmittance and sky LUTs), clouds_launch.cpp (the cloud kernel
// launch), api_sky.cpp (compositor, radiance cubemap), api_shadow.cpp (cloud shadow map), api_depth.cpp (cloud depth frame), api_aerial.cpp
// (aerial-perspective volume, air in front of a cloud frame), api_rays.cpp (the direct cloud march), api_external.cpp (zero-copy frames),
// api_multi.cpp (the multi-device handle).
// Ownership: every device buffer, pinned buffer, event and stream of the context is a member of one of the owner types of owners.h and dies with
// the context (csky_destroy: bind the device, wait for it, delete).  A buffer's count() is its capacity; raw pointers and raw handles in the
// struct are views of something owned elsewhere and say so.
// The blocking host forms share one staging buffer (`stage`, host_stage.h) and go through it one way (HostCall): a new feature's host form adds no
// member here.  The cloud frame's own host forms keep d_frame.
// The per-frame ring is one member (FrameRing, below): each of its RING slots owns its frame constants, its two events and its order table, and the
// ring hands out slot k's share of the four allocations the slots share.  What a slot remembers about its cached orders is frame_ring.h's.
// Member order: `stream` is declared before everything recorded on it or ordered by it, and HostSlot::s before the rest of its slot; members die
// in reverse order, so a stream is destroyed after the events and buffers that were used on it.  Keep new members below it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/cloudsky_internal.h"
#include "kernels.h"
#include "owners.h"
#include "frame_ring.h"
#include "host_stage.h"
#include "noise_set.h"
#include "sky_lut_reuse.h"

// Depth of the per-frame rings (frame constants, launch order, cost feedback, pop counters, events): the number of frames a caller may keep
// in flight on as many streams (csky_set_frames_in_flight).  The slots rotate over all RING entries whatever that number is.
constexpr int RING = 8;
constexpr int HOST_RING = 8;   // pinned host frames of the asynchronous host form (a single context uses up to RING of them, csky_multi up to groups x frames in flight)

namespace csky {

// The context's sky LUT: what it holds (sky_lut_reuse.h: the state and its transitions) and the memory it holds it in.
// The ring is two slots deep: the sky LUT and the frame set-up of frame k+1 run on the context's stream beside the march of frame k, and every
// reader of the LUT runs on that stream too, so a render goes to the slot the readers ahead of it are not using (csky_ctx, frame prologue pipeline).
// Two sizes, because no reader can do with one: aw x ah is what both slots are allocated for, which is the size of the whole LUT in memory (Whole,
// Shared: ensure_sky comes before every launch into a slot); st.w x st.h is the size of the LUT a Rows or Shared context renders its own taps for.
// The rows form allocates nothing, so a Rows context's ring may still be sized for an earlier whole LUT of another size.
struct SkyLut {
    SkyLutHeld st;
    DevBuf<uint16_t> ring_h[2]; DevBuf<float4> ring_f[2];   // RGBA16F image + float4 copy of the rounded values
    int cur = 0;                                             // the slot readers use
    int aw = 0, ah = 0;                                      // 0 x 0: not allocated (ensure_sky)
    // Shared: the other devices' rows of the slot have been stored (csky_multi_render_sky_lut); readers of the memory copy wait for them first.
    // Empty in every other state.
    std::vector<hipEvent_t> writers;                         // views, not owned: copies of events the csky_multi handle owns
    long long launches = 0;                                  // LUT kernels launched, whole and rows form (csky_sky_lut_launches)

    uint16_t* cur_h() const { return ring_h[cur]; }
    float4* cur_f() const { return ring_f[cur]; }
    // the slot to render into: the other one while readers may be using the current one (they are ahead on the context's stream)
    int render_slot() const { return st.in_memory() ? cur ^ 1 : cur; }
    // slot k has been rendered into: readers use it from here on.  (The caller names what it holds: st.became_whole / st.became_shared.)
    void publish(int k) { cur = k; writers.clear(); }
    void drop() { st.drop(); writers.clear(); }
};

// The bound noise set (csky_set_noise*; cloud_sky.gd:298-341): what the context knows about it (noise_set.h: the state, its steps and every size)
// and the memory it is held in.
struct NoiseSet {
    NoiseHeld st;
    DevBuf<uint8_t> d_raw_large, d_raw_small, d_raw_weather, d_bake_meta;   // 8-bit mip chains (inputs of the device bake) and the bake's counters
    DevBuf<ShapeTexel> d_shape; DevBuf<uint4> d_detail, d_weather; DevBuf<uint16_t> d_detail_h;   // fp16-pair cells
    DevBuf<float> d_brick;                                                  // CSKY_BRICK_BOUND experiment build only
    // exact cells (bake_core.h): fp32-coefficient layouts, held while st.cell32()
    DevBuf<float4> d_shape32, d_detail32, d_weather32;
};

// csky_render_sky_lut_rows_device: the compact rows of st.rows_key, copied behind the kernel that rendered them into a caller's buffer; a call with
// the same key copies them out on the caller's stream instead of rendering.  Events and buffer are made by the first fill.
// Its readers and writers sit on CALLER streams, several of them with frames in flight:
//   fill -> read   every copy out waits for ev_fill (until the event has been seen complete once)
//   read -> fill   every copy out records an event of the ring ev_read; a fill waits for all that are pending.  A ring slot that comes round
//                  while still pending is waited for by its new user first, so the newer record stands for the older one too
//   fill -> fill   a fill waits for the one before it
struct RowsCache {
    DevBuf<uint2> d; Event ev_fill, ev_read[RING];
    bool fill_done = true, read_pending[RING] = {}; int read_cur = 0;
    int fill(csky_ctx* c, const void* d_rows, size_t px, hipStream_t s);     // api_lut.cpp
    int read(csky_ctx* c, void* d_rows_out, size_t px, hipStream_t s);
};

// One frame in flight: what the set-up kernel writes for it, the events that order it, and the workgroup orders cached for it.  The slots rotate
// (= frame parity), so two frames in flight with different geometries never share a table, costs or pop counters.
struct FrameSlot {
    DevBuf<FrameConsts> fc;                // written by the frame set-up on the context's stream, read by the march
    Event ev_setup, ev_clouds;             // set-up -> march; march (and its feedback sort) -> the next writer of this slot
    bool pending = false;                  // ev_clouds has been recorded at least once: the next user of the slot waits for it.  Never cleared
    DevBuf<uint32_t> order;                // static workgroup order (physical workgroup -> slab), written on the device, cached per launch geometry
    OrderTableState order_st;
    FeedbackState feedback;                // cost-feedback schedule (mode 7): per-workgroup costs of the last launch -> heaviest-first order of the next one
};

// The per-frame ring.  Frame prologue pipeline: the sky LUT and the frame set-up of frame k+1 are small dependent kernels; enqueued behind the cloud
// kernel of frame k they cost their run time plus two launch gaps per frame (6 % of one GPU's 1/8-frame share).  They run on the context's own
// stream instead, beside the caller's, into the next slot of a ring (the sky LUT two deep: every reader of it runs on that stream; the frame
// constants RING deep: the marches of up to RING frames in flight read them) (the reference keeps three-deep texture rings for the same reason,
// sky_lut.gd:143-146), so they overlap the march of the previous frame; events order set-up -> clouds (ev_setup) and clouds -> the next writer of
// that slot (ev_clouds).  A march that itself runs on the context's stream (NULL hip_stream, the blocking host forms) has its prologue in line
// with it: nothing overlaps there.
struct FrameRing {
    FrameSlot slot[RING]; int cur = 0;     // cur: the slot of the last set-up, which a launch without set-up uses again
    // shared by the slots, RING equal shares each: costs and feedback orders of capacity() workgroups per slot, 2048 words of sort scratch,
    // 16 words of pop counters of the persistent launch form (8 per XCD + the exit counter; zero between launches)
    DevBuf<uint32_t> d_cost, d_feedback_order, d_sort_scratch, d_heads;

    FrameConsts* fc() const { return slot[cur].fc; }
    size_t capacity() const { return d_feedback_order.count() / RING; }
    uint32_t* cost(int k) const { return d_cost + (size_t)k * capacity(); }
    uint32_t* feedback_order(int k) const { return d_feedback_order + (size_t)k * capacity(); }
    uint32_t* sort_scratch(int k) const { return d_sort_scratch + k * 2048; }
    uint32_t* heads(int k) const { return d_heads + k * 16; }

    // Prologue, first half: the slot the next set-up writes.  Its last reader, the march RING frames ago, must be done before `ctx_stream` writes it.
    int next_slot(csky_ctx* c, hipStream_t ctx_stream, int& f) {
        f = (cur + 1) % RING;
        if (slot[f].pending) HIPCHK(c, hipStreamWaitEvent(ctx_stream, slot[f].ev_clouds, 0));
        return CSKY_OK;
    }
    // Prologue, second half: the set-up of slot f was enqueued on ctx_stream.  The slot is current and the launch stream s waits for it.
    // (Round 5 bounded what folding the set-up INTO the march launch could return by simply not waiting here -- legal in a timing run with constant
    // parameters: whole frame one at a time 2.014 -> 2.000 ms, a 1/8 share 0.408 -> 0.404, eight in flight 0.224 -> 0.227: the prologue of frame k + 1
    // already runs under the march of frame k; profiles/r05/rows_overlap_ab.txt.)
    int setup_enqueued(csky_ctx* c, int f, hipStream_t ctx_stream, hipStream_t s) {
        HIPCHK(c, hipEventRecord(slot[f].ev_setup, ctx_stream));
        cur = f;
        HIPCHK(c, hipStreamWaitEvent(s, slot[f].ev_setup, 0));
        return CSKY_OK;
    }
    // Every order table grows to `grid` entries.  Growing is rare and costs a device-wide wait (an older launch may still read the old table): grow
    // EVERY slot's table now, so that it happens once, at the first frame of a geometry, and not again at the first use of each of the other ring
    // slots (with rings eight deep and a five-frame warm-up that was three synchronisations inside a timed region).  A table that is large enough
    // keeps its memory and its key.
    int grow_order_tables(csky_ctx* c, size_t grid) {
        HIPCHK(c, hipDeviceSynchronize());
        for (FrameSlot& k : slot) {
            if (k.order.count() >= grid) continue;
            if (const int rc = k.order.alloc(c, grid)) return rc;
            k.order_st.forget();
        }
        return CSKY_OK;
    }
    // Room for the feedback of `need` workgroups per slot.  (Re)allocation is rare; frames may be in flight on other streams.  The order, allocated
    // last, carries the capacity of the pair: a failure on the way leaves it empty.  The sort kernels leave costs and scratch zeroed afterwards.
    int reserve_feedback(csky_ctx* c, size_t need) {
        if (d_feedback_order.count() >= RING * need) return CSKY_OK;
        HIPCHK(c, hipDeviceSynchronize());
        d_cost.reset(); d_feedback_order.reset();
        for (FrameSlot& k : slot) k.feedback.forget();
        int rc; if ((rc = d_cost.alloc(c, RING * need))) return rc;
        if (!d_sort_scratch) {
            if ((rc = d_sort_scratch.alloc(c, RING * 2048))) return rc;
            HIPCHK(c, hipMemset(d_sort_scratch, 0, RING * 2048 * sizeof(uint32_t)));
        }
        HIPCHK(c, hipMemset(d_cost, 0, RING * need * sizeof(uint32_t)));
        return d_feedback_order.alloc(c, RING * need);
    }
    // Finish: the march of slot k (and the sort behind it) was enqueued on s.
    int march_enqueued(csky_ctx* c, int k, hipStream_t s) {
        HIPCHK(c, hipEventRecord(slot[k].ev_clouds, s));
        slot[k].pending = true;
        return CSKY_OK;
    }
};

// Optional per-launch timing of the cloud kernel (csky_set_kernel_timing): HIP event pairs recorded around the launch on ITS stream.
struct TimingPool {
    bool on = false; std::vector<Event> ev; int count = 0;   // count: launches timed since the last read-out, two events each
    // The pool grows to `want` events.  All or nothing: an event that cannot be made part-way used to leave null entries in the pool for
    // later timed launches to record on; now the new events made so far go with the resize and the pool keeps its old size.
    int grow(csky_ctx* c, size_t want) {
        const size_t old_n = ev.size();
        if (want <= old_n) return CSKY_OK;
        ev.resize(want);
        for (size_t i = old_n; i < want; i++)
            if (const int rc = ev[i].create(c, hipEventDefault)) { ev.resize(old_n); return rc; }
        return CSKY_OK;
    }
    // the event pair of the next timed launch.  The pool doubles on demand: no launch is ever dropped from the sum
    int next_pair(csky_ctx* c, const Event*& pair) {
        if ((size_t)count * 2 + 2 > ev.size())
            if (const int rc = grow(c, ev.empty() ? 512 : ev.size() * 2)) return rc;
        pair = &ev[(size_t)count * 2]; count++;
        return CSKY_OK;
    }
    // the summed time of every launch since the last read-out, which it waits for
    int read_out(csky_ctx* c, float* total_ms, int* launches) {
        float sum = 0.0f;
        for (int i = 0; i < count; i++) {
            HIPCHK(c, hipEventSynchronize(ev[(size_t)i * 2 + 1]));
            float ms = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&ms, ev[(size_t)i * 2], ev[(size_t)i * 2 + 1]));
            sum += ms;
        }
        *total_ms = sum; *launches = count; count = 0;
        return CSKY_OK;
    }
};

}  // namespace csky

struct csky_ctx {
    int device = 0;
    // The context's ONE stream: loads and bakes, the LUTs, the frame prologue (below), the blocking host forms, and what a NULL hip_stream selects.
    // One and not two (until round 11 the prologue had a stream of its own): the HIP runtime spreads a process's streams over GPU_MAX_HW_QUEUES
    // hardware queues, four by default, and a stream that has been used keeps its share of one for good.  With two internal streams, the host's
    // default stream and two frame streams, the second frame stream landed on the first one's queue and two frames in flight ran strictly one
    // after the other (profiles/r11/queue_overlap_ab.txt); with one, the four queues go round.
    csky::Stream stream;
    csky::HostStage stage;                            // what the blocking host forms upload into and copy out of (host_stage.h), grow-only
    csky::Event ev0, ev1, ev_copy;
    csky::NoiseSet noise;
    bool use_window = true;                           // csky_set_height_window: the exact rejects of a density sample (noise_set.h)
    // LUTs: RGBA16F image + float4 copy of the rounded values
    csky::DevBuf<uint16_t> d_trans_h; csky::DevBuf<float4> d_trans_f; int tw = 0, th = 0; bool have_trans = false;
    int tlut = CSKY_TLUT_REFERENCE;                   // the transmittance LUT's parametrization (csky_set_transmittance_mapping, tlut_core.h): its writer and every reader get it
    // The frame prologue pipeline (FrameRing, above) runs on `stream`, and so do all sky-LUT readers.
    csky::SkyLut lut;
    csky::RowsCache rows_cache;
    csky::FrameRing ring;
    csky::DevBuf<unsigned long long> d_stats;
    // internal frame of csky_render_clouds / csky_time_clouds / csky_census_clouds, in pixels, grow-only.  Not part of `stage` on purpose: the
    // benchmark times through csky_time_clouds, and the frame path keeps the allocation it has always had
    csky::DevBuf<uint2> d_frame;
    int primary_steps = 128, light_steps = 6;        // clouds.glsl:228, :186
    float early_eps = 0.0f;
    int variant = CSKY_DEFAULT_VARIANT;
    int sched_mode = -1;                              // -1 = auto (5 for large launches, 2 for small ones)
    int segments = 0;                                 // ray segments per ray: 0 = auto, 1, 2, 4
    int frames_in_flight = 1;                         // csky_set_frames_in_flight: the caller alternates that many streams
    int frames_overlapping = 1;                       // how many of them the hardware queues in effect can keep apart: the launch policy's hint (clouds_dev)
    int persistent = 1; int resident_wgs = 0;         // the persistent launch form: allowed; workgroups resident at once
    int resident_wgs_slim = 0;                        // ... of the forms that run eight workgroups per CU (kernels.h cloud_resident_workgroups_per_cu_slim)
    csky::TimingPool kt;                              // csky_set_kernel_timing
    // radiance cubemap (csky_render_radiance*, csky_prefilter_cube): source-record table and block cones, grow-only.  `rad` is the snapshot
    // of the last layer-0 call, which later calls filter from; csky_prefilter_cube works in `rad_pf` and leaves the snapshot alone
    struct RadSet { csky::DevBuf<float4> tab, src_cones, out_cones;
                    int cones_ss = 0, cones_s = 0; int S = 0, L = 0, Ss = 0; bool valid = false; };
    RadSet rad, rad_pf;
    csky::Event ev_rad;                                                    // the transmittance LUT (prologue stream) -> layer 0 (caller's stream)
    csky_cloud_stats last_stats = {0, 0, 0};
    bool shadow_exact_end = true;                                          // csky_set_shadow_exact_end (shadow_core.h shadow_march)
    csky::Event ev_aerial;                                                 // the transmittance LUT (the context's stream) -> the volume (caller's stream)
    // the direct march (csky_render_clouds_dirs / _view, api_rays.cpp): frame constants of its own, written by the cloud frame's set-up kernel on the
    // context's stream (no slot of the frame ring).  One event orders both ways: recorded behind the set-up, the caller's stream waits for it; recorded
    // again behind the march, the context's stream waits for it before the next call's set-up overwrites the block.  Both are made by the first call.
    csky::DevBuf<csky::FrameConsts> d_rays_fc;
    csky::Event ev_rays; bool rays_pending = false;
    bool census_lean = false;                                 // csky_census_clouds unless CSKY_CENSUS_TALLY=1: count the blocks of the kernel form that keeps no in-cloud tally (kernels.h launch_clouds)
    // asynchronous host form (csky_submit_clouds / csky_collect): a ring of pinned host frames + device frames on rotating internal streams
    // (a slot's capacity is h.count(), in bytes; d holds as many pixels of 8 bytes)
    struct HostSlot { csky::Stream s; csky::Event done; csky::DevBuf<uint2> d; csky::PinnedBuf h; long long ticket = -1; int w = 0, hh = 0; bool busy = false; };
    HostSlot hring[HOST_RING]; int hslots = 2; long long next_ticket = 0;
    char err[512] = {0};
    char warn[512] = {0};                              // csky_last_warning: text of the last call that succeeded with a caveat (never mixed into err)
};

namespace csky {

extern thread_local char g_err[512];   // error text of calls without a context (csky_last_error(NULL))

// (fail and HIPCHK: owners.h)
inline int bind(csky_ctx* c) { HIPCHK(c, hipSetDevice(c->device)); return CSKY_OK; }
// the stream a _device entry point launches on: the caller's, or the context's for a NULL hip_stream
inline hipStream_t stream_of(const csky_ctx* c, void* hip_stream) { return hip_stream ? (hipStream_t)hip_stream : (hipStream_t)c->stream; }
// the blocking host form `fn`'s way through the context's stage, on the context's stream, with room for regions of `bytes`
inline HostCall host_call(csky_ctx* c, const char* fn, std::initializer_list<size_t> bytes) { return HostCall(c, c->stage, c->stream, fn, bytes); }
// the result of a kernel launch made for the entry point `fn` as a CSKY code
inline int launched(csky_ctx* c, const char* fn, hipError_t e) { return e == hipSuccess ? CSKY_OK : fail(c, CSKY_ERR_HIP, "%s: kernel launch failed: %s", fn, hipGetErrorString(e)); }
// a camera view as the aerial volume and the direct march take it: a finite basis, a field of view in (0, 180).  fn: the entry point's name
inline int view_check(csky_ctx* c, const char* fn, const csky_view* view) {
    for (int k = 0; k < 9; k++) if (!std::isfinite(view->basis[k])) return fail(c, CSKY_ERR_INVALID, "%s: the view's basis is not finite", fn);
    if (!(view->fov_y_degrees > 0.0f && view->fov_y_degrees < 180.0f)) return fail(c, CSKY_ERR_INVALID, "%s: fov_y_degrees must be in (0, 180)", fn);
    return CSKY_OK;
}

// api.cpp
int host_slot_prepare(csky_ctx* c, csky_ctx::HostSlot& hs, size_t px);

// api_lut.cpp
inline SkyLutState sky_lut_state(const csky_ctx* c) { return sky_lut_state(c->lut.st, c->lut.writers.empty()); }
// both ring slots at w x h.  A size change drops what the context holds first, so a failed allocation leaves a context that holds nothing
int ensure_sky(csky_ctx* c, int w, int h);
int render_trans_dev(csky_ctx* c, int w, int h, hipStream_t s);
int ensure_default_trans(csky_ctx* c);   // the table at its default size (transmittance_lut.gd:6) on the context's stream, unless the context has one
// a LUT request's texture_size as integers; `fn` is the entry point the error text names.  The text goes where fail() puts it: c, or g_err without one
int lut_size(csky_ctx* c, const char* fn, const float texture_size[2], int& w, int& h);

// clouds_launch.cpp
TexSet texset(const csky_ctx* c);       // the bound textures as the kernels take them: fp16-pair cells, and the exact fp32 cells of a context in that mode
TexSet32 texset32(const csky_ctx* c);
// the exact cells as a launch takes them: `t32` filled and its address for a context in that mode, NULL otherwise
inline const TexSet32* texset32_if(const csky_ctx* c, TexSet32& t32) { if (!c->noise.st.cell32()) return nullptr; t32 = texset32(c); return &t32; }
int check_bands(csky_ctx* c, const csky_bands* b, int tile_w);
// frame set-up (when `setup`) + the cloud kernel on stream s into d_out.  d_stats: optional device counters.
int clouds_dev(csky_ctx* c, const csky_cloud_params* p, int tile_w, const csky_bands* b, uint2* d_out, size_t pitch_bytes, hipStream_t s,
               unsigned long long* d_stats, bool setup, bool out_full = false);

}  // namespace csky
