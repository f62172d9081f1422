// context.h -- the context of libcloudsky (csky_ctx) and the host helpers its C ABI sources share.  Internal to libcloudsky:
// api.cpp (lifecycle, textures, LUTs, cloud entry points, host ring), clouds_launch.cpp (the cloud kernel launch), api_sky.cpp (compositor,
// radiance cubemap), api_external.cpp (zero-copy frames), api_multi.cpp (the multi-device handle).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/cloudsky_internal.h"
#include "kernels.h"

// Depth of the per-frame rings (frame constants, launch order, cost feedback, pop counters, events): the number of frames a caller may keep
// in flight on as many streams (csky_set_frames_in_flight).  The slots rotate over all RING entries whatever that number is.
constexpr int RING = 8;
constexpr int HOST_RING = 8;   // pinned host frames of the asynchronous host form (a single context uses up to RING of them, csky_multi up to groups x frames in flight)

struct csky_ctx {
    int device = 0;
    // The context's ONE stream: loads and bakes, the LUTs, the frame prologue (below), the blocking host forms, and what a NULL hip_stream selects.
    // One and not two (until round 11 the prologue had a stream of its own): the HIP runtime spreads a process's streams over GPU_MAX_HW_QUEUES
    // hardware queues, four by default, and a stream that has been used keeps its share of one for good.  With two internal streams, the host's
    // default stream and two frame streams, the second frame stream landed on the first one's queue and two frames in flight ran strictly one
    // after the other (profiles/r11/queue_overlap_ab.txt); with one, the four queues go round.
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_copy = nullptr;
    // noise set (cloud_sky.gd:298-341)
    uint8_t* d_raw_large = nullptr; uint8_t* d_raw_small = nullptr; uint8_t* d_raw_weather = nullptr; uint8_t* d_bake_meta = nullptr;   // 8-bit mip chains (inputs of the device bake)
    csky::ShapeTexel* d_shape = nullptr; unsigned long long inexact_coeffs = 0; uint4* d_detail = nullptr; uint4* d_weather = nullptr; uint16_t* d_detail_h = nullptr; bool have_noise = false;
    float* d_brick = nullptr;                                               // CSKY_BRICK_BOUND experiment build only
    // exact cells (bake_core.h): fp32-coefficient layouts, built when a coefficient of the bound textures does not fit fp16 (or exact_cells == 1)
    float4* d_shape32 = nullptr; float4* d_detail32 = nullptr; float4* d_weather32 = nullptr; bool cell32 = false; int exact_cells = 0;
    uint32_t shape_off[csky::SHAPE_LEVELS] = {}, detail_off[csky::DETAIL_LEVELS] = {};
    float detail_lod5 = 0.0f;
    double w_rmin = 0.0, w_rmax = 1.0, w_bmax = 1.0;   // range of the weather map's cloud-type / coverage channels
    float win_cov = -1e30f, win_lo = -1.0f, win_hi = 2.0f; bool use_window = true;
    // LUTs: RGBA16F image + float4 copy of the rounded values
    uint16_t* d_trans_h = nullptr; float4* d_trans_f = nullptr; int tw = 0, th = 0; bool have_trans = false;
    int tlut = CSKY_TLUT_REFERENCE;                   // the transmittance LUT's parametrization (csky_set_transmittance_mapping, tlut_core.h): its writer and every reader get it
    uint16_t* d_sky_h = nullptr; float4* d_sky_f = nullptr; int sw = 0, sh = 0; bool have_sky = false;   // = ring slot sky_cur
    csky::FrameConsts* d_fc = nullptr;                                                                    // = ring slot fc_cur
    // Frame prologue pipeline.  The sky LUT and the frame set-up of frame k+1 are small dependent kernels; enqueued behind the
    // cloud kernel of frame k they cost their run time plus two launch gaps per frame (6 % of one GPU's 1/8-frame share).  They
    // run on the context's own stream (`stream`, above) instead, beside the caller's, into the next slot of a ring (the sky LUT two deep: every
    // reader of it runs on `stream`; the frame constants RING deep: the marches of up to RING frames in flight read them) (the reference keeps
    // three-deep texture rings for the same reason, sky_lut.gd:143-146), so they overlap the march of the previous frame; events order
    // set-up -> clouds (ev_setup) and clouds -> the next writer of that slot (ev_clouds).  All sky-LUT readers run on `stream`.
    // A march that itself runs on `stream` (NULL hip_stream, the blocking host forms) has its prologue in line with it: nothing overlaps there.
    uint16_t* sky_h_ring[2] = {nullptr, nullptr}; float4* sky_f_ring[2] = {nullptr, nullptr}; int sky_cur = 0;
    // csky_render_sky_lut_rows_device: the LUT of sun sky_sun exists only as the rows the caller's buffer received (one rank of an N-way frame
    // split); the texels this context's frame set-up filters are rendered by the set-up kernel itself (clouds_dev)
    bool sky_partial = false; float sky_sun[3] = {0, 1, 0}; int psw = 0, psh = 0;
    // csky_multi_render_sky_lut: the whole LUT IS in this context's memory (ring slot sky_cur), written row by row by the devices of the handle;
    // readers of the memory copy wait for those writers first.  (sky_partial stays set: the frame set-ups never read the memory copy.)
    bool sky_in_memory = false; std::vector<hipEvent_t> lut_writers;
    csky::FrameConsts* fc_ring[RING] = {}; int fc_cur = 0;
    hipEvent_t ev_setup[RING] = {}, ev_clouds[RING] = {}; bool clouds_pending[RING] = {};
    unsigned long long* d_stats = nullptr;
    uint2* d_frame = nullptr; size_t frame_px = 0;  // internal frame for the host-buffer form / timing
    int primary_steps = 128, light_steps = 6;        // clouds.glsl:228, :186
    float early_eps = 0.0f;
    int variant = CSKY_DEFAULT_VARIANT;
    int sched_mode = -1;                              // -1 = auto (5 for large launches, 2 for small ones)
    int segments = 0;                                 // ray segments per ray: 0 = auto, 1, 2, 4
    int frames_in_flight = 1;                         // csky_set_frames_in_flight: the caller alternates that many streams
    int frames_overlapping = 1;                       // how many of them the hardware queues in effect can keep apart: the launch policy's hint (clouds_dev)
    // static workgroup order (physical workgroup -> slab), written on the device, one table per ring slot (= frame parity, so two
    // frames in flight with different geometries never share one), cached per launch geometry
    uint32_t* d_order_ring[RING] = {}; size_t order_cap[RING] = {}; int order_grid_ring[RING] = {};
    long long order_key_ring[RING][4];     // csky_create fills them with -1
    // cost-feedback schedule (mode 7): per-workgroup costs of the last launch -> heaviest-first order of the next one
    uint32_t* d_wg_cost = nullptr; uint32_t* d_lpt_order = nullptr; uint32_t* d_lpt_hist = nullptr; size_t lpt_cap = 0;
    uint32_t* d_heads = nullptr; int persistent = 1; int resident_wgs = 0;   // persistent launches: 2 ring slots x (8 per-XCD pop counters + exit counter)
    bool lpt_valid[RING] = {}; long long lpt_key[RING][11];   // csky_create fills the keys with -1
    // optional per-launch timing of the cloud kernel (csky_set_kernel_timing): HIP event pairs recorded around the launch on ITS stream
    bool kt_on = false; std::vector<hipEvent_t> kt_ev; int kt_count = 0;   // the event pool grows on demand (clouds_dev)
    uint8_t* d_composite = nullptr; size_t composite_cap = 0;              // grow-only scratch of csky_composite_sky
    // radiance cubemap (csky_render_radiance*, csky_prefilter_cube): source-record table and block cones, grow-only.  `rad` is the snapshot
    // of the last layer-0 call, which later calls filter from; csky_prefilter_cube works in `rad_pf` and leaves the snapshot alone
    struct RadSet { float4* tab = nullptr; float4* src_cones = nullptr; float4* out_cones = nullptr; size_t tab_n = 0, sc_n = 0, oc_n = 0;
                    int cones_ss = 0, cones_s = 0; int S = 0, L = 0, Ss = 0; bool valid = false; };
    RadSet rad, rad_pf;
    uint8_t* d_rad_io = nullptr; size_t rad_io_cap = 0;                    // host forms: uploaded inputs + the requested output layers
    hipEvent_t ev_rad = nullptr;                                           // the transmittance LUT (prologue stream) -> layer 0 (caller's stream)
    csky_cloud_stats last_stats = {0, 0, 0};
    bool census_lean = false;                                  // csky_census_clouds unless CSKY_CENSUS_TALLY=1: count the blocks of the kernel form that keeps no in-cloud tally (kernels.h launch_clouds)
    // asynchronous host form (csky_submit_clouds / csky_collect): a ring of pinned host frames + device frames on rotating internal streams
    struct HostSlot { hipStream_t s = nullptr; hipEvent_t done = nullptr; uint2* d = nullptr; void* h = nullptr; size_t px = 0; long long ticket = -1; int w = 0, hh = 0; bool busy = false; };
    HostSlot hring[HOST_RING]; int hslots = 2; long long next_ticket = 0;
    char err[512] = {0};
    char warn[512] = {0};                              // csky_last_warning: text of the last call that succeeded with a caveat (never mixed into err)
};

namespace csky {

extern thread_local char g_err[512];   // error text of calls without a context (csky_last_error(NULL))

// writes the error text into c->err (g_err when c is NULL) and returns `code`
int fail(csky_ctx* c, int code, const char* fmt, ...);
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail((c), CSKY_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

inline int bind(csky_ctx* c) { HIPCHK(c, hipSetDevice(c->device)); return CSKY_OK; }

template <class T> int dev_alloc(csky_ctx* c, T** p, size_t count) {
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)));
    return CSKY_OK;
}

// api.cpp
int ensure_sky(csky_ctx* c, int w, int h);
int render_trans_dev(csky_ctx* c, int w, int h, hipStream_t s);
int host_slot_prepare(csky_ctx* c, csky_ctx::HostSlot& hs, size_t px, bool need_device);

// clouds_launch.cpp
int check_bands(csky_ctx* c, const csky_bands* b, int tile_w);
int grow_timing_pool(csky_ctx* c, size_t want);
// frame set-up (when `setup`) + the cloud kernel on stream s into d_out.  d_stats: optional device counters.
int clouds_dev(csky_ctx* c, const csky_cloud_params* p, int tile_w, const csky_bands* b, uint2* d_out, size_t pitch_bytes, hipStream_t s,
               unsigned long long* d_stats, bool setup, bool out_full = false);

}  // namespace csky
