// api.cpp -- the C ABI of libcloudsky (include/cloudsky.h; the measurement / tuning / test entry points: include/cloudsky_internal.h): context
// lifecycle, settings, noise upload and bake, the cloud entry points, the asynchronous host ring, read-backs and kernel timing.  The LUTs are
// api_lut.cpp; the launch of the cloud kernel clouds_launch.cpp; the compositor and the radiance cubemap api_sky.cpp; the cloud shadow map
// api_shadow.cpp; zero-copy frames api_external.cpp; the multi-device handle api_multi.cpp.
// GPU resources are held by the owner types of owners.h, as members of csky_ctx (context.h) or as locals of the entry point that needs a scratch
// buffer: nothing here releases a handle by hand, and an early return leaks nothing.
// Mirrors the resource ownership of the reference's GDScript driver cloud_sky.gd (`_initialize_compute_code`, `_render_process`, `cleanup`).
// There is no CPU render path here: every render entry point needs a live HIP device.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <vector>
#include "context.h"
#include "bake_core.h"
#include "mip_args.h"
#include "cloud_core.h"
#include "order_core.h"
#include "primitives_core.h"

using namespace csky;

// Two frames in flight (csky_set_frames_in_flight) need the caller's two streams on DIFFERENT hardware queues.  The HIP runtime
// multiplexes a process's streams onto GPU_MAX_HW_QUEUES queues (default 4); each stream that has been used holds on to one, and once all
// exist a further stream shares one.  Per context the library uses ONE stream of its own (context.h), so the runtime's default of four carries
// two frames in flight beside a host that uses its default stream: frames + 2 queues are what csky_set_frames_in_flight asks for (measured,
// profiles/r11/queue_overlap_ab.txt: 1.52 ms per frame at 4 queues and at 16; with a second internal stream, as until round 11, 1.87 at 4).
// More frames in flight, or a host with further streams of its own, need more queues.  The runtime reads the variable when it initialises, at
// the first HIP call; this runs when libcloudsky.so is loaded, so a host that cannot set environment variables (a GDExtension inside Godot)
// gets 16 as long as it has not used HIP before loading the library.  An existing value is never overwritten.
// Opt-out: CSKY_NO_ENV=1 in the environment leaves the process's environment alone (a host that loads other HIP users and wants the runtime's
// defaults); csky_set_frames_in_flight then warns through csky_last_warning when the variable is not in effect.
__attribute__((constructor)) static void csky_runtime_defaults() {
    const char* no = getenv("CSKY_NO_ENV");
    if (no && no[0] && no[0] != '0') return;
    if (!getenv("GPU_MAX_HW_QUEUES")) setenv("GPU_MAX_HW_QUEUES", "16", /*overwrite=*/0);
}

static_assert(sizeof(csky_cloud_params) == sizeof(CloudParams), "ABI struct mismatch");

namespace {
constexpr size_t CSKY_STATS_WORDS = 2 + 128;             // [0..1] the kernel's own tallies; then 256 32-bit basic-block counters of the census build (tools/isa_profile.py; zero in the product build)

// the stream, events and buffers a context has from the start (csky_create)
int create_resources(csky_ctx* c) {
    int rc; if ((rc = bind(c))) return rc;
    // (The frame prologue runs on `stream` too: context.h.  A HIGH-PRIORITY prologue stream was measured in round 2: whole frames with two frames in
    // flight 1.78 -> 2.02 ms, one rank's 1/8 share 0.329 -> 0.335 ms: the priority queue breaks the overlap of the two frame streams.)
    if ((rc = c->stream.create(c, hipStreamNonBlocking)) || (rc = c->ev0.create(c, hipEventDefault)) || (rc = c->ev1.create(c, hipEventDefault))) return rc;
    if ((rc = c->ev_copy.create(c, hipEventDisableTiming)) || (rc = c->ev_rad.create(c, hipEventDisableTiming)) ||
        (rc = c->ev_aerial.create(c, hipEventDisableTiming))) return rc;
    for (FrameSlot& k : c->ring.slot)
        if ((rc = k.ev_setup.create(c, hipEventDisableTiming)) || (rc = k.ev_clouds.create(c, hipEventDisableTiming)) || (rc = k.fc.alloc(c, 1))) return rc;
    if ((rc = c->d_stats.alloc(c, CSKY_STATS_WORDS)) || (rc = c->ring.d_heads.alloc(c, RING * 16))) return rc;
    HIPCHK(c, hipMemset(c->ring.d_heads, 0, RING * 16 * sizeof(uint32_t)));   // persistent launches leave them zero
    return CSKY_OK;
}

}  // namespace

namespace csky {

thread_local char g_err[512];

int fail(csky_ctx* c, int code, const char* fmt, ...) {
    char* dst = c ? c->err : g_err;
    va_list ap; va_start(ap, fmt); vsnprintf(dst, 512, fmt, ap); va_end(ap);
    if (code == CSKY_ERR_HIP) (void)hipGetLastError();       // the runtime's last-error slot is sticky: a failed call must not resurface as the "launch error" of a later kernel
    return code;
}

int host_slot_prepare(csky_ctx* c, csky_ctx::HostSlot& hs, size_t px) {
    int rc;
    if (!hs.s && (rc = hs.s.create(c, hipStreamNonBlocking))) return rc;
    if (!hs.done && (rc = hs.done.create(c, hipEventDisableTiming))) return rc;
    if (hs.h.count() >= px * 8) return CSKY_OK;
    HIPCHK(c, hipStreamSynchronize(hs.s));                    // the slot's last frame may still be on its way into the buffers
    hs.d.reset(); hs.h.reset();                                // both go before either comes back: the pinned buffer, allocated last, carries the slot's capacity
    if ((rc = hs.d.alloc(c, px))) return rc;
    return hs.h.alloc(c, px * 8);
}

}  // namespace csky

extern "C" {

int csky_abi_version(void) { return CSKY_ABI_VERSION; }

int csky_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* csky_last_error(const csky_ctx* ctx) { return ctx ? ctx->err : g_err; }
const char* csky_last_warning(const csky_ctx* ctx) { return ctx ? ctx->warn : ""; }

int csky_create(csky_ctx** out, int device_id) {
    if (!out) return fail(nullptr, CSKY_ERR_INVALID, "csky_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, CSKY_ERR_NO_DEVICE, "csky_create: no HIP device available (%s); libcloudsky has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, CSKY_ERR_INVALID, "csky_create: device_id %d out of range [0,%d)", device_id, n);
    csky_ctx* c = new (std::nothrow) csky_ctx();
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_create: out of host memory");
    c->device = device_id;
    // a step that fails leaves its text in the half-built context: hand it to the caller's thread, release what was made
    if (const int rc = create_resources(c)) { fail(nullptr, rc, "csky_create: %s", c->err); csky_destroy(c); return rc; }
    { int cus = 0; (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id); cus = cus > 0 ? cus : 256;
      c->resident_wgs = cus * cloud_resident_workgroups_per_cu(); c->resident_wgs_slim = cus * cloud_resident_workgroups_per_cu_slim(); }
    // A/B switch (CSKY_PERSISTENT; the A/B of profiles/r02/persistent_launch_ab.txt): 0 = never, 1 = the policy of clouds_dev (default), 2 = every whole-ray launch
    if (const char* pe = getenv("CSKY_PERSISTENT")) c->persistent = atoi(pe);
    if (const char* pe = getenv("CSKY_PERSISTENT_WGS")) { const int n = atoi(pe); if (n > 0) c->resident_wgs = c->resident_wgs_slim = n; }
    *out = c;
    return CSKY_OK;
}

void csky_destroy(csky_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();                              // launches may sit on caller streams too
    delete c;                                                  // every member releases what it owns (context.h)
}

#ifdef CSKY_BRICK_BOUND
static int upload_brick_bounds(csky_ctx* c, const uint8_t* large_rgba8) {
    // per 8^3 brick (+1 apron on the high side, REPEAT): bmax = (rmax + 1 - fmin) / (2 - fmin), a hair above (the kernel's rcp is approximate)
    std::vector<float> tab(16 * 16 * 16);
    for (int bz = 0; bz < 16; bz++) for (int by = 0; by < 16; by++) for (int bx = 0; bx < 16; bx++) {
        int rm = 0, fm = 1 << 30;
        for (int z = bz * 8; z <= bz * 8 + 8; z++) for (int y = by * 8; y <= by * 8 + 8; y++) for (int x = bx * 8; x <= bx * 8 + 8; x++) {
            const uint8_t* tx = large_rgba8 + ((((size_t)(z & 127) * 128 + (y & 127)) * 128 + (x & 127)) * 4);
            rm = std::max(rm, (int)tx[0]); fm = std::min(fm, 5 * tx[1] + 2 * tx[2] + tx[3]);
        }
        const float r = rm * (1.0f / 255.0f), f = fm * (1.0f / (8.0f * 255.0f));
        tab[((size_t)bz * 16 + by) * 16 + bx] = (r + (1.0f - f)) / (2.0f - f) * 1.000004f;
    }
    if (const int rc = c->noise.d_brick.grow(c, tab.size())) return rc;
    HIPCHK(c, hipMemcpy(c->noise.d_brick, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    return CSKY_OK;
}
#endif

// The steps of a bind and what each leaves the context knowing: NoiseHeld (noise_set.h), which also has every size used here.
static int set_noise(csky_ctx* c, const uint8_t* large_rgba8, const uint8_t* small_rgb8, const uint8_t* weather_rgb8, bool chains_given) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_noise: ctx is NULL");
    if (!large_rgba8 || !small_rgb8 || !weather_rgb8) return fail(c, CSKY_ERR_INVALID, "csky_set_noise: NULL texture pointer");
    int rc; if ((rc = bind(c))) return rc;
    // the kernels' level offsets (cloud_core.h: closed forms shared with device code, not constexpr) are those of the chains as allocated and baked
    for (int l = 0; l < SHAPE_LEVELS; l++) if (chain_texels(SHAPE_N, l) != shape_level_offset(l)) return fail(c, CSKY_ERR_INVALID, "internal: shape mip offset mismatch");
    for (int l = 0; l < DETAIL_LEVELS; l++) if (chain_texels(DETAIL_N, l) != detail_level_offset(l)) return fail(c, CSKY_ERR_INVALID, "internal: detail mip offset mismatch");
    HIPCHK(c, hipDeviceSynchronize());                        // frames reading the old textures may be in flight on caller streams
    NoiseSet& n = c->noise;
    n.st.begin_rebind();                                      // a failure below leaves freed / half-baked textures: no render until a later call reaches ready()
    if ((rc = n.d_raw_large.alloc(c, RAW_SHAPE_CHAIN)) || (rc = n.d_raw_small.alloc(c, RAW_DETAIL_CHAIN)) || (rc = n.d_raw_weather.alloc(c, RAW_WEATHER))) return rc;
    if ((rc = n.d_shape.alloc(c, SHAPE_CELLS)) || (rc = n.d_detail.alloc(c, DETAIL_CELLS)) || (rc = n.d_weather.alloc(c, WEATHER_CELLS))) return rc;
    if ((rc = n.d_detail_h.alloc(c, DETAIL_H_HALFS)) || (rc = n.d_bake_meta.grow(c, 32))) return rc;
    // The level-0 textures go to the device as they are (9.2 MB); mip chains (mipmaps/generate=true, perlworlnoise.tga.import:24,
    // worlnoise.bmp.import:24) and the device layouts are built there (bake_kernels.hip::launch_mip_chain / launch_bake).
    struct { unsigned long long inexact; int range[3]; int pad; } meta = {0ull, {255, 0, 0}, 0};   // the bake's counters: min R, max R, max B of the weather map
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(n.d_bake_meta, &meta, sizeof meta, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(n.d_raw_large, large_rgba8, chains_given ? RAW_SHAPE_CHAIN : RAW_SHAPE_L0, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(n.d_raw_small, small_rgb8, chains_given ? RAW_DETAIL_CHAIN : RAW_DETAIL_L0, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(n.d_raw_weather, weather_rgb8, RAW_WEATHER, hipMemcpyHostToDevice, s));
    if (!chains_given) {                                      // csky_set_noise_mips: the caller's chains (e.g. the importer's own, csky_load_ctex3d) are used as they are
        HIPCHK(c, launch_mip_chain(n.d_raw_large, SHAPE_N, 4, SHAPE_LEVELS, s));
        HIPCHK(c, launch_mip_chain(n.d_raw_small, DETAIL_N, 3, DETAIL_LEVELS, s));
    }
    HIPCHK(c, launch_bake(n.d_raw_large, n.d_raw_small, n.d_raw_weather, n.d_shape, n.d_detail, n.d_detail_h, n.d_weather,
                          reinterpret_cast<unsigned long long*>(n.d_bake_meta.get()), reinterpret_cast<int*>(n.d_bake_meta + 8), s));
#ifdef CSKY_BRICK_BOUND
    if ((rc = upload_brick_bounds(c, large_rgba8))) return rc;
#endif
    uint8_t t5[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&meta, n.d_bake_meta, sizeof meta, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(t5, n.d_raw_small + RAW_DETAIL_LOD5, 3, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    c->warn[0] = 0;
    if (n.st.bound(meta.inexact, WeatherRange{meta.range[0], meta.range[1], meta.range[2]}, detail_lod5_value(t5))) {
        if ((rc = n.d_shape32.alloc(c, SHAPE32_F4)) || (rc = n.d_detail32.alloc(c, DETAIL32_F4)) || (rc = n.d_weather32.alloc(c, WEATHER32_F4))) return rc;
        HIPCHK(c, launch_bake32(n.d_raw_large, n.d_raw_small, n.d_raw_weather, n.d_shape32, n.d_detail32, n.d_weather32, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (n.st.inexact())   // (rounds 1-3 marched such textures on the rounded fp16 cells and warned)
            snprintf(c->warn, sizeof c->warn, "csky_set_noise: %llu finite-difference coefficients of these textures do not fit fp16: marching on exact fp32 cells "
                     "(twice the bytes per tap; the whole-ray compact kernel)", n.st.inexact());
    } else {
        // textures that fit fp16 again: the ~150 MB of exact cells of an earlier bind are not kept until csky_destroy (nothing is in flight: the device was synchronised above)
        n.d_shape32.reset(); n.d_detail32.reset(); n.d_weather32.reset();
    }
    n.st.ready();
    return CSKY_OK;
}

int csky_set_noise(csky_ctx* c, const uint8_t* large_rgba8, const uint8_t* small_rgb8, const uint8_t* weather_rgb8) {
    return set_noise(c, large_rgba8, small_rgb8, weather_rgb8, false);
}
int csky_set_noise_mips(csky_ctx* c, const uint8_t* large_chain_rgba8, const uint8_t* small_chain_rgb8, const uint8_t* weather_rgb8) {
    return set_noise(c, large_chain_rgba8, small_chain_rgb8, weather_rgb8, true);
}

// ---- the weather map alone (include/cloudsky.h).  Where the 8-bit map comes from: host memory, memory of this device, or the
// generator kernel writing into the context's own buffer.
namespace {
struct WeatherSource { const void* host; const void* dev; const WeatherNoiseParams* gen; uint32_t seed; };

// the bake itself: d_raw_weather filled, the cells of both formats the context marches on rebuilt, the range read back.  Every buffer exists (have())
int bake_weather(csky_ctx* c, const WeatherSource& src, WeatherRange& range) {
    NoiseSet& n = c->noise;
    hipStream_t s = c->stream;
    struct { unsigned long long inexact; int range[3]; int pad; } meta = {0ull, {255, 0, 0}, 0};   // the bake's counters, as in set_noise; a weather cell never adds to inexact
    HIPCHK(c, hipMemcpyAsync(n.d_bake_meta, &meta, sizeof meta, hipMemcpyHostToDevice, s));
    if (src.gen) {
        const Event* kt = nullptr;                              // timing pair of the generator's launch (csky_set_kernel_timing)
        int rc; if (c->kt.on && (rc = c->kt.next_pair(c, kt))) return rc;
        if (kt) HIPCHK(c, hipEventRecord(kt[0], s));
        HIPCHK(c, launch_weather_noise(src.seed, *src.gen, n.d_raw_weather, s));
        if (kt) HIPCHK(c, hipEventRecord(kt[1], s));
    } else if (src.dev) {
        HIPCHK(c, hipMemcpyAsync(n.d_raw_weather, src.dev, RAW_WEATHER, hipMemcpyDeviceToDevice, s));
    } else {
        HIPCHK(c, hipMemcpyAsync(n.d_raw_weather, src.host, RAW_WEATHER, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, launch_bake_weather(n.d_raw_weather, n.d_weather, reinterpret_cast<unsigned long long*>(n.d_bake_meta.get()), reinterpret_cast<int*>(n.d_bake_meta + 8), s));
    if (n.st.cell32()) HIPCHK(c, launch_bake_weather32(n.d_raw_weather, n.d_weather32, s));
    HIPCHK(c, hipMemcpyAsync(&meta, n.d_bake_meta, sizeof meta, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (meta.inexact) return fail(c, CSKY_ERR_INVALID, "internal: a weather cell's coefficients do not fit fp16");
    range = WeatherRange{meta.range[0], meta.range[1], meta.range[2]};
    return CSKY_OK;
}

// arguments are valid when this is called; `name` is the entry point's
int set_weather(csky_ctx* c, const char* name, const WeatherSource& src) {
    if (!c->noise.st.have()) return fail(c, CSKY_ERR_STATE, "%s: csky_set_noise has not been called", name);
    int rc; if ((rc = bind(c))) return rc;
    HIPCHK(c, hipDeviceSynchronize());                        // frames reading the old cells may be in flight on caller streams; a device source has been produced after this
    WeatherRange range;
    if ((rc = bake_weather(c, src, range))) { c->noise.st.begin_rebind(); return rc; }   // half-baked cells are not marched: nothing bound until a csky_set_noise* succeeds
    c->noise.st.reweathered(range);
    return CSKY_OK;
}
}  // namespace

int csky_set_weather(csky_ctx* c, const uint8_t* weather_rgb8) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_weather: ctx is NULL");
    if (!weather_rgb8) return fail(c, CSKY_ERR_INVALID, "csky_set_weather: NULL texture pointer");
    return set_weather(c, "csky_set_weather", WeatherSource{weather_rgb8, nullptr, nullptr, 0});
}
int csky_set_weather_device(csky_ctx* c, const void* d_weather_rgb8) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_weather_device: ctx is NULL");
    if (!d_weather_rgb8) return fail(c, CSKY_ERR_INVALID, "csky_set_weather_device: NULL texture pointer");
    return set_weather(c, "csky_set_weather_device", WeatherSource{nullptr, d_weather_rgb8, nullptr, 0});
}
int csky_set_weather_generated(csky_ctx* c, uint32_t seed, const csky_weather_params* params) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_weather_generated: ctx is NULL");
    WeatherNoiseParams P = weather_noise_defaults();
    if (params) {
        if (csky_check_weather_params(params)) return fail(c, CSKY_ERR_INVALID, "csky_set_weather_generated: %s", csky_assets_last_error());
        memcpy(&P, params, sizeof P);
    }
    return set_weather(c, "csky_set_weather_generated", WeatherSource{nullptr, nullptr, &P, seed});
}
int csky_generate_weather_device(csky_ctx* c, uint32_t seed, const csky_weather_params* params, uint8_t* out_rgb8) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_generate_weather_device: ctx is NULL");
    if (!out_rgb8) return fail(c, CSKY_ERR_INVALID, "csky_generate_weather_device: out is NULL");
    WeatherNoiseParams P = weather_noise_defaults();
    if (params) {
        if (csky_check_weather_params(params)) return fail(c, CSKY_ERR_INVALID, "csky_generate_weather_device: %s", csky_assets_last_error());
        memcpy(&P, params, sizeof P);
    }
    int rc; if ((rc = bind(c))) return rc;
    DevBuf<uint8_t> d; if ((rc = d.alloc(c, RAW_WEATHER))) return rc;
    HIPCHK(c, launch_weather_noise(seed, P, d, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_rgb8, d, RAW_WEATHER, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_read_baked_texture(csky_ctx* c, int which, void* out, size_t capacity, size_t* bytes) {
    if (!c || !bytes) return fail(c, CSKY_ERR_INVALID, "csky_read_baked_texture: NULL argument");
    if (!c->noise.st.have()) return fail(c, CSKY_ERR_STATE, "csky_read_baked_texture: csky_set_noise has not been called");
    int rc; if ((rc = bind(c))) return rc;
    const NoiseSet& ns = c->noise;
    const void* src = nullptr; size_t n = 0;
    // 9: what the context HOLDS from the bake (NoiseHeld, not the device scratch): the values the kernels are launched with
    struct { uint64_t inexact; int32_t rmin, rmax, bmax; float lod5; } held;
    static_assert(sizeof held == 24, "which == 9 is 24 bytes");
    if (which >= 6 && which <= 8 && !ns.st.cell32())          // released (or never built) by the last bind: nothing to read
        return fail(c, CSKY_ERR_STATE, "csky_read_baked_texture: the bound textures have no exact cells (which = %d; they fit fp16 and csky_set_exact_cells is 0)", which);
    switch (which) {
        case 0: src = ns.d_shape; n = SHAPE_CELLS * sizeof(ShapeTexel); break;
        case 1: src = ns.d_detail; n = DETAIL_CELLS * sizeof(uint4); break;
        case 2: src = ns.d_weather; n = WEATHER_CELLS * sizeof(uint4); break;
        case 3: src = ns.d_raw_large; n = RAW_SHAPE_CHAIN; break;
        case 4: src = ns.d_raw_small; n = RAW_DETAIL_CHAIN; break;
        case 5: src = ns.d_detail_h; n = DETAIL_CELLS * sizeof(uint16_t); break;      // without the 8-half pad of the allocation
        case 6: src = ns.d_shape32; n = SHAPE32_F4 * sizeof(float4); break;
        case 7: src = ns.d_detail32; n = DETAIL32_F4 * sizeof(float4); break;
        case 8: src = ns.d_weather32; n = WEATHER32_F4 * sizeof(float4); break;
        case 9: {
            const WeatherRange w = ns.st.range();
            held.inexact = (uint64_t)ns.st.inexact(); held.rmin = w.rmin; held.rmax = w.rmax; held.bmax = w.bmax; held.lod5 = ns.st.detail_lod5();
            n = sizeof held; break;
        }
        default: return fail(c, CSKY_ERR_INVALID, "csky_read_baked_texture: which must be 0..9");
    }
    *bytes = n;
    if (!out) return CSKY_OK;
    if (capacity < n) return fail(c, CSKY_ERR_INVALID, "csky_read_baked_texture: buffer too small (%zu < %zu)", capacity, n);
    if (which == 9) { memcpy(out, &held, n); return CSKY_OK; }
    HIPCHK(c, hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
    return CSKY_OK;
}

int csky_test_sqrt_shell(csky_ctx* c, const float* in, float* out, size_t n) {
    if (!c || !in || !out) return fail(c, CSKY_ERR_INVALID, "csky_test_sqrt_shell: NULL argument");
    int rc; if ((rc = bind(c))) return rc;
    DevBuf<float> d; if ((rc = d.alloc(c, 2 * n + 4))) return rc;
    HIPCHK(c, hipMemcpyAsync(d, in, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_sqrt_shell(d, d + n, n, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, d + n, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_test_primitive(csky_ctx* c, int op, const void* in0, const void* in1, const void* in2, void* out0, void* out1, size_t n) {
    if (!c) return fail(c, CSKY_ERR_INVALID, "csky_test_primitive: NULL context");
    if (op < 0 || op >= PRIM_COUNT || n > ((size_t)1 << 24)) return fail(c, CSKY_ERR_INVALID, "csky_test_primitive: op in [0, %d), n <= 2^24", (int)PRIM_COUNT);
    const PrimShape sh = prim_shape(op);
    const void* const in[3] = {in0, in1, in2};
    void* const out[2] = {out0, out1};
    size_t words = 4;
    for (int k = 0; k < 3; k++) { if (sh.in[k] && !in[k]) return fail(c, CSKY_ERR_INVALID, "csky_test_primitive: op %d needs input %d", op, k); words += (size_t)sh.in[k] * n; }
    for (int k = 0; k < 2; k++) { if (sh.out[k] && !out[k]) return fail(c, CSKY_ERR_INVALID, "csky_test_primitive: op %d needs output %d", op, k); words += (size_t)sh.out[k] * n; }
    if (n == 0) return CSKY_OK;
    int rc; if ((rc = bind(c))) return rc;
    DevBuf<uint32_t> d; if ((rc = d.alloc(c, words))) return rc;
    const uint32_t* d_in[3] = {nullptr, nullptr, nullptr};
    uint32_t* d_out[2] = {nullptr, nullptr};
    uint32_t* at = d;
    for (int k = 0; k < 3; k++) if (sh.in[k]) {
        d_in[k] = at;
        HIPCHK(c, hipMemcpyAsync(at, in[k], (size_t)sh.in[k] * n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        at += (size_t)sh.in[k] * n;
    }
    for (int k = 0; k < 2; k++) if (sh.out[k]) { d_out[k] = at; at += (size_t)sh.out[k] * n; }
    HIPCHK(c, launch_primitive(op, d_in, d_out, n, c->stream));
    for (int k = 0; k < 2; k++) if (sh.out[k]) HIPCHK(c, hipMemcpyAsync(out[k], d_out[k], (size_t)sh.out[k] * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_test_static_order(csky_ctx* c, int mode, int tiles_x, int slabs, uint32_t* table, size_t capacity, int* grid_out) {
    if (!c || !grid_out) return fail(c, CSKY_ERR_INVALID, "csky_test_static_order: NULL argument");
    if ((mode != 1 && mode != 2 && mode != 5) || tiles_x < 1 || slabs < 1 || (long long)tiles_x * slabs > (1ll << 24))
        return fail(c, CSKY_ERR_INVALID, "csky_test_static_order: mode 1, 2 or 5, tiles_x and slabs >= 1, at most 2^24 footprints");
    const int grid = static_order_grid(mode, tiles_x, slabs);            // what ensure_order launches with
    *grid_out = grid;
    if (!table) return CSKY_OK;
    if (capacity < (size_t)grid) return fail(c, CSKY_ERR_INVALID, "csky_test_static_order: table too small (%zu < %d entries)", capacity, grid);
    int rc; if ((rc = bind(c))) return rc;
    DevBuf<uint32_t> d; if ((rc = d.alloc(c, (size_t)grid))) return rc;
    HIPCHK(c, hipMemsetAsync(d, 0x5a, (size_t)grid * sizeof(uint32_t), c->stream));     // neither a footprint nor the idle entry: an entry the kernel leaves out shows
    HIPCHK(c, launch_static_order(mode, tiles_x, slabs, grid, d, c->stream));
    HIPCHK(c, hipMemcpyAsync(table, d, (size_t)grid * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_test_lpt_order(csky_ctx* c, const uint32_t* cost, int n, int shift, int rounds, uint32_t* order_out, uint32_t* cost_out, uint32_t* scratch_out) {
    if (!c || !cost || !order_out || !cost_out || !scratch_out) return fail(c, CSKY_ERR_INVALID, "csky_test_lpt_order: NULL argument");
    if (n < 1 || n > (1 << 24) || shift < 0 || shift > 31 || rounds < 1 || rounds > 64)
        return fail(c, CSKY_ERR_INVALID, "csky_test_lpt_order: n in [1, 2^24], shift in [0, 31], rounds in [1, 64]");
    int rc; if ((rc = bind(c))) return rc;
    DevBuf<uint32_t> d_cost, d_order, d_scratch;
    if ((rc = d_cost.alloc(c, (size_t)n)) || (rc = d_order.alloc(c, (size_t)n)) || (rc = d_scratch.alloc(c, 2 * LPT_BUCKETS))) return rc;
    HIPCHK(c, hipMemsetAsync(d_scratch, 0, 2 * LPT_BUCKETS * sizeof(uint32_t), c->stream));   // once, like clouds_dev at allocation: the kernels leave the histogram zeroed
    for (int r = 0; r < rounds; r++) {
        HIPCHK(c, hipMemcpyAsync(d_cost, cost, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(d_order, 0xff, (size_t)n * sizeof(uint32_t), c->stream));   // an entry this round does not write is not the previous round's
        HIPCHK(c, launch_lpt_order(d_cost, n, shift, d_scratch, d_order, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(order_out, d_order, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cost_out, d_cost, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(scratch_out, d_scratch, 2 * LPT_BUCKETS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_census_clouds(csky_ctx* c, const csky_cloud_params* p, int tile_w, const csky_bands* bands, uint32_t* counts, int n) {
    if (!c || !counts || n < 1 || n > 256) return fail(c, CSKY_ERR_INVALID, "csky_census_clouds: bad arguments (1 .. 256 counters)");
    int rc; if ((rc = bind(c))) return rc;
    if ((rc = check_bands(c, bands, tile_w))) return rc;
    const size_t rows = (size_t)bands->n_bands * bands->band_rows;
    if ((rc = c->d_frame.grow(c, (size_t)tile_w * (rows ? rows : 1)))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_stats, 0, CSKY_STATS_WORDS * sizeof(unsigned long long), c->stream));
    // the blocks of the form the headline path and the timed launches of csky_time_clouds run (no stats buffer there: no in-cloud tally, latched rays stop
    // marching), which is what the hardware counters of those launches are compared with; CSKY_CENSUS_TALLY=1: the form a stats launch runs
    const char* te = getenv("CSKY_CENSUS_TALLY");
    c->census_lean = !(te && atoi(te) != 0);
    rc = clouds_dev(c, p, tile_w, bands, c->d_frame, (size_t)tile_w * 8, c->stream, c->d_stats, true);
    c->census_lean = false;
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(counts, reinterpret_cast<const char*>(c->d_stats.get()) + 16, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_build_mips_device(csky_ctx* c, uint8_t* vol, int n, int ch, int levels) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_build_mips_device: ctx is NULL");
    // mip_args.h: the host rule (levels <= 31 and a texel left at the last level, no undefined shift) and a power-of-two n <= 1024, ch <= 4
    if (!mip_args_ok(vol, n, ch, levels, true)) return fail(c, CSKY_ERR_INVALID, "csky_build_mips_device: bad arguments");
    int rc; if ((rc = bind(c))) return rc;
    const size_t total = chain_offset(n, levels, ch), l0 = (size_t)n * n * n * ch;
    DevBuf<uint8_t> d; if ((rc = d.alloc(c, total))) return rc;
    HIPCHK(c, hipMemcpyAsync(d, vol, l0, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_mip_chain(d, n, ch, levels, c->stream));
    HIPCHK(c, hipMemcpyAsync(vol + l0, d + l0, total - l0, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_generate_detail_noise_device(csky_ctx* c, uint32_t seed, int n, uint8_t* out_rgb8) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_generate_detail_noise_device: ctx is NULL");
    if (!out_rgb8 || n < 8 || n > 256 || (n & (n - 1))) return fail(c, CSKY_ERR_INVALID, "csky_generate_detail_noise_device: n must be a power of two in [8, 256]");
    int rc; if ((rc = bind(c))) return rc;
    const size_t bytes = (size_t)n * n * n * 3;
    DevBuf<uint8_t> d; if ((rc = d.alloc(c, bytes))) return rc;
    HIPCHK(c, launch_detail_noise(seed, n, d, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_rgb8, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_encode_bc7(csky_ctx* c, const uint8_t* rgba8, int w, int h, int n_images, uint8_t* blocks_out) { return csky_encode_bc7_quality(c, rgba8, w, h, n_images, 0, blocks_out); }
int csky_encode_bc7_quality(csky_ctx* c, const uint8_t* rgba8, int w, int h, int n_images, int quality, uint8_t* blocks_out) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_encode_bc7: ctx is NULL");
    if (quality < 0 || quality > 1) return fail(c, CSKY_ERR_INVALID, "csky_encode_bc7_quality: quality is 0 or 1");
    if (!rgba8 || !blocks_out || w < 1 || h < 1 || n_images < 1 || w > 16384 || h > 16384 || n_images > 16384) return fail(c, CSKY_ERR_INVALID, "csky_encode_bc7: NULL argument or size out of range");
    int rc; if ((rc = bind(c))) return rc;
    const size_t in_bytes = (size_t)w * h * 4 * (size_t)n_images, out_bytes = (size_t)((w + 3) / 4) * ((h + 3) / 4) * 16 * (size_t)n_images;
    const size_t in_pad = (in_bytes + 15) & ~(size_t)15;        // the blocks follow the texels, 16-byte aligned
    DevBuf<uint8_t> d; if ((rc = d.alloc(c, in_pad + out_bytes))) return rc;
    uint8_t* d_out = d + in_pad;
    HIPCHK(c, hipMemcpyAsync(d, rgba8, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_bc7_encode(d, w, h, n_images, quality, reinterpret_cast<uint4*>(d_out), c->stream));
    HIPCHK(c, hipMemcpyAsync(blocks_out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_noise_inexact_coeffs(csky_ctx* c, uint64_t* n) {
    if (!c || !n) return CSKY_ERR_INVALID;
    if (!c->noise.st.have()) return fail(c, CSKY_ERR_STATE, "csky_noise_inexact_coeffs: csky_set_noise has not been called");
    *n = (uint64_t)c->noise.st.inexact();
    return CSKY_OK;
}

int csky_set_march(csky_ctx* c, int primary_steps, int light_steps) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_march: ctx is NULL");
    if (primary_steps < 1 || primary_steps > 1024 || light_steps < 0 || light_steps > 6)
        return fail(c, CSKY_ERR_INVALID, "csky_set_march: primary_steps in [1,1024], light_steps in [0,6] (RANDOM_VECTORS has 6 entries, clouds.glsl:140)");
    c->primary_steps = primary_steps; c->light_steps = light_steps; return CSKY_OK;
}

int csky_set_early_out(csky_ctx* c, float eps) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_early_out: ctx is NULL");
    if (!(eps >= 0.0f) || eps > 0.5f) return fail(c, CSKY_ERR_INVALID, "csky_set_early_out: eps must be in [0, 0.5]");
    c->early_eps = eps; return CSKY_OK;
}

int csky_set_variant(csky_ctx* c, int variant) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_variant: ctx is NULL");
    if (variant < -1 || variant >= cloud_variant_count()) return fail(c, CSKY_ERR_INVALID, "csky_set_variant: unknown variant %d", variant);
    c->variant = variant < 0 ? CSKY_DEFAULT_VARIANT : variant; return CSKY_OK;
}
int csky_set_schedule(csky_ctx* c, int mode) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_schedule: ctx is NULL");
    if (!(mode == -1 || mode == 1 || mode == 2 || mode == 5 || mode == 7))
        return fail(c, CSKY_ERR_INVALID, "csky_set_schedule: mode must be -1 (auto), 1, 2, 5 or 7 (see cloudsky.h)");
    c->sched_mode = mode; return CSKY_OK;
}
int csky_set_frames_in_flight(csky_ctx* c, int frames) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_frames_in_flight: ctx is NULL");
    if (frames < 1 || frames > RING) return fail(c, CSKY_ERR_INVALID, "csky_set_frames_in_flight: 1 .. 8 (the rings are eight deep)");
    c->frames_in_flight = c->frames_overlapping = frames;
    c->warn[0] = 0;
    if (frames >= 2) {   // CSKY_OK, but never silent: without enough hardware queues the frames' streams share one and do not overlap (csky_last_warning)
        const char* q = getenv("GPU_MAX_HW_QUEUES");
        const int qn = q ? atoi(q) : 4;                         // the HIP runtime's default
        // a queue per frame stream, one for the context's stream (the prologue runs beside the marches) and one for the host's default stream, which
        // a host that allocates or copies through HIP has used before the first frame.  Two frames at the default of four: enough (api.cpp, top)
        if (qn < frames + 2) {
            c->frames_overlapping = qn - 2 >= 2 ? qn - 2 : 1;   // what the launch policy plans for (clouds_dev): 1 = the forms that are fastest alone
            snprintf(c->warn, sizeof c->warn, "csky_set_frames_in_flight: GPU_MAX_HW_QUEUES is %s: the %d streams of consecutive frames, the library's stream and the host's default "
                     "stream need %d hardware queues or some of them share one and do not overlap (planning for %d); set it (16 is what libcloudsky sets at load time "
                     "unless CSKY_NO_ENV=1) before the process's first HIP call", q ? q : "unset (4)", frames, frames + 2, c->frames_overlapping);
        }
    }
    return CSKY_OK;
}
int csky_set_segments(csky_ctx* c, int segments) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_segments: ctx is NULL");
    if (segments != 0 && segments != 1 && segments != 2 && segments != 4 && segments != 5) return fail(c, CSKY_ERR_INVALID, "csky_set_segments: 0 (auto), 1, 2, 4 (step ranges) or 5 (4 interleaved)");
    c->segments = segments; return CSKY_OK;
}
int csky_set_exact_cells(csky_ctx* c, int mode) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_exact_cells: ctx is NULL");
    if (mode != 0 && mode != 1) return fail(c, CSKY_ERR_INVALID, "csky_set_exact_cells: 0 (only when a coefficient does not fit fp16) or 1 (always)");
    c->noise.st.request_exact(mode); return CSKY_OK;           // takes effect at the next csky_set_noise*
}
int csky_set_height_window(csky_ctx* c, int enabled) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_height_window: ctx is NULL");
    c->use_window = enabled != 0; return CSKY_OK;
}
int csky_variant_count(void) { return cloud_variant_count(); }
const char* csky_variant_name(int v) { return cloud_variant_name(v); }

int csky_sync(csky_ctx* c) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_sync: ctx is NULL");
    int rc; if ((rc = bind(c))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_render_clouds_device(csky_ctx* c, const csky_cloud_params* p, int tile_w, const csky_bands* bands, void* d_out, size_t pitch, void* hip_stream) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_clouds_device: ctx is NULL");
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "csky_render_clouds_device: d_out is NULL");
    int rc; if ((rc = bind(c))) return rc;
    hipStream_t s = stream_of(c, hip_stream);
    return clouds_dev(c, p, tile_w, bands, (uint2*)d_out, pitch, s, nullptr, true);
}

int csky_render_clouds(csky_ctx* c, const csky_cloud_params* p, int tile_w, int tile_h, uint16_t* out, size_t pitch) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_clouds: ctx is NULL");
    if (tile_w < 1 || tile_h < 1) return fail(c, CSKY_ERR_INVALID, "csky_render_clouds: empty tile");
    if (out && (pitch < (size_t)tile_w * 8)) return fail(c, CSKY_ERR_INVALID, "csky_render_clouds: row_pitch_bytes < tile_w*8");
    int rc; if ((rc = bind(c))) return rc;
    if ((rc = c->d_frame.grow(c, (size_t)tile_w * tile_h))) return rc;
    csky_bands b = {tile_h, 0, 1, 1};
    HIPCHK(c, hipMemsetAsync(c->d_stats, 0, 16, c->stream));
    if ((rc = clouds_dev(c, p, tile_w, &b, c->d_frame, (size_t)tile_w * 8, c->stream, c->d_stats, true))) return rc;
    unsigned long long st[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(st, c->d_stats, 16, hipMemcpyDeviceToHost, c->stream));
    if (out) HIPCHK(c, hipMemcpy2DAsync(out, pitch, c->d_frame, (size_t)tile_w * 8, (size_t)tile_w * 8, tile_h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last_stats.rays = (uint64_t)tile_w * tile_h; c->last_stats.incloud_samples = st[0]; c->last_stats.primary_samples = st[1] * (uint64_t)c->primary_steps;
    return CSKY_OK;
}

// ---- asynchronous host form: submit / collect over a ring of pinned frames (cloudsky.h) -----------------------------------------
int csky_set_host_ring(csky_ctx* c, int slots) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_host_ring: ctx is NULL");
    if (slots < 1 || slots > RING) return fail(c, CSKY_ERR_INVALID, "csky_set_host_ring: 1 .. 8 frames");
    for (auto& hs : c->hring) if (hs.busy) return fail(c, CSKY_ERR_STATE, "csky_set_host_ring: collect the outstanding tickets first");
    c->hslots = slots;
    return csky_set_frames_in_flight(c, slots >= 2 ? 2 : 1);    // launch policy: two frames in flight is the best choice for whole frames (csky_set_frames_in_flight)
}

int csky_submit_clouds(csky_ctx* c, const csky_cloud_params* p, int tile_w, int tile_h, int64_t* ticket) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_submit_clouds: ctx is NULL");
    if (!ticket) return fail(c, CSKY_ERR_INVALID, "csky_submit_clouds: ticket is NULL");
    if (tile_w < 1 || tile_h < 1 || tile_w > 16384 || tile_h > 16384) return fail(c, CSKY_ERR_INVALID, "csky_submit_clouds: tile size out of range");
    int rc; if ((rc = bind(c))) return rc;
    csky_ctx::HostSlot& hs = c->hring[c->next_ticket % c->hslots];
    if (hs.busy) return fail(c, CSKY_ERR_STATE, "csky_submit_clouds: %d frames are already in flight (csky_set_host_ring); collect ticket %lld first", c->hslots, (long long)hs.ticket);
    const size_t px = (size_t)tile_w * tile_h;
    if ((rc = host_slot_prepare(c, hs, px))) return rc;
    const csky_bands b = {tile_h, 0, 1, 1};
    if ((rc = clouds_dev(c, p, tile_w, &b, hs.d, (size_t)tile_w * 8, hs.s, nullptr, true))) return rc;
    HIPCHK(c, hipMemcpyAsync(hs.h, hs.d, px * 8, hipMemcpyDeviceToHost, hs.s));
    HIPCHK(c, hipEventRecord(hs.done, hs.s));
    hs.busy = true; hs.ticket = c->next_ticket; hs.w = tile_w; hs.hh = tile_h;
    *ticket = c->next_ticket++;
    return CSKY_OK;
}

int csky_collect(csky_ctx* c, int64_t ticket, const uint16_t** frame, size_t* bytes) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_collect: ctx is NULL");
    if (!frame) return fail(c, CSKY_ERR_INVALID, "csky_collect: frame is NULL");
    csky_ctx::HostSlot* hs = nullptr;
    for (auto& k : c->hring) if (k.busy && k.ticket == ticket) hs = &k;
    if (!hs) return fail(c, CSKY_ERR_STATE, "csky_collect: ticket %lld is not outstanding (never submitted, or collected already)", (long long)ticket);
    int rc; if ((rc = bind(c))) return rc;
    HIPCHK(c, hipEventSynchronize(hs->done));
    hs->busy = false;
    *frame = static_cast<const uint16_t*>(static_cast<void*>(hs->h));
    if (bytes) *bytes = (size_t)hs->w * hs->hh * 8;
    return CSKY_OK;
}

int csky_poll(csky_ctx* c, int64_t ticket) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_poll: ctx is NULL");
    for (auto& k : c->hring)
        if (k.busy && k.ticket == ticket) {
            const hipError_t e = hipEventQuery(k.done);
            if (e == hipSuccess) return 1;
            if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
            return fail(c, CSKY_ERR_HIP, "csky_poll: %s", hipGetErrorString(e));
        }
    return fail(c, CSKY_ERR_STATE, "csky_poll: ticket %lld is not outstanding", (long long)ticket);
}

int csky_set_kernel_timing(csky_ctx* c, int enabled) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_kernel_timing: ctx is NULL");
    int rc; if ((rc = bind(c))) return rc;
    c->kt.on = enabled != 0; c->kt.count = 0;
    if (c->kt.on && c->kt.ev.empty()) {      // the first pool is made HERE, not by the first timed launch: creating 512 events is ~1 ms of host time, 3 % of a 20-frame timed region
        if ((rc = c->kt.grow(c, 512))) { c->kt.on = false; return rc; }
    }
    return CSKY_OK;
}

int csky_get_kernel_ms(csky_ctx* c, float* total_ms, int* launches) {
    if (!c || !total_ms || !launches) return fail(c, CSKY_ERR_INVALID, "csky_get_kernel_ms: NULL argument");
    int rc; if ((rc = bind(c))) return rc;
    return c->kt.read_out(c, total_ms, launches);              // every launch since the last call (the pool grows on demand)
}

// The stats launch delivers the exact counts (the tally form of the kernel); the warm-up and timed launches pass no stats buffer and take the form
// the headline path takes (march_compact.h march_compact, TALLY = false): what is reported is that path's time beside the full march's counts.
int csky_time_clouds(csky_ctx* c, const csky_cloud_params* p, int tile_w, const csky_bands* bands, int warmup, int iters, float* mean_ms, csky_cloud_stats* stats) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_time_clouds: ctx is NULL");
    if (iters < 1 || warmup < 0 || !mean_ms) return fail(c, CSKY_ERR_INVALID, "csky_time_clouds: bad iters/warmup/mean_ms");
    int rc; if ((rc = bind(c))) return rc;
    if ((rc = check_bands(c, bands, tile_w))) return rc;
    const size_t rows = (size_t)bands->n_bands * bands->band_rows;
    if ((rc = c->d_frame.grow(c, (size_t)tile_w * (rows ? rows : 1)))) return rc;
    const size_t pitch = (size_t)tile_w * 8;
    HIPCHK(c, hipMemsetAsync(c->d_stats, 0, 16, c->stream));
    if ((rc = clouds_dev(c, p, tile_w, bands, c->d_frame, pitch, c->stream, c->d_stats, true))) return rc;   // stats launch (+ frame setup)
    for (int i = 0; i < warmup; i++) if ((rc = clouds_dev(c, p, tile_w, bands, c->d_frame, pitch, c->stream, nullptr, false))) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < iters; i++) if ((rc = clouds_dev(c, p, tile_w, bands, c->d_frame, pitch, c->stream, nullptr, false))) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *mean_ms = ms / (float)iters;
    unsigned long long st[2] = {0, 0};
    HIPCHK(c, hipMemcpy(st, c->d_stats, 16, hipMemcpyDeviceToHost));
    c->last_stats.rays = (uint64_t)tile_w * rows; c->last_stats.incloud_samples = st[0]; c->last_stats.primary_samples = st[1] * (uint64_t)c->primary_steps;
    if (stats) *stats = c->last_stats;
    return CSKY_OK;
}

int csky_generate_shape_noise_device(csky_ctx* c, uint32_t seed, int n, uint8_t* out_rgba8) { return csky_generate_shape_noise_tuned_device(c, seed, n, nullptr, out_rgba8); }
int csky_generate_shape_noise_tuned_device(csky_ctx* c, uint32_t seed, int n, const csky_shape_noise_params* params, uint8_t* out_rgba8) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_generate_shape_noise_device: ctx is NULL");
    if (!out_rgba8 || n < 8 || n > 512 || (n & (n - 1))) return fail(c, CSKY_ERR_INVALID, "csky_generate_shape_noise_device: n must be a power of two in [8, 512]");
    ShapeNoiseParams P = shape_noise_defaults();
    if (params) {
        if (csky_check_shape_noise_params(params, n)) return fail(c, CSKY_ERR_INVALID, "csky_generate_shape_noise_tuned_device: %s", csky_assets_last_error());
        memcpy(&P, params, sizeof P);
    }
    int rc; if ((rc = bind(c))) return rc;
    const size_t bytes = (size_t)n * n * n * 4;
    DevBuf<uint32_t> d; if ((rc = d.alloc(c, bytes / 4))) return rc;
    HIPCHK(c, launch_shape_noise(seed, n, P, d, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_rgba8, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_get_cloud_stats(csky_ctx* c, csky_cloud_stats* stats) {
    if (!c || !stats) return fail(c, CSKY_ERR_INVALID, "csky_get_cloud_stats: NULL argument");
    *stats = c->last_stats; return CSKY_OK;
}

int csky_interleave_bands_device(csky_ctx* c, const void* d_gathered, size_t member_stride_bytes, int members, size_t band_bytes, int total_bands, void* d_frame, void* hip_stream) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_interleave_bands_device: ctx is NULL");
    if (!d_gathered || !d_frame || members < 1 || total_bands < 0) return fail(c, CSKY_ERR_INVALID, "csky_interleave_bands_device: NULL argument or bad counts");
    if (band_bytes % 16 || member_stride_bytes % 16 || ((uintptr_t)d_gathered & 15) || ((uintptr_t)d_frame & 15))
        return fail(c, CSKY_ERR_INVALID, "csky_interleave_bands_device: band size, member stride and both pointers must be multiples of 16 bytes");
    const size_t local = ((size_t)total_bands + members - 1) / members;
    if (local * band_bytes > member_stride_bytes) return fail(c, CSKY_ERR_INVALID, "csky_interleave_bands_device: a member's %zu bands of %zu bytes do not fit its stride of %zu", local, band_bytes, member_stride_bytes);
    int rc; if ((rc = bind(c))) return rc;
    HIPCHK(c, launch_interleave_bands(d_gathered, member_stride_bytes, members, band_bytes, total_bands, d_frame, hip_stream ? (hipStream_t)hip_stream : c->stream));
    return CSKY_OK;
}

}  // extern "C"
