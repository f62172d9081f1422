// noise_set.h -- what a context knows about its bound noise textures (csky_set_noise*): the sizes of every buffer of the set, the values derived
// from the textures once per bind (the weather map's channel ranges, the one texel of detail LOD 5) and per coverage (the exact rejects of a density
// sample), and the steps that keep them consistent across a rebind.  context.h (NoiseSet) holds the memory; api.cpp, clouds_launch.cpp and
// api_shadow.cpp change and read the state through NoiseHeld alone; the host tools (tests/hostsim, tilewalk, satwalk, shadow_host,
// tools/stage_trace) derive the same values from the same functions.
// Free of HIP, like sky_lut_reuse.h and frame_ring.h: tests/noise_set_host builds this header with g++ and walks it against a model.
#pragma once
#include <cstddef>
#include <cstdint>
#include "bake.h"

namespace csky {

// ---- sizes.  A chain is every mip level of an n^3 volume back to back, level 0 first.
constexpr size_t chain_texels(int n, int levels) {             // texels of the first `levels` levels = the texel offset of level `levels`
    size_t t = 0;
    for (int l = 0; l < levels; l++) { const size_t m = (size_t)(n >> l); t += m * m * m; }
    return t;
}
constexpr size_t SHAPE_CHAIN_TEXELS = chain_texels(SHAPE_N, SHAPE_LEVELS), WEATHER_TEXELS = (size_t)WEATHER_N * WEATHER_N;
static_assert(chain_texels(DETAIL_N, DETAIL_LEVELS) == (size_t)DETAIL_CHAIN_TEXELS, "detail chain size");
// the 8-bit inputs, in bytes (RGBA shape, RGB detail, RGB weather); == bake_core.h chain_offset(n, levels, channels)
constexpr size_t RAW_SHAPE_L0 = chain_texels(SHAPE_N, 1) * 4, RAW_SHAPE_CHAIN = SHAPE_CHAIN_TEXELS * 4;
constexpr size_t RAW_DETAIL_L0 = chain_texels(DETAIL_N, 1) * 3, RAW_DETAIL_CHAIN = (size_t)DETAIL_CHAIN_TEXELS * 3;
constexpr size_t RAW_DETAIL_LOD5 = chain_texels(DETAIL_N, 5) * 3;   // byte offset of the one texel of detail LOD 5
constexpr size_t RAW_WEATHER = WEATHER_TEXELS * 3;
// the baked layouts, in elements: fp16-pair cells (csky_common.h; one ShapeTexel / uint4 per texel, the unpacked detail numerators padded to a
// 16-byte multiple) and exact cells (bake_core.h; float4s per texel)
constexpr size_t SHAPE_CELLS = SHAPE_CHAIN_TEXELS, DETAIL_CELLS = DETAIL_CHAIN_TEXELS, WEATHER_CELLS = WEATHER_TEXELS, DETAIL_H_HALFS = DETAIL_CELLS + 8;
constexpr size_t SHAPE32_F4 = SHAPE_CHAIN_TEXELS * 4, DETAIL32_F4 = DETAIL_CELLS * 2, WEATHER32_F4 = WEATHER_TEXELS * 2;

// ---- derived values
// Range of the weather map's cloud-type (R) and coverage (B) channels as texel values 0..255: what the device bake delivers and what
// weather_range scans on the host.
struct WeatherRange { int rmin = 0, rmax = 255, bmax = 255; };

inline WeatherRange weather_range(const uint8_t* rgb8) {
    WeatherRange w; w.rmin = 255; w.rmax = 0; w.bmax = 0;
    for (size_t i = 0; i < WEATHER_TEXELS; i++) {
        const int r = rgb8[3 * i], b = rgb8[3 * i + 2];
        w.rmin = r < w.rmin ? r : w.rmin; w.rmax = r > w.rmax ? r : w.rmax; w.bmax = b > w.bmax ? b : w.bmax;
    }
    return w;
}

// detail LOD 5 is one texel: every tap at that level returns it as hfbm (cloud_core.h::detail_tap, clouds.glsl:133)
inline float detail_lod5_value(const uint8_t t5[3]) { return (float)(5 * t5[0] + 2 * t5[1] + t5[2]) * (1.0f / (8.0f * 255.0f)); }

// What the exact specialisations of a density sample take (csky_set_height_window switches them together): the height window outside which
// density() is 0 for the whole weather map (bake.h height_window), and FrameConsts::ct_mode -- every cloud-type texel >= 128 (1) or <= 127 (2)
// fixes the branch of the height gradient, 0 leaves it to the sample.  Window off: nothing is rejected and nothing specialised.
struct ExactRejects { float hf_lo, hf_hi; int ct_mode; };

inline ExactRejects exact_rejects(const WeatherRange& w, float coverage, bool use_window) {
    ExactRejects r = {-1.0f, 2.0f, 0};
    if (!use_window) return r;
    height_window((double)coverage, w.rmin / 255.0, w.rmax / 255.0, w.bmax / 255.0, r.hf_lo, r.hf_hi);
    r.ct_mode = w.rmin >= 128 ? 1 : (w.rmax <= 127 ? 2 : 0);
    return r;
}

// ---- the state.  None of the steps touches a buffer: the caller does what the names say, in this order (api.cpp set_noise):
//   arguments valid -> begin_rebind -> allocate, upload, bake, read back -> bound -> exact layouts built or released -> ready
// and for the weather map alone (api.cpp set_weather), legal only while a set is had:
//   arguments valid, have() -> the weather cells (and the exact ones when cell32()) baked, range read back -> reweathered
// (a runtime failure after that bake has begun goes through begin_rebind: half-baked cells are not marched)
// A step that fails returns between begin_rebind and ready, which leaves freed or half-baked textures: nothing is had, and no render runs until
// a later bind succeeds.
class NoiseHeld {
    bool have_ = false, cell32_ = false, exact_requested_ = false;
    unsigned long long inexact_ = 0;
    WeatherRange range_;
    float lod5_ = 0.0f;
    bool cached_ = false; float cached_cov_ = 0.0f; ExactRejects cached_rej_ = {-1.0f, 2.0f, 0};   // rejects(): one entry, window on
public:
    void request_exact(int mode) { exact_requested_ = mode == 1; }   // csky_set_exact_cells: takes effect at the next bound()
    void begin_rebind() { have_ = false; cached_ = false; }
    // The bake's results.  Textures whose cells do not fit fp16 (white noise, checkerboards: inexact > 0) are marched on EXACT cells: the same
    // polynomial with fp32 coefficients (bake_core.h), twice the bytes per tap, the compact whole-ray kernel on TexSet32; a request asks for them
    // regardless (A/B, tests).  Returns cell32(): whether the caller builds the exact layouts or releases those of an earlier bind.
    bool bound(unsigned long long inexact, const WeatherRange& range, float lod5) {
        inexact_ = inexact; range_ = range; lod5_ = lod5; cached_ = false;
        return cell32_ = inexact != 0 || exact_requested_;
    }
    void ready() { have_ = true; }
    // A rebind of the weather map alone (api.cpp set_weather), between two frames of a set that is had: its range replaces the bound one and the
    // cached rejects of the old range go.  A weather cell's coefficients always fit fp16 (bake_core.h::bake_weather_texel: all in [-510, 510]), so
    // neither the inexact count nor the cell format can change, and a request for exact cells still waits for the next bound().  Returns whether
    // the step was legal; without a set that is had it changes nothing.
    bool reweathered(const WeatherRange& range) {
        if (!have_) return false;
        range_ = range; cached_ = false;
        return true;
    }
    // exact_rejects for the bound weather map, cached per coverage value (the bisections of height_window are not per-frame work).  Keyed on !=, so
    // a NaN coverage is computed every time.
    ExactRejects rejects(float coverage, bool use_window) {
        if (!use_window) return exact_rejects(range_, coverage, false);
        if (!cached_ || cached_cov_ != coverage) { cached_rej_ = exact_rejects(range_, coverage, true); cached_cov_ = coverage; cached_ = true; }
        return cached_rej_;
    }
    bool have() const { return have_; }
    bool cell32() const { return cell32_; }
    unsigned long long inexact() const { return inexact_; }
    float detail_lod5() const { return lod5_; }
    WeatherRange range() const { return range_; }             // what rejects() decides with (csky_read_baked_texture, which == 9)
};

}  // namespace csky
