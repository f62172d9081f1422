// view_update_host.cpp -- TEST TOOL ONLY.  Compiles the per-lane core of the temporal split of a view frame (csrc/view_update_core.h: what the lanes of
// clouds_view_fresh_kernel and clouds_view_reproject_kernel run around the march) and cloud_core.h's march() for the HOST with g++, so that the
// `-m "not gpu"` suite can hold it to the numpy restatement of its definition (tests/view_update_reference.py) without a GPU, and the GPU tests have
// the core's own taps to compare against.  It is NOT part of libcloudsky and is never a render fallback: the product has no CPU path.
#include <cstdint>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/view_update_core.h"
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/noise_set.h"

using namespace csky;

namespace {
std::vector<float4> widen(const uint16_t* img, int w, int h) {
    std::vector<float4> f((size_t)w * h);
    for (size_t i = 0; i < f.size(); i++) f[i] = float4{h2f(img[4 * i]), h2f(img[4 * i + 1]), h2f(img[4 * i + 2]), h2f(img[4 * i + 3])};
    return f;
}
// same_mode: 0 = the rule (view_update_geom decides), 1 = forced off (the formula even for equal cameras)
ViewUpdateGeom geom(const float view[10], const float* prev_view, int w, int h, uint32_t prev_pitch_px, int block, int phase, int same_mode) {
    ViewUpdateGeom g = view_update_geom(view, prev_view, w, h, (uint32_t)w, prev_pitch_px, block, phase);
    if (same_mode == 1) g.same = 0;
    return g;
}
}  // namespace

extern "C" {

// The block's integer fields as view_update_geom fills them: out[0..6] = block, px, py, sub_w, sub_h, same, has_history
void view_update_host_geom(const float view[10], const float* prev_view, int w, int h, int block, int phase, int* out) {
    const ViewUpdateGeom g = geom(view, prev_view, w, h, (uint32_t)w, block, phase, 0);
    out[0] = g.block; out[1] = g.px; out[2] = g.py; out[3] = g.sub_w; out[4] = g.sub_h; out[5] = g.same; out[6] = g.has_history;
}

// Every pixel of a w x h update: kind [h][w] (ViewUpdateKind), uxuy [h][w][2] as view_update_classify leaves them, dirs [h][w][3] (may be NULL).
void view_update_host_classify(const float view[10], const float* prev_view, int w, int h, int block, int phase, int same_mode, uint8_t* kind, float* uxuy, float* dirs) {
    const ViewUpdateGeom g = geom(view, prev_view, w, h, (uint32_t)w, block, phase, same_mode);
    for (int j = 0; j < h; j++) for (int i = 0; i < w; i++) {
        const size_t at = (size_t)j * w + i;
        float ex, ey, ez;
        view_update_dir(g, i, j, ex, ey, ez);
        const ViewUpdateClass c = view_update_classify(g, i, j, ex, ey, ez);
        kind[at] = (uint8_t)c.kind; uxuy[2 * at] = c.ux; uxuy[2 * at + 1] = c.uy;
        if (dirs) { dirs[3 * at] = ex; dirs[3 * at + 1] = ey; dirs[3 * at + 2] = ez; }
    }
}

// view_update_tap at n coordinates of a w x h image of pitch_px pixels per row: out [n][4] halfs
void view_update_host_tap(const uint16_t* prev, uint32_t pitch_px, int w, int h, int n, const float* uxuy, uint16_t* out) {
    for (int k = 0; k < n; k++) {
        const uint2 t = view_update_tap(reinterpret_cast<const uint2*>(prev), pitch_px, w, h, uxuy[2 * k], uxuy[2 * k + 1]);
        memcpy(out + 4 * (size_t)k, &t, 8);
    }
}

// A whole update as the two kernels' lanes compute it, with the lock-step march() where they march: mip chains -> baked layouts (as
// tests/rays_host rays_host_march), then per pixel classify -> zero / prev's texel / tap / march.  prev (tightly packed; NULL with prev_view NULL),
// out [h][w][4] halfs, kind [h][w], taps (may be NULL): how many texels of prev were read.
void view_update_host_update(const uint8_t* large_chain, const uint8_t* small_chain, const uint8_t* weather_rgb8, const float params[28], int primary_steps, int light_steps,
                             const uint16_t* sky_h, int sw, int sh, const float view[10], const float* prev_view, int w, int h, int block, int phase, const uint16_t* prev,
                             uint16_t* out, uint8_t* kind, uint64_t* taps) {
    std::vector<uint8_t> lc(large_chain, large_chain + RAW_SHAPE_CHAIN);
    std::vector<uint8_t> sc(small_chain, small_chain + RAW_DETAIL_CHAIN);
    std::vector<ShapeTexel> shape; std::vector<uint4> detail, weather;
    uint32_t so[SHAPE_LEVELS], dof[DETAIL_LEVELS];
    bake_shape(lc, shape, so); bake_detail(sc, detail, dof); bake_weather(weather_rgb8, weather);
    std::vector<float4> sky = widen(sky_h, sw, sh);
    TexSet T;
    T.shape = shape.data(); T.detail = detail.data(); T.weather = weather.data(); T.sky = sky.data(); T.sky_w = sw; T.sky_h = sh;
    T.detail_h = nullptr; T.detail_lds = nullptr;
    T.detail_lod5 = detail_lod5_value(sc.data() + RAW_DETAIL_LOD5);
    CloudParams P; memcpy(&P, params, sizeof P);
    P.texture_size[0] = P.texture_size[1] = 1.0f; P.update_position[0] = P.update_position[1] = 0.0f;   // not read by this path (api_rays.cpp)
    const ExactRejects rej = exact_rejects(weather_range(weather_rgb8), P.cloud_coverage, true);
    FrameConsts fc;
    frame_setup(P, sky.data(), sw, sh, primary_steps, light_steps, 0.0f, rej.hf_lo, rej.hf_hi, fc);
    fc.ct_mode = rej.ct_mode;
    const ViewUpdateGeom g = geom(view, prev ? prev_view : nullptr, w, h, (uint32_t)w, block, phase, 0);
    const uint2* pv = reinterpret_cast<const uint2*>(prev);
    uint64_t read = 0;
    for (int j = 0; j < h; j++) for (int i = 0; i < w; i++) {
        const size_t at = (size_t)j * w + i;
        float ex, ey, ez;
        view_update_dir(g, i, j, ex, ey, ez);
        const ViewUpdateClass c = view_update_classify(g, i, j, ex, ey, ez);
        uint2 t; t.x = 0u; t.y = 0u;
        if (c.kind == VU_COPY) { t = pv[(size_t)j * g.prev_pitch_px + i]; read += 1; }
        else if (c.kind == VU_TAP) { t = view_update_tap(pv, g.prev_pitch_px, w, h, c.ux, c.uy); read += 4; }
        else if (c.kind == VU_FRESH || c.kind == VU_HOLE) {
            const MarchOut o = march(T, fc, rays_ray(fc, ex, ey, ez));
            t = pack_half4(f2h(o.r), f2h(o.g), f2h(o.b), f2h(o.a));
        }
        memcpy(out + 4 * at, &t, 8);
        kind[at] = (uint8_t)c.kind;
    }
    if (taps) *taps = read;
}

}
