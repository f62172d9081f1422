// stage_trace.cpp -- ANALYSIS TOOL (host, g++): runs the kernel cores over a frame and records, for every primary sample and
// every light-march sample, how far density() got before an exact reject (0 window, 1 weather/gradient, 2 shape, 3 detail with
// t <= 0, 4 t > 0).  tools/stage_trace/analyse.py turns the trace into per-stage lane utilisation of 8x8-ray wavefronts.
// stage_trace() counts the UNSKIPPED march: every in-cloud sample with its light march.  stage_trace_ex(skip = 1) applies the saturation skip
// (cloud_core.h ray_saturated): a ray latches before the first in-cloud sample at which the predicate holds and its later in-cloud samples are
// counted in skipped_out, not light-marched.  The kernel tests once per flush, i.e. latches up to one flush of its wavefront later: the share
// reported here is the upper bound of what the kernel leaves out.
#include <cstdint>
#include <cstring>
#include <vector>
#define CSKY_TRACE_STAGES 1
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/cloud_core.h"
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/lut_core.h"
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/noise_set.h"
namespace csky { thread_local int csky_stage = 0; }
using namespace csky;

extern "C" void stage_trace_ex(const uint8_t* large_chain, const uint8_t* small_chain, const uint8_t* weather_rgb8, const float params[28],
                               int primary_steps, int light_steps, int w, int h, uint8_t* primary_stage /* [h][w][steps] */,
                               uint64_t* light_hist /* [7][5] */, float* window_out, int skip, uint64_t* skipped_out /* [2]: rays latched, in-cloud samples skipped */) {
    std::vector<uint8_t> lc(large_chain, large_chain + RAW_SHAPE_CHAIN);
    std::vector<uint8_t> sc(small_chain, small_chain + RAW_DETAIL_CHAIN);
    std::vector<ShapeTexel> shape; std::vector<uint4> detail, weather;
    uint32_t so[SHAPE_LEVELS], dof[DETAIL_LEVELS];
    bake_shape(lc, shape, so); bake_detail(sc, detail, dof); bake_weather(weather_rgb8, weather);
    // LUTs with the kernel cores (transmittance 256x64, sky 200x100), fp16-rounded like the device textures
    const int tw = 256, th = 64, sw = 200, sh = 100;
    std::vector<float4> tf((size_t)tw * th), sky((size_t)sw * sh);
    for (int y = 0; y < th; y++) for (int x = 0; x < tw; x++) { F4 t = transmittance_texel(x, y, (float)tw, (float)th); tf[(size_t)y * tw + x] = float4{h2f(f2h(t.x)), h2f(f2h(t.y)), h2f(f2h(t.z)), h2f(f2h(t.w))}; }
    CloudParams P; memcpy(&P, params, sizeof P);
    const float sun[3] = {P.LIGHT_DIRECTION[0], P.LIGHT_DIRECTION[1], P.LIGHT_DIRECTION[2]};
    for (int y = 0; y < sh; y++) for (int x = 0; x < sw; x++) { F4 c = sky_texel(x, y, (float)sw, (float)sh, sun, tf.data(), tw, th); sky[(size_t)y * sw + x] = float4{h2f(f2h(c.x)), h2f(f2h(c.y)), h2f(f2h(c.z)), h2f(f2h(c.w))}; }
    TexSet T; T.shape = shape.data(); T.detail = detail.data(); T.weather = weather.data(); T.sky = sky.data(); T.sky_w = sw; T.sky_h = sh;
    T.detail_h = nullptr; T.detail_lds = nullptr;
    T.detail_lod5 = detail_lod5_value(sc.data() + RAW_DETAIL_LOD5);
    const ExactRejects rej = exact_rejects(weather_range(weather_rgb8), P.cloud_coverage, true);   // the window alone: ct_mode stays at the general form
    window_out[0] = rej.hf_lo; window_out[1] = rej.hf_hi;
    FrameConsts fc;
    frame_setup(P, sky.data(), sw, sh, primary_steps, light_steps, 0.0f, rej.hf_lo, rej.hf_hi, fc);
    for (int k = 0; k < 35; k++) light_hist[k] = 0;
    if (skipped_out) skipped_out[0] = skipped_out[1] = 0;
    const float nd = -fc.density;
    for (int gy = 0; gy < h; gy++) for (int gx = 0; gx < w; gx++) {
        uint8_t* st = primary_stage + ((size_t)gy * w + gx) * primary_steps;
        Ray ray = ray_setup(fc, gx, gy);
        if (!ray.above) { memset(st, 255, primary_steps); continue; }
        float px = ray.px, py = ray.py, pz = ray.pz;
        const float ct = fc.ldir[0] * ray.dx + fc.ldir[1] * ray.dy + fc.ldir[2] * ray.dz;
        const float phase = fmaxf(fmaxf(henyey_greenstein(ct, 0.6f), henyey_greenstein(ct, fc.hg_g2)), henyey_greenstein(ct, -0.2f));
        float B[3], Tr = 1.0f, alpha = 0.0f, L[3] = {0.0f, 0.0f, 0.0f};
        ray_saturation_bound(fc, phase, B);
        bool latched = false;
        for (int i = 0; i < primary_steps; i++) {
            advance(px, py, pz, ray.sx, ray.sy, ray.sz);
            const float hf = height_fraction(length3_exact(px, py, pz));
            const float t = sample_density(T, fc, px, py, pz, hf, fc.wpos_x, fc.wpos_y, 0, 0);
            st[i] = (uint8_t)(t > 0.0f ? 4 : csky_stage);
            if (t > 0.0f) {
                if (skip && fc.sat_skip && !latched && ray_saturated(fc, Tr, alpha, L, B)) { latched = true; if (skipped_out) skipped_out[0]++; }
                if (latched) { if (skipped_out) skipped_out[1]++; continue; }
                float lx = px, ly = py, lz = pz, cd = 0.0f;
                for (int j = 0; j < light_steps; j++) {
                    advance(lx, ly, lz, fc.linc[j][0], fc.linc[j][1], fc.linc[j][2]);
                    const float lhf = height_fraction(length3_exact(lx, ly, lz));
                    const float d = sample_density(T, fc, lx, ly, lz, lhf, fc.wpos_x, fc.wpos_y, j > 2 ? j - 2 : 0, j);
                    light_hist[j * 5 + (d > 0.0f ? 4 : csky_stage)]++;
                    cd += d;
                }
                lx = px; ly = py; lz = pz;
                advance(lx, ly, lz, fc.ldist[0], fc.ldist[1], fc.ldist[2]);
                const float lhf = height_fraction(length3_exact(lx, ly, lz));
                const float d = sample_density(T, fc, lx, ly, lz, lhf, 0.0f, 0.0f, 3, 5);
                light_hist[6 * 5 + (d > 0.0f ? 4 : csky_stage)]++;
                cd += fast_pow(d, (1.0f - lhf) * 0.8f + 0.5f);
                shade_sample(fc, phase, t, hf, fast_exp(nd * t * ray.ss), cd, Tr, alpha, L[0], L[1], L[2]);
            }
        }
    }
}
extern "C" void stage_trace(const uint8_t* large_chain, const uint8_t* small_chain, const uint8_t* weather_rgb8, const float params[28],
                            int primary_steps, int light_steps, int w, int h, uint8_t* primary_stage /* [h][w][steps] */,
                            uint64_t* light_hist /* [7][5] */, float* window_out) {
    stage_trace_ex(large_chain, small_chain, weather_rgb8, params, primary_steps, light_steps, w, h, primary_stage, light_hist, window_out, 0, nullptr);
}
