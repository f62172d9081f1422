// sat_walk.cpp -- TEST TOOL ONLY.  Walks every ray of a frame with the kernel cores (cloud_core.h, compiled for the host) twice in one pass:
// the full march, and the march that FREEZES the ray's (L, alpha) the first time the saturation predicate (cloud_core.h ray_saturated: exact
// reject (4)) holds -- evaluated before every in-cloud sample, the earliest any flush of march_compact could latch the ray.  Reports how many
// rays fired, how many in-cloud samples fall behind the firing, and how many rays store a different half in the two marches (must be 0).
// alpha_min < 0 uses ray_saturated() itself; alpha_min >= 0 is the MUTATION CONTROL: the same test with that alpha threshold and the colour
// bound B scaled by b_scale, which must produce differing halfs or the comparison proves nothing.
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/cloud_core.h"
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/noise_set.h"

using namespace csky;

static bool mutated_saturated(const FrameConsts& fc, float T, float alpha, const float L[3], const float B[3], float alpha_min, float b_scale) {
    bool s = alpha >= alpha_min;
    for (int c = 0; c < 3; c++) {
        const float hi = L[c] + (B[c] * b_scale * T * fc.sat_kT + L[c] * fc.sat_kL);
        s = s && L[c] >= 6.103515625e-5f && hi < 65504.0f && f2h(hi) == f2h(L[c]);
    }
    return s;
}

struct Tally { double rays = 0, ic_full = 0, ic_frozen = 0, fired = 0, after = 0, differ = 0; };

static void walk_rows(const TexSet& T, const FrameConsts& fc, int w, int y0, int y1, float alpha_min, float b_scale, uint8_t* fired_map, Tally& out) {
    const float nd = -fc.density;
    for (int gy = y0; gy < y1; gy++) for (int gx = 0; gx < w; gx++) {
        Ray ray = ray_setup(fc, gx, gy);
        if (!ray.above) continue;
        out.rays++;
        const float ct = fc.ldir[0] * ray.dx + fc.ldir[1] * ray.dy + fc.ldir[2] * ray.dz;
        const float phase = fmaxf(fmaxf(henyey_greenstein(ct, 0.6f), henyey_greenstein(ct, fc.hg_g2)), henyey_greenstein(ct, -0.2f));
        float B[3];
        ray_saturation_bound(fc, phase, B);
        float Tr = 1.0f, alpha = 0.0f, L[3] = {0.0f, 0.0f, 0.0f};
        bool fired = false;
        float Lf[3] = {0.0f, 0.0f, 0.0f}, af = 0.0f;
        uint32_t ic = 0, composited = 0, skipped = 0;
        float px = ray.px, py = ray.py, pz = ray.pz;
        for (int i = 0; i < fc.primary_steps; i++) {
            advance(px, py, pz, ray.sx, ray.sy, ray.sz);
            const float hf = height_fraction(length3_shell(px, py, pz));
            const float t = sample_density(T, fc, px, py, pz, hf, fc.wpos_x, fc.wpos_y, 0, 0);
            if (!(t > 0.0f)) continue;
            ic++;
            if (!fired && fc.sat_skip) {
                const bool s = alpha_min < 0.0f ? ray_saturated(fc, Tr, alpha, L, B) : mutated_saturated(fc, Tr, alpha, L, B, alpha_min, b_scale);
                if (s) { fired = true; Lf[0] = L[0]; Lf[1] = L[1]; Lf[2] = L[2]; af = alpha; }
            }
            if (fired) skipped++; else composited++;
            float lx = px, ly = py, lz = pz, cd = 0.0f;
            for (int j = 0; j < fc.light_steps; j++) {
                advance(lx, ly, lz, fc.linc[j][0], fc.linc[j][1], fc.linc[j][2]);
                const float lhf = height_fraction(length3_shell(lx, ly, lz));
                cd += sample_density(T, fc, lx, ly, lz, lhf, fc.wpos_x, fc.wpos_y, j > 2 ? j - 2 : 0, j);
            }
            lx = px; ly = py; lz = pz;
            advance(lx, ly, lz, fc.ldist[0], fc.ldist[1], fc.ldist[2]);
            const float lhf = height_fraction(length3_shell(lx, ly, lz));
            const float ld = sample_density(T, fc, lx, ly, lz, lhf, 0.0f, 0.0f, 3, 5);
            cd += fast_pow(ld, (1.0f - lhf) * 0.8f + 0.5f);
            const float dt = fast_exp(nd * t * ray.ss);
            shade_sample(fc, phase, t, hf, dt, cd, Tr, alpha, L[0], L[1], L[2]);
        }
        out.ic_full += ic; out.ic_frozen += composited + skipped;
        if (fired) {
            out.fired++; out.after += skipped;
            if (fired_map) fired_map[(size_t)gy * w + gx] = 1;
            if (f2h(Lf[0]) != f2h(L[0]) || f2h(Lf[1]) != f2h(L[1]) || f2h(Lf[2]) != f2h(L[2]) || f2h(sat(af)) != f2h(sat(alpha))) out.differ++;
        }
    }
}

extern "C" {
// out[8] = above-horizon rays, in-cloud samples of the full march, of the frozen march (composited + counted behind the firing), rays fired,
// in-cloud samples behind the firing, rays with a differing stored half, fc.sat_skip, 0.  fired_map (may be NULL): h x w bytes, 1 where the ray fired.
void sat_walk(const uint8_t* large_chain, const uint8_t* small_chain, const uint8_t* weather_rgb8, const float params[28], int primary_steps, int light_steps,
              const uint16_t* sky_h, int sw, int sh, int w, int h, float alpha_min, float b_scale, int threads, double out[8], uint8_t* fired_map) {
    std::vector<uint8_t> lc(large_chain, large_chain + RAW_SHAPE_CHAIN);
    std::vector<uint8_t> sc(small_chain, small_chain + RAW_DETAIL_CHAIN);
    std::vector<ShapeTexel> shape; std::vector<uint4> detail, weather;
    uint32_t so[SHAPE_LEVELS], dof[DETAIL_LEVELS];
    bake_shape(lc, shape, so); bake_detail(sc, detail, dof); bake_weather(weather_rgb8, weather);
    std::vector<float4> sky((size_t)sw * sh);
    for (size_t i = 0; i < sky.size(); i++) sky[i] = float4{h2f(sky_h[4 * i]), h2f(sky_h[4 * i + 1]), h2f(sky_h[4 * i + 2]), h2f(sky_h[4 * i + 3])};
    TexSet T; T.shape = shape.data(); T.detail = detail.data(); T.weather = weather.data(); T.sky = sky.data(); T.sky_w = sw; T.sky_h = sh;
    T.detail_h = nullptr; T.detail_lds = nullptr;
    T.detail_lod5 = detail_lod5_value(sc.data() + RAW_DETAIL_LOD5);
    CloudParams P; memcpy(&P, params, sizeof P);
    const ExactRejects rej = exact_rejects(weather_range(weather_rgb8), P.cloud_coverage, true);
    FrameConsts fc;
    frame_setup(P, sky.data(), sw, sh, primary_steps, light_steps, 0.0f, rej.hf_lo, rej.hf_hi, fc);
    fc.ct_mode = rej.ct_mode;
    if (fired_map) memset(fired_map, 0, (size_t)w * h);
    const int nt = threads < 1 ? 1 : threads;
    std::vector<Tally> tl(nt);
    std::vector<std::thread> th;
    const int rows = (h + nt * 4 - 1) / (nt * 4);               // interleaved row blocks: the cloudy rows are not one thread's
    for (int k = 0; k < nt; k++) th.emplace_back([&, k] {
        for (int y0 = k * rows; y0 < h; y0 += nt * rows) walk_rows(T, fc, w, y0, y0 + rows < h ? y0 + rows : h, alpha_min, b_scale, fired_map, tl[k]);
    });
    for (auto& t : th) t.join();
    Tally s;
    for (const Tally& t : tl) { s.rays += t.rays; s.ic_full += t.ic_full; s.ic_frozen += t.ic_frozen; s.fired += t.fired; s.after += t.after; s.differ += t.differ; }
    out[0] = s.rays; out[1] = s.ic_full; out[2] = s.ic_frozen; out[3] = s.fired; out[4] = s.after; out[5] = s.differ; out[6] = fc.sat_skip; out[7] = 0;
}

// the frame-constant guard alone: fc.sat_skip for a push-constant block (the sky LUT as above)
int sat_walk_guard(const float params[28], int primary_steps, const uint16_t* sky_h, int sw, int sh) {
    std::vector<float4> sky((size_t)sw * sh);
    for (size_t i = 0; i < sky.size(); i++) sky[i] = float4{h2f(sky_h[4 * i]), h2f(sky_h[4 * i + 1]), h2f(sky_h[4 * i + 2]), h2f(sky_h[4 * i + 3])};
    CloudParams P; memcpy(&P, params, sizeof P);
    FrameConsts fc;
    frame_setup(P, sky.data(), sw, sh, primary_steps, 6, 0.0f, -1.0f, 2.0f, fc);
    return fc.sat_skip;
}
}
