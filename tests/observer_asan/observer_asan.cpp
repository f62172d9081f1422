// observer_asan.cpp -- TEST TOOL ONLY.  The front end of the direct cloud march from an observer's position (csrc/observer_core.h) and the lock-step
// march behind it (cloud_core.h march()) in a program of its own built with -fsanitize=address,undefined (tests/test_observer_edges_host.py runs it on
// the CPU): cells baked from a seeded random texture set, then the rays whose cap lies within the fp32 quantum of their segment's start (the corner
// observer_ray's last clause closes) and 10 000 seeded random unit directions from each observer at the ends of what observer_invalid accepts
// (tests/observers.py EDGE, restated here: a program of its own reads no Python).  Every texel must be finite, a ray that is not marched must give a
// zero texel, and no corner ray may come back marched with a field that is not finite.
// Prints "observer asan ok <rays marched> <rays in cloud>" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/observer_core.h"
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/noise_set.h"

using namespace csky;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { if (failures < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }
static float unit() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }
static void direction(float e[3]) {                            // uniform on the sphere: a point of the cube inside the ball, normalised
    for (;;) {
        const double x = 2.0 * unit() - 1.0, y = 2.0 * unit() - 1.0, z = 2.0 * unit() - 1.0, l2 = x * x + y * y + z * z;
        if (l2 < 1e-4 || l2 > 1.0) continue;
        const double l = std::sqrt(l2);
        e[0] = (float)(x / l); e[1] = (float)(y / l); e[2] = (float)(z / l);
        return;
    }
}

struct Observer { const char* name; float pos[3]; float cap; };

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<uint8_t> lc(RAW_SHAPE_CHAIN), sc(RAW_DETAIL_CHAIN), wm(RAW_WEATHER);
    for (uint8_t& b : lc) b = (uint8_t)rnd();
    for (uint8_t& b : sc) b = (uint8_t)rnd();
    for (uint8_t& b : wm) b = (uint8_t)rnd();
    std::vector<ShapeTexel> shape; std::vector<uint4> detail, weather;
    uint32_t so[SHAPE_LEVELS], dof[DETAIL_LEVELS];
    bake_shape(lc, shape, so); bake_detail(sc, detail, dof); bake_weather(wm.data(), weather);
    std::vector<float4> sky((size_t)8 * 4);
    for (float4& t : sky) t = float4{unit(), unit(), unit(), 1.0f};
    TexSet T;
    T.shape = shape.data(); T.detail = detail.data(); T.weather = weather.data(); T.sky = sky.data(); T.sky_w = 8; T.sky_h = 4;
    T.detail_h = nullptr; T.detail_lds = nullptr;
    T.detail_lod5 = detail_lod5_value(sc.data() + RAW_DETAIL_LOD5);
    CloudParams P; memset(&P, 0, sizeof P);
    P.texture_size[0] = P.texture_size[1] = 1.0f;
    P.ground_color[0] = 0.27f; P.ground_color[1] = 0.19f; P.ground_color[2] = 0.03f; P.ground_color[3] = 1.0f;
    P.LIGHT_DIRECTION[0] = 0.70710678f; P.LIGHT_DIRECTION[1] = 0.70710678f; P.LIGHT_ENERGY = 1.0f;
    P.LIGHT_COLOR[0] = P.LIGHT_COLOR[1] = P.LIGHT_COLOR[2] = 1.0f;
    P.density = 0.05f; P.cloud_coverage = 0.2f;

    const WeatherRange range = weather_range(wm.data());
    const ExactRejects rejects[2] = {exact_rejects(range, P.cloud_coverage, false), exact_rejects(range, P.cloud_coverage, true)};   // without and with the height window

    long marched = 0, cloudy = 0;
    auto run = [&](int primary, int light, bool window, const float pos[3], float cap, const float e[3], bool corner) {
        EXPECT(observer_invalid(pos, cap) == 0);
        const ExactRejects& rej = rejects[window ? 1 : 0];
        FrameConsts fc;
        frame_setup(P, sky.data(), 8, 4, primary, light, 0.0f, rej.hf_lo, rej.hf_hi, fc);
        fc.ct_mode = rej.ct_mode;
        const ObserverGeom G = observer_geom(nullptr, 0.0f, 1, 1, 1u, pos, cap);
        const Ray r = observer_ray(fc, G, e[0], e[1], e[2]);
        const float f[10] = {r.px, r.py, r.pz, r.sx, r.sy, r.sz, r.dx, r.dy, r.dz, r.ss};
        for (float v : f) EXPECT(std::isfinite(v));
        if (r.above) {
            EXPECT(r.ss > 0.0f);
            EXPECT(std::fabs((double)r.dx * r.dx + (double)r.dy * r.dy + (double)r.dz * r.dz - 1.0) < 1e-6);
        } else {
            for (float v : f) EXPECT(v == 0.0f);
        }
        const MarchOut o = march(T, fc, r);
        EXPECT(std::isfinite(o.r) && std::isfinite(o.g) && std::isfinite(o.b) && std::isfinite(o.a));
        if (!r.above) EXPECT(o.r == 0.0f && o.g == 0.0f && o.b == 0.0f && o.a == 0.0f && o.incloud == 0);
        if (!corner) { marched += r.above ? 1 : 0; cloudy += o.a > 0.0f ? 1 : 0; }
    };

    // the corner: a cap within the fp32 quantum of t0, or so small that the ray step's squares underflow
    const float ground[3] = {0.0f, 0.0f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    float cap = 1500.0f;
    for (int k = 0; k < 4096; k++) { cap = std::nextafter(cap, inf); run(128, 6, true, ground, cap, up, true); }
    const float off[3] = {30000.0f, 2750.0f, -20000.0f}, mid[3] = {0.0f, 2750.0f, 0.0f};
    const float caps[6] = {1e-30f, 1e-10f, 1e-3f, 0.1f, 0.3f, 1.0f};
    for (int k = 0; k < 2000; k++) {
        float e[3]; direction(e);
        for (float c : caps) { run(128, 6, true, off, c, e, true); run(30, 4, false, mid, c, e, true); }
    }

    // the ends of the accepted domain
    const Observer edge[] = {
        {"above_graze", {0.0f, 8000.0f, 0.0f}, inf},       {"inside_dip", {0.0f, 2750.0f, 0.0f}, inf},
        {"high", {0.0f, 100000.0f, 0.0f}, inf},            {"far_ground", {1.0e6f, -83000.0f, 0.0f}, inf},
        {"far_above", {-1.0e6f, -60000.0f, 5.0e5f}, inf},  {"on_bottom", {0.0f, 1500.0f, 0.0f}, inf},
        {"on_top", {0.0f, 4000.0f, 0.0f}, inf},            {"capped_ring", {0.0f, 0.0f, 0.0f}, 6000.0f},
        {"far_corner", {1.0e6f, -100000.0f, -1.0e6f}, inf},
    };
    for (const Observer& ob : edge) {
        const long before = marched;
        for (int k = 0; k < 10000; k++) {
            float e[3]; direction(e);
            run(k % 4 == 0 ? 128 : 32, k % 4 == 0 ? 6 : 4, k % 2 == 0, ob.pos, ob.cap, e, false);
        }
        EXPECT(marched - before > 1000);                       // (the solid angle of the layer from the highest observer: 13 % of the sphere)
    }
    EXPECT(cloudy > 1000);
    if (failures) { fprintf(stderr, "%d expectations failed\n", failures); return 1; }
    printf("observer asan ok %ld %ld\n", marched, cloudy);
    return 0;
}
