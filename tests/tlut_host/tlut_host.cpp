// tlut_host.cpp -- TEST TOOL ONLY.  Compiles the LUT cores (csrc/tlut_core.h, lut_core.h: the per-lane code the HIP kernels instantiate) for the
// HOST in both parametrizations of the transmittance LUT, so the `-m "not gpu"` suite can check the Bruneton mapping's writer and readers against
// tests/tlut_reference.py without a GPU.  Not part of libcloudsky and never a render fallback: the product has no CPU path.
#include <cstdint>
#include <vector>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/lut_core.h"

using namespace csky;

namespace {
std::vector<float4> widen(const uint16_t* img, int w, int h) {
    std::vector<float4> f((size_t)w * h);
    for (size_t i = 0; i < f.size(); i++) f[i] = float4{h2f(img[4 * i]), h2f(img[4 * i + 1]), h2f(img[4 * i + 2]), h2f(img[4 * i + 3])};
    return f;
}
void store(uint16_t* o, const F4& c) { o[0] = f2h(c.x); o[1] = f2h(c.y); o[2] = f2h(c.z); o[3] = f2h(c.w); }
}  // namespace

extern "C" {

// the whole w x h transmittance LUT (RGBA16F) in `mapping` (0 reference, 1 Bruneton)
void tlut_host_transmittance(int mapping, int w, int h, uint16_t* out_h) {
    for (int py = 0; py < h; py++) for (int px = 0; px < w; px++)
        store(out_h + ((size_t)py * w + px) * 4, mapping ? transmittance_texel<TLUT_BRUNETON>(px, py, (float)w, (float)h) : transmittance_texel<TLUT_REFERENCE>(px, py, (float)w, (float)h));
}

// the w x h sky LUT of `sun` from a tw x th transmittance LUT of the same mapping
void tlut_host_sky(int mapping, int w, int h, const float sun[3], const uint16_t* trans_h, int tw, int th, uint16_t* out_h) {
    const std::vector<float4> tf = widen(trans_h, tw, th);
    for (int py = 0; py < h; py++) for (int px = 0; px < w; px++)
        store(out_h + ((size_t)py * w + px) * 4, mapping ? sky_texel<TLUT_BRUNETON>(px, py, (float)w, (float)h, sun, tf.data(), tw, th) : sky_texel<TLUT_REFERENCE>(px, py, (float)w, (float)h, sun, tf.data(), tw, th));
}

// the readers' look-up at n points (radius km, zenith cosine): float RGBA out.  Mapping 0 derives the normalised altitude as sky_step does.
void tlut_host_lookup(int mapping, const uint16_t* trans_h, int tw, int th, const float* r, const float* mu, int n, float* out) {
    const std::vector<float4> tf = widen(trans_h, tw, th);
    for (int i = 0; i < n; i++) {
        const F4 t = mapping ? transmittance_from_lut_bruneton(tf.data(), tw, th, mu[i], r[i])
                             : transmittance_from_lut(tf.data(), tw, th, mu[i], (r[i] - EARTH_RADIUS) / ATMOSPHERE_THICKNESS);
        out[4 * i] = t.x; out[4 * i + 1] = t.y; out[4 * i + 2] = t.z; out[4 * i + 3] = t.w;
    }
}

// the ray texel (px, py) of a mapping-1 table stores: out = {r, mu, d}
void tlut_host_texel_ray(int px, int py, int w, int h, float out[3]) { tlut_texel_ray(px, py, w, h, out[0], out[1], out[2]); }

}  // extern "C"
