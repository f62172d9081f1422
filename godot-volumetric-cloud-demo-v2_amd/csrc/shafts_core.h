// shafts_core.h -- light shafts: the cloud shadow map (shadow_core.h) inside the aerial-perspective volume (aerial_core.h; §14).
// The volume lights every step of every column with the full sun; here a step's direct sun is multiplied by one factor s, what the clouds between
// the step and the sun let through, read from an R16F shadow map by the lookup include/cloudsky.h documents for it.  Everything
// else is aerial_core.h's and lut_core.h's: the columns, the rays, the skip rule, the accumulation, the slice texel.  sky_step_shadowed restates
// sky_step with the one product added rather than sharing lines with it: factoring lines out of verified cores has moved instructions in their
// kernels before (aerial_core.h, aerial_ray).  Host+device like the other cores: shafts_column is the definition, what tests/shafts_host runs and
// what shafts.hip must equal bit for bit.  FP contraction off.  Units: km in the LUT frame, metres in the map's.
#pragma once
#include "csky_common.h"
#include "lut_core.h"
#include "aerial_core.h"

namespace csky {
#pragma clang fp contract(off)

constexpr float SHAFTS_BASE_M = 1500.0f;      // Rb - Rg: the cloud layer's base above the ground (clouds.glsl:43-45)
constexpr float SHAFTS_TOP_M = 4000.0f;       // Rt - Rg: its top
constexpr float SHAFTS_LAYER_M = 2500.0f;     // Rt - Rb

// The map as a reader sees it, and the sun it was rendered with: a kernel argument.
struct ShaftsMap {
    const uint16_t* texels;            // rows of pitch_h halfs; texel (i, j) at texels[j * pitch_h + i]
    uint32_t pitch_h;
    int w, h;
    float cx, cz, ex, ez;              // csky_shadow_params center and extent, metres
    float lx, ly, lz;                  // shafts_sun of the call's sun direction
};

// The sun's unit vector, once per call: the kernel, the host tool and csky_aerial_shadow_rect see the same floats.  A zero vector gives NaN,
// which every reader treats as a sun that is not up.
CSKY_HD void shafts_sun(const float sun[3], float l[3]) {
    const float ll = sqrtf((sun[0] * sun[0] + sun[1] * sun[1]) + sun[2] * sun[2]);
    l[0] = sun[0] / ll; l[1] = sun[1] / ll; l[2] = sun[2] / ll;
}

// A step at (x, y) of the LUT frame (km), h metres up, projected to the ground along the sun: world (wx, wz) = (-x, -y) * 1000 is the inverse of
// ray_dir = (-e.x, -e.z, e.y).
CSKY_HD void shafts_project(const ShaftsMap& m, float x, float y, float h, float& gx, float& gz) {
    const float wx = -x * 1000.0f, wz = -y * 1000.0f;
    const float k = h / m.ly;
    gx = wx - m.lx * k; gz = wz - m.lz * k;
}

// one texel of the filter's footprint: outside the map the sky is clear
CSKY_HD float shafts_texel(const ShaftsMap& m, int i, int j) {
    return (i >= 0 && i < m.w && j >= 0 && j < m.h) ? h2f(m.texels[(size_t)j * m.pitch_h + i]) : 1.0f;
}

// The map's bilinear filter at the ground point (gx, gz); false (no texel read) when the footprint lies wholly outside the map.  The range test
// also catches NaN and inf and comes before any conversion to int.
CSKY_HD bool shafts_filter(const ShaftsMap& m, float gx, float gz, float& v) {
    const float u = (gx - m.cx) / m.ex + 0.5f, w = (gz - m.cz) / m.ez + 0.5f;
    const float fx = u * (float)m.w - 0.5f, fy = w * (float)m.h - 0.5f;
    if (!(fx >= -1.0f && fx < (float)m.w && fy >= -1.0f && fy < (float)m.h)) return false;
    const float fi = floorf(fx), fj = floorf(fy), ax = fx - fi, ay = fy - fj;
    const int i0 = (int)fi, j0 = (int)fj;
    const float t00 = shafts_texel(m, i0, j0), t10 = shafts_texel(m, i0 + 1, j0), t01 = shafts_texel(m, i0, j0 + 1), t11 = shafts_texel(m, i0 + 1, j0 + 1);
    v = lerpf(lerpf(t00, t10, ax), lerpf(t01, t11, ax), ay);
    return true;
}

// Through the layer the whole-layer map over-shadows: below the base the factor is the map's value, at the top it is the clear value.
CSKY_HD float shafts_blend(float v, float h) {
    const float w = clampf((h - SHAFTS_BASE_M) / SHAFTS_LAYER_M, 0.0f, 1.0f);
    return v + (1.0f - v) * w;
}

// The factor s of a step at (x, y) of the LUT frame, `altitude` km above the atmosphere model's ground.
CSKY_HD float shafts_factor(const ShaftsMap& m, float x, float y, float altitude) {
    if (!(m.ly > 0.0f)) return 1.0f;                       // the planet's own shadow is the transmittance table's business
    const float h = altitude * 1000.0f;
    if (h >= SHAFTS_TOP_M) return 1.0f;                    // above the layer
    float gx, gz, v;
    shafts_project(m, x, y, h, gx, gz);
    if (!shafts_filter(m, gx, gz, v)) return 1.0f;
    return shafts_blend(v, h);
}

// sky_step (lut_core.h) with the direct sun of the step multiplied by the map's factor.  ms, step_tr and with them Tr do not see the map.
template <int TLUT> CSKY_HD SkyStep sky_step_shadowed(const SkyRay& r, int i, const float4* trans, int tw, int th, const ShaftsMap& m) {
    const float dt = r.dt;
    const float t = ((float)i + 0.5f) * dt;
    const float x = 0.0f + r.rdx * t, y = 0.0f + r.rdy * t, z = r.oz + r.rdz * t;
    const float dist = sqrtf(x * x + y * y + z * z);
    const float zx = x / dist, zy = y / dist, zz = z / dist;
    const float altitude = dist - EARTH_RADIUS;
    const float nalt = altitude / ATMOSPHERE_THICKNESS;
    const float sct = zx * r.sdx + zy * r.sdy + zz * r.sdz;                          // S:243
    const Coeffs cf = atmosphere_collision_coefficients(altitude);
    const F4 t_sun = sky_tlut_tap<TLUT>(trans, tw, th, sct, nalt, dist) * shafts_factor(m, x, y, altitude);   // S:254, times s
    // get_multiple_scattering, S:144-164
    const float omega = (float)(2.0 * LUT_PI) * (1.0f - sqrtf(dist * dist - EARTH_RADIUS * EARTH_RADIUS) / dist);
    const F4 T_to_ground = sky_tlut_tap<TLUT>(trans, tw, th, sct, 0.0f, EARTH_RADIUS);
    const F4 T_g2s = sky_tlut_tap<TLUT>(trans, tw, th, 1.0f, 0.0f, EARTH_RADIUS) / sky_tlut_tap<TLUT>(trans, tw, th, 1.0f, nalt, dist);
    const float ks = (float)(0.25 * (1.0 / LUT_PI)) * omega * (float)(0.3 / LUT_PI);
    const F4 L_ground = f4(ks, ks, ks, ks) * T_to_ground * T_g2s * sct;
    const float fm = 1.0f / (1.0f + 5.0f * exp_cr(-17.92f * sct));
    const F4 L_ms = f4((float)(0.02 * 0.217), (float)(0.02 * 0.347), (float)(0.02 * 0.594), (float)(0.02 * 1.0)) * fm;
    const F4 ms = L_ms + L_ground;
    const F4 irr = f4(1.679f, 1.828f, 1.986f, 1.307f);                               // S:67
    const F4 S = irr * (cf.molecular_scattering * (t_sun * r.molecular_phase + ms) + cf.aerosol_scattering * (t_sun * r.aerosol_phase + ms));  // S:261-263
    SkyStep o;
    o.step_tr = exp4(cf.extinction * (-dt));                                         // S:265
    const F4 ext_c = f4(fmaxf(cf.extinction.x, 1e-7f), fmaxf(cf.extinction.y, 1e-7f), fmaxf(cf.extinction.z, 1e-7f), fmaxf(cf.extinction.w, 1e-7f));
    o.S_int = (S - S * o.step_tr) / ext_c;                                           // S:270
    return o;
}

// The whole column on one lane (aerial_column with the shadowed step); store(k, L, Tr) takes the state behind slice k's last step.
template <int TLUT, class Store> CSKY_HD void shafts_column(const AerialRay& a, int D, int S, const float4* trans, int tw, int th, const ShaftsMap& m, Store store) {
    F4 L = f4(0, 0, 0, 0), Tr = f4(1, 1, 1, 1);
    for (int k = 0; k < D; ++k) {
        for (int i = k * S; i < (k + 1) * S; ++i)
            if (!aerial_skipped(a, i)) sky_accumulate(L, Tr, sky_step_shadowed<TLUT>(a.r, i, trans, tw, th, m));
        store(k, L, Tr);
    }
}

// csky_aerial_shadow_rect: the rectangle that holds the projection of every step below the layer's top within far_m metres of the observer.
// false: the sun is not up.  (The caller checks the result against the range of csky_shadow_params.)
CSKY_HD bool shafts_rect(const float sun[3], float far_m, float center[2], float extent[2]) {
    float l[3];
    shafts_sun(sun, l);
    if (!(l[1] > 0.0f)) return false;
    const float k = SHAFTS_TOP_M / l[1];
    const float shift[2] = {-l[0] * k, -l[2] * k};
    for (int a = 0; a < 2; a++) { center[a] = shift[a] * 0.5f; extent[a] = 2.0f * far_m + fabsf(shift[a]); }
    return true;
}

}  // namespace csky
