// tlut_core.h -- the two parametrizations of the transmittance LUT (host+device; cloudsky.h CSKY_TLUT_*).
//
//   0  CSKY_TLUT_REFERENCE  transmittance-lut.glsl as written: u linear in the sun's zenith cosine over [-1, 1], v linear in altitude over
//                           100 km, texel (x, y) written for uv = (x, y) / size and sampled at texel centres.  lut_core.h / composite_core.h
//                           hold that code; nothing of it lives here.
//   1  CSKY_TLUT_BRUNETON   the mapping of Bruneton's 2017 precomputed-atmospheric-scattering implementation (the reference's README TODO 2):
//                           v from rho = the distance to the horizon, u from the distance d to the top of the atmosphere between its least
//                           (Rt - r) and greatest (rho + H) value, texel centres on the ends of both ranges.
//
// THE ONE SEMANTIC DIFFERENCE OF MAPPING 1: its table holds only rays that reach the top of the atmosphere.  A reader asked for a ray that meets
// the ground (tlut_hits_ground) returns transmittance 0 and does not tap, where the reference's table stores such rays marched THROUGH the planet
// at ground-level density.
//
// Precision: the differences below cancel in fp32 (r^2 is 4e7, its ulp 4), so everything is evaluated in double from the caller's fp32 (r, mu)
// and rounded to fp32 once -- as lut_core.h does for its transcendentals.  Every operation is an IEEE add / mul / div / sqrt in a fixed order
// with FP contraction off, so the hit decision and the tap coordinates are the same on the host, on the device and in a float64 restatement.
// Units: km.
#pragma once
#include "csky_common.h"

namespace csky {
#pragma clang fp contract(off)

constexpr int TLUT_REFERENCE = 0, TLUT_BRUNETON = 1;
constexpr double TLUT_RG = 6371.0, TLUT_RT = 6471.0;                   // lut_core.h EARTH_RADIUS, ATMOSPHERE_RADIUS
constexpr double TLUT_H2 = TLUT_RT * TLUT_RT - TLUT_RG * TLUT_RG;      // H^2 = 1 284 200 (exact)

CSKY_HD double tlut_clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// does the ray from radius r with zenith cosine mu meet the ground?  (r, mu already clamped)
CSKY_HD bool tlut_hits_ground_d(double r, double mu) { return mu < 0.0 && r * r * (mu * mu - 1.0) + TLUT_RG * TLUT_RG >= 0.0; }

// (r, mu) -> where a reader taps a w x h table (w, h >= 2).  Returns true when the ray meets the ground (then u, v are still those of the clamped d).
CSKY_HD bool tlut_uv(int w, int h, float r_km, float mu_f, float& u, float& v) {
    const double r = tlut_clampd((double)r_km, TLUT_RG, TLUT_RT), mu = tlut_clampd((double)mu_f, -1.0, 1.0);
    const double H = sqrt(TLUT_H2);
    const double rho2 = (r - TLUT_RG) * (r + TLUT_RG), rho = sqrt(rho2 > 0.0 ? rho2 : 0.0);
    const double disc = r * r * (mu * mu - 1.0) + TLUT_RT * TLUT_RT;
    const double d0 = -r * mu + sqrt(disc > 0.0 ? disc : 0.0), d = d0 > 0.0 ? d0 : 0.0;
    const double d_min = TLUT_RT - r, d_max = rho + H;
    const double x_mu = tlut_clampd((d - d_min) / (d_max - d_min), 0.0, 1.0), x_r = rho / H;
    u = (float)(0.5 / (double)w + x_mu * (1.0 - 1.0 / (double)w));
    v = (float)(0.5 / (double)h + x_r * (1.0 - 1.0 / (double)h));
    return tlut_hits_ground_d(r, mu);
}

// texel (px, py) of a w x h table -> the ray it stores: radius r, zenith cosine mu, length d to the top of the atmosphere
CSKY_HD void tlut_texel_ray(int px, int py, int w, int h, float& r_km, float& mu_f, float& d_f) {
    const double H = sqrt(TLUT_H2);
    const double x_mu = (double)px / (double)(w - 1), x_r = (double)py / (double)(h - 1);
    const double rho = H * x_r, r = sqrt(rho * rho + TLUT_RG * TLUT_RG);
    const double d_min = TLUT_RT - r, d_max = rho + H;
    const double d = d_min + x_mu * (d_max - d_min);
    const double mu = d == 0.0 ? 1.0 : tlut_clampd((TLUT_H2 - rho * rho - d * d) / (2.0 * r * d), -1.0, 1.0);
    r_km = (float)r; mu_f = (float)mu; d_f = (float)d;
}

}  // namespace csky
