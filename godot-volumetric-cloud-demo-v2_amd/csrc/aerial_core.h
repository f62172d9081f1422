// aerial_core.h -- the aerial-perspective volume (include/cloudsky.h): what the atmosphere between the eye and a surface at a finite
// distance adds (in-scattered light) and removes (transmittance), per view direction and depth slice.  It is sky-lut.glsl's compute_inscattering
// (S:219-276) stopped early: the ray, the per-step body and the output matrix are lut_core.h's own (sky_step, sky_accumulate, sky_output, unchanged),
// the camera is composite_core.h's composite_eyedir.  Host+device like the other cores: aerial_column is the definition, what tests/aerial_host runs
// and what aerial.hip must equal bit for bit.  FP contraction off, the *_cr transcendentals of lut_core.h.  Units: km.
#pragma once
#include "csky_common.h"
#include "lut_core.h"
#include "composite_core.h"

namespace csky {
#pragma clang fp contract(off)

// What a volume is rendered for, besides the transmittance table: a kernel argument.
struct AerialGeom {
    int w, h, d, s;                    // columns W x H, D slices of S steps each
    float far_km;                      // distance of the last slice along the ray
    float sun[3];                      // used as given, like csky_sky_params.sun_direction
    int view_mode;                     // composite_eyedir's: 0 = the equirectangular panorama, 1 = a perspective camera
    float cam[9];                      // view_mode 1: basis columns, tan(fov_y / 2) and the aspect ratio
    float tan_half_fov_y, aspect;
};

// csky_view.fov_y_degrees -> tan(fov_y / 2), the expression of csky_composite_view
CSKY_HD float tan_half_fov(float fov_y_degrees) { return tanf(fov_y_degrees * 0.5f * 3.14159265358979323846f / 180.0f); }

// EYEDIR of column (i, j): composite_eyedir, which reads these fields of its argument block and no other.  (view_mode is 0 or 1 in a way the compiler
// sees: the cube-face branch and the scratch copy of its camera table fold away.)
CSKY_HD void aerial_eyedir(const AerialGeom& g, int i, int j, float& ex, float& ey, float& ez) {
    CompositeArgs A{};
    A.out_w = g.w; A.out_h = g.h; A.view_mode = g.view_mode ? 1 : 0; A.tan_half_fov_y = g.tan_half_fov_y; A.aspect = g.aspect;
    for (int k = 0; k < 9; k++) A.cam[k] = g.cam[k];
    composite_eyedir(A, i, j, ex, ey, ez);
}

// A column's ray in the LUT frame.  The compositor's convention (getValFromSkyLUT, clouds.gdshader:34-45, against S:221-223,286-297):
// ray_dir = (-e.x, -e.z, e.y) from (0, 0, 6371.5), sun_dir = (-s.x, -s.z, s.y).  n = D * S steps of dt = far_km / n; steps whose midpoint has
// reached t_stop (the ground, or the top of the atmosphere: S:299-309) are skipped.
struct AerialRay { SkyRay r; float t_stop; };
CSKY_HD AerialRay aerial_ray(float ex, float ey, float ez, const float sun[3], float far_km, int n) {
    AerialRay a;
    SkyRay& r = a.r;
    r.rdx = -ex; r.rdy = -ez; r.rdz = ey;
    r.oz = 6371.5f;                                                                   // S:61-62
    const float atmos_dist = ray_sphere_intersection(0, 0, r.oz, r.rdx, r.rdy, r.rdz, ATMOSPHERE_RADIUS);
    const float ground_dist = ray_sphere_intersection(0, 0, r.oz, r.rdx, r.rdy, r.rdz, EARTH_RADIUS);
    a.t_stop = (ground_dist < 0.0f) ? atmos_dist : ground_dist;                       // S:303-309
    // the sun and the two phase functions: sky_ray's own lines.  (Factoring them out of sky_ray for both to call moved three instructions of the
    // mapping-1 sky-LUT kernels; those stay as they were verified.)
    r.sdx = -sun[0]; r.sdy = -sun[2]; r.sdz = sun[1];                                 // S:221-223
    const float cos_theta = (-r.rdx) * r.sdx + (-r.rdy) * r.sdy + (-r.rdz) * r.sdz;   // S:224
    r.molecular_phase = (float)((3.0 / 16.0) * (1.0 / LUT_PI)) * (1.0f + cos_theta * cos_theta);  // S:114-117
    const float den = (float)(1.0 + 0.8 * 0.8) + (float)(2.0 * 0.8) * cos_theta;      // S:124
    r.aerosol_phase = (float)(0.25 * (1.0 / LUT_PI)) * (1.0f - (float)(0.8 * 0.8)) / (den * sqrtf(den));  // S:125
    r.dt = far_km / (float)n;                                                         // with far_km = t_d and n = 30 this is S:229 itself
    return a;
}
// the skip rule: step i's midpoint, as sky_step computes it, has reached the stop
CSKY_HD bool aerial_skipped(const AerialRay& a, int i) { return ((float)i + 0.5f) * a.r.dt >= a.t_stop; }

// a slice's texel from the state behind its last step: rgb = M * L in the sky LUT's units (S:207-217), a = the mean of the four transmittances
struct AerialTexel { uint16_t h[4]; };
CSKY_HD AerialTexel aerial_slice(const F4& L, const F4& Tr) {
    const F4 c = sky_output(L);
    const float a = (((Tr.x + Tr.y) + Tr.z) + Tr.w) * 0.25f;
    AerialTexel t; t.h[0] = f2h(c.x); t.h[1] = f2h(c.y); t.h[2] = f2h(c.z); t.h[3] = f2h(a);
    return t;
}

// The whole column on one lane; store(k, L, Tr) takes the state behind slice k's last step (host-compiled unit test; the kernel spreads the steps
// over lanes).
template <int TLUT, class Store> CSKY_HD void aerial_column(const AerialRay& a, int D, int S, const float4* trans, int tw, int th, Store store) {
    F4 L = f4(0, 0, 0, 0), Tr = f4(1, 1, 1, 1);
    for (int k = 0; k < D; ++k) {
        for (int i = k * S; i < (k + 1) * S; ++i)
            if (!aerial_skipped(a, i)) sky_accumulate(L, Tr, sky_step<TLUT>(a.r, i, trans, tw, th));
        store(k, L, Tr);
    }
}
// column (i, j) of the volume g, its ray built the way the kernel builds it
CSKY_HD AerialRay aerial_volume_ray(const AerialGeom& g, int i, int j) {
    float ex, ey, ez;
    aerial_eyedir(g, i, j, ex, ey, ez);
    return aerial_ray(ex, ey, ez, g.sun, g.far_km, g.d * g.s);
}

}  // namespace csky
