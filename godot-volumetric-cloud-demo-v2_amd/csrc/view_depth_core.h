// view_depth_core.h -- the depth frame and the aerial step for view frames and ray frames (cloudsky.h csky_render_cloud_depth_dirs / _view,
// csky_apply_cloud_aerial_dirs / _view), written for one pixel per lane.
//
// depth_core.h depth_march takes a Ray and a t0 and never looks at the grid; aerial_core.h aerial_ray takes a direction.  Only depth_pixel and
// cloud_aerial_column tie them to the hemi-octahedral grid, through cloud_core.h pixel_dir.  This file is the other front end of both: the
// direction is the caller's (a buffer of directions, or a camera view through rays_core.h rays_view_dir), accepted by rays_core.h's rule and
// made a ray by rays_ray, exactly as the direct cloud march does (§17).  The cores' arithmetic is used unchanged, so a grid pixel's own
// direction gives the grid pixel's own texel.
//
// Host+device (CSKY_HD) like the cores: tests/view_depth_host runs this per-lane code on a CPU.  The product instantiates it inside depth.hip
// and cloud_aerial.hip only.
#pragma once
#include "depth_core.h"
#include "cloud_aerial_core.h"
#include "rays_core.h"

namespace csky {

// =================================================================================================
// Exact fp32 (no contraction): the order of the definition in cloudsky.h.
// =================================================================================================
#pragma clang fp contract(off)

// One direction, as a lane of depth_rays_kernel runs it: depth_pixel with (dx, dy, dz) in place of pixel_dir's direction and rays_ray's accept
// rule in front of the ray.  valid: the lane has a pixel.  A direction that is not accepted gives `above = false`: no sample, a zero texel, the
// lane takes part in the votes only.  t0 is the parameter of the shell entry along the direction as given (metres for a unit direction).
// t0_out, ss_out (may be null): the ray's entry distance and step length, 0 where the direction is not accepted.
template <class TS>
CSKY_HD DepthTexel depth_dir(const TS& T, const FrameConsts& fc, const DepthConsts& dc, float dx, float dy, float dz, bool valid, unsigned long long* taken,
                             unsigned long long* incloud, float* t0_out = nullptr, float* ss_out = nullptr) {
    const Ray ray = rays_ray(fc, dx, dy, dz);
    const float t0 = ray.above ? intersect_sphere_cam(dx, dy, dz, SKY_B_RADIUS) : 0.0f;
    if (t0_out) *t0_out = t0;
    if (ss_out) *ss_out = ray.ss;
    return depth_march(T, fc, dc, ray, t0, valid && ray.above, taken, incloud);
}

// A pixel of a ray frame that leaves as it came: cloud_aerial_passes' rule, or a direction the march would not have taken.
CSKY_HD bool cloud_aerial_dir_passes(const uint2& c, const uint2& z, float ex, float ey, float ez) {
    return cloud_aerial_passes(c, z) || !rays_accept(ex, ey, ez);
}

// The air in front of a pixel whose direction is (ex, ey, ez), used as given like aerial_ray's: cloud_aerial_column with the direction handed in.
template <int TLUT> CSKY_HD void cloud_aerial_dir_column(const CloudAerialGeom& g, float ex, float ey, float ez, const uint2& z, const float4* trans, int tw, int th,
                                                         F4& L, F4& Tr) {
    const AerialRay a = aerial_ray(ex, ey, ez, g.sun, h2f(half_of(z, 0)), g.n);
    L = f4(0, 0, 0, 0); Tr = f4(1, 1, 1, 1);
    for (int s = 0; s < g.n; ++s)
        if (!aerial_skipped(a, s)) sky_accumulate(L, Tr, sky_step<TLUT>(a.r, s, trans, tw, th));
}

// A pixel that does not pass: c the cloud texel, z the depth texel.
template <int TLUT> CSKY_HD uint2 cloud_aerial_dir(const CloudAerialGeom& g, float ex, float ey, float ez, const uint2& c, const uint2& z, const float4* trans, int tw,
                                                   int th) {
    F4 L, Tr;
    cloud_aerial_dir_column<TLUT>(g, ex, ey, ez, z, trans, tw, th, L, Tr);
    return cloud_aerial_composite(c, L, Tr);
}

#pragma clang fp contract(fast)   // as depth_core.h and rays_core.h leave it

}  // namespace csky
