// rays_core.h -- the front end of the direct cloud march (cloudsky.h csky_render_clouds_dirs / _view), written for one pixel per lane.
//
// A cloud texel is a function of a direction: clouds.glsl:218-236 sky(dir).  Only main() ties it to the hemi-octahedral grid.  This file makes the
// march's Ray from a direction the caller gives (a buffer of directions, or a camera view through composite_core.h's composite_eyedir) instead of from
// a grid pixel: ray_from_dir restates the tail of cloud_core.h ray_setup (lines 121-135), the way depth_core.h pixel_dir restates its head, and
// ray_setup itself stays as it is.  tests/test_clouds_rays_host.py holds ray_from_dir(pixel_dir(i, j)) and ray_setup(i, j) together bit for bit.
//
// Host+device (CSKY_HD) like cloud_core.h: tests/rays_host runs this per-lane code on a CPU.  The product instantiates it inside cloud_kernels.hip only.
#pragma once
#include "cloud_core.h"
#include "composite_core.h"
#include "aerial_core.h"

namespace csky {

// What a rays launch needs besides the frame constants: the image's size and addressing and, for a view, the camera.  A kernel argument.
struct RaysGeom {
    int w, h;                 // pixels
    uint32_t pitch_px;        // output row pitch in pixels (8 bytes each)
    float cam[9];             // view form: csky_view.basis, column-major
    float tan_half_fov_y, aspect;
};

// =================================================================================================
// Exact fp32 (no contraction): the order of the definition in cloudsky.h.
// =================================================================================================
#pragma clang fp contract(off)

// The projection of a w x h perspective view, as csky_composite_view hands it to composite_eyedir: view_mode 1, the basis columns, Godot's vertical
// field of view and the image's own aspect ratio.  The one place that computes it: the compositor, the view march and the host tests all call this.
CSKY_HD void composite_view_args(CompositeArgs& A, const float basis[9], float fov_y_degrees, int w, int h) {
    A.view_mode = 1;
    for (int k = 0; k < 9; k++) A.cam[k] = basis[k];
    A.tan_half_fov_y = tan_half_fov(fov_y_degrees);
    A.aspect = (float)w / (float)h;
    A.out_w = w; A.out_h = h;
}

// EYEDIR of pixel (i, j) of the view g: composite_eyedir, which reads these fields of its argument block and no other.  (view_mode is 1 in a way the
// compiler sees: the panorama and cube-face branches fold away.)
CSKY_HD void rays_view_dir(const RaysGeom& g, int i, int j, float& ex, float& ey, float& ez) {
    CompositeArgs A{};
    A.out_w = g.w; A.out_h = g.h; A.view_mode = 1; A.tan_half_fov_y = g.tan_half_fov_y; A.aspect = g.aspect;
    for (int k = 0; k < 9; k++) A.cam[k] = g.cam[k];
    composite_eyedir(A, i, j, ex, ey, ez);
}

// Which directions are marched: above the horizon, and of length 1 within 1 % in |e|^2.  NaN fails every comparison, +-inf the upper one.  The band
// is no tolerance on the result (a direction inside it is used as given): it keeps a lane with a garbage direction from computing texture addresses.
CSKY_HD bool rays_accept(float dx, float dy, float dz) {
    const float l2 = (dx * dx + dy * dy) + dz * dz;
    return dy > 0.0f && l2 >= 0.99f && l2 <= 1.01f;
}

// cloud_core.h ray_setup from `r.above = dy > 0.0f` on (clouds.glsl:221-230, :143-145), for a direction that has passed rays_accept.
CSKY_HD Ray ray_from_dir(const FrameConsts& fc, float dx, float dy, float dz) {
    Ray r;
    r.above = dy > 0.0f;
    if (!r.above) { r.px = r.py = r.pz = r.sx = r.sy = r.sz = r.dx = r.dy = r.dz = r.ss = 0.0f; return r; }
    const float t0 = intersect_sphere_cam(dx, dy, dz, SKY_B_RADIUS);
    const float t1 = intersect_sphere_cam(dx, dy, dz, SKY_T_RADIUS);
    const float s0x = 0.0f + dx * t0, s0y = G_RADIUS + dy * t0, s0z = 0.0f + dz * t0;  // start, clouds.glsl:224
    const float e0x = 0.0f + dx * t1, e0y = G_RADIUS + dy * t1, e0z = 0.0f + dz * t1;  // end,   clouds.glsl:225
    const float shelldist = length3_exact(e0x - s0x, e0y - s0y, e0z - s0z);
    const float rx = dx * shelldist / fc.steps_f, ry = dy * shelldist / fc.steps_f, rz = dz * shelldist / fc.steps_f;  // :230
    r.ss = length3_exact(rx, ry, rz);                                                  // :143
    r.dx = rx / r.ss; r.dy = ry / r.ss; r.dz = rz / r.ss;                              // :144
    r.sx = r.dx * r.ss; r.sy = r.dy * r.ss; r.sz = r.dz * r.ss;
    r.px = s0x; r.py = s0y; r.pz = s0z;                                                // :145 (hash() == 0: ray_setup)
    return r;
}

// The ray of a direction as a lane uses it: marched when accepted, `above = false` (no sample, a zero texel) otherwise.
CSKY_HD Ray rays_ray(const FrameConsts& fc, float dx, float dy, float dz) {
    const bool ok = rays_accept(dx, dy, dz);
    Ray r = ray_from_dir(fc, ok ? dx : 0.0f, ok ? dy : 0.0f, ok ? dz : 0.0f);
    return r;
}

#pragma clang fp contract(fast)

}  // namespace csky
