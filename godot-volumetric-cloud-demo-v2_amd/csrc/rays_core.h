// rays_core.h -- the front end of the direct cloud march (cloudsky.h csky_render_clouds_dirs / _view), written for one pixel per lane.
//
// A cloud texel is a function of a direction: clouds.glsl:218-236 sky(dir).  Only main() ties it to the hemi-octahedral grid.  This file makes the
// march's Ray from a direction the caller gives (a buffer of directions, or a camera view through composite_core.h's composite_eyedir) instead of from
// a grid pixel, with cloud_core.h ray_from_dir: the half of ray_setup behind the pixel's direction, so a grid pixel's own direction gives its own ray.
//
// Host+device (CSKY_HD) like cloud_core.h: tests/rays_host runs this per-lane code on a CPU.  The product instantiates it inside cloud_kernels.hip,
// depth.hip and cloud_aerial.hip; rays_lane_dir at the end is device-only (it takes csky_common.h's TilePixel).
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

// The geometry block of a w x h rays launch: the projection above for the view forms (basis: csky_view.basis), an identity camera nobody reads for
// the dirs forms (basis NULL).  The one place that fills it: the direct march, the depth frame and the aerial step of a ray frame all call this.
CSKY_HD RaysGeom rays_geom(const float* basis, float fov_y_degrees, int w, int h, uint32_t pitch_px) {
    RaysGeom g;
    g.w = w; g.h = h; g.pitch_px = pitch_px;
    for (int k = 0; k < 9; k++) g.cam[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    g.tan_half_fov_y = 1.0f; g.aspect = 1.0f;
    if (basis) {
        CompositeArgs a{};
        composite_view_args(a, basis, fov_y_degrees, w, h);   // the projection of csky_composite_view
        for (int k = 0; k < 9; k++) g.cam[k] = a.cam[k];
        g.tan_half_fov_y = a.tan_half_fov_y; g.aspect = a.aspect;
    }
    return g;
}

// What every launcher of the direct march asks of its geometry block (a RaysGeom, or a block that carries the same three fields): the image's size
// range, and a row pitch that holds a row.
template <class G> CSKY_HD bool rays_geom_ok(const G& g) { return g.w >= 1 && g.h >= 1 && g.w <= 8192 && g.h <= 8192 && g.pitch_px >= (uint32_t)g.w; }

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

// The ray of a direction as a lane uses it: cloud_core.h ray_from_dir when accepted, `above = false` (no sample, a zero texel) otherwise.
CSKY_HD Ray rays_ray(const FrameConsts& fc, float dx, float dy, float dz) {
    const bool ok = rays_accept(dx, dy, dz);
    Ray r = ray_from_dir(fc, ok ? dx : 0.0f, ok ? dy : 0.0f, ok ? dz : 0.0f);
    return r;
}

#if defined(__HIPCC__)
// The direction of the lane's pixel p (csky_common.h tile_pixel) of a ray frame: the one direction source of every kernel that takes one
// (cloud_kernels.hip, depth.hip, cloud_aerial.hip).  SRC 0: from `dirs` ([g.h][g.w][3] floats, tightly packed, three dword loads); a lane outside the
// image loads nothing and gets (0, 0, 0), which fails rays_accept and observer_accept.  SRC 1: the view of g (rays_view_dir; dirs is not read); a lane
// outside the image gets pixel (0, 0)'s direction, and its caller keeps it from marching and storing.
template <int SRC> CSKY_D void rays_lane_dir(const RaysGeom& g, const float* __restrict__ dirs, const TilePixel& p, float& ex, float& ey, float& ez) {
    if constexpr (SRC == 0) {
        ex = 0.0f; ey = 0.0f; ez = 0.0f;
        if (p.valid) { const float* __restrict__ d = dirs + ((size_t)p.j * (size_t)g.w + (size_t)p.i) * 3; ex = d[0]; ey = d[1]; ez = d[2]; }
    } else {
        rays_view_dir(g, p.valid ? p.i : 0, p.valid ? p.j : 0, ex, ey, ez);
    }
}
#endif

#pragma clang fp contract(fast)

}  // namespace csky
