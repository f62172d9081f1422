// view_update_core.h -- the temporal split of a view frame (cloudsky.h csky_render_clouds_view_update), written for one pixel per lane.
//
// One pixel of every B x B block of a view is marched per call; every other pixel is taken from the previous view frame through the previous camera.
// The observer of this model does not move (every ray starts at camPos), so a cloud texel is a function of a direction alone and the reprojection is
// a pure rotation: the pixel's EYEDIR, expressed in the previous camera's axes and projected onto its screen.  No depth, no motion vectors.  A pixel
// the previous frame does not cover is a *hole* and is marched.
//
// This file holds what a lane does in front of the march and instead of it: the kernel-argument block, the classification of a pixel and the bilinear
// tap of the previous frame.  Host+device (CSKY_HD) like rays_core.h: tests/view_update_host runs this per-lane code on a CPU.  The product
// instantiates it inside cloud_kernels.hip only.
#pragma once
#include "rays_core.h"

namespace csky {

// What an update launch needs besides the frame constants.  A kernel argument.  RaysGeom and CompositeArgs are not touched: the kernels of §17 keep
// their argument blocks, and so their code.
struct ViewUpdateGeom {
    int w, h;                 // pixels
    uint32_t pitch_px;        // output row pitch in pixels (8 bytes each)
    float cam[9];             // the current csky_view.basis, column-major
    float tan_half_fov_y, aspect;
    int block;                // B: one pixel of every B x B block is fresh
    int px, py;               // the fresh pixel of a block: phase % B, phase / B
    int sub_w, sub_h;         // the sub-grid of fresh pixels: ceil((w - px) / B) x ceil((h - py) / B), 0 where the image has none
    float prev_cam[9];        // the previous csky_view.basis, column-major
    float prev_th, prev_asp;  // composite_view_args(prev_view, w, h)'s tan_half_fov_y and aspect
    uint32_t prev_pitch_px;   // the previous frame's row pitch in pixels
    int same;                 // the ten floats of the two views are equal bit for bit (decided once on the host)
    int has_history;          // prev != NULL
};

// What becomes of a pixel.
enum ViewUpdateKind : int {
    VU_ZERO = 0,    // not accepted: (0, 0, 0, 0), no sample, no tap
    VU_FRESH = 1,   // this call's pixel of its block: marched
    VU_COPY = 2,    // `same`: prev(i, j), bit for bit
    VU_TAP = 3,     // a bilinear tap of prev at (ux, uy)
    VU_HOLE = 4,    // no valid history: marched
};
struct ViewUpdateClass { int kind; float ux, uy; };   // ux, uy: defined for VU_TAP and VU_HOLE of a moved camera, 0 otherwise

// =================================================================================================
// Exact fp32 (no contraction): the order of the definition in cloudsky.h.
// =================================================================================================
#pragma clang fp contract(off)

// The block of a w x h update, filled on the host.  view / prev_view: the csky_view's ten floats (prev_view NULL without history).
inline ViewUpdateGeom view_update_geom(const float* view, const float* prev_view, int w, int h, uint32_t pitch_px, uint32_t prev_pitch_px, int block, int phase) {
    ViewUpdateGeom g;
    const RaysGeom r = rays_geom(view, view[9], w, h, pitch_px);
    g.w = w; g.h = h; g.pitch_px = pitch_px;
    for (int k = 0; k < 9; k++) g.cam[k] = r.cam[k];
    g.tan_half_fov_y = r.tan_half_fov_y; g.aspect = r.aspect;
    g.block = block; g.px = phase % block; g.py = phase / block;
    g.sub_w = g.px < w ? (w - g.px + block - 1) / block : 0;
    g.sub_h = g.py < h ? (h - g.py + block - 1) / block : 0;
    for (int k = 0; k < 9; k++) g.prev_cam[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    g.prev_th = 1.0f; g.prev_asp = 1.0f; g.prev_pitch_px = prev_pitch_px;
    g.same = 0; g.has_history = prev_view ? 1 : 0;
    if (prev_view) {
        CompositeArgs a{};
        composite_view_args(a, prev_view, prev_view[9], w, h);
        for (int k = 0; k < 9; k++) g.prev_cam[k] = a.cam[k];
        g.prev_th = a.tan_half_fov_y; g.prev_asp = a.aspect;
        g.same = memcmp(view, prev_view, 10 * sizeof(float)) == 0 ? 1 : 0;   // bit for bit: -0 is not 0
    }
    return g;
}

// EYEDIR of pixel (i, j) of the current view: rays_view_dir on this block's copy of RaysGeom's fields.
CSKY_HD void view_update_dir(const ViewUpdateGeom& g, int i, int j, float& ex, float& ey, float& ez) {
    RaysGeom r;
    r.w = g.w; r.h = g.h; r.pitch_px = g.pitch_px; r.tan_half_fov_y = g.tan_half_fov_y; r.aspect = g.aspect;
    for (int k = 0; k < 9; k++) r.cam[k] = g.cam[k];
    rays_view_dir(r, i, j, ex, ey, ez);
}

CSKY_HD bool view_update_fresh(const ViewUpdateGeom& g, int i, int j) { return i % g.block == g.px && j % g.block == g.py; }

// Pixel (i, j) with EYEDIR e.  The order of the definition: accept, fresh, history.  Every comparison of `valid` is false for a NaN, so a
// VU_TAP's (ux, uy) lies in [0, w - 1] x [0, h - 1]: no address is ever computed from anything else.
CSKY_HD ViewUpdateClass view_update_classify(const ViewUpdateGeom& g, int i, int j, float ex, float ey, float ez) {
    ViewUpdateClass c = {VU_ZERO, 0.0f, 0.0f};
    if (!rays_accept(ex, ey, ez)) return c;
    if (view_update_fresh(g, i, j)) { c.kind = VU_FRESH; return c; }
    if (!g.has_history) { c.kind = VU_HOLE; return c; }
    if (g.same) { c.kind = VU_COPY; return c; }
    const float* q = g.prev_cam;
    const float qx = (q[0] * ex + q[1] * ey) + q[2] * ez;
    const float qy = (q[3] * ex + q[4] * ey) + q[5] * ez;
    const float qz = (q[6] * ex + q[7] * ey) + q[8] * ez;
    const bool front = qz < 0.0f;
    const float nx = qx / (-qz), ny = qy / (-qz);
    const float u = (nx / (g.prev_th * g.prev_asp) + 1.0f) * 0.5f;
    const float v = (1.0f - ny / g.prev_th) * 0.5f;
    c.ux = u * (float)g.w - 0.5f;
    c.uy = v * (float)g.h - 0.5f;
    const bool valid = front && c.ux >= 0.0f && c.ux <= (float)(g.w - 1) && c.uy >= 0.0f && c.uy <= (float)(g.h - 1);
    c.kind = valid ? VU_TAP : VU_HOLE;
    return c;
}

// lerp(a, b, f) = a + (b - a) * f of the definition, its three operations rounded one by one.  Not csky_common.h's lerpf: that header states no
// contraction mode of its own, so lerpf's multiply and add carry the mode of whoever includes it first, and in the device build they fuse into one
// fma even when inlined here.  A fused tap differs from the definition in the last bit of about one half in 3000
// (tests/test_gpu_view_cameras.py).
CSKY_HD float view_update_lerp(float a, float b, float f) {
    const float d = b - a;
    const float m = d * f;
    return a + m;
}

// The tap: composite_core.h tap_half_clamp's arithmetic from (ux, uy) on, over an image of `pitch_px` pixels per row, each channel stored with f2h.
// For a VU_TAP's coordinates the clamps only ever move x1 / y1 from w / h to w - 1 / h - 1.
CSKY_HD uint2 view_update_tap(const uint2* __restrict__ prev, uint32_t pitch_px, int w, int h, float ux, float uy) {
    const float fx0 = floorf(ux), fy0 = floorf(uy), ax = ux - fx0, ay = uy - fy0;
    int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    x0 = x0 < 0 ? 0 : (x0 > w - 1 ? w - 1 : x0); x1 = x1 < 0 ? 0 : (x1 > w - 1 ? w - 1 : x1);
    y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0); y1 = y1 < 0 ? 0 : (y1 > h - 1 ? h - 1 : y1);
    const uint2 a = prev[(size_t)y0 * pitch_px + x0], b = prev[(size_t)y0 * pitch_px + x1], c = prev[(size_t)y1 * pitch_px + x0], d = prev[(size_t)y1 * pitch_px + x1];
    uint16_t o[4];
    for (int k = 0; k < 4; k++) {
        const uint32_t wa = k < 2 ? a.x : a.y, wb = k < 2 ? b.x : b.y, wc = k < 2 ? c.x : c.y, wd = k < 2 ? d.x : d.y;
        const int sh = (k & 1) * 16;
        const float fa = h2f((uint16_t)(wa >> sh)), fb = h2f((uint16_t)(wb >> sh)), fc = h2f((uint16_t)(wc >> sh)), fd = h2f((uint16_t)(wd >> sh));
        o[k] = f2h(view_update_lerp(view_update_lerp(fa, fb, ax), view_update_lerp(fc, fd, ax), ay));
    }
    return pack_half4(o[0], o[1], o[2], o[3]);
}

#pragma clang fp contract(fast)

}  // namespace csky
