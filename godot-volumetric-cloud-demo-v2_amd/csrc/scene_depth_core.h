// scene_depth_core.h -- the front end of the observer's cloud march behind a per-pixel scene depth (cloudsky.h csky_render_clouds_view_from_depth /
// _dirs_from_depth), written for one pixel per lane.
//
// observer_core.h ends every ray of a frame at one max_distance.  This file ends each ray at its own pixel's depth as well: the distance along the ray
// (CSKY_DEPTH_DISTANCE) or along the camera's forward axis (CSKY_DEPTH_VIEW_Z, a rasteriser's linear depth) at which the host's scene stands in the
// way.  The cap re-spaces the N samples over the shortened segment, exactly as max_distance does; the march behind it is the same.
//
// Host+device (CSKY_HD) like observer_core.h: tests/scene_depth_host runs this per-lane code on a CPU.  The product instantiates it inside
// cloud_kernels.hip only.  observer_core.h itself gains nothing.
#pragma once
#include "observer_core.h"

namespace csky {

constexpr int DEPTH_DISTANCE = 0, DEPTH_VIEW_Z = 1;           // csky_scene_depth.kind

// What a depth launch needs: an observer launch's geometry, the depth buffer's row pitch in floats and the kind of its texels.  The argument block of
// clouds_observer_depth_kernel.
struct SceneDepthGeom {
    ObserverGeom og;
    uint32_t depth_pitch;     // floats
    int kind;                 // DEPTH_DISTANCE or DEPTH_VIEW_Z
};

// Which csky_scene_depth the calls refuse (CSKY_ERR_INVALID), as a rule number for the error text; 0: accepted.  `texels` and `out` are addresses in
// one address space (both device, or `out` 0 for the host forms, whose depth is staged and cannot overlap).  w, h, out_pitch: the image's, already
// checked or out of range (then the ranges are not compared: the image's own check refuses the call).
//   1 texels is NULL   2 kind outside {0, 1}   3 view-z on a dirs form   4 a pitch that is no multiple of 4 or below 4 * w (0: tight, host forms only)
//   5 the byte ranges of the depth buffer and of out overlap
CSKY_HD int scene_depth_invalid(uintptr_t texels, size_t pitch_bytes, int kind, bool is_view, bool host_form, int w, int h, uintptr_t out, size_t out_pitch) {
    if (!texels) return 1;
    if (kind != DEPTH_DISTANCE && kind != DEPTH_VIEW_Z) return 2;
    if (kind == DEPTH_VIEW_Z && !is_view) return 3;
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return 0;
    if (host_form && pitch_bytes == 0) pitch_bytes = (size_t)w * 4;
    if (pitch_bytes % 4 || pitch_bytes < (size_t)w * 4) return 4;
    if (!out || out_pitch < (size_t)w * 8) return 0;
    const size_t na = (size_t)(h - 1) * pitch_bytes + (size_t)w * 4, nb = (size_t)(h - 1) * out_pitch + (size_t)w * 8;
    if (texels < out + nb && out < texels + na) return 5;
    return 0;
}

// The geometry block of a w x h depth launch: observer_geom's and the depth buffer's addressing.  The one place that fills it, on the host.
CSKY_HD SceneDepthGeom scene_depth_geom(const float* basis, float fov_y_degrees, int w, int h, uint32_t pitch_px, const float position[3], float max_distance,
                                        uint32_t depth_pitch, int kind) {
    SceneDepthGeom G;
    G.og = observer_geom(basis, fov_y_degrees, w, h, pitch_px, position, max_distance);
    G.depth_pitch = depth_pitch;
    G.kind = kind;
    return G;
}

// =================================================================================================
// Exact fp32 (no contraction): the order of the definition in cloudsky.h.
// =================================================================================================
#pragma clang fp contract(off)

// The definition's `d` and `valid` for the texel z of the pixel whose direction is e: the distance along the ray at which the scene stands, and
// whether the texel leaves anything to march.  NaN, 0, -0, negatives and -inf fail (geometry at the lens); +inf passes (nothing in the way).  KIND is
// a template value: the distance form carries no dot product and no divide.
template <int KIND> CSKY_HD bool scene_depth_cap_k(const float cam[9], float ex, float ey, float ez, float z, float& d) {
    if constexpr (KIND == DEPTH_DISTANCE) {
        d = z;
        return z > 0.0f;
    } else {
        const float f = -((cam[6] * ex + cam[7] * ey) + cam[8] * ez);   // e along the camera's forward axis (cam[6..8]: the back axis)
        d = z / f;
        return f > 0.0f && z > 0.0f && d > 0.0f;
    }
}
CSKY_HD bool scene_depth_cap(const SceneDepthGeom& G, float ex, float ey, float ez, float z, float& d) {
    return G.kind == DEPTH_VIEW_Z ? scene_depth_cap_k<DEPTH_VIEW_Z>(G.og.g.cam, ex, ey, ez, z, d) : scene_depth_cap_k<DEPTH_DISTANCE>(G.og.g.cam, ex, ey, ez, z, d);
}

// The ray of a direction and its pixel's depth texel as a lane uses it; `above` means "marched".  observer_ray's lines with the depth's cap behind
// max_distance's and two more clauses of `marched`: a valid texel, and a segment long enough to have a direction.  World positions are near 6e6 m,
// where fp32 has a quantum of 0.5 m: along a silhouette inside the layer a depth buffer holds texels within that quantum of t0, where the end rounds
// onto the start, ss = 0 and dir = 0 / 0.  `shelldist > 0` alone does not keep that out: from an observer on the axis inside the layer (o.x = o.z = 0,
// t0 = 0) a depth of 1e-22 m gives a shelldist near 1e-22 > 0, a raystep whose squares underflow, ss = 0 and a NaN ray all the same.  The clause is
// therefore that BOTH square roots of the tail take an argument inside sqrt_exact's specified range: |end - start|^2 >= 2^-102 and
// |raystep|^2 >= 2^-102 (shelldist >= 4.4e-16 m, which implies shelldist > 0).  On that range host and device agree bit for bit and dir is a unit
// vector.  Such a ray is not marched.  The tail restates observer_ray's as that one restates ray_from_dir's: with +inf texels all eleven fields are
// observer_ray's bit for bit (tests/test_scene_depth_host.py D1).
template <int KIND> CSKY_HD Ray scene_depth_ray_k(const FrameConsts& fc, const ObserverGeom& G, float ex, float ey, float ez, float z) {
    Ray r;
    float t0 = 0.0f, t1 = 0.0f, d = 0.0f;
    r.above = observer_accept(ex, ey, ez) && observer_segment(G.o, G.max_dist, ex, ey, ez, t0, t1) && scene_depth_cap_k<KIND>(G.g.cam, ex, ey, ez, z, d);
    float s0x = 0.0f, s0y = 0.0f, s0z = 0.0f, rx = 0.0f, ry = 0.0f, rz = 0.0f, ss2 = 0.0f;
    if (r.above) {
        t1 = fminf(t1, d);
        r.above = t1 > t0;
    }
    if (r.above) {
        s0x = G.o[0] + ex * t0; s0y = G.o[1] + ey * t0; s0z = G.o[2] + ez * t0;                                            // start
        const float e0x = G.o[0] + ex * t1, e0y = G.o[1] + ey * t1, e0z = G.o[2] + ez * t1;                                // end
        const float qx = e0x - s0x, qy = e0y - s0y, qz = e0z - s0z;
        const float sd2 = qx * qx + qy * qy + qz * qz;                                 // length3_exact's own argument
        const float shelldist = sqrt_exact(sd2);
        rx = ex * shelldist / fc.steps_f; ry = ey * shelldist / fc.steps_f; rz = ez * shelldist / fc.steps_f;              // clouds.glsl:230
        ss2 = rx * rx + ry * ry + rz * rz;
        r.above = sd2 >= SQRT_EXACT_MIN && ss2 >= SQRT_EXACT_MIN;
    }
    if (!r.above) { r.px = r.py = r.pz = r.sx = r.sy = r.sz = r.dx = r.dy = r.dz = r.ss = 0.0f; return r; }
    r.ss = sqrt_exact(ss2);                                                            // :143
    r.dx = rx / r.ss; r.dy = ry / r.ss; r.dz = rz / r.ss;                              // :144
    r.sx = r.dx * r.ss; r.sy = r.dy * r.ss; r.sz = r.dz * r.ss;
    r.px = s0x; r.py = s0y; r.pz = s0z;                                                // hash() == 0 (ray_from_dir): p = start
    return r;
}
CSKY_HD Ray scene_depth_ray(const FrameConsts& fc, const SceneDepthGeom& G, float ex, float ey, float ez, float z) {
    return G.kind == DEPTH_VIEW_Z ? scene_depth_ray_k<DEPTH_VIEW_Z>(fc, G.og, ex, ey, ez, z) : scene_depth_ray_k<DEPTH_DISTANCE>(fc, G.og, ex, ey, ez, z);
}

#pragma clang fp contract(fast)

}  // namespace csky
