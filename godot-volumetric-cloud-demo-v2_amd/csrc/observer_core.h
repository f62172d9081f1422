// observer_core.h -- the front end of the direct cloud march for an observer who is not the reference's (cloudsky.h csky_render_clouds_view_from /
// _dirs_from), written for one pixel per lane.
//
// rays_core.h makes the march's Ray from a direction as clouds.glsl does: from camPos = (0, g_radius, 0), inner shell to outer shell.  This file
// makes it from a direction and a POSITION: the observer may stand under the layer, inside it or above it, the ray's first segment through the layer
// runs up, down or level, and a distance cap may end it early.  The march behind it is the same (march_compact.h march_compact, cloud_core.h
// march()): density, height window and light march are functions of position.
//
// Host+device (CSKY_HD) like rays_core.h: tests/observer_host runs this per-lane code on a CPU.  The product instantiates it inside
// cloud_kernels.hip only.
#pragma once
#include "rays_core.h"

namespace csky {

// What an observer launch needs: a rays launch's geometry, the observer's world position (metres, the planet's centre at the origin) and the cap on
// the distance along a ray.  The argument block of clouds_observer_kernel; RaysGeom itself gains nothing.
struct ObserverGeom {
    RaysGeom g;
    float o[3];
    float max_dist;           // metres from the observer; +inf: no cap
};

// Where an observer may stand (csky_observer): horizontally within 1000 km of the reference's camera, between the ground sphere and 100 km above it.
constexpr float OBSERVER_MAX_OFFSET = 1.0e6f, OBSERVER_MAX_ALTITUDE = 100000.0f;

// =================================================================================================
// Exact fp32 (no contraction): the order of the definition in cloudsky.h.
// =================================================================================================
#pragma clang fp contract(off)

// The world position of csky_observer.position: relative to the reference's camera (0, G_RADIUS, 0), formed once on the host.
CSKY_HD void observer_origin(const float position[3], float o[3]) {
    o[0] = position[0]; o[1] = G_RADIUS + position[1]; o[2] = position[2];
}

// Which csky_observer the calls refuse (CSKY_ERR_INVALID), as a rule number for the error text; 0: accepted.
//   1 a non-finite position   2 |position[0]| or |position[2]| above OBSERVER_MAX_OFFSET   3 |o| below G_RADIUS   4 |o| above G_RADIUS + OBSERVER_MAX_ALTITUDE
//   5 max_distance not > 0 (NaN included; +inf is no cap)
CSKY_HD int observer_invalid(const float position[3], float max_distance) {
    for (int k = 0; k < 3; k++) if (!(fabsf(position[k]) <= 3.0e38f)) return 1;
    if (fabsf(position[0]) > OBSERVER_MAX_OFFSET || fabsf(position[2]) > OBSERVER_MAX_OFFSET) return 2;
    float o[3];
    observer_origin(position, o);
    const float r = length3_ieee(o[0], o[1], o[2]);
    if (!(r >= G_RADIUS)) return 3;
    if (!(r <= G_RADIUS + OBSERVER_MAX_ALTITUDE)) return 4;
    if (!(max_distance > 0.0f)) return 5;
    return 0;
}

// The geometry block of a w x h observer launch: rays_geom's, the observer's world position and the cap.  The one place that fills it, on the host.
CSKY_HD ObserverGeom observer_geom(const float* basis, float fov_y_degrees, int w, int h, uint32_t pitch_px, const float position[3], float max_distance) {
    ObserverGeom G;
    G.g = rays_geom(basis, fov_y_degrees, w, h, pitch_px);
    observer_origin(position, G.o);
    G.max_dist = max_distance;
    return G;
}

// Which directions may be marched: rays_accept without its `above the horizon`.  NaN fails every comparison, +-inf the upper one.
CSKY_HD bool observer_accept(float dx, float dy, float dz) {
    const float l2 = (dx * dx + dy * dy) + dz * dz;
    return l2 >= 0.99f && l2 <= 1.01f;
}

// clouds.glsl:97-105 with pos = o, in intersect_sphere_cam's operation order; both roots, and the discriminant for "does the line meet the sphere".
struct SphereHit { float D, near, far; };
CSKY_HD float observer_c(const float o[3], float r) { return (o[0] * o[0] + o[1] * o[1] + o[2] * o[2]) - (r * r); }
CSKY_HD SphereHit observer_isect(float a, float b, float c) {
    SphereHit s;
    s.D = (b * b) - 4.0f * a * c;
    const float d = sqrtf(s.D);
    const float p = -b - d, p2 = -b + d;
    s.near = fminf(p, p2) / (2.0f * a);
    s.far = fmaxf(p, p2) / (2.0f * a);
    return s;
}

// The first segment [t0, t1] of the line o + e t, t >= 0, through the cloud layer, capped; false where there is none.  The definition's `segment`,
// `cap` and the last clause of `marched`, for an accepted direction.
CSKY_HD bool observer_segment(const float o[3], float max_dist, float dx, float dy, float dz, float& t0, float& t1) {
    const float a = dx * dx + dy * dy + dz * dz;
    const float b = 2.0f * (dx * o[0] + dy * o[1] + dz * o[2]);
    const float cb = observer_c(o, SKY_B_RADIUS), ct = observer_c(o, SKY_T_RADIUS);
    const SphereHit hb = observer_isect(a, b, cb), ht = observer_isect(a, b, ct);
    if (cb < 0.0f) {                                            // under the layer: up through it, unless the ground is in the way
        const SphereHit hg = observer_isect(a, b, observer_c(o, G_RADIUS));
        if (b <= 0.0f && hg.D >= 0.0f) return false;
        t0 = hb.far; t1 = ht.far;
    } else if (ct > 0.0f) {                                     // above it: down into it, out through the bottom or, past the inner shell, the top
        if (!(b < 0.0f && ht.D >= 0.0f)) return false;
        t0 = ht.near; t1 = hb.D >= 0.0f ? hb.near : ht.far;
    } else {                                                    // inside
        t0 = 0.0f; t1 = (b < 0.0f && hb.D >= 0.0f) ? hb.near : ht.far;
    }
    t1 = fminf(t1, max_dist);
    return t1 > t0;                                             // NaN fails
}

// The ray of a direction as a lane uses it; `above` means "marched".  Not marched: `above = false`, zero fields (no sample, a zero texel), as
// rays_ray's.  The tail from `shelldist` on restates cloud_core.h ray_from_dir's (sharing it through a helper would change that function's own
// compiled code): with position (0, 0, 0) and no cap all eleven fields are rays_ray's bit for bit (tests/test_observer_host.py O1).
//
// The last clause of `marched`: a segment long enough to have a direction.  World positions are near 6e6 m, where fp32 has a quantum of 0.5 m, so a
// max_distance within that quantum of t0 (1500.2 m straight up from the ground: t0 = 1500) passes `t1 > t0` and still rounds the end onto the start:
// shelldist = 0, ss = 0, dir = 0 / 0.  From inside the layer on the axis (t0 = 0, o.x = o.z = 0) a cap of 1e-22 m gives a shelldist > 0 whose raystep's
// squares underflow, and the same NaN.  So both square roots of the tail must take an argument inside sqrt_exact's specified range:
// |end - start|^2 >= 2^-102 and |raystep|^2 >= 2^-102, scene_depth_core.h scene_depth_ray_k's clause.  On that range host and device agree bit for
// bit and dir is a unit vector.  Otherwise the ray is not marched.
CSKY_HD Ray observer_ray(const FrameConsts& fc, const ObserverGeom& G, float ex, float ey, float ez) {
    Ray r;
    float t0 = 0.0f, t1 = 0.0f;
    r.above = observer_accept(ex, ey, ez) && observer_segment(G.o, G.max_dist, ex, ey, ez, t0, t1);
    float s0x = 0.0f, s0y = 0.0f, s0z = 0.0f, rx = 0.0f, ry = 0.0f, rz = 0.0f, ss2 = 0.0f;
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

#pragma clang fp contract(fast)

}  // namespace csky
