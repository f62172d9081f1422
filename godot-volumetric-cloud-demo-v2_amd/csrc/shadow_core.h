// shadow_core.h -- the cloud shadow map (cloudsky.h csky_render_cloud_shadow), written for one texel per lane.
//
// T(i, j) is the transmittance of the cloud layer from a ground point g of the observer's tangent plane towards the sun: the primary march's own
// extinction (clouds.glsl:172-178, :207, :210) along the parallel ray g + l t between the two cloud shells, N samples at the mid-points of N equal
// steps, without the view march's jitter.  What is new here is only the general sphere intersection (cloud_core.h's assumes the camera position), the
// texel -> ray set-up and its three kinds of texel; a sample is cloud_core.h's sample_density_eager<false> behind its exact rejects, as in the primary march.
//
// Host+device (CSKY_HD) like cloud_core.h: tests/shadow_host runs this per-lane code on a CPU against a numpy restatement of the definition that calls
// the oracle per sample.  The product instantiates it inside shadow.hip only.
#pragma once
#include "cloud_core.h"

namespace csky {

// What a launch needs besides the FrameConsts below: the map's geometry and addressing.  A kernel argument, like the FrameConsts of this path: a
// shadow call takes no slot of the cloud frames' constants ring and leaves nothing behind on the device.
struct ShadowConsts {
    int w, h;                 // texels
    float cx, cz, ex, ez;     // centre and side lengths, metres (csky_shadow_params)
    int steps;                // N
    int exact_end;            // 1: a lane whose stored half is already 0 stops sampling (shadow_march)
    int night;                // 1: l.y <= 0 (or no direction at all): every texel is 0
    uint32_t pitch_h;         // output row pitch in halfs
};

// =================================================================================================
// Section A: exact fp32 (no contraction), the order of the definition in cloudsky.h.
// =================================================================================================
#pragma clang fp contract(off)

// clouds.glsl:97-105 for any position (dot products summed left to right), taken apart: the line g + l t is tested against both shells before a
// root is taken.  disc < 0: the line does not meet the sphere.
struct SphereLine { float a, b; };
CSKY_HD SphereLine sphere_line(float px, float py, float pz, float dx, float dy, float dz) {
    SphereLine q;
    q.a = dx * dx + dy * dy + dz * dz;
    q.b = 2.0f * (dx * px + dy * py + dz * pz);
    return q;
}
CSKY_HD float sphere_disc(const SphereLine& q, float px, float py, float pz, float r) {
    const float c = (px * px + py * py + pz * pz) - (r * r);
    return (q.b * q.b) - 4.0f * q.a * c;
}
// the larger (the shader's) and the smaller root for a discriminant >= 0
CSKY_HD float sphere_far(const SphereLine& q, float disc) {
    const float d = sqrtf(disc);
    const float p = -q.b - d, p2 = -q.b + d;
    return fmaxf(p, p2) / (2.0f * q.a);
}
CSKY_HD float sphere_near(const SphereLine& q, float disc) {
    const float d = sqrtf(disc);
    const float p = -q.b - d, p2 = -q.b + d;
    return fminf(p, p2) / (2.0f * q.a);
}

// What a shadow ray reads of FrameConsts: the density constants and the sun's direction (cloud_core.h), which frame_setup_f fills the same way
// but only with a sky LUT, for the colours this path never reads.  Everything else is zero.
CSKY_HD void shadow_frame_consts(const CloudParams& P, int steps, float hf_lo, float hf_hi, int ct_mode, FrameConsts& fc) {
    memset(&fc, 0, sizeof fc);
    density_frame_consts(P, steps, hf_lo, hf_hi, fc);
    light_dir_consts(P, fc);
    fc.ct_mode = ct_mode;
}

// The three kinds of texel (cloudsky.h).  A ground point of the tangent plane lies above the inner shell from 134 km out, and under a low sun its
// line can pass over that shell (CHORD: it crosses the layer from the outer shell to the outer shell) or over both (MISS: no cloud on it).
enum ShadowKind { SHADOW_ORDINARY = 0, SHADOW_CHORD = 1, SHADOW_MISS = 2 };

struct ShadowRay {
    float px, py, pz;     // first sample position: start + step / 2
    float sx, sy, sz;     // step
    float ss;             // step length
    int kind;             // ShadowKind; a SHADOW_MISS ray has no samples and all-zero fields
};

// texel (i, j) -> its ray.  fc.ldir = normalize(LIGHT_DIRECTION), fc.steps_f = N.
CSKY_HD ShadowRay shadow_ray_setup(const ShadowConsts& sc, const FrameConsts& fc, int i, int j) {
    ShadowRay r;
    const float u = ((float)i + 0.5f) / (float)sc.w, v = ((float)j + 0.5f) / (float)sc.h;
    const float gx = sc.cx + (u - 0.5f) * sc.ex, gy = G_RADIUS, gz = sc.cz + (v - 0.5f) * sc.ez;
    const float lx = fc.ldir[0], ly = fc.ldir[1], lz = fc.ldir[2];
    const SphereLine q = sphere_line(gx, gy, gz, lx, ly, lz);
    const float disc_b = sphere_disc(q, gx, gy, gz, SKY_B_RADIUS), disc_t = sphere_disc(q, gx, gy, gz, SKY_T_RADIUS);
    r.kind = disc_b >= 0.0f ? SHADOW_ORDINARY : disc_t >= 0.0f ? SHADOW_CHORD : SHADOW_MISS;
    if (r.kind == SHADOW_MISS) { r.px = r.py = r.pz = r.sx = r.sy = r.sz = r.ss = 0.0f; return r; }
    const float t0 = r.kind == SHADOW_ORDINARY ? sphere_far(q, disc_b) : sphere_near(q, disc_t);
    const float t1 = sphere_far(q, disc_t);
    const float s0x = gx + lx * t0, s0y = gy + ly * t0, s0z = gz + lz * t0;                   // start
    const float e0x = gx + lx * t1, e0y = gy + ly * t1, e0z = gz + lz * t1;                   // end
    const float sd = length3_exact(e0x - s0x, e0y - s0y, e0z - s0z);
    r.ss = sd / fc.steps_f;
    r.sx = lx * sd / fc.steps_f; r.sy = ly * sd / fc.steps_f; r.sz = lz * sd / fc.steps_f;    // clouds.glsl:230 with N for 128
    r.px = s0x + r.sx * 0.5f; r.py = s0y + r.sy * 0.5f; r.pz = s0z + r.sz * 0.5f;
    return r;
}

// =================================================================================================
// Section B: the samples and the final exp (contraction allowed, hardware exp2).
// =================================================================================================
#pragma clang fp contract(fast)

// exp(-x) is stored as the half 0 from here on: exp(-18) = 1.52e-8 < 2^-25, the smallest value that does not round to 0 (ties to even)
constexpr float SHADOW_TAU_END = 18.0f;

// The N samples of one texel; returns the stored half.  `live`: the lane has a texel (a ragged tile's other lanes only take part in the votes).
// Exact end: x = (density ss) tau never decreases -- every sample is >= 0, fp32 addition and the multiplication by density ss >= 0 round monotonically
// (a negative or NaN density never reaches the threshold) -- so once x >= 18 the final x is too, and fast_exp(-x) is stored as 0 whatever follows:
// the lane stops sampling and its own x, as it stands, gives that 0.  Every fourth step the wavefront stops when each of its lanes has ended or is above
// the height window for good (|p| only grows along a ray that starts on the inner shell: the argument and the margins of cloud_kernels.hip
// march_compact).  `taken` (may be null): += the samples this lane took.
template <class TS>
CSKY_HD uint16_t shadow_march(const TS& T, const FrameConsts& fc, const ShadowConsts& sc, const ShadowRay& r, bool live, unsigned long long* taken) {
    float px = r.px, py = r.py, pz = r.pz, tau = 0.0f;
    const float k = fc.density * r.ss;
    const bool chord = r.kind == SHADOW_CHORD;
    unsigned n = 0;
    for (int i = 0; i < sc.steps; i++) {
        bool more = false;                                                                   // this lane may still meet a non-zero sample that matters
        if (live) {
            const float hf = height_fraction(length3_shell(px, py, pz));
            tau += sample_density_eager<false>(T, fc, px, py, pz, hf, fc.wpos_x, fc.wpos_y, 0, 0);   // clouds.glsl:174 + :109-137, mip 0
            advance(px, py, pz, r.sx, r.sy, r.sz);
            n++;
            if (sc.exact_end && k * tau >= SHADOW_TAU_END) live = false;
            more = live && (chord || !(hf >= fc.hf_hi));
        }
        if ((i & 3) == 3 && CSKY_WAVE_ALL(!more)) break;
    }
    if (taken) *taken += n;
    return f2h(fast_exp(-(k * tau)));
}

// One texel, as a lane of shadow.hip runs it.  valid: (i, j) lies inside the map.
template <class TS>
CSKY_HD uint16_t shadow_texel(const TS& T, const FrameConsts& fc, const ShadowConsts& sc, int i, int j, bool valid, unsigned long long* taken) {
    if (sc.night) return 0;                                                                  // uniform over the launch
    const ShadowRay r = shadow_ray_setup(sc, fc, valid ? i : 0, valid ? j : 0);
    const uint16_t h = shadow_march(T, fc, sc, r, valid && r.kind != SHADOW_MISS, taken);     // a line that meets no cloud is not live: it only votes
    return r.kind == SHADOW_MISS ? (uint16_t)0x3C00 : h;                                      // and stores the half 1.0
}

}  // namespace csky
