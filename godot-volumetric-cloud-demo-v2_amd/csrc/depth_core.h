// depth_core.h -- the cloud depth frame (cloudsky.h csky_render_cloud_depth), written for one pixel per lane.
//
// Where along each ray of a hemisphere frame the cloud sits: the primary march of clouds.glsl:172-178, :207, :210 over the frame's own rays
// (cloud_core.h pixel_dir and ray_from_dir, ray_setup's two halves) without the light march, keeping per ray the distance of the first and the
// last in-cloud sample and the mean of the sample distances weighted by what each sample adds to alpha, T (1 - dt).  What is new here is only
// that bookkeeping and the distance t0 of the shell entry, which depth_pixel takes from the direction with the ray's own intersect_sphere_cam; a
// sample is cloud_core.h's sample_density_eager<false> behind its exact rejects, as in the primary march.
//
// Host+device (CSKY_HD) like cloud_core.h: tests/cloud_aerial_host runs this per-lane code on a CPU against a numpy restatement of the
// definition that calls the oracle per sample.  The product instantiates it inside depth.hip only.
#pragma once
#include "cloud_core.h"

namespace csky {

// What a launch needs besides the FrameConsts below: the frame's size and addressing.  A kernel argument, like the FrameConsts of this path: a
// depth call takes no slot of the cloud frames' constants ring and leaves nothing behind on the device.
struct DepthConsts {
    int w, h;                 // pixels
    int steps;                // N
    uint32_t pitch_px;        // output row pitch in pixels (8 bytes each)
};

// =================================================================================================
// Section A: exact fp32 (no contraction), the order of the definition in cloudsky.h.
// =================================================================================================
#pragma clang fp contract(off)

// The frame is the whole W x H image, update position 0, and reads no sun: the density constants (cloud_core.h).  Everything else is zero.
CSKY_HD void depth_frame_consts(const CloudParams& P, int w, int h, int steps, float hf_lo, float hf_hi, int ct_mode, FrameConsts& fc) {
    memset(&fc, 0, sizeof fc);
    fc.tex_w = (float)w; fc.tex_h = (float)h;
    density_frame_consts(P, steps, hf_lo, hf_hi, fc);
    fc.ct_mode = ct_mode;
}

// What a ray has met so far.  front < 0: no in-cloud sample yet (a distance is > 0).
struct DepthAcc { float sw, swd, front, back; };

// In-cloud sample k (0-based) of a ray that entered the shell t0 metres from the observer: T is the transmittance in front of it, dt its own.
CSKY_HD void depth_accumulate(DepthAcc& a, float t0, float ss, int k, float T, float dt) {
    const float s = t0 + (float)(k + 1) * ss;
    const float w = T * (1.0f - dt);
    a.sw = a.sw + w;
    a.swd = a.swd + w * s;
    if (a.front < 0.0f) a.front = s;
    a.back = s;
}

struct DepthTexel { uint16_t h[4]; };   // mean, front, back in km; the frame's alpha

CSKY_HD DepthTexel depth_texel_of(const DepthAcc& a, float alpha) {
    DepthTexel t; t.h[0] = t.h[1] = t.h[2] = t.h[3] = 0;
    if (!(a.sw > 0.0f)) return t;
    const float mean = fminf(fmaxf(a.swd / a.sw, a.front), a.back);
    t.h[0] = f2h(mean / 1000.0f); t.h[1] = f2h(a.front / 1000.0f); t.h[2] = f2h(a.back / 1000.0f); t.h[3] = f2h(sat(alpha));
    return t;
}

// =================================================================================================
// Section B: the samples and their exp (contraction allowed, hardware exp2): the march's expressions.
// =================================================================================================
#pragma clang fp contract(fast)

// The N samples of one ray; returns the stored texel.  `live`: the lane has a pixel whose ray is above the horizon (the other lanes only take
// part in the votes).  Every fourth step the wavefront stops when each of its lanes is above the height window for good: |p| only grows along
// a ray that starts on the inner shell (the argument and the margins of march_compact.h march_compact).  `taken`, `incloud` (may be null):
// += the samples this lane took, and those of them with t > 0.
template <class TS>
CSKY_HD DepthTexel depth_march(const TS& T, const FrameConsts& fc, const DepthConsts& dc, const Ray& ray, float t0, bool live, unsigned long long* taken,
                               unsigned long long* incloud) {
    float px = ray.px, py = ray.py, pz = ray.pz;
    float Tr = 1.0f, alpha = 0.0f;
    DepthAcc a; a.sw = 0.0f; a.swd = 0.0f; a.front = -1.0f; a.back = 0.0f;
    const float nd = -fc.density;
    unsigned n = 0, nin = 0;
    for (int k = 0; k < dc.steps; k++) {
        bool below_top = false;
        if (live) {
            advance(px, py, pz, ray.sx, ray.sy, ray.sz);                                                          // :173
            const float hf = height_fraction(length3_shell(px, py, pz));                                          // :175
            const float t = sample_density_eager<false>(T, fc, px, py, pz, hf, fc.wpos_x, fc.wpos_y, 0, 0);       // :174, :177
            n++;
            if (t > 0.0f) {                                                                                       // :184
                nin++;
                const float dt = fast_exp(nd * t * ray.ss);                                                       // :178
                depth_accumulate(a, t0, ray.ss, k, Tr, dt);
                alpha += (1.0f - dt) * (1.0f - alpha);                                                            // :207
                Tr *= dt;                                                                                         // :210
            }
            below_top = !(hf >= fc.hf_hi);
        }
        if ((k & 3) == 3 && CSKY_WAVE_ALL(!below_top)) break;
    }
    if (taken) *taken += n;
    if (incloud) *incloud += nin;
    return depth_texel_of(a, alpha);
}

// One pixel, as a lane of depth.hip runs it.  valid: (i, j) lies inside the frame.  t0_out, ss_out (may be null): the ray's entry distance
// and step length, 0 under the horizon.
template <class TS>
CSKY_HD DepthTexel depth_pixel(const TS& T, const FrameConsts& fc, const DepthConsts& dc, int i, int j, bool valid, unsigned long long* taken,
                               unsigned long long* incloud, float* t0_out = nullptr, float* ss_out = nullptr) {
    const int pi = valid ? i : 0, pj = valid ? j : 0;
    float dx, dy, dz;
    pixel_dir(fc.tex_w, fc.tex_h, pi, pj, dx, dy, dz);
    const Ray ray = ray_from_dir(fc, dx, dy, dz);
    const float t0 = ray.above ? intersect_sphere_cam(dx, dy, dz, SKY_B_RADIUS) : 0.0f;
    if (t0_out) *t0_out = t0;
    if (ss_out) *ss_out = ray.ss;
    return depth_march(T, fc, dc, ray, t0, valid && ray.above, taken, incloud);
}

}  // namespace csky
