// cloud_kernels.hip -- gfx950 (CDNA4, wave64) kernels of clouds.glsl main(): one ray per lane, one 8x8-pixel tile per wavefront.
//
//   march_queue / march_compact / march_interleaved : the wave-cooperative marches (the lock-step one is cloud_core.h march())
//   render_block, clouds_kernel<VARIANT, SEG, TS>   : a workgroup footprint of 4 / SEG tiles; <3, 1, TexSet> is the product's kernel
//   clouds_kernel_persistent                        : the same as a launch the size of the chip that pops footprints from the order
//   clouds_kernel_lds / clouds_kernel_interleaved   : measured alternatives (variant 2, segments 5)
//   lpt_*_kernel, static_order_kernel               : the launch orders
//   interleave_bands_kernel, sqrt_shell_kernel      : the band interleave of a gathered frame (what becomes of the bands these kernels
//                                                     write when N ranks split a frame) and the test hook of cloud_core.h::sqrt_shell
//   march_store and the direct march                : whole rays of a W x H image in natural order, one pixel per lane; each kernel is a lane pixel,
//                                                     a direction, its own ray maker and the shared tail march_store:
//     clouds_rays_kernel<SRC, TS>                   :   caller-given directions or a camera view, from the reference's observer (§17)
//     clouds_view_fresh_kernel / _reproject_kernel  :   the temporal split of a view frame: the fresh sub-grid; history taps and holes (§20)
//     clouds_observer_kernel<SRC, TS>               :   the same rays from an observer's position (§21)
//     clouds_observer_depth_kernel<SRC, KIND, TS>   :   those behind a per-pixel scene depth (§22)
//
// No MFMA anywhere: the path is fetch/latency-bound gather + fp32 VALU, not a contraction.
// What was built here, measured and removed again is recorded in docs/EXPERIMENTS.md §5.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "cloud_core.h"
#include "order_core.h"
#include <type_traits>
// FP contraction OFF for the code of this file, like section A of cloud_core.h: what a march adds and multiplies itself (the phase value's dot product,
// the segments' compositing sums) rounds as written.  Stated here because otherwise the last header decides it, and cloud_core.h ends with contraction on.
#pragma clang fp contract(off)

namespace csky {

// ---- wave-cooperative march (variant "queue") --------------------------------------------------------------
// The lock-step march (cloud_core.h march()) runs the (light_steps+1)-sample light march on all 64 lanes whenever
// ANY lane of the wavefront is inside a cloud.  Measured on the headline frame: a lane is in cloud on 15 % of its
// steps, a wavefront on ~70 % of them, so ~4/5 of the light-march VALU work is masked off.  Here the two loops
// are decoupled through a per-wavefront event queue in LDS:
//   A. all lanes march their primary samples in lock step (uniform loop, clouds.glsl:172-178); every in-cloud
//      sample (t > 0, clouds.glsl:184) is appended to the queue (position, t, height fraction) at
//      slot = running count + mbcnt(ballot);
//   B. when the queue may overflow (or the march ends) the n queued samples need n*(light_steps+1) independent
//      density evaluations (clouds.glsl:186-199).  They are flattened as e = j*n + k and dealt out 64 per round,
//      so every round runs with all lanes busy no matter which rays were in cloud;
//   C. the queue is replayed step by step: the owning lane sums its light samples in the reference's order and
//      composites the sample front to back (clouds.glsl:202-210).
// No __syncthreads: wavefronts are independent; LDS operations of one wavefront complete in issue order and
// wavefront-scope fences keep the compiler from reordering them.  Per-ray arithmetic and its order are unchanged.
constexpr int QCAP = 96;                                    // events per wavefront queue (a flush is forced above QCAP-64)
constexpr int QSTEPS = 48;                                  // steps-with-events per chunk (a flush is forced when full)
constexpr int Q_FLOATS = 5 * QCAP + 7 * QCAP + 3 * QSTEPS;  // pos(3) t hf | lt[7] | per-step mask lo/hi + base  = 5.1 KB per wavefront

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the phase value of a ray's samples (0 for a ray that does not march)
__device__ __forceinline__ float ray_phase(const FrameConsts& fc, const Ray& ray) {
    float phase = 0.0f;
    if (ray.above) {
        const float ct = fc.ldir[0] * ray.dx + fc.ldir[1] * ray.dy + fc.ldir[2] * ray.dz;                       // clouds.glsl:158
        phase = fmaxf(fmaxf(henyey_greenstein(ct, 0.6f), henyey_greenstein(ct, fc.hg_g2)), henyey_greenstein(ct, -0.2f));  // :160
    }
    return phase;
}

// Step B of the queue marches: the nb * (ls + 1) light-march evaluations of nb queued samples (clouds.glsl:186-199), flattened as e = j * nb + k
// and dealt out 64 per round, so every round runs with all lanes busy no matter which rays were in cloud.  pos(k, x, y, z) delivers sample k's
// position; the density of its cone sample j (j == ls: the distant sample) goes to lt[j * pitch + k].
template <class Pos> __device__ __forceinline__ void light_march_batch(const TexSet& T, const FrameConsts& fc, const int ls, const int nb, const int lane, Pos&& pos,
                                                                      float* __restrict__ lt, const int pitch) {
    const int total = nb * (ls + 1);
    const float rn = 1.0f / (float)nb;
    for (int e0 = 0; e0 < total; e0 += 64) {
        const int e = e0 + lane;
        if (e < total) {
            const int j = (int)(((float)e + 0.5f) * rn);          // e = j*nb + k (exact: e < 672, nb <= 96)
            const int k = e - j * nb;
            float lx, ly, lz;
            pos(k, lx, ly, lz);
            const bool distant = (j == ls);
            // cone sample j: lp = p + sum_{i<=j} (ldir + RANDOM_VECTORS[i]*i)*lss, added one by one in fp32 like :187.
            // e grows with the lane, so j is non-decreasing across the wavefront: the additions up to the first lane's j
            // are wave-uniform (plain adds under a scalar branch), only the few beyond it need per-lane predication.
            const int j_lo = __builtin_amdgcn_readfirstlane(j);
            if (distant) {
                advance(lx, ly, lz, fc.ldist[0], fc.ldist[1], fc.ldist[2]);                                // :195
            } else {
#pragma unroll
                for (int jj = 0; jj < 6; jj++) {
                    if (jj <= j_lo) advance(lx, ly, lz, fc.linc[jj][0], fc.linc[jj][1], fc.linc[jj][2]);
                    else if (jj <= j) advance(lx, ly, lz, fc.linc[jj][0], fc.linc[jj][1], fc.linc[jj][2]);
                }
            }
            const float lhf = height_fraction(length3_shell(lx, ly, lz));                                  // :188 / :196
            const int lod_s = distant ? 3 : (j > 2 ? j - 2 : 0), lod_d = distant ? 5 : j;                  // textureLod(.., mip-2) / (.., mip)
            float d = sample_density(T, fc, lx, ly, lz, lhf, distant ? 0.0f : fc.wpos_x, distant ? 0.0f : fc.wpos_y, lod_s, lod_d);  // :189-190 / :197-198
            if (distant) d = fast_pow(d, (1.0f - lhf) * 0.8f + 0.5f);                                      // :198 second pow
            lt[j * pitch + k] = d;
        }
    }
}

__device__ __forceinline__ MarchOut march_queue(const TexSet& T, const FrameConsts& fc, Ray ray, float* __restrict__ q, int step_begin, int step_end) {
    float* __restrict__ ev_px = q;
    float* __restrict__ ev_py = q + QCAP;
    float* __restrict__ ev_pz = q + 2 * QCAP;
    float* __restrict__ ev_t = q + 3 * QCAP;
    float* __restrict__ ev_hf = q + 4 * QCAP;
    float* __restrict__ ev_lt = q + 5 * QCAP;                               // [7][QCAP]
    unsigned* __restrict__ st_lo = reinterpret_cast<unsigned*>(q + 12 * QCAP);   // [QSTEPS]
    unsigned* __restrict__ st_hi = st_lo + QSTEPS;
    unsigned* __restrict__ st_base = st_hi + QSTEPS;

    MarchOut o; o.r = o.g = o.b = o.a = 0.0f; o.t = 1.0f; o.incloud = 0;
    const int lane = threadIdx.x & 63;
    const int ls = fc.light_steps, nl = ls + 1;
    const float phase = ray_phase(fc, ray);
    float Tr = 1.0f, alpha = 0.0f, Lr = 0.0f, Lg = 0.0f, Lb = 0.0f;
    float px = ray.px, py = ray.py, pz = ray.pz;
    const float nd = -fc.density;
    bool live = ray.above;
    int count = 0, cs = 0;                                    // queued events / steps-with-events in the current chunk (uniform)
    if (!__any(live)) return o;
    // a ray segment starts where the sequential march would be after step_begin steps: replay the fp32 additions
    // (clouds.glsl:173) so every sample position is bit-identical to the unsegmented march
    for (int i = 0; i < step_begin; i++) advance(px, py, pz, ray.sx, ray.sy, ray.sz);
    for (int i = step_begin; i < step_end; i++) {
        // ---- A: one primary sample per lane
        float t = 0.0f, hf = 0.0f;
        if (live) {
            advance(px, py, pz, ray.sx, ray.sy, ray.sz);                                                       // :173
            hf = height_fraction(length3_shell(px, py, pz));                                                   // :175
            t = sample_density(T, fc, px, py, pz, hf, fc.wpos_x, fc.wpos_y, 0, 0);                             // :174, :177
        }
        const bool have = t > 0.0f;                                                                            // :184
        const unsigned long long m = __ballot(have);
        if (m != 0ull) {
            const int slot = count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (have) { ev_px[slot] = px; ev_py[slot] = py; ev_pz[slot] = pz; ev_t[slot] = t; ev_hf[slot] = hf; }
            if (lane == 0) { st_lo[cs] = (unsigned)m; st_hi[cs] = (unsigned)(m >> 32); st_base[cs] = (unsigned)count; }
            count += __popcll(m);
            cs++;
        }
        if (count <= QCAP - 64 && cs < QSTEPS && i + 1 < step_end) continue;
        if (count == 0) continue;
        // ---- B: count*(ls+1) light-march evaluations, 64 per round, all lanes busy
        wave_lds_fence();
        light_march_batch(T, fc, ls, count, lane, [&](int k, float& x, float& y, float& z) { x = ev_px[k]; y = ev_py[k]; z = ev_pz[k]; }, ev_lt, QCAP);
        wave_lds_fence();
        // ---- C: replay the chunk in step order; owners composite (:191,:199 sums in the reference's order, :202-210)
        for (int s = 0; s < cs; s++) {
            const unsigned lo = st_lo[s], hi = st_hi[s];
            const bool mine = lane < 32 ? ((lo >> lane) & 1u) : ((hi >> (lane - 32)) & 1u);
            if (mine) {
                const int slot = (int)st_base[s] + (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
                float cd = 0.0f;
                for (int j = 0; j < nl; j++) cd += ev_lt[j * QCAP + slot];
                const float et = ev_t[slot], ehf = ev_hf[slot];
                const float dt = fast_exp(nd * et * ray.ss);                                                   // :178
                shade_sample(fc, phase, et, ehf, dt, cd, Tr, alpha, Lr, Lg, Lb);
                o.incloud++;
            }
        }
        wave_lds_fence();
        count = 0; cs = 0;
        if (fc.early_eps > 0.0f) {                                     // build-side early-out (off by default, bounded error)
            if (Tr < fc.early_eps) live = false;
            if (!__any(live)) break;
        }
    }
    o.r = Lr; o.g = Lg; o.b = Lb; o.a = sat(alpha); o.t = Tr;                                                  // :213-214
    return o;
}

// ---- compacted light march (variant "compact") ------------------------------------------------------------------
// Same decoupling as march_queue, but a flush always takes EXACTLY 64 queued samples, one per lane (k = lane): every lane
// then runs the reference's whole light march (clouds.glsl:186-199) for its sample in registers.  The loop index j is
// wave-uniform, so the LOD, the mip extent and offsets, the cone increment and the distant-sample special case are scalar
// (SALU / immediates) instead of per-lane VALU selects, the cone position is carried in registers (3 adds per sample instead
// of re-adding j+1 increments under predication), and the per-sample densities are summed in place (no lt[7][QCAP] array).
// Samples beyond the 64th stay queued (moved to the front) together with the part of the last step that owns them; only
// the final flush of a ray segment runs with idle lanes.
constexpr int CQ_CAP = 128;                                  // a flush is taken as soon as 64 samples are queued: count <= 63 + 64
constexpr int CQ_STEPS = 66;                                 // steps-with-events between flushes: <= 1 carried + 64 (>= 1 event each)
constexpr int CQ_FLOATS = 5 * CQ_CAP + CQ_CAP / 4 + 3 * CQ_STEPS + 2 + 128 + 320;   // pos(3) t hf (after the light march: D(3) q dt) | owner lane (bytes) | per-step mask lo/hi + base | in-cloud tally | per-ray ss, phase | per-ray T, alpha, L between flushes = 5.2 KB per wavefront
// The SLIM layout (march_compact<.., SLIM = true>: the specialised persistent forms only, so that eight of their workgroups fit a CU's LDS).  Same samples,
// same order, same flushes; two arrays go:
//   * st_base[CQ_STEPS]: a step's first slot is the previous step's plus the popcount of its mask, and the replay holds the mask as a scalar pair anyway;
//   * ev_hf[64 .. CQ_CAP): a flush evaluates slots 0..63 only, so a sample queued at slot >= 64 is never read there: it is carried to the front first.  The
//     carry recomputes its height fraction from the queued position (the same function of the same three floats as step A: the same bits), once per
//     carried flush with all its lanes at once, not once per queued sample.
constexpr int CQ_HF_SLIM = 64;
// the first slot of the replayed step s: read from st_base, or (SLIM) counted up from the masks of the steps before it (the carried step, or the first
// one after an empty queue, starts at 0).  Two types, so that the wide layout's replay is the code it was.
template <bool SLIM> struct ReplayBase {
    __device__ __forceinline__ int first(const unsigned* __restrict__ st_base, int s) const { return (int)st_base[s]; }
    __device__ __forceinline__ void next(unsigned, unsigned) {}
};
template <> struct ReplayBase<true> {
    int base = 0;
    __device__ __forceinline__ int first(const unsigned* __restrict__, int) const { return base; }
    __device__ __forceinline__ void next(unsigned lo, unsigned hi) { base += __builtin_popcount(lo) + __builtin_popcount(hi); }
};
constexpr int CQ_FLOATS_SLIM = 4 * CQ_CAP + CQ_HF_SLIM + CQ_CAP / 4 + 2 * CQ_STEPS + 2 + 128 + 320;   // 4 760 bytes per wavefront

#ifndef CSKY_EAGER_LIGHT
#define CSKY_EAGER_LIGHT 1
#endif
#if CSKY_EAGER_LIGHT
#define CSKY_LIGHT_SAMPLE(CT) sample_density_eager<true, false, CT>
#else
#define CSKY_LIGHT_SAMPLE(CT) sample_density<CT>
#endif
#ifndef CSKY_EAGER_PRIMARY
#define CSKY_EAGER_PRIMARY 0   // eager fetches in the PRIMARY march measured slower (1: weather + shape together +1 %, 2: all three +4.5 %): only
                               // 56 % / 22 % of its samples need the shape / detail cell, the extra gathers cost more than the latency they hide
#endif
#if CSKY_EAGER_PRIMARY == 1
#define CSKY_PRIMARY_SAMPLE(CT) sample_density_eager<false, false, CT>
#elif CSKY_EAGER_PRIMARY == 2
#define CSKY_PRIMARY_SAMPLE(CT) sample_density_eager<true, false, CT>
#else
#define CSKY_PRIMARY_SAMPLE(CT) sample_density<CT>
#endif
// Step B of the compact march for ONE queued in-cloud sample: the reference's light march (clouds.glsl:186-199) from its position and the
// state-independent half of its shading (:178, :202-209).  In: position, density t, height fraction, the owner ray's step length and phase
// value.  Out: D.rgb, 1 / max(1e-7, t), dt (shade_terms).  A function of those seven floats alone (round 4's packet exchange ran it on other
// CUs' wavefronts and got byte-identical frames: docs/EXPERIMENTS.md §5).
// `late(et, ehf, ess, eph)` delivers the four inputs the light march itself does not need AFTER it (the owner reads them from its LDS queue
// then: four registers fewer across the march).
#ifndef CSKY_LIGHT_STRAIGHT
#define CSKY_LIGHT_STRAIGHT 1   // 0: the specialised persistent forms keep round 19's two loops (the A/B of the mode alone, profiles/r22/march_specialised_ab.txt)
#endif
#if CSKY_EAGER_LIGHT
// Cone samples J, J + 1, ... 5 of the persistent form's light march as straight-line code: every sample index has its own copy of the body, so its
// levels, their extents and offsets, the offset of linc[J] and whether the detail tap reads the LDS table (J = 3, 4), the global cell (J < 3) or nothing
// (J = 5) are constants of the place, not scalar arithmetic and scalar branches per sample (round 19's rule carried to every index).  The wave-uniform
// exit `J >= ls` stays in front of every sample: 0..6 light steps.
template <int CT, int J, class TS>
__device__ __forceinline__ void light_samples_from(const TS& T, const FrameConsts& fc, const int ls, float& lx, float& ly, float& lz, float& cd) {
    if constexpr (J < 6) {
        if (J >= ls) return;
        advance(lx, ly, lz, fc.linc[J][0], fc.linc[J][1], fc.linc[J][2]);                              // :187
        const float lhf = height_fraction(length3_shell(lx, ly, lz));                                  // :188
        cd += sample_density_eager<true, (J > 2), CT>(T, fc, lx, ly, lz, lhf, fc.wpos_x, fc.wpos_y, J > 2 ? J - 2 : 0, J);   // :189-191
        light_samples_from<CT, J + 1>(T, fc, ls, lx, ly, lz, cd);
    }
}
#endif
// CT: the cloud-type mode of cloud_core.h density_height_gradient (0: read from fc per evaluation).
template <int CT = 0, class TS, class Late>
__device__ __forceinline__ void light_march_terms(const TS& T, const FrameConsts& fc, const int ls, const float nd, float ex, float ey, float ez, Late&& late,
                                                  float& Dr, float& Dg, float& Db, float& rq, float& dt) {
    float lx = ex, ly = ey, lz = ez, cd = 0.0f;
#if CSKY_EAGER_LIGHT
    constexpr int JS = TS::small_detail ? 3 : 6;                // persistent launches: samples j = 3, 4 (and a j = 5 that taps nothing) run in code of their own
    // persistent launches whose cloud-type mode is compiled in: one copy of the body per sample index (light_samples_from).  The generic form keeps the
    // two loops: straight-line it has 273 / 288 basic blocks (the census build counts 256) and spills inside the flush loop (profiles/r22/march_specialised_ab.txt)
    constexpr bool STRAIGHT = CSKY_LIGHT_STRAIGHT && TS::small_detail && CT != 0;
#else
    constexpr int JS = 6;
    constexpr bool STRAIGHT = false;
#endif
    if constexpr (!STRAIGHT) {
#pragma unroll 1                                                 // scalar j: one loop body (the plain kernel: 6x the code bought nothing in rounds 2 and 5, profiles/r05/kernel_experiments.txt)
        for (int j = 0; j < JS; j++) {                                                                 // :186 (light_steps <= 6)
            if (j >= ls) break;
            advance(lx, ly, lz, fc.linc[j][0], fc.linc[j][1], fc.linc[j][2]);                          // :187
            const float lhf = height_fraction(length3_shell(lx, ly, lz));                              // :188
            cd += CSKY_LIGHT_SAMPLE(CT)(T, fc, lx, ly, lz, lhf, fc.wpos_x, fc.wpos_y, j > 2 ? j - 2 : 0, j);   // :189-191
        }
    }
#if CSKY_EAGER_LIGHT
    if constexpr (STRAIGHT) {
        light_samples_from<CT, 0>(T, fc, ls, lx, ly, lz, cd);
    } else if constexpr (TS::small_detail) {
        // the same samples with their detail tap (LODs 3, 4) served from the LDS table: a second copy of the loop body, so that which path a tap takes is
        // decided by where the code is, not by a branch per sample.  The one-loop form (a scalar branch on the level inside the tap: two more branches and
        // ~4 SALU per light sample) took the same loads off the TA and gained 0.4 % of the headline; this form 3.5 %, of which 2.3 are the split's own (with j >= 3
        // known the shape level and the levels' extents fold: SALU -13 %) and 1.2 the table's (profiles/r19/small_detail_lds_ab.txt)
#pragma unroll 1
        for (int j = JS; j < 6; j++) {
            if (j >= ls) break;
            advance(lx, ly, lz, fc.linc[j][0], fc.linc[j][1], fc.linc[j][2]);                          // :187
            const float lhf = height_fraction(length3_shell(lx, ly, lz));                              // :188
            cd += sample_density_eager<true, true, CT>(T, fc, lx, ly, lz, lhf, fc.wpos_x, fc.wpos_y, j - 2, j);   // :189-191
        }
    }
#endif
    {   // distant sample, :195-199
        lx = ex; ly = ey; lz = ez;
        advance(lx, ly, lz, fc.ldist[0], fc.ldist[1], fc.ldist[2]);
        const float lhf = height_fraction(length3_shell(lx, ly, lz));
        const float ld = CSKY_LIGHT_SAMPLE(CT)(T, fc, lx, ly, lz, lhf, 0.0f, 0.0f, 3, 5);              // :197 has no weather_pos
        cd += fast_pow(ld, (1.0f - lhf) * 0.8f + 0.5f);                                                // :198 (second pow)
    }
    float et, ehf, ess, eph;
    late(et, ehf, ess, eph);
    dt = fast_exp(nd * et * ess);                                                                      // :178
    shade_terms(fc, eph, et, ehf, dt, cd, Dr, Dg, Db, rq);                                             // :202-209
}

// WHOLE: the call marches whole rays (step_begin == 0, step_end == primary_steps; render_block with SEG == 1).  Only then, and only for the fp16-pair
// texture set, the saturation skip applies (cloud_core.h ray_saturated: exact reject (4)): ray segments are combined as fp32 partial (L, T, alpha), which
// the proof does not cover, and TexSet32 and variants 0-2 stay as they are for A/B.  A lane whose ray is saturated LATCHES: it keeps taking its primary
// samples, but a t > 0 one is counted (ballot + popcount into a wave-uniform tally) instead of queued, so its light march and shading are never run and
// `incloud` is what the full march counts.  The test runs once per flush, after the replay, on the state already in registers, and only when some lane not
// yet latched has reached the alpha threshold; samples a latched ray still has in the queue are composited as usual (the bound covers any subset).
// TALLY: the launch delivers `incloud` (launch_clouds: it was given d_stats or d_wg_cost).  Without it the count has no reader, and with SAT a latched
// ray is DEAD: `live` goes false as on the early_eps path, the lane takes no further primary sample (weather, shape and detail taps, pow) and answers
// false to `below_top`, so the every-4th-step ballot ends the wavefront once every lane is latched or above the window.  The queue receives the same
// samples in the same order either way (a latched ray's were never queued), so flushes, latch tests and the stored halfs are those of TALLY = true
// (tests/tilewalk emulates both per tile; tests/test_gpu_latched_rays.py compares the frames).  MarchOut::incloud is 0 and must not be read.
// CT: the cloud-type mode of the frame as a compile-time value (cloud_core.h density_height_gradient); 0 reads fc.ct_mode per evaluation.
// RISING: every ray of the call starts on the inner shell and runs outwards (every caller but clouds_observer_kernel).  It guards the early end below and
// nothing else; without it the wavefront ends once no lane is live, which needs no assumption about the rays.
// SLIM: the queue has the CQ_FLOATS_SLIM layout (above).
template <bool WHOLE, bool TALLY, int CT = 0, class TS, bool RISING = true, bool SLIM = false>
__device__ __forceinline__ MarchOut march_compact(const TS& T, const FrameConsts& fc, Ray ray, float* __restrict__ q, int step_begin, int step_end) {
    constexpr bool SAT = WHOLE && !TS::cell32;
    constexpr bool DEAD = SAT && !TALLY;                      // a latched ray stops marching
    float* __restrict__ ev_px = q;
    float* __restrict__ ev_py = q + CQ_CAP;
    float* __restrict__ ev_pz = q + 2 * CQ_CAP;
    float* __restrict__ ev_t = q + 3 * CQ_CAP;
    float* __restrict__ ev_hf = q + 4 * CQ_CAP;                 // [CQ_CAP], SLIM: [CQ_HF_SLIM]
    constexpr int HF_CAP = SLIM ? CQ_HF_SLIM : CQ_CAP;
    unsigned char* __restrict__ ev_owner = reinterpret_cast<unsigned char*>(q + (4 * CQ_CAP + HF_CAP));   // the sample's owner lane: its step length and phase value are read from ray_ss / ray_ph
    unsigned* __restrict__ st_lo = reinterpret_cast<unsigned*>(q + (4 * CQ_CAP + HF_CAP) + CQ_CAP / 4);  // [CQ_STEPS]
    unsigned* __restrict__ st_hi = st_lo + CQ_STEPS;
    unsigned* __restrict__ st_base = st_hi + CQ_STEPS;          // [CQ_STEPS], SLIM: absent (derived in the replay)

    MarchOut o; o.r = o.g = o.b = o.a = 0.0f; o.t = 1.0f; o.incloud = 0;
    const int lane = threadIdx.x & 63;
    const int ls = fc.light_steps;
    const float phase = ray_phase(fc, ray);
    float px = ray.px, py = ray.py, pz = ray.pz;
    const float nd = -fc.density;
    bool live = ray.above;
    int count = 0, cs = 0;                                    // queued samples / steps owning them (uniform)
    bool latched = false;                                     // saturation skip: this lane's ray is saturated (SAT && TALLY only: a DEAD ray is `!live`)
    unsigned skipped = 0u;                                    // in-cloud samples of latched rays, counted and not queued (uniform; TALLY only)
    unsigned* __restrict__ tally = st_base + (SLIM ? 0 : CQ_STEPS);   // in-cloud samples composited by this wavefront, kept in LDS (round 4: neither a per-lane accumulator register
    if constexpr (TALLY) { if (lane == 0) tally[0] = 0u; }    // in the march loops nor a scalar one in the SGPR-starved persistent form; one ds_add per flush)
    // the two per-ray constants a queued sample carries (step length, phase value) live in LDS, not in registers held across the whole march: the
    // persistent form had spilled `phase` to scratch and re-loaded it, behind a vmcnt(0), at every step with an in-cloud sample (round 4 census)
    float* __restrict__ ray_ss = reinterpret_cast<float*>(tally + 2);
    float* __restrict__ ray_ph = ray_ss + 64;
    ray_ss[lane] = ray.ss; ray_ph[lane] = phase;
    // The running state of the ray (T, alpha, L: clouds.glsl:151-153) is touched only while a flush is composited, ~20 times per tile: between
    // flushes it rests in LDS, not in five registers the allocator had to copy between register sets around every light march (20 M v_mov per
    // C3 frame, round-4 census) and hold across both march loops.
    float* __restrict__ acc = ray_ph + 64;                      // [5][64]
    acc[lane] = 1.0f; acc[64 + lane] = 0.0f; acc[128 + lane] = 0.0f; acc[192 + lane] = 0.0f; acc[256 + lane] = 0.0f;
    if (__builtin_amdgcn_ballot_w64(live) == 0ull) return o;   // (the builtin takes the compare's own lane mask: HIP's __any / __ballot wrappers cost a v_cndmask + v_cmp_ne each)
    for (int i = 0; i < step_begin; i++) advance(px, py, pz, ray.sx, ray.sy, ray.sz);   // segment start: replay the fp32 additions (:173)
    int end = step_end;                                       // shrinks when the whole wavefront has left the height window
    for (int i = step_begin;;) {
        // ---- A: one primary sample per lane (none once the segment is exhausted and only carried samples remain)
        if (i < end) {
            float t, hf;                                     // (meaningful in live lanes only: every use below is guarded by `live` or by `have`)
            bool have = false, below_top = false;
            if (live) {
                advance(px, py, pz, ray.sx, ray.sy, ray.sz);                                                   // :173
                hf = height_fraction(length3_shell(px, py, pz));                                               // :175
                t = CSKY_PRIMARY_SAMPLE(CT)(T, fc, px, py, pz, hf, fc.wpos_x, fc.wpos_y, 0, 0);                // :174, :177
                have = t > 0.0f;                                                                               // :184
                below_top = !(hf >= fc.hf_hi);
            }
            if constexpr (SAT && TALLY) {
                skipped += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(have && latched));
                have = have && !latched;
            }
            // Exact early end of the march: a ray starts on the inner shell and |p| only grows along it (>= 14 m per step at 128 steps even
            // for a grazing ray, 1.7 m at 1024 steps, against 0.5 m of fp32 noise; every ray of the C3 / C5 frames is walked by
            // tests/test_hostsim_core.py), so once EVERY live ray of the wavefront is above the height window
            // (density() == 0 there, cloud_core.h) all remaining samples are 0 too.  Checked every 4th step: one compare + ballot.
            // 21 % of the wave-steps of the headline view lie above the window (tools/stage_trace).
            if constexpr (RISING) {
                if ((i & 3) == 3 && __builtin_amdgcn_ballot_w64(below_top) == 0ull) end = i + 1;
            } else {                                         // rays that descend, or dip and rise: a lane above the window may come back into it
                if ((i & 3) == 3 && __builtin_amdgcn_ballot_w64(live) == 0ull) end = i + 1;
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(have);
            if (m != 0ull) {
                const int slot = count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                if constexpr (SLIM) {
                    if (have) { ev_px[slot] = px; ev_py[slot] = py; ev_pz[slot] = pz; ev_t[slot] = t; ev_owner[slot] = (unsigned char)lane; if (slot < CQ_HF_SLIM) ev_hf[slot] = hf; }
                    if (lane == 0) { st_lo[cs] = (unsigned)m; st_hi[cs] = (unsigned)(m >> 32); }
                } else {
                if (have) { ev_px[slot] = px; ev_py[slot] = py; ev_pz[slot] = pz; ev_t[slot] = t; ev_hf[slot] = hf; ev_owner[slot] = (unsigned char)lane; }
                if (lane == 0) { st_lo[cs] = (unsigned)m; st_hi[cs] = (unsigned)(m >> 32); st_base[cs] = (unsigned)count; }
                }
                count += __popcll(m);
                cs++;
            }
            i++;
        }
        const bool last = i >= end;
        if (count == 0) { if (last) break; continue; }
        if (count < 64 && !last) continue;
        // ---- B: the light march of the first n = min(count, 64) queued samples, one per lane, and the state-independent half of their
        //         shading (clouds.glsl:178, :202-209) while all lanes are busy: the replay below runs with ~1/6 of them (round 3: the census
        //         put 15 % of the kernel's issue time in the replay loop, 43 VALU instructions per step incl. 4 transcendentals)
        wave_lds_fence();
        const int n = count < 64 ? count : 64;
        unsigned long long carry = 0ull;                     // lanes of the last step whose sample is still queued
        if constexpr (TALLY) { if (lane == 0) tally[0] += (unsigned)n; }
        if (lane < n) {
            float Dr, Dg, Db, rq, dt;
            light_march_terms<CT>(T, fc, ls, nd, ev_px[lane], ev_py[lane], ev_pz[lane],
                              [&](float& et, float& ehf, float& ess, float& eph) { et = ev_t[lane]; ehf = ev_hf[lane]; const int ow = ev_owner[lane]; ess = ray_ss[ow]; eph = ray_ph[ow]; }, Dr, Dg, Db, rq, dt);
            ev_px[lane] = Dr; ev_py[lane] = Dg; ev_pz[lane] = Db; ev_t[lane] = rq; ev_hf[lane] = dt;           // the sample's slot now holds its terms
        }
        wave_lds_fence();
        // ---- C: replay the steps in order; owners of evaluated samples (slot < n) composite (:207-210)
        float Tr = acc[lane], alpha = acc[64 + lane], Lr = acc[128 + lane], Lg = acc[192 + lane], Lb = acc[256 + lane];
        ReplayBase<SLIM> sb;
        for (int s = 0; s < cs; s++) {
            // the step's lane mask is wave-uniform: as a scalar pair it IS the execution mask of the owners (inverse ballot: no per-lane bit test)
            const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)st_lo[s]), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)st_hi[s]);
            const bool mine = __builtin_amdgcn_inverse_ballot_w64(((unsigned long long)hi << 32) | lo);
            const int slot = sb.first(st_base, s) + (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
            sb.next(lo, hi);
            if (mine && slot < n) {
                composite_sample(ev_hf[slot], ev_t[slot], ev_px[slot], ev_py[slot], ev_pz[slot], Tr, alpha, Lr, Lg, Lb);
            }
            if (s == cs - 1) carry = __builtin_amdgcn_ballot_w64(mine && slot >= n);
        }
        if constexpr (DEAD) {
            const bool cand = live && alpha >= SAT_ALPHA_MIN;
            if (fc.sat_skip != 0 && __builtin_amdgcn_ballot_w64(cand) != 0ull) {
                float B[3];
                ray_saturation_bound(fc, ray_ph[lane], B);
                const float L[3] = {Lr, Lg, Lb};
                if (cand && ray_saturated(fc, Tr, alpha, L, B)) live = false;
            }
        } else if constexpr (SAT) {
            const bool cand = !latched && alpha >= SAT_ALPHA_MIN;
            if (fc.sat_skip != 0 && __builtin_amdgcn_ballot_w64(cand) != 0ull) {
                float B[3];
                ray_saturation_bound(fc, ray_ph[lane], B);
                const float L[3] = {Lr, Lg, Lb};
                latched = latched || (cand && ray_saturated(fc, Tr, alpha, L, B));
            }
        }
        acc[lane] = Tr; acc[64 + lane] = alpha; acc[128 + lane] = Lr; acc[192 + lane] = Lg; acc[256 + lane] = Lb;
        wave_lds_fence();
        // ---- keep what was not evaluated: samples n..count-1 move to the front, the last step keeps its unevaluated lanes
        const int rem = count - n;
        if (rem > 0) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, a4 = 0.0f; unsigned char a5 = 0;
            if constexpr (SLIM) {                            // rem > 0: n == 64 == CQ_HF_SLIM, every carried sample lies where no height fraction was stored
                if (lane < rem) { a0 = ev_px[n + lane]; a1 = ev_py[n + lane]; a2 = ev_pz[n + lane]; a3 = ev_t[n + lane]; a5 = ev_owner[n + lane]; a4 = height_fraction(length3_shell(a0, a1, a2)); }
            } else {
            if (lane < rem) { a0 = ev_px[n + lane]; a1 = ev_py[n + lane]; a2 = ev_pz[n + lane]; a3 = ev_t[n + lane]; a4 = ev_hf[n + lane]; a5 = ev_owner[n + lane]; }
            }
            wave_lds_fence();
            if (lane < rem) { ev_px[lane] = a0; ev_py[lane] = a1; ev_pz[lane] = a2; ev_t[lane] = a3; ev_hf[lane] = a4; ev_owner[lane] = a5; }
            if constexpr (SLIM) { if (lane == 0) { st_lo[0] = (unsigned)carry; st_hi[0] = (unsigned)(carry >> 32); } }
            else { if (lane == 0) { st_lo[0] = (unsigned)carry; st_hi[0] = (unsigned)(carry >> 32); st_base[0] = 0u; } }
            wave_lds_fence();
            count = rem; cs = 1;
        } else {
            count = 0; cs = 0;
        }
        if (fc.early_eps > 0.0f) {                                     // build-side early-out (off by default, bounded error)
            if (Tr < fc.early_eps) live = false;
            if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        }
        if (last && count == 0) break;                               // carried samples get one more (partial) flush
    }
    wave_lds_fence();
    o.r = acc[128 + lane]; o.g = acc[192 + lane]; o.b = acc[256 + lane]; o.a = sat(acc[64 + lane]); o.t = acc[lane];   // :213-214
    if constexpr (TALLY) o.incloud = lane == 0 ? tally[0] + skipped : 0u;
    return o;
}

// (two primary steps and two light samples in flight per wavefront, kernel variant "compact-ilp": docs/EXPERIMENTS.md §5, removed experiments)

// ---- the pixel of a lane -----------------------------------------------------------------------------------------------------
// Workgroup footprint `logical` = slab * tiles_x + bx is bw x 8 pixels; the wavefront's 8x8 tile is its tile-th (lane = ly*8 + lx).  The front ends of
// the two alternatives below; render_block keeps its own copy of this arithmetic (through this function the product kernel's code is not the parent's).
struct Pixel { int gx, gy, lr; bool valid; };   // column and row in the frame (gl_GlobalInvocationID), row among the rows this launch renders, inside the launch
__device__ __forceinline__ Pixel footprint_pixel(const RenderGeom& G, const uint32_t logical, const int tiles_x, const int bw, const int tile, const int lane) {
    const int local_rows = G.n_bands * G.band_rows;
    const int slab = (int)logical / tiles_x, bx = (int)logical - slab * tiles_x;
    Pixel p;
    p.gx = bx * bw + tile * 8 + (lane & 7);
    p.lr = slab * 8 + (lane >> 3);
    p.valid = p.gx < G.tile_w && p.lr < local_rows;
    const int band = p.lr / G.band_rows, rib = p.lr - band * G.band_rows;
    p.gy = (G.first_band + band * G.band_stride) * G.band_rows + rib;
    return p;
}
__device__ __forceinline__ void store_pixel(uint2* __restrict__ out, const RenderGeom& G, int gx, int gy, int lr, float r, float g, float b, float a) {
    out[(size_t)(G.out_full ? gy : lr) * G.pitch_px + gx] = pack_half4(f2h(r), f2h(g), f2h(b), f2h(a));   // imageStore, clouds.glsl:264
}

// ---- interleaved ray segments (small launches) ------------------------------------------------------------------
// One workgroup = ONE 8x8 tile; wavefront w marches the primary samples i = 4m + w of every ray of the tile.  In-cloud
// samples cluster in a few step ranges of a ray, so splitting a ray by step RANGE leaves one wavefront with most of the
// light march; dealing the steps out round-robin gives all four SIMDs of the CU a quarter of the tile's light march
// (the heaviest tile of the headline frame has 4.2x the mean in-cloud samples and is the critical path of a launch that
// holds only a few wavefronts per SIMD: one GPU's share of a frame split 8 ways).
// Front-to-back compositing needs T_i = prod_{k<i} dt_k across ALL wavefronts' samples: per chunk of 32 steps every
// wavefront publishes the step transmittances dt of its samples (1 for samples outside cloud), 16 lanes per wavefront
// scan them into exclusive prefix products, and each wavefront then shades its own samples with L_w += T_i * (...).
// The partial L_w are summed in wavefront order and alpha = 1 - T_end (clouds.glsl:207 is the same product).  Sample
// positions and densities are bit-identical to the sequential march; only the compositing sums are re-associated.
constexpr int IL_CHUNK = 32, IL_OWN = IL_CHUNK / 4, IL_BATCH = 96;
constexpr int IL_WAVE_FLOATS = 5 * IL_OWN * 64 + (IL_OWN * 64) / 2 + 7 * IL_BATCH;     // dense px,py,pz,t,hf | idx (u16) | lt
constexpr int IL_BLOCK_FLOATS = 4 * IL_WAVE_FLOATS + 2 * IL_CHUNK * 64 + 4 * 4 * 64;     // + D, P planes + combine

__device__ __forceinline__ void march_interleaved(const TexSet& T, const FrameConsts& fc, const Ray& ray, float* __restrict__ smem, int wave, int lane,
                                                  float& out_r, float& out_g, float& out_b, float& out_a, unsigned& incloud) {
    float* __restrict__ wq = smem + wave * IL_WAVE_FLOATS;
    float* __restrict__ d_px = wq;                              // [IL_OWN][64]; reused for cd after the light march
    float* __restrict__ d_py = wq + IL_OWN * 64;
    float* __restrict__ d_pz = wq + 2 * IL_OWN * 64;
    float* __restrict__ d_t = wq + 3 * IL_OWN * 64;
    float* __restrict__ d_hf = wq + 4 * IL_OWN * 64;
    unsigned short* __restrict__ ev_idx = reinterpret_cast<unsigned short*>(wq + 5 * IL_OWN * 64);   // [IL_OWN*64]
    float* __restrict__ lt = wq + 5 * IL_OWN * 64 + (IL_OWN * 64) / 2;                                  // [7][IL_BATCH]
    float* __restrict__ D = smem + 4 * IL_WAVE_FLOATS;          // [IL_CHUNK][64] step transmittance of every sample of the chunk
    float* __restrict__ P = D + IL_CHUNK * 64;                  // [IL_CHUNK][64] exclusive prefix products
    float* __restrict__ comb = P + IL_CHUNK * 64;               // [4][4][64]

    const int steps = fc.primary_steps, ls = fc.light_steps, nl = ls + 1;
    const float nd = -fc.density;
    const float phase = ray_phase(fc, ray);
    float Lr = 0.0f, Lg = 0.0f, Lb = 0.0f;
    float px = ray.px, py = ray.py, pz = ray.pz;
    int replay = wave + 1;                                      // additions of dir*ss needed to reach this wavefront's next sample
    float carry = 1.0f;                                         // scan lanes (lane < 16): T of ray 16*wave + lane after the chunks so far
    incloud = 0;
    const int nchunks = (steps + IL_CHUNK - 1) / IL_CHUNK;
    for (int c = 0; c < nchunks; c++) {
        // ---- A: this wavefront's 8 samples of the chunk
        int count = 0;
        for (int q = 0; q < IL_OWN; q++) {
            const int i = c * IL_CHUNK + 4 * q + wave;
            float t = 0.0f, hf = 0.0f;
            if (ray.above && i < steps) {
                for (int a = 0; a < replay; a++) advance(px, py, pz, ray.sx, ray.sy, ray.sz);     // clouds.glsl:173, one add per step
                hf = height_fraction(length3_shell(px, py, pz));
                t = sample_density(T, fc, px, py, pz, hf, fc.wpos_x, fc.wpos_y, 0, 0);
            }
            replay = 4;
            const bool have = t > 0.0f;
            d_t[q * 64 + lane] = t;
            D[(4 * q + wave) * 64 + lane] = have ? fast_exp(nd * t * ray.ss) : 1.0f;               // clouds.glsl:178
            const unsigned long long m = __ballot(have);
            if (m != 0ull) {
                const int slot = count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                if (have) { ev_idx[slot] = (unsigned short)(q * 64 + lane); d_px[q * 64 + lane] = px; d_py[q * 64 + lane] = py; d_pz[q * 64 + lane] = pz; d_hf[q * 64 + lane] = hf; }
                count += __popcll(m);
            }
        }
        wave_lds_fence();
        // ---- B: light march of the chunk's events, IL_BATCH events at a time, 64 evaluations per round
        for (int b0 = 0; b0 < count; b0 += IL_BATCH) {
            const int nb = (count - b0) < IL_BATCH ? (count - b0) : IL_BATCH;
            light_march_batch(T, fc, ls, nb, lane, [&](int k, float& x, float& y, float& z) { const int id = ev_idx[b0 + k]; x = d_px[id]; y = d_py[id]; z = d_pz[id]; }, lt, IL_BATCH);
            wave_lds_fence();
            for (int k = lane; k < nb; k += 64) {               // cd of each event, summed in the reference's order (:191, :199)
                float cd = 0.0f;
                for (int j = 0; j < nl; j++) cd += lt[j * IL_BATCH + k];
                d_px[ev_idx[b0 + k]] = cd;                      // the position is consumed: its x slot now holds cd
            }
            wave_lds_fence();
        }
        __syncthreads();
        // ---- scan: exclusive prefix products of the chunk's step transmittances, 16 rays per wavefront
        if (lane < 16) {
            const int r = wave * 16 + lane;
            float Tp = carry;
            for (int s = 0; s < IL_CHUNK; s++) { P[s * 64 + r] = Tp; Tp *= D[s * 64 + r]; }
            carry = Tp;
        }
        __syncthreads();
        // ---- C: shade this wavefront's in-cloud samples (clouds.glsl:202-209) with T_i from the scan
        for (int q = 0; q < IL_OWN; q++) {
            const float t = d_t[q * 64 + lane];
            if (t > 0.0f) {
                const float hf = d_hf[q * 64 + lane], cd = d_px[q * 64 + lane];
                const float dt = D[(4 * q + wave) * 64 + lane];
                float Tr = P[(4 * q + wave) * 64 + lane], alpha_unused = 0.0f;
                shade_sample(fc, phase, t, hf, dt, cd, Tr, alpha_unused, Lr, Lg, Lb);
                incloud++;
            }
        }
        __syncthreads();                                        // D/P/dense buffers are rewritten by the next chunk
    }
    // ---- combine: L = sum of the wavefronts' partial sums (wavefront order), alpha = 1 - T_end
    comb[(wave * 4 + 0) * 64 + lane] = Lr; comb[(wave * 4 + 1) * 64 + lane] = Lg; comb[(wave * 4 + 2) * 64 + lane] = Lb;
    if (lane < 16) comb[(0 * 4 + 3) * 64 + wave * 16 + lane] = carry;
    __syncthreads();
    out_r = comb[(0 * 4 + 0) * 64 + lane]; out_g = comb[(0 * 4 + 1) * 64 + lane]; out_b = comb[(0 * 4 + 2) * 64 + lane];
#pragma unroll
    for (int w = 1; w < 4; w++) { out_r += comb[(w * 4 + 0) * 64 + lane]; out_g += comb[(w * 4 + 1) * 64 + lane]; out_b += comb[(w * 4 + 2) * 64 + lane]; }
    out_a = sat(1.0f - comb[(0 * 4 + 3) * 64 + lane]);
}

template <int DUMMY>
__global__ __launch_bounds__(256) void clouds_kernel_interleaved(TexSet T, const FrameConsts* __restrict__ fcp, RenderGeom G, const uint32_t* __restrict__ order,
                                                                 uint2* __restrict__ out, unsigned long long* __restrict__ stats, uint32_t* __restrict__ wg_cost) {
    extern __shared__ __attribute__((aligned(16))) float il_smem[];
    const uint32_t logical = order[blockIdx.x];
    if (logical == 0xffffffffu) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Pixel pix = footprint_pixel(G, logical, (G.tile_w + 7) >> 3, 8, 0, lane);
    const bool valid = pix.valid;
    const FrameConsts& fc = *fcp;
    T.detail_lds = nullptr;
    Ray ray = ray_setup(fc, valid ? pix.gx : 0, valid ? pix.gy : 0);
    if (!valid) ray.above = false;
    float r, g, b, a; unsigned ic;
    march_interleaved(T, fc, ray, il_smem, wave, lane, r, g, b, a, ic);
    if (valid && wave == 0) {
        store_pixel(out, G, pix.gx, pix.gy, pix.lr, r, g, b, a);
    }
    if (stats) {
        unsigned ab = (ray.above && wave == 0) ? 1u : 0u;
        for (int off = 32; off > 0; off >>= 1) { ic += __shfl_down(ic, off); ab += __shfl_down(ab, off); }
        if (lane == 0) { atomicAdd(&stats[0], (unsigned long long)ic); atomicAdd(&stats[1], (unsigned long long)ab); }
    }
}

// ---- "lds" variant: the detail noise volume staged in LDS (north star) ---------------------------------------------
// A 1024-thread workgroup (16 wavefronts = a 128 x 8 pixel strip) copies the whole 32^3 detail mip chain (37 449 fp16
// numerators, 73 KB) into LDS once and every wavefront runs the queue march with its detail taps served from LDS.  LDS:
// 73 KB + 16 x 5.1 KB of event queues = 155 KB, i.e. ONE workgroup per CU (4 wavefronts per SIMD).  Kept as a measured
// alternative; the default keeps the detail volume oct-packed in L2 (one 16-byte gather per tap).
template <int DUMMY>
__global__ __launch_bounds__(1024) void clouds_kernel_lds(TexSet T, const FrameConsts* __restrict__ fcp, RenderGeom G, const uint32_t* __restrict__ order,
                                                          uint2* __restrict__ out, unsigned long long* __restrict__ stats, uint32_t* __restrict__ wg_cost) {
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    uint16_t* detail_s = reinterpret_cast<uint16_t*>(lds_all);
    constexpr int DETAIL_FLOATS = (DETAIL_CHAIN_TEXELS + 7) / 8 * 4;            // rounded up to 16 bytes
    float* queues = lds_all + DETAIL_FLOATS;
    {   // stage the detail chain: 16-byte copies, all 1024 threads
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(T.detail_h);
        uint4* dst = reinterpret_cast<uint4*>(lds_all);
        for (int i = threadIdx.x; i < DETAIL_FLOATS / 4; i += 1024) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t logical = order[blockIdx.x];
    if (logical == 0xffffffffu) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Pixel pix = footprint_pixel(G, logical, (G.tile_w + 127) >> 7, 128, wave, lane);
    const bool valid = pix.valid;
    const FrameConsts& fc = *fcp;
    Ray ray = ray_setup(fc, valid ? pix.gx : 0, valid ? pix.gy : 0);
    if (!valid) ray.above = false;
    TexSet Tl = T;
    Tl.detail_lds = detail_s;
    const MarchOut o = march_queue(Tl, fc, ray, queues + wave * Q_FLOATS, 0, fc.primary_steps);
    if (valid) {
        store_pixel(out, G, pix.gx, pix.gy, pix.lr, o.r, o.g, o.b, o.a);
    }
    if (stats || wg_cost) {
        unsigned ic = o.incloud, ab = ray.above ? 1u : 0u;
        for (int off = 32; off > 0; off >>= 1) { ic += __shfl_down(ic, off); ab += __shfl_down(ab, off); }
        if (lane == 0) {
            if (stats) { atomicAdd(&stats[0], (unsigned long long)ic); atomicAdd(&stats[1], (unsigned long long)ab); }
            if (wg_cost) atomicAdd(&wg_cost[logical], ic + 16u * ab);   // cost model of the feedback schedule: light marches + live primary marches
        }
    }
}

// Pixel <-> lane mapping: a wavefront owns one 8x8-pixel tile (lane = ly*8 + lx), the reference's workgroup footprint
// (clouds.glsl:5): its 64 rays are angularly adjacent, so their texture footprints overlap (L1/TA coalescing) and
// they enter/leave cloud together.  A 256-thread workgroup = 4 wavefronts covers 4/SEG tiles side by side:
//   SEG = 1: 4 tiles (32x8 px), every wavefront marches its rays end to end;
//   SEG = 2/4: the primary march of each ray is cut into SEG segments marched by SEG wavefronts in parallel and
//              combined front to back through LDS (L = L0 + T0*L1 + ..., T = prod T_s, 1-alpha = prod (1-alpha_s)):
//              a wavefront's latency (0.65 ms for 128 steps) is what limits small launches (one GPU's 1/8 frame), and
//              segments divide it by SEG.  Sample positions stay bit-identical; the compositing sums are re-associated.
// Workgroup order: physical workgroup b runs on XCD b % 8 (observed, speed only); `order` (clouds_launch.cpp::clouds_dev)
// maps b to a workgroup footprint.
#ifndef CSKY_COMPACT_WAVES
#define CSKY_COMPACT_WAVES 7   // waves/SIMD asked of the "compact" variant.  With the eager light-march fetches (three gathers of a sample in flight
                               // together) 7 waves x 72 VGPRs beat 8 waves x 64 VGPRs + spills: whole frame 1.83 -> 1.80 ms, 1/4 frame 0.49 -> 0.48
#endif
#ifndef CSKY_PERSISTENT_SLIM_WAVES
#define CSKY_PERSISTENT_SLIM_WAVES 8   // waves/SIMD asked of the specialised persistent forms (clouds_kernel_persistent<3, false, 1 | 2>) alone: 64 VGPRs without a
                                       // VGPR spill since round 22's straight-line light march, and the slim queue (CQ_FLOATS_SLIM) lets eight workgroups share a CU's LDS
#endif
// which persistent instantiations those are
constexpr bool persistent_slim(int variant, bool tally, int ct) { return variant == 3 && !tally && ct != 0; }
// One workgroup's footprint (4 tiles / SEG): `logical` = slab * tiles_x + bx, `rec` = its position in the launch order (the persistent form: its cost-feedback slot).
template <int VARIANT, int SEG, class TS = TexSet, bool TALLY = true, int CT = 0, bool SLIM = false>
__device__ __forceinline__ void render_block(TS T, const FrameConsts* __restrict__ fcp, const RenderGeom& G, const uint32_t logical, const uint32_t rec,
                                             uint2* __restrict__ out, unsigned long long* __restrict__ stats, uint32_t* __restrict__ wg_cost, const int tile_of_wave = -1) {
    constexpr int BW = 32 / SEG;                               // workgroup footprint width in pixels
    // (Round 6, measured and removed, profiles/r06/foot16_ab.txt: 16 x 16-pixel footprints (2 x 2 tiles) for whole-ray workgroups: frame identical, kernel alone
    // +4.4 %, two frames in flight unchanged)
    const int tiles_x = (G.tile_w + BW - 1) / BW;
    const int local_rows = G.n_bands * G.band_rows;
    const int slab = (int)logical / tiles_x, bx = (int)logical - slab * tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = tile_of_wave >= 0 ? tile_of_wave : wave / SEG, seg = tile_of_wave >= 0 ? 0 : wave - tile * SEG;   // tile_of_wave: SEG == 1 only
    // (lanes in Morton order or in 2x2 quads inside the tile instead of rows of 8: 1.701 / 1.700 vs 1.702 ms per frame, no difference)
    const int gx = bx * BW + tile * 8 + (lane & 7);
    const int lr = slab * 8 + (lane >> 3);
    const bool valid = gx < G.tile_w && lr < local_rows;
    const int band = lr / G.band_rows, rib = lr - band * G.band_rows;
    const int gy = (G.first_band + band * G.band_stride) * G.band_rows + rib;

    const FrameConsts& fc = *fcp;
    T.detail_lds = nullptr;                                    // compile-time constant here: the LDS tap path folds away
    Ray ray = ray_setup(fc, valid ? gx : 0, valid ? gy : 0);
    if (!valid) ray.above = false;
    MarchOut o;
    if constexpr (VARIANT == 0) {
        static_assert(SEG == 1, "the lock-step reference variant marches whole rays");
        o = march(T, fc, ray);
    } else {
        static_assert(!SLIM || (VARIANT == 3 && SEG == 1), "the slim queue is the compact whole-ray march's");
        __shared__ float lds[4][VARIANT == 3 ? (SLIM ? CQ_FLOATS_SLIM : CQ_FLOATS) : Q_FLOATS];
        const int s0 = (fc.primary_steps * seg) / SEG, s1 = (fc.primary_steps * (seg + 1)) / SEG;
        if constexpr (VARIANT == 3) o = march_compact<SEG == 1, TALLY, CT, TS, true, SLIM>(T, fc, ray, &lds[wave][0], s0, s1);
        else o = march_queue(T, fc, ray, &lds[wave][0], s0, s1);
        if constexpr (SEG > 1) {
            __shared__ float comb[4][5][64];
            comb[wave][0][lane] = o.r; comb[wave][1][lane] = o.g; comb[wave][2][lane] = o.b; comb[wave][3][lane] = o.t; comb[wave][4][lane] = o.a;
            __syncthreads();
            if (seg == 0) {
                float Tr = o.t, na = 1.0f - o.a;
#pragma unroll
                for (int s = 1; s < SEG; s++) {
                    const int w = tile * SEG + s;
                    o.r += Tr * comb[w][0][lane]; o.g += Tr * comb[w][1][lane]; o.b += Tr * comb[w][2][lane];
                    Tr *= comb[w][3][lane]; na *= 1.0f - comb[w][4][lane];
                }
                o.a = sat(1.0f - na); o.t = Tr;
            }
        }
    }
    if (valid && seg == 0) {
        store_pixel(out, G, gx, gy, lr, o.r, o.g, o.b, o.a);
    }
    if constexpr (TALLY) {
    if (stats || wg_cost) {
        unsigned ic = o.incloud, ab = (ray.above && seg == 0) ? 1u : 0u;
        for (int off = 32; off > 0; off >>= 1) { ic += __shfl_down(ic, off); ab += __shfl_down(ab, off); }
        if (lane == 0) {
            if (stats) { atomicAdd(&stats[0], (unsigned long long)ic); atomicAdd(&stats[1], (unsigned long long)ab); }
            if (wg_cost) atomicAdd(&wg_cost[logical], ic + 16u * ab);   // cost model of the feedback schedule: light marches + live primary marches
        }
    }
    }
}

// TALLY = false (the whole-ray compact kernel only): a launch nobody asked for counts; `stats` and `wg_cost` keep their place in the argument list and are not touched
template <int VARIANT, int SEG, class TS = TexSet, bool TALLY = true>
__global__ __launch_bounds__(256, VARIANT == 3 ? CSKY_COMPACT_WAVES : 7) void clouds_kernel(TS T, const FrameConsts* __restrict__ fcp, RenderGeom G, const uint32_t* __restrict__ order,
                                                     uint2* __restrict__ out, unsigned long long* __restrict__ stats, uint32_t* __restrict__ wg_cost) {
    const uint32_t logical = order[blockIdx.x];
    if (logical == 0xffffffffu) return;                        // workgroup-uniform
    render_block<VARIANT, SEG, TS, TALLY>(T, fcp, G, logical, blockIdx.x, out, stats, wg_cost);
}

// Persistent form of the whole-ray kernel: the launch is only as large as the chip holds (CUs x resident workgroups) and its
// wavefronts pull work from the launch order until it is empty.  The order is read as eight interleaved sequences (entry 8j + x
// belongs to XCD x, the same assignment the hardware's round-robin gives a plain launch, so the per-XCD L2 locality of mode 5 is
// kept); a footprint is popped from the workgroup's own XCD's sequence (one returning device-scope atomic) and, when that is
// empty, from the others in turn, so that XCDs that finish early take over work of the ones that run late.
//   * The four wavefronts of a workgroup never meet at a barrier: each draws a workgroup-local ticket t from LDS = tile t & 3 of
//     the workgroup's footprint number t >> 2.  The drawer of tile 0 pops that footprint and publishes it in one of two LDS slots;
//     the others wait for the publication (a global atomic's latency at most).  A slot is rewritten only after the three readers
//     of its previous footprint are through (slot_reads).  So a workgroup's wavefronts stay on neighbouring tiles (shared L1
//     lines) without waiting for each other.  Measured alternatives: one pop per workgroup behind a barrier 1.757 ms per C3
//     frame (tickets: 1.724; plain launches 1.806); popping single tiles globally per wavefront scatters a footprint over CUs
//     (2.12 -> 2.34 ms).  Everything that steers the loop is made wave-uniform with readfirstlane: with per-lane values the
//     structurizer wrapped the body in a lane loop that re-entered with ticket 0.
//   * heads[0..7] = the sequences' pop counters, heads[8] = wavefronts that have left; all nine are zero at launch and the last
//     wavefront out zeroes them again (a memset node in front of every launch cost 46 us on a busy chip).
// Used for launches of 12 Ki - 64 Ki wavefronts while two frames are in flight (launch_policy.h has the policy and the
// numbers; profiles/r02/persistent_launch_ab.txt).
//   * CT: the cloud-type mode the frame set-up wrote into *fcp (launch_clouds picks the instantiation from the same value), 0 for a mixed map or
//     csky_set_height_window(0): the march reads the mode from the frame constants as every other kernel does.
template <int VARIANT, bool TALLY = true, int CT = 0>
__global__ __launch_bounds__(256, persistent_slim(VARIANT, TALLY, CT) ? CSKY_PERSISTENT_SLIM_WAVES : VARIANT == 3 ? CSKY_COMPACT_WAVES : 7) void clouds_kernel_persistent(TexSet T, const FrameConsts* __restrict__ fcp, RenderGeom G,
        const uint32_t* __restrict__ order, const uint32_t n_items, uint32_t* __restrict__ heads, uint2* __restrict__ out, unsigned long long* __restrict__ stats,
        uint32_t* __restrict__ wg_cost) {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 7u;                                                 // eight sequences: MI355X has 8 XCDs; a part with fewer just leaves sequences to be stolen, one with more folds two XCDs onto one sequence (both still correct: every entry is popped exactly once)
    __shared__ uint32_t ticket, slot_ready[2], slot_reads[2], slot_entry[2], slot_rec[2];
    if (threadIdx.x == 0) { ticket = 0; slot_ready[0] = slot_ready[1] = 0; slot_reads[0] = slot_reads[1] = 0; }
    // Detail LODs 3 and 4 (72 cells, 1 152 bytes) in LDS for the light march's taps j = 3, 4: a workgroup lives for the whole launch, so one 16-byte
    // load by 72 threads in front of the barrier it has anyway is all the staging costs (round 2 staged per 4-tile workgroup of a plain launch, behind
    // a barrier of its own, and lost: docs/EXPERIMENTS.md §5).  Staged from the set THIS launch was given: a rebind needs no care.
    static_assert(VARIANT == 3, "the persistent form exists for the compact march only: its light march is the one that reads the table");
    __shared__ __attribute__((aligned(16))) uint4 det_small[TexSetSmallDetail::SMALL_DETAIL_CELLS];
    constexpr bool SLIM = persistent_slim(VARIANT, TALLY, CT);
    // eight workgroups per CU: four queues, the nine ticket words and the table within an eighth of the CU's 160 KB
    static_assert(!SLIM || 4 * CQ_FLOATS_SLIM * sizeof(float) + 9 * sizeof(uint32_t) + sizeof(det_small) <= 163840 / CSKY_PERSISTENT_SLIM_WAVES,
                  "the specialised persistent forms no longer fit eight workgroups into a CU's LDS");
    if (threadIdx.x < (unsigned)TexSetSmallDetail::SMALL_DETAIL_CELLS) det_small[threadIdx.x] = T.detail[detail_level_offset(TexSetSmallDetail::SMALL_DETAIL_FIRST) + threadIdx.x];
    __syncthreads();
    const bool lane0 = (threadIdx.x & 63) == 0;
    for (;;) {
        uint32_t tv = 0;
        if (lane0) tv = __hip_atomic_fetch_add(&ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)tv);
        const uint32_t f = t >> 2, sl = f & 1u;
        const int tile = (int)(t & 3u);
        uint32_t logical = 0xfffffffeu, rec = 0;               // 0xfffffffe: every sequence is empty
        if (tile == 0) {
            for (unsigned k = 0; k < 8u; k++) {
                const unsigned y = (xcc + k) & 7u;             // (own, then xcc ^ k = the XCD on the same IO die first: 0.3 % slower)
                uint32_t jv = 0;
                if (lane0) jv = atomicAdd(&heads[y], 1u);
                const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)jv);
                uint32_t i;
                if (persistent_pop_index(j, y, n_items, i)) { logical = order[i]; rec = i; break; }                // order_core.h
            }
            for (;;) {                                         // the slot's previous footprint (f - 2) had three readers
                const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&slot_reads[sl], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (r == 3u * (f >> 1)) break;
                __builtin_amdgcn_s_sleep(1);
            }
            if (lane0) {
                slot_entry[sl] = logical; slot_rec[sl] = rec;
                __hip_atomic_store(&slot_ready[sl], f + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        } else {
            for (;;) {
                const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&slot_ready[sl], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
                if (r == f + 1u) break;
                __builtin_amdgcn_s_sleep(1);
            }
            logical = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot_entry[sl]);
            rec = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot_rec[sl]);
            if (lane0) __hip_atomic_fetch_add(&slot_reads[sl], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (logical == 0xfffffffeu) {
            if (lane0 && atomicAdd(&heads[8], 1u) == gridDim.x * 4u - 1u) {
                for (unsigned k = 0; k < 9u; k++) atomicExch(&heads[k], 0u);
            }
            return;
        }
        if (logical != 0xffffffffu) {
            TexSetSmallDetail Ts;
            static_cast<TexSet&>(Ts) = T;
            Ts.det_small = (SmallDetailTable)det_small;                        // generic -> LDS: a C-style cast is the only one that may change the address space
            render_block<VARIANT, 1, TexSetSmallDetail, TALLY, CT, SLIM>(Ts, fcp, G, logical, rec, out, stats, wg_cost, tile);
        }
    }
}

// (helpers serving other wavefronts' light marches once the order is empty, and three ways of filling a launch's tail: docs/EXPERIMENTS.md §5, removed experiments)

// ---- cost-feedback schedule (clouds_launch.cpp, schedule mode 7) ------------------------------------------------------------
// Workgroups differ 10x in cost (in-cloud samples per tile) and a C3 frame is only ~4 waves of resident workgroups deep, so
// the order they start in decides the tail.  Every launch records a cost per workgroup (wg_cost: in-cloud samples + live rays);
// these three kernels turn it into the NEXT launch's order, heaviest first (longest-processing-time-first list scheduling;
// consecutive blocks land on consecutive XCDs, so each XCD also receives a descending sequence).  Counting sort on 1024 cost
// buckets; ties are placed in arrival order (the schedule may differ run to run, the frame cannot: every ray's arithmetic is
// independent of where and when its workgroup runs, tests/test_gpu_parity.py::test_variants_and_schedules_agree).
// (LPT_BUCKETS and lpt_bucket: order_core.h; bucket 0 = heaviest)
__global__ __launch_bounds__(256) void lpt_hist_kernel(const uint32_t* __restrict__ cost, int n, int shift, uint32_t* __restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&hist[lpt_bucket(cost[i], shift)], 1u);
}
__global__ __launch_bounds__(LPT_BUCKETS) void lpt_scan_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t sh[LPT_BUCKETS];                       // counts -> exclusive offsets; the histogram is left zeroed for the next launch
    const int t = threadIdx.x;
    const uint32_t own = hist[t];
    hist[t] = 0u;
    sh[t] = own;
    __syncthreads();
    for (int off = 1; off < LPT_BUCKETS; off <<= 1) {
        const uint32_t v = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    offsets[t] = sh[t] - own;
}
__global__ __launch_bounds__(256) void lpt_scatter_kernel(uint32_t* __restrict__ cost, int n, int shift, uint32_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        order[atomicAdd(&offsets[lpt_bucket(cost[i], shift)], 1u)] = (uint32_t)i;
        cost[i] = 0u;                                          // the next launch accumulates into a clean array: no memset nodes per frame
    }
}
// d_cost[n] and d_scratch[2 * LPT_BUCKETS] must be zero before their first use (clouds_launch.cpp clears them at allocation); both are left zeroed
hipError_t launch_lpt_order(uint32_t* d_cost, int n, int shift, uint32_t* d_scratch, uint32_t* d_order, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    lpt_hist_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_cost, n, shift, d_scratch);
    lpt_scan_kernel<<<1, LPT_BUCKETS, 0, s>>>(d_scratch, d_scratch + LPT_BUCKETS);
    lpt_scatter_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_cost, n, shift, d_scratch + LPT_BUCKETS, d_order);
    return hipGetLastError();
}

// ---- static workgroup orders, generated on the device (clouds_launch.cpp::ensure_order) --------------------------------
// Physical workgroup b runs on XCD b % 8 (observed placement, used for speed only).  A "slab" is one 32 x 8 pixel workgroup
// footprint (bw x 8 for segmented launches); `grid` entries, 0xffffffff = idle padding.
// The entry of workgroup b in modes 1, 2 and 5 is order_core.h::static_order_entry, which the host tests walk too.
// Written by a kernel on the launch's own stream: no host table, no pageable copy, no device-wide synchronisation when the
// geometry changes (a 64-tile walk re-uses the table anyway: these orders depend on the launch geometry only).
__global__ __launch_bounds__(256) void static_order_kernel(int mode, int tiles_x, int slabs, int grid, uint32_t* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= grid) return;
    out[b] = static_order_entry(mode, tiles_x, slabs, b);
}
hipError_t launch_static_order(int mode, int tiles_x, int slabs, int grid, uint32_t* d_order, hipStream_t s) {
    if (grid <= 0) return hipSuccess;
    static_order_kernel<<<(grid + 255) / 256, 256, 0, s>>>(mode, tiles_x, slabs, grid, d_order);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ band interleave (gathering rank, N > 1)
// The gather leaves rank-major compact bands ([member][local band][rows]); the frame wants band k = member k % n, local band k / n.  A plain
// strided copy, deliberately on FEW workgroups: it is HBM-bound (32 MiB per 2048x1024 frame) beside marches that are not, so 48 workgroups
// streaming 16-byte chunks take it off the critical path instead of sweeping the whole chip for 15 us per frame (torch's permute + copy).
__global__ __launch_bounds__(256) void interleave_bands_kernel(const uint4* __restrict__ src, size_t member_stride16, int members, uint32_t band16, uint32_t total_bands,
                                                              uint4* __restrict__ dst) {
    const size_t total = (size_t)band16 * total_bands;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const uint32_t k = (uint32_t)(i / band16), c = (uint32_t)(i - (size_t)k * band16);
        dst[i] = src[(size_t)(k % members) * member_stride16 + (size_t)(k / members) * band16 + c];
    }
}
hipError_t launch_interleave_bands(const void* d_gathered, size_t member_stride_bytes, int members, size_t band_bytes, int total_bands, void* d_frame, hipStream_t s) {
    const size_t chunks = band_bytes / 16 * (size_t)total_bands;
    if (!chunks) return hipSuccess;
    const unsigned grid = (unsigned)(chunks / 256 + 1 < 48 ? chunks / 256 + 1 : 48);
    interleave_bands_kernel<<<grid, 256, 0, s>>>(reinterpret_cast<const uint4*>(d_gathered), member_stride_bytes / 16, members, (uint32_t)(band_bytes / 16), (uint32_t)total_bands,
                                                 reinterpret_cast<uint4*>(d_frame));
    return hipGetLastError();
}

// test hook (csky_test_sqrt_shell): cloud_core.h::sqrt_shell over an array, for the exhaustive check against the host's sqrtf
__global__ __launch_bounds__(256) void sqrt_shell_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sqrt_shell(in[i]);
}
hipError_t launch_sqrt_shell(const float* d_in, float* d_out, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    sqrt_shell_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_in, d_out, n);
    return hipGetLastError();
}

static const char* const kVariantNames[] = {"lockstep", "queue", "queue-lds", "compact"};
int cloud_resident_workgroups_per_cu() { return CSKY_COMPACT_WAVES; }
int cloud_resident_workgroups_per_cu_slim() {
    // what the runtime says the current device holds of each of the two forms, the launch bound at the most: a workgroup that is not resident only waits
    // its turn (no workgroup of a persistent launch waits for another), but a grid that is too large wastes the launch's tail
    int per_cu = CSKY_PERSISTENT_SLIM_WAVES;
    const void* const forms[2] = {reinterpret_cast<const void*>(&clouds_kernel_persistent<3, false, 1>), reinterpret_cast<const void*>(&clouds_kernel_persistent<3, false, 2>)};
    for (const void* f : forms) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, 256, 0) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = CSKY_COMPACT_WAVES; }
        if (n < per_cu) per_cu = n;
    }
    return per_cu;
}
int cloud_variant_count() { return (int)(sizeof(kVariantNames) / sizeof(kVariantNames[0])); }
const char* cloud_variant_name(int v) { return (v >= 0 && v < cloud_variant_count()) ? kVariantNames[v] : nullptr; }

hipError_t launch_clouds(int variant, int seg, const TexSet& t, const FrameConsts* d_fc, const RenderGeom& g, const uint32_t* d_order, int grid,
                         uint2* d_out, unsigned long long* d_stats, uint32_t* d_wg_cost, hipStream_t s, uint32_t* d_heads, int resident, const TexSet32* t32, bool census_lean,
                         int ct_mode, int resident_slim) {
    if (grid <= 0) return hipSuccess;
    if (ct_mode < 0 || ct_mode > 2) return hipErrorInvalidValue;
    // the in-cloud count has a reader only when the launch was given somewhere to put it: without one the whole-ray compact kernel runs in the form whose
    // latched rays stop marching (march_compact, TALLY = false).  census_lean: that form WITH a stats buffer, which only the census build's counters write.
    const bool tally = (d_stats != nullptr || d_wg_cost != nullptr) && !census_lean;
    if (t32) {                                                 // exact fp32-coefficient cells: the compact whole-ray kernel on the other texture-set type
        if (variant != 3 || seg != 1) return hipErrorInvalidValue;
        clouds_kernel<3, 1, TexSet32><<<grid, 256, 0, s>>>(*t32, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
        return hipGetLastError();
    }
    if (d_heads && variant == 3 && seg == 1) {                 // persistent form, see clouds_kernel_persistent
        // the instantiation of the frame's cloud-type mode: ct_mode is what the set-up of d_fc was given (clouds_launch.cpp setup_args), so the compiled-in
        // branch is the one the generic form would take on fc.ct_mode
        const auto go = [&](auto tl, auto ct) {
            const int res = persistent_slim(3, decltype(tl)::value, decltype(ct)::value) && resident_slim > 0 ? resident_slim : resident;   // the instantiation's own resident count
            const unsigned n = (unsigned)(grid < res ? grid : res);
            clouds_kernel_persistent<3, decltype(tl)::value, decltype(ct)::value><<<n, 256, 0, s>>>(t, d_fc, g, d_order, (uint32_t)grid, d_heads, d_out, d_stats, d_wg_cost);
        };
        const auto with_mode = [&](auto tl) {
            if (ct_mode == 1) go(tl, std::integral_constant<int, 1>());
            else if (ct_mode == 2) go(tl, std::integral_constant<int, 2>());
            else go(tl, std::integral_constant<int, 0>());
        };
        if (tally) with_mode(std::true_type()); else with_mode(std::false_type());
        return hipGetLastError();
    }
    if (variant == 0 && seg == 1) clouds_kernel<0, 1><<<grid, 256, 0, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    else if (variant == 1 && seg == 1) clouds_kernel<1, 1><<<grid, 256, 0, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    else if (variant == 1 && seg == 2) clouds_kernel<1, 2><<<grid, 256, 0, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    else if (variant == 1 && seg == 4) clouds_kernel<1, 4><<<grid, 256, 0, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    else if (variant == 3 && seg == 1 && tally) clouds_kernel<3, 1, TexSet, true><<<grid, 256, 0, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    else if (variant == 3 && seg == 1) clouds_kernel<3, 1, TexSet, false><<<grid, 256, 0, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    else if (variant == 3 && seg == 2) clouds_kernel<3, 2><<<grid, 256, 0, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    else if (variant == 3 && seg == 4) clouds_kernel<3, 4><<<grid, 256, 0, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    else if ((variant == 1 || variant == 3) && seg == 5) {                      // 5 = 4 interleaved segments, one tile per workgroup, 76 KB of LDS
        // > 64 KB of dynamic LDS needs the opt-in attribute; it is per device, so set it on every launch (cheap, idempotent)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&clouds_kernel_interleaved<0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(IL_BLOCK_FLOATS * sizeof(float)));
        if (e != hipSuccess) return e;
        clouds_kernel_interleaved<0><<<grid, 256, IL_BLOCK_FLOATS * sizeof(float), s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    }
    else if (variant == 2) {                                  // detail noise staged in LDS, 16 wavefronts per workgroup
        constexpr size_t bytes = ((DETAIL_CHAIN_TEXELS + 7) / 8 * 4 + 16 * Q_FLOATS) * sizeof(float);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&clouds_kernel_lds<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        clouds_kernel_lds<0><<<grid, 1024, bytes, s>>>(t, d_fc, g, d_order, d_out, d_stats, d_wg_cost);
    }
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace csky

// ---- the direct march: caller-given rays ------------------------------------------------------------------------
// clouds.glsl sky(dir) for the directions of a W x H image the caller describes (a buffer of directions, or a camera view) instead of the
// hemi-octahedral grid's: render_block's whole-ray form with another front end.  One pixel per lane, an 8x8 tile per wavefront, four tiles side by
// side per workgroup (32 x 8 pixels), march_compact<true, false> (whole rays, no tally: nobody reads a count here) on the frame constants the cloud
// frame's own set-up kernel wrote.  A plain launch in natural order: workgroup b is footprint b, row-major.  Lanes outside the image and lanes whose
// direction fails rays_core.h rays_accept do not march (`above = false`): they take no sample and compute no texture address; the latter store zeros.
//
// Every kernel from here to the end of the file is this one with another front end, and is written as: the lane's pixel (csky_common.h tile_pixel),
// its direction (rays_core.h rays_lane_dir, or the update's view_update_dir), the kernel's own ray maker, march_store.
#include "rays_core.h"
#pragma clang fp contract(off)   // (rays_core.h ends with contraction on, like cloud_core.h)

namespace csky {

// The shared tail.  The lanes with `marches` run `ray` whole through march_compact on their wavefront's quarter of the workgroup's queues and store
// the texel at pixel (i, j) of `out` (store_pixel's packing); the others take no sample, compute no texture address and store nothing.  The queues
// are this function's: a kernel that ends here has no other LDS.  RISING: march_compact's.
template <bool RISING, class TS>
__device__ __forceinline__ void march_store(TS T, const FrameConsts& fc, Ray ray, bool marches, int wave, uint2* __restrict__ out, uint32_t pitch_px, int i, int j) {
    __shared__ float lds[4][CQ_FLOATS];
    T.detail_lds = nullptr;                                    // compile-time constant here: the LDS tap path folds away
    if (!marches) ray.above = false;
    const MarchOut o = march_compact<true, false, 0, TS, RISING>(T, fc, ray, &lds[wave][0], 0, fc.primary_steps);
    if (marches) out[(size_t)j * pitch_px + i] = pack_half4(f2h(o.r), f2h(o.g), f2h(o.b), f2h(o.a));
}

// SRC: rays_lane_dir's (0: directions from `dirs`; 1: the view of G)
template <int SRC, class TS>
__global__ __launch_bounds__(256, CSKY_COMPACT_WAVES) void clouds_rays_kernel(TS T, const FrameConsts* __restrict__ fcp, RaysGeom G, const float* __restrict__ dirs,
                                                                              uint2* __restrict__ out) {
    const TilePixel p = tile_pixel(G.w, G.h);
    float ex, ey, ez;
    rays_lane_dir<SRC>(G, dirs, p, ex, ey, ez);
    march_store<true>(T, *fcp, rays_ray(*fcp, ex, ey, ez), p.valid, p.wave, out, G.pitch_px, p.i, p.j);
}

hipError_t launch_clouds_rays(const TexSet& t, const TexSet32* t32, const FrameConsts* d_fc, const RaysGeom& g, const float* d_dirs, uint2* d_out, hipStream_t s) {
    if (!rays_geom_ok(g)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)tile_grid(g.w, g.h);
    with_texset(t, t32, [&](const auto& ts) {
        if (d_dirs) clouds_rays_kernel<0><<<grid, 256, 0, s>>>(ts, d_fc, g, d_dirs, d_out);
        else clouds_rays_kernel<1><<<grid, 256, 0, s>>>(ts, d_fc, g, d_dirs, d_out);
    });
    return hipGetLastError();
}

}  // namespace csky

// ---- the temporal split of a view frame ----------------------------------------------------------------------------
// One pixel of every B x B block of a view is marched per call (the fresh pixels), the others are taken from the previous view frame through the
// previous camera, and a pixel that frame does not cover (a hole) is marched.  Two launches that write disjoint pixels: the order between them does
// not matter.  Both are clouds_rays_kernel's shape: one pixel per lane, an 8x8 tile per wavefront, four tiles per workgroup, the same LDS queue and
// launch bound, march_compact<true, false> on the frame constants the cloud frame's set-up kernel wrote.
#include "view_update_core.h"
#pragma clang fp contract(off)   // (view_update_core.h ends with contraction on, like rays_core.h)

namespace csky {

// The fresh pixels, run over the SUB-GRID: lane (p.i, p.j) of G.sub_w x G.sub_h marches pixel (p.i * B + px, p.j * B + py) and stores there.  The
// fresh rays fill whole 8x8 tiles: a wavefront of 64 fresh rays, not 4 lanes of every wavefront of the image.
template <class TS>
__global__ __launch_bounds__(256, CSKY_COMPACT_WAVES) void clouds_view_fresh_kernel(TS T, const FrameConsts* __restrict__ fcp, ViewUpdateGeom G, uint2* __restrict__ out) {
    const TilePixel p = tile_pixel(G.sub_w, G.sub_h);
    const int i = p.valid ? p.i * G.block + G.px : 0, j = p.valid ? p.j * G.block + G.py : 0;   // < G.w, G.h by the sub-grid's size
    float ex, ey, ez;
    view_update_dir(G, i, j, ex, ey, ez);
    march_store<true>(T, *fcp, rays_ray(*fcp, ex, ey, ez), p.valid, p.wave, out, G.pitch_px, i, j);
}

// Every other pixel, one per lane over the full image.  A lane that is not fresh stores zeros (not accepted), its history texel, or is a hole.  A
// wavefront without a hole returns before it touches its LDS queue; otherwise its hole lanes march and store.  Fresh lanes store nothing.
// prev: the previous frame (NULL without history: every accepted lane that is not fresh is then a hole); it does not overlap out.
template <class TS>
__global__ __launch_bounds__(256, CSKY_COMPACT_WAVES) void clouds_view_reproject_kernel(TS T, const FrameConsts* __restrict__ fcp, ViewUpdateGeom G,
                                                                                        const uint2* __restrict__ prev, uint2* __restrict__ out) {
    const TilePixel p = tile_pixel(G.w, G.h);
    float ex, ey, ez;
    view_update_dir(G, p.valid ? p.i : 0, p.valid ? p.j : 0, ex, ey, ez);
    const ViewUpdateClass c = view_update_classify(G, p.i, p.j, ex, ey, ez);
    const int kind = p.valid ? c.kind : VU_FRESH;              // a lane outside the image stores nothing, like a fresh one
    uint2* __restrict__ dst = out + ((size_t)p.j * G.pitch_px + p.i);
    if (kind == VU_ZERO) { uint2 z; z.x = 0u; z.y = 0u; *dst = z; }
    else if (kind == VU_COPY) *dst = prev[(size_t)p.j * G.prev_pitch_px + p.i];
    else if (kind == VU_TAP) *dst = view_update_tap(prev, G.prev_pitch_px, G.w, G.h, c.ux, c.uy);
    const bool hole = kind == VU_HOLE;
    if (__builtin_amdgcn_ballot_w64(hole) == 0ull) return;
    // (0, 0, 0) fails rays_accept: no sample, no address
    march_store<true>(T, *fcp, rays_ray(*fcp, hole ? ex : 0.0f, hole ? ey : 0.0f, hole ? ez : 0.0f), hole, p.wave, out, G.pitch_px, p.i, p.j);
}

hipError_t launch_clouds_view_update(const TexSet& t, const TexSet32* t32, const FrameConsts* d_fc, const ViewUpdateGeom& g, const uint2* d_prev, uint2* d_out, hipStream_t s) {
    if (!rays_geom_ok(g)) return hipErrorInvalidValue;
    if (g.block < 1 || g.block > 8 || g.px < 0 || g.px >= g.block || g.py < 0 || g.py >= g.block) return hipErrorInvalidValue;
    if ((g.has_history != 0) != (d_prev != nullptr) || (d_prev && g.prev_pitch_px < (uint32_t)g.w)) return hipErrorInvalidValue;
    if (g.sub_w != (g.px < g.w ? (g.w - g.px + g.block - 1) / g.block : 0) || g.sub_h != (g.py < g.h ? (g.h - g.py + g.block - 1) / g.block : 0)) return hipErrorInvalidValue;
    with_texset(t, t32, [&](const auto& ts) {
        if (g.sub_w > 0 && g.sub_h > 0) clouds_view_fresh_kernel<<<tile_grid(g.sub_w, g.sub_h), 256, 0, s>>>(ts, d_fc, g, d_out);
        if (g.block > 1) clouds_view_reproject_kernel<<<tile_grid(g.w, g.h), 256, 0, s>>>(ts, d_fc, g, d_prev, d_out);   // B = 1: every pixel is fresh
    });
    return hipGetLastError();
}

}  // namespace csky

// ---- the direct march from an observer's position -------------------------------------------------------------------
// clouds_rays_kernel with another front end: observer_core.h observer_ray makes the lane's Ray from its direction AND the observer's position (under,
// inside or above the layer; the first segment through the layer, capped).  The same shape: one pixel per lane, an 8x8 tile per wavefront, four
// tiles per workgroup, the same LDS queue and launch bound, a plain launch in natural order.  march_compact<true, false, 0, TS, false>: these rays
// descend, or dip and rise, so the wavefront's early end is "no lane is live" and not "every lane is above the window".
#include "observer_core.h"
#pragma clang fp contract(off)   // (observer_core.h ends with contraction on, like rays_core.h)

namespace csky {

// SRC: rays_lane_dir's, on G.g
template <int SRC, class TS>
__global__ __launch_bounds__(256, CSKY_COMPACT_WAVES) void clouds_observer_kernel(TS T, const FrameConsts* __restrict__ fcp, ObserverGeom G, const float* __restrict__ dirs,
                                                                                  uint2* __restrict__ out) {
    const TilePixel p = tile_pixel(G.g.w, G.g.h);
    float ex, ey, ez;
    rays_lane_dir<SRC>(G.g, dirs, p, ex, ey, ez);
    march_store<false>(T, *fcp, observer_ray(*fcp, G, ex, ey, ez), p.valid, p.wave, out, G.g.pitch_px, p.i, p.j);
}

hipError_t launch_clouds_observer(const TexSet& t, const TexSet32* t32, const FrameConsts* d_fc, const ObserverGeom& g, const float* d_dirs, uint2* d_out, hipStream_t s) {
    if (!rays_geom_ok(g.g)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)tile_grid(g.g.w, g.g.h);
    with_texset(t, t32, [&](const auto& ts) {
        if (d_dirs) clouds_observer_kernel<0><<<grid, 256, 0, s>>>(ts, d_fc, g, d_dirs, d_out);
        else clouds_observer_kernel<1><<<grid, 256, 0, s>>>(ts, d_fc, g, d_dirs, d_out);
    });
    return hipGetLastError();
}

}  // namespace csky

// ---- the observer's march behind a per-pixel scene depth -------------------------------------------------------------
// clouds_observer_kernel with one more input: scene_depth_core.h scene_depth_ray ends the lane's segment at its own pixel's depth texel (metres along
// the ray, or along the camera's forward axis) as well as at the frame's max_distance.  The same shape: one pixel per lane, an 8x8 tile per wavefront,
// four tiles per workgroup, the same LDS queue and launch bound, a plain launch in natural order, march_compact<true, false, 0, TS, false>.  A lane
// inside the image makes one 4-byte load of its texel (a row of a tile is eight consecutive floats); a lane outside it loads nothing.  A wavefront
// whose lanes are all occluded returns at march_compact's first ballot.
#include "scene_depth_core.h"
#pragma clang fp contract(off)   // (scene_depth_core.h ends with contraction on, like observer_core.h)

namespace csky {

// SRC as clouds_observer_kernel's (0: directions from `dirs`, [H][W][3] floats; 1: the view of G.og.g).  KIND: DEPTH_DISTANCE or DEPTH_VIEW_Z (view form only), compiled in: the distance form has no dot product or divide.
// depth: G.og.g.h rows of G.og.g.w floats, G.depth_pitch floats apart; it does not overlap out.
template <int SRC, int KIND, class TS>
__global__ __launch_bounds__(256, CSKY_COMPACT_WAVES) void clouds_observer_depth_kernel(TS T, const FrameConsts* __restrict__ fcp, SceneDepthGeom G, const float* __restrict__ dirs,
                                                                                        const float* __restrict__ depth, uint2* __restrict__ out) {
    const TilePixel p = tile_pixel(G.og.g.w, G.og.g.h);
    float z = 0.0f;                                            // 0 is no valid texel
    if (p.valid) z = depth[(size_t)p.j * G.depth_pitch + p.i];
    // rays_lane_dir<SRC>(G.og.g, dirs, p, ...), kept as its own copy: through that function the view forms of this kernel are the parent's
    // instructions in another order, and that order missed the timing rule on two of tools/scene_depth_profile.py's eight lines
    float ex = 0.0f, ey = 0.0f, ez = 0.0f;                     // (0, 0, 0) fails observer_accept
    if constexpr (SRC == 0) {
        if (p.valid) { const float* __restrict__ d = dirs + ((size_t)p.j * (size_t)G.og.g.w + (size_t)p.i) * 3; ex = d[0]; ey = d[1]; ez = d[2]; }
    } else {
        rays_view_dir(G.og.g, p.valid ? p.i : 0, p.valid ? p.j : 0, ex, ey, ez);
    }
    march_store<false>(T, *fcp, scene_depth_ray_k<KIND>(*fcp, G.og, ex, ey, ez, z), p.valid, p.wave, out, G.og.g.pitch_px, p.i, p.j);
}

hipError_t launch_clouds_observer_depth(const TexSet& t, const TexSet32* t32, const FrameConsts* d_fc, const SceneDepthGeom& g, const float* d_dirs, const float* d_depth,
                                        uint2* d_out, hipStream_t s) {
    if (!rays_geom_ok(g.og.g)) return hipErrorInvalidValue;
    if (!d_depth || g.depth_pitch < (uint32_t)g.og.g.w) return hipErrorInvalidValue;
    if ((g.kind != DEPTH_DISTANCE && g.kind != DEPTH_VIEW_Z) || (g.kind == DEPTH_VIEW_Z && d_dirs)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)tile_grid(g.og.g.w, g.og.g.h);
    with_texset(t, t32, [&](const auto& ts) {
        if (d_dirs) clouds_observer_depth_kernel<0, DEPTH_DISTANCE><<<grid, 256, 0, s>>>(ts, d_fc, g, d_dirs, d_depth, d_out);
        else if (g.kind == DEPTH_VIEW_Z) clouds_observer_depth_kernel<1, DEPTH_VIEW_Z><<<grid, 256, 0, s>>>(ts, d_fc, g, d_dirs, d_depth, d_out);
        else clouds_observer_depth_kernel<1, DEPTH_DISTANCE><<<grid, 256, 0, s>>>(ts, d_fc, g, d_dirs, d_depth, d_out);
    });
    return hipGetLastError();
}

}  // namespace csky
