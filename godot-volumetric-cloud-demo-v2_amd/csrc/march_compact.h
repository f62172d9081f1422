// march_compact.h -- the compact wave-cooperative march (kernel variant 3, "compact"): what every product frame (cloud_kernels.hip) and every
// direct-march frame runs.  Device only: a .hip file includes it and restates contraction after its last include.
//
//   wave_lds_fence, ray_phase                    : the wavefront's LDS fence; the phase value of a ray's samples
//   CQ_* / ReplayBase                            : the per-wavefront queue's two layouts (wide, and SLIM for the specialised persistent forms)
//   CSKY_EAGER_* / CSKY_LIGHT_STRAIGHT           : the measured build switches of the two marches' texture fetches
//   light_samples_from, light_march_terms        : step B, the light march of one queued sample
//   march_compact<WHOLE, TALLY, CT, TS, RISING, SLIM> : the march
//   CSKY_COMPACT_WAVES                           : waves per SIMD asked of the kernels that run it
//
// The marches it replaced as the product's, kept for A/B, are in march_variants.h; the lock-step one is cloud_core.h march().
#pragma once
#include "cloud_core.h"
// FP contraction OFF for the code of this file, like section A of cloud_core.h: what the march adds and multiplies itself (the phase value's dot product)
// rounds as written.  Stated here because otherwise the last header decides it, and cloud_core.h ends with contraction on.
#pragma clang fp contract(off)

namespace csky {

// No __syncthreads in a wave-cooperative march: wavefronts are independent; LDS operations of one wavefront complete in issue order and
// wavefront-scope fences keep the compiler from reordering them.
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

// ---- compacted light march (variant "compact") ------------------------------------------------------------------
// Same decoupling as march_queue (march_variants.h), but a flush always takes EXACTLY 64 queued samples, one per lane (k = lane): every lane
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

#ifndef CSKY_COMPACT_WAVES
#define CSKY_COMPACT_WAVES 7   // waves/SIMD asked of the "compact" variant.  With the eager light-march fetches (three gathers of a sample in flight
                               // together) 7 waves x 72 VGPRs beat 8 waves x 64 VGPRs + spills: whole frame 1.83 -> 1.80 ms, 1/4 frame 0.49 -> 0.48
#endif

}  // namespace csky
