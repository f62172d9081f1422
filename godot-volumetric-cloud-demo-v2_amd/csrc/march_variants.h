// march_variants.h -- the wave-cooperative marches the compact one (march_compact.h) replaced as the product's, kept selectable for A/B.  Device only;
// cloud_kernels.hip alone includes it, and the kernels that call these marches stay there.
//
//   light_march_batch, march_queue : variants 1 and 2 ("queue", "queue-lds"): render_block<1, SEG>, clouds_kernel_lds
//   march_interleaved              : segments 5 (four interleaved ray segments, one tile per workgroup): clouds_kernel_interleaved
#pragma once
#include "march_compact.h"
#pragma clang fp contract(off)   // the compositing sums of these marches round as written

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
// The fences between the steps are march_compact.h wave_lds_fence.  Per-ray arithmetic and its order are unchanged.
constexpr int QCAP = 96;                                    // events per wavefront queue (a flush is forced above QCAP-64)
constexpr int QSTEPS = 48;                                  // steps-with-events per chunk (a flush is forced when full)
constexpr int Q_FLOATS = 5 * QCAP + 7 * QCAP + 3 * QSTEPS;  // pos(3) t hf | lt[7] | per-step mask lo/hi + base  = 5.1 KB per wavefront

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

}  // namespace csky
