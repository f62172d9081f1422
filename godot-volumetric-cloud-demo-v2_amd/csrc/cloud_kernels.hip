// cloud_kernels.hip -- gfx950 (CDNA4, wave64) kernels of clouds.glsl main(): one ray per lane, one 8x8-pixel tile per wavefront.
//
//   Pixel, footprint_pixel, store_pixel             : the pixel of a lane (the front ends of the two alternatives; render_block keeps its own copy)
//   clouds_kernel_interleaved / clouds_kernel_lds   : measured alternatives (segments 5, variant 2)
//   render_block, clouds_kernel<VARIANT, SEG, TS>   : a workgroup footprint of 4 / SEG tiles; <3, 1, TexSet> is the product's kernel
//   clouds_kernel_persistent                        : the same as a launch the size of the chip that pops footprints from the order
//   cloud_variant_*, cloud_resident_workgroups_per_cu*, launch_clouds : the variants' names, the size of a persistent launch, the launcher
//   march_store and the direct march                : whole rays of a W x H image in natural order, one pixel per lane; each kernel is a lane pixel,
//                                                     a direction, its own ray maker and the shared tail march_store.  In this file
//                                                     because in a file of its own its fp16-pair kernels are not the same code:
//     clouds_rays_kernel<SRC, TS>                   :   caller-given directions or a camera view, from the reference's observer (§17)
//     clouds_view_fresh_kernel / _reproject_kernel  :   the temporal split of a view frame: the fresh sub-grid; history taps and holes (§20)
//     clouds_observer_kernel<SRC, TS>               :   the same rays from an observer's position (§21)
//     clouds_observer_depth_kernel<SRC, KIND, TS>   :   those behind a per-pixel scene depth (§22)
//
// What these kernels call and what runs beside them:
//   march_compact.h     : the compact march (variant 3), which every product frame and every direct-march frame runs
//   march_variants.h    : march_queue and march_interleaved (variants 1 and 2, segments 5); the lock-step one is cloud_core.h march() (variant 0)
//   order_kernels.hip   : the launch orders these kernels read and the band interleave of the frames they write
//   primitives.hip      : the test hooks of the march's arithmetic (sqrt_shell among them)
//
// No MFMA anywhere: the path is fetch/latency-bound gather + fp32 VALU, not a contraction.
// What was built here, measured and removed again is recorded in docs/EXPERIMENTS.md §5.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "cloud_core.h"
#include "order_core.h"
#include "march_compact.h"
#include "march_variants.h"
#include "rays_core.h"
#include "view_update_core.h"
#include "observer_core.h"
#include "scene_depth_core.h"
#include <type_traits>
// FP contraction OFF for the code of this file, like section A of cloud_core.h: what a kernel adds and multiplies itself (the segments' compositing
// sums) rounds as written.  Stated here, once, because otherwise the last header decides it, and every core header ends with contraction on.
#pragma clang fp contract(off)

namespace csky {

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

// ---- interleaved ray segments (small launches): march_variants.h march_interleaved, one 8x8 tile per workgroup ---------------------
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
// (CSKY_COMPACT_WAVES, the waves/SIMD asked of the "compact" variant: march_compact.h)
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

// ---- the direct march: caller-given rays ------------------------------------------------------------------------
// clouds.glsl sky(dir) for the directions of a W x H image the caller describes (a buffer of directions, or a camera view) instead of the
// hemi-octahedral grid's: render_block's whole-ray form with another front end.  One pixel per lane, an 8x8 tile per wavefront, four tiles side by
// side per workgroup (32 x 8 pixels), march_compact<true, false> (whole rays, no tally: nobody reads a count here) on the frame constants the cloud
// frame's own set-up kernel wrote.  A plain launch in natural order: workgroup b is footprint b, row-major.  Lanes outside the image and lanes whose
// direction fails rays_core.h rays_accept do not march (`above = false`): they take no sample and compute no texture address; the latter store zeros.
//
// Every kernel from here to the end of the file is this one with another front end, and is written as: the lane's pixel (csky_common.h tile_pixel),
// its direction (rays_core.h rays_lane_dir, or the update's view_update_dir), the kernel's own ray maker, march_store.

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

// ---- the temporal split of a view frame ----------------------------------------------------------------------------
// One pixel of every B x B block of a view is marched per call (the fresh pixels), the others are taken from the previous view frame through the
// previous camera, and a pixel that frame does not cover (a hole) is marched.  Two launches that write disjoint pixels: the order between them does
// not matter.  Both are clouds_rays_kernel's shape: one pixel per lane, an 8x8 tile per wavefront, four tiles per workgroup, the same LDS queue and
// launch bound, march_compact<true, false> on the frame constants the cloud frame's set-up kernel wrote.

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

// ---- the direct march from an observer's position -------------------------------------------------------------------
// clouds_rays_kernel with another front end: observer_core.h observer_ray makes the lane's Ray from its direction AND the observer's position (under,
// inside or above the layer; the first segment through the layer, capped; a segment too short to have a direction in fp32 is not marched: a zero
// Ray, as scene_depth_ray_k's).  The same shape: one pixel per lane, an 8x8 tile per wavefront, four
// tiles per workgroup, the same LDS queue and launch bound, a plain launch in natural order.  march_compact<true, false, 0, TS, false>: these rays
// descend, or dip and rise, so the wavefront's early end is "no lane is live" and not "every lane is above the window".

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

// ---- the observer's march behind a per-pixel scene depth -------------------------------------------------------------
// clouds_observer_kernel with one more input: scene_depth_core.h scene_depth_ray ends the lane's segment at its own pixel's depth texel (metres along
// the ray, or along the camera's forward axis) as well as at the frame's max_distance.  The same shape: one pixel per lane, an 8x8 tile per wavefront,
// four tiles per workgroup, the same LDS queue and launch bound, a plain launch in natural order, march_compact<true, false, 0, TS, false>.  A lane
// inside the image makes one 4-byte load of its texel (a row of a tile is eight consecutive floats); a lane outside it loads nothing.  A wavefront
// whose lanes are all occluded returns at march_compact's first ballot.

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
