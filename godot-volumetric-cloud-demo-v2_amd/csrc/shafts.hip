// shafts.hip -- the shadowed aerial-perspective volume's kernel (shafts_core.h), one instantiation per mapping of the transmittance
// table.  aerial_kernel's shape (aerial.hip), with the step that taps the cloud shadow map:
//   one column per wavefront, four per 256-thread workgroup; the column's n = D * S steps go by in chunks of 64:
//   1. lane l evaluates step base + l and parks S_int / step_tr in LDS; a skipped step parks 0 / 1, which leaves L and Tr exactly unchanged.
//      A chunk that starts at or beyond t_stop evaluates nothing: the midpoints only grow
//   2. lane 0 replays the accumulation in the column's own order, carries (L, Tr) into the next chunk and parks the state at every slice end
//   3. the lanes convert and store the slices that ended in the chunk, one each (at most 64: S >= 1)
// Bit-identical to shafts_column on one lane.  Geometry, the map's geometry and the sun's unit vector are kernel arguments: the call takes no
// slot of any ring.  The map is read with plain 2-byte loads, bounds-checked per texel (shafts_texel); nothing but the volume is written.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "shafts_core.h"
#pragma clang fp contract(off)   // for the code of this file, whatever the last header left (the cores state their own)

namespace csky {

namespace {

template <int TLUT> __global__ __launch_bounds__(256) void shafts_kernel(const AerialGeom g, const ShaftsMap m, const float4* __restrict__ trans, int tw, int th,
                                                                           uint2* __restrict__ out) {
    __shared__ float steps[4][64][8];     // this chunk's S_int, step_tr
    __shared__ float ends[4][64][8];      // (L, Tr) behind the slices that ended in this chunk
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int columns = g.w * g.h, column = blockIdx.x * 4 + wave;
    const bool live = column < columns;                           // the last workgroup's spare wavefronts march column 0 and store nothing
    const int ci = live ? column % g.w : 0, cj = live ? column / g.w : 0;
    const int n = g.d * g.s;
    const AerialRay a = aerial_volume_ray(g, ci, cj);
    F4 L = f4(0, 0, 0, 0), Tr = f4(1, 1, 1, 1);                   // lane 0's
    for (int base = 0; base < n; base += 64) {                    // n is the launch's: every wavefront of the workgroup meets every barrier
        const int cnt = n - base < 64 ? n - base : 64;
        if (lane < cnt) {
            SkyStep s; s.S_int = f4(0, 0, 0, 0); s.step_tr = f4(1, 1, 1, 1);
            if (!aerial_skipped(a, base) && !aerial_skipped(a, base + lane)) s = sky_step_shadowed<TLUT>(a.r, base + lane, trans, tw, th, m);
            float* d = steps[wave][lane];
            d[0] = s.S_int.x; d[1] = s.S_int.y; d[2] = s.S_int.z; d[3] = s.S_int.w;
            d[4] = s.step_tr.x; d[5] = s.step_tr.y; d[6] = s.step_tr.z; d[7] = s.step_tr.w;
        }
        __syncthreads();
        const int k0 = base / g.s, k1 = (base + cnt) / g.s;       // slices [k0, k1) end in this chunk: slice k's last step is (k + 1) * S - 1
        if (lane == 0) {
            int k = k0;
            for (int i = 0; i < cnt; ++i) {
                const float* d = steps[wave][i];
                SkyStep s; s.S_int = f4(d[0], d[1], d[2], d[3]); s.step_tr = f4(d[4], d[5], d[6], d[7]);
                sky_accumulate(L, Tr, s);
                if (base + i + 1 == (k + 1) * g.s) {
                    float* e = ends[wave][k - k0];
                    e[0] = L.x; e[1] = L.y; e[2] = L.z; e[3] = L.w; e[4] = Tr.x; e[5] = Tr.y; e[6] = Tr.z; e[7] = Tr.w;
                    ++k;
                }
            }
        }
        __syncthreads();
        if (live && lane < k1 - k0) {
            const float* e = ends[wave][lane];
            const AerialTexel t = aerial_slice(f4(e[0], e[1], e[2], e[3]), f4(e[4], e[5], e[6], e[7]));
            out[(size_t)(k0 + lane) * columns + column] = pack_half4(t.h[0], t.h[1], t.h[2], t.h[3]);
        }
        // the next chunk's steps are parked behind this barrier pair, its slice ends behind its own first barrier: no third one
    }
}

}  // namespace

hipError_t launch_shafts(const AerialGeom& g, const ShaftsMap& m, const float4* d_trans, int tw, int th, uint2* d_out, hipStream_t s, int tlut) {
    const int grid = (g.w * g.h + 3) / 4;                         // <= 65 536 for the largest volume
    if (tlut == TLUT_BRUNETON) shafts_kernel<TLUT_BRUNETON><<<grid, 256, 0, s>>>(g, m, d_trans, tw, th, d_out);
    else shafts_kernel<TLUT_REFERENCE><<<grid, 256, 0, s>>>(g, m, d_trans, tw, th, d_out);
    return hipGetLastError();
}

}  // namespace csky
