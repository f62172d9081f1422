// shadow.hip -- the cloud shadow map's kernel (shadow_core.h): one texel per lane, a wavefront owns an 8x8 tile of texels and a 256-thread
// workgroup four tiles side by side (32 x 8 texels), the cloud kernel's footprint.  The rays of a map are parallel, so the lanes of a tile gather
// neighbouring cells of every texture at every step.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "shadow_core.h"

namespace csky {

namespace {

// Both constant blocks are kernel arguments (scalar loads from the kernarg segment): nothing of a shadow call lives in device memory besides the map.
template <class TS>
__global__ __launch_bounds__(256) void shadow_kernel(TS T, const FrameConsts fc, const ShadowConsts sc, uint16_t* __restrict__ out) {
    const int tiles_x = (sc.w + 31) >> 5;
    const int slab = (int)blockIdx.x / tiles_x, bx = (int)blockIdx.x - slab * tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = bx * 32 + wave * 8 + (lane & 7);
    const int j = slab * 8 + (lane >> 3);
    const bool valid = i < sc.w && j < sc.h;                   // a ragged map masks the lanes of its partial tiles: they take part in the votes only
    T.detail_lds = nullptr;                                    // compile-time constant here: the LDS tap path folds away
    const uint16_t hlf = shadow_texel(T, fc, sc, i, j, valid, nullptr);
    if (valid) out[(size_t)j * sc.pitch_h + (size_t)i] = hlf;
}

}  // namespace

hipError_t launch_cloud_shadow(const TexSet& t, const TexSet32* t32, const FrameConsts& fc, const ShadowConsts& sc, uint16_t* d_out, hipStream_t s) {
    const int grid = ((sc.w + 31) >> 5) * ((sc.h + 7) >> 3);   // <= 256 x 1024 for the largest map
    if (t32) shadow_kernel<TexSet32><<<grid, 256, 0, s>>>(*t32, fc, sc, d_out);
    else shadow_kernel<TexSet><<<grid, 256, 0, s>>>(t, fc, sc, d_out);
    return hipGetLastError();
}

}  // namespace csky
