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
    const TilePixel p = tile_pixel(sc.w, sc.h);                // the lanes outside a ragged map take part in the votes only
    T.detail_lds = nullptr;                                    // compile-time constant here: the LDS tap path folds away
    const uint16_t hlf = shadow_texel(T, fc, sc, p.i, p.j, p.valid, nullptr);
    if (p.valid) out[(size_t)p.j * sc.pitch_h + (size_t)p.i] = hlf;
}

}  // namespace

hipError_t launch_cloud_shadow(const TexSet& t, const TexSet32* t32, const FrameConsts& fc, const ShadowConsts& sc, uint16_t* d_out, hipStream_t s) {
    const int grid = tile_grid(sc.w, sc.h);
    with_texset(t, t32, [&](const auto& ts) { shadow_kernel<<<grid, 256, 0, s>>>(ts, fc, sc, d_out); });
    return hipGetLastError();
}

}  // namespace csky
