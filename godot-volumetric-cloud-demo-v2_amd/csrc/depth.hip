// depth.hip -- the cloud depth frame's kernel (depth_core.h): shadow_kernel's shape (shadow.hip).  One pixel per lane, a wavefront owns an 8x8
// tile of pixels and a 256-thread workgroup four tiles side by side (32 x 8 pixels), the cloud kernel's footprint: the rays of a tile are
// neighbours on the hemisphere and gather neighbouring cells of every texture at every step.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "depth_core.h"

namespace csky {

namespace {

// Both constant blocks are kernel arguments (scalar loads from the kernarg segment): nothing of a depth call lives in device memory besides the frame.
template <class TS>
__global__ __launch_bounds__(256) void depth_kernel(TS T, const FrameConsts fc, const DepthConsts dc, uint2* __restrict__ out) {
    const TilePixel p = tile_pixel(dc.w, dc.h);                // the lanes outside a ragged frame take part in the votes only
    T.detail_lds = nullptr;                                    // compile-time constant here: the LDS tap path folds away
    const DepthTexel t = depth_pixel(T, fc, dc, p.i, p.j, p.valid, nullptr, nullptr);
    if (p.valid) out[(size_t)p.j * dc.pitch_px + (size_t)p.i] = pack_half4(t.h[0], t.h[1], t.h[2], t.h[3]);
}

}  // namespace

hipError_t launch_cloud_depth(const TexSet& t, const TexSet32* t32, const FrameConsts& fc, const DepthConsts& dc, uint2* d_out, hipStream_t s) {
    const int grid = tile_grid(dc.w, dc.h);
    if (t32) depth_kernel<TexSet32><<<grid, 256, 0, s>>>(*t32, fc, dc, d_out);
    else depth_kernel<TexSet><<<grid, 256, 0, s>>>(t, fc, dc, d_out);
    return hipGetLastError();
}

}  // namespace csky
