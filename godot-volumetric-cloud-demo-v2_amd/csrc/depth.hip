// depth.hip -- the cloud depth frame's kernels (depth_core.h; view_depth_core.h for ray frames): shadow_kernel's shape (shadow.hip).  One pixel per lane, a wavefront owns an 8x8
// tile of pixels and a 256-thread workgroup four tiles side by side (32 x 8 pixels), the cloud kernel's footprint: the rays of a tile are
// neighbours on the hemisphere and gather neighbouring cells of every texture at every step.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "depth_core.h"
#include "view_depth_core.h"

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

// The depth frame of a ray frame (view_depth_core.h depth_dir): depth_kernel's shape with the direct march's front end.  SRC
// (rays_core.h rays_lane_dir) 0: directions from `dirs` ([H][W][3] floats, tightly packed, three dword loads); 1: the view of G.  Lanes outside a
// ragged image and lanes whose direction fails rays_accept take part in the votes only; the latter store zeros.
template <int SRC, class TS>
__global__ __launch_bounds__(256) void depth_rays_kernel(TS T, const FrameConsts fc, const DepthConsts dc, const RaysGeom G, const float* __restrict__ dirs,
                                                         uint2* __restrict__ out) {
    const TilePixel p = tile_pixel(dc.w, dc.h);
    T.detail_lds = nullptr;                                    // compile-time constant here: the LDS tap path folds away
    float ex, ey, ez;
    rays_lane_dir<SRC>(G, dirs, p, ex, ey, ez);   // G.w x G.h = dc.w x dc.h (launch_cloud_depth_rays)
    const DepthTexel t = depth_dir(T, fc, dc, ex, ey, ez, p.valid, nullptr, nullptr);
    if (p.valid) out[(size_t)p.j * dc.pitch_px + (size_t)p.i] = pack_half4(t.h[0], t.h[1], t.h[2], t.h[3]);
}

}  // namespace

hipError_t launch_cloud_depth_rays(const TexSet& t, const TexSet32* t32, const FrameConsts& fc, const DepthConsts& dc, const RaysGeom& g, const float* d_dirs,
                                   uint2* d_out, hipStream_t s) {
    if (dc.w < 1 || dc.h < 1 || dc.w > 8192 || dc.h > 8192 || dc.pitch_px < (uint32_t)dc.w || g.w != dc.w || g.h != dc.h) return hipErrorInvalidValue;
    const int grid = tile_grid(dc.w, dc.h);
    with_texset(t, t32, [&](const auto& ts) {
        if (d_dirs) depth_rays_kernel<0><<<grid, 256, 0, s>>>(ts, fc, dc, g, d_dirs, d_out);
        else depth_rays_kernel<1><<<grid, 256, 0, s>>>(ts, fc, dc, g, d_dirs, d_out);
    });
    return hipGetLastError();
}

hipError_t launch_cloud_depth(const TexSet& t, const TexSet32* t32, const FrameConsts& fc, const DepthConsts& dc, uint2* d_out, hipStream_t s) {
    const int grid = tile_grid(dc.w, dc.h);
    with_texset(t, t32, [&](const auto& ts) { depth_kernel<<<grid, 256, 0, s>>>(ts, fc, dc, d_out); });
    return hipGetLastError();
}

}  // namespace csky
