// cloud_aerial.hip -- the kernel that puts the air in front of a cloud frame (cloud_aerial_core.h), one instantiation per mapping
// of the transmittance table.  One pixel per lane in the cloud kernel's tiling: a wavefront owns an 8x8 tile of pixels, a 256-thread workgroup
// four tiles side by side.  A wavefront none of whose pixels holds a cloud with a distance copies its texels and leaves (one ballot); every
// other lane loops its own n steps of sky_step: n <= 64 is far below a wavefront's width, so aerial_kernel's steps-across-lanes shape does not
// fit.  Bit-identical to cloud_aerial_pixel on one lane.  The geometry and the sun are kernel arguments: the call takes no slot of any ring.
// A lane reads its own two texels before it writes its own one: `out` may be the cloud frame.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "cloud_aerial_core.h"
#include "view_depth_core.h"
#pragma clang fp contract(off)   // for the code of this file, whatever the last header left (the cores state their own)

namespace csky {

namespace {

template <int TLUT> __global__ __launch_bounds__(256) void cloud_aerial_kernel(const CloudAerialGeom g, const float4* __restrict__ trans, int tw, int th,
                                                                                 const uint2* cloud, const uint2* depth, uint2* out) {
    const TilePixel p = tile_pixel(g.w, g.h);
    const size_t at = (size_t)(p.valid ? p.j : 0) * (size_t)g.w + (size_t)(p.valid ? p.i : 0);
    uint2 c, z;
    c.x = c.y = z.x = z.y = 0u;
    if (p.valid) { c = cloud[at]; z = depth[at]; }
    const bool work = p.valid && !cloud_aerial_passes(c, z);
    if (__builtin_amdgcn_ballot_w64(work) == 0ull) {           // clear sky, or the frame's edge under the horizon
        if (p.valid) out[at] = c;
        return;
    }
    if (work) c = cloud_aerial_pixel<TLUT>(g, p.i, p.j, c, z, trans, tw, th);
    if (p.valid) out[at] = c;
}

// The same step on a ray frame (view_depth_core.h cloud_aerial_dir).  SRC (rays_core.h rays_lane_dir) 0: directions from `dirs`
// ([H][W][3] floats, tightly packed); 1: the view of G.  A pixel whose direction the march would not have taken passes like one without a cloud.
template <int SRC, int TLUT> __global__ __launch_bounds__(256) void cloud_aerial_rays_kernel(const CloudAerialGeom g, const RaysGeom G, const float* __restrict__ dirs,
                                                                                              const float4* __restrict__ trans, int tw, int th, const uint2* cloud,
                                                                                              const uint2* depth, uint2* out) {
    const TilePixel p = tile_pixel(g.w, g.h);
    const size_t at = (size_t)(p.valid ? p.j : 0) * (size_t)g.w + (size_t)(p.valid ? p.i : 0);
    uint2 c, z;
    c.x = c.y = z.x = z.y = 0u;
    float ex, ey, ez;
    if (p.valid) { c = cloud[at]; z = depth[at]; }
    rays_lane_dir<SRC>(G, dirs, p, ex, ey, ez);   // G.w x G.h = g.w x g.h (launch_cloud_aerial_rays)
    const bool work = p.valid && !cloud_aerial_dir_passes(c, z, ex, ey, ez);
    if (__builtin_amdgcn_ballot_w64(work) == 0ull) {           // clear sky, or a tile under the horizon
        if (p.valid) out[at] = c;
        return;
    }
    if (work) c = cloud_aerial_dir<TLUT>(g, ex, ey, ez, c, z, trans, tw, th);
    if (p.valid) out[at] = c;
}

}  // namespace

hipError_t launch_cloud_aerial_rays(const CloudAerialGeom& g, const RaysGeom& rg, const float* d_dirs, const float4* d_trans, int tw, int th, const uint2* d_cloud,
                                    const uint2* d_depth, uint2* d_out, hipStream_t s, int tlut) {
    if (g.w < 1 || g.h < 1 || g.w > 8192 || g.h > 8192 || rg.w != g.w || rg.h != g.h) return hipErrorInvalidValue;
    const int grid = tile_grid(g.w, g.h);
    if (tlut == TLUT_BRUNETON) {
        if (d_dirs) cloud_aerial_rays_kernel<0, TLUT_BRUNETON><<<grid, 256, 0, s>>>(g, rg, d_dirs, d_trans, tw, th, d_cloud, d_depth, d_out);
        else cloud_aerial_rays_kernel<1, TLUT_BRUNETON><<<grid, 256, 0, s>>>(g, rg, d_dirs, d_trans, tw, th, d_cloud, d_depth, d_out);
    } else {
        if (d_dirs) cloud_aerial_rays_kernel<0, TLUT_REFERENCE><<<grid, 256, 0, s>>>(g, rg, d_dirs, d_trans, tw, th, d_cloud, d_depth, d_out);
        else cloud_aerial_rays_kernel<1, TLUT_REFERENCE><<<grid, 256, 0, s>>>(g, rg, d_dirs, d_trans, tw, th, d_cloud, d_depth, d_out);
    }
    return hipGetLastError();
}

hipError_t launch_cloud_aerial(const CloudAerialGeom& g, const float4* d_trans, int tw, int th, const uint2* d_cloud, const uint2* d_depth, uint2* d_out,
                               hipStream_t s, int tlut) {
    const int grid = tile_grid(g.w, g.h);
    if (tlut == TLUT_BRUNETON) cloud_aerial_kernel<TLUT_BRUNETON><<<grid, 256, 0, s>>>(g, d_trans, tw, th, d_cloud, d_depth, d_out);
    else cloud_aerial_kernel<TLUT_REFERENCE><<<grid, 256, 0, s>>>(g, d_trans, tw, th, d_cloud, d_depth, d_out);
    return hipGetLastError();
}

}  // namespace csky
