// cloud_aerial.hip -- the kernel that puts the air in front of a cloud frame (cloud_aerial_core.h), one instantiation per mapping
// of the transmittance table.  One pixel per lane in the cloud kernel's tiling: a wavefront owns an 8x8 tile of pixels, a 256-thread workgroup
// four tiles side by side.  A wavefront none of whose pixels holds a cloud with a distance copies its texels and leaves (one ballot); every
// other lane loops its own n steps of sky_step: n <= 64 is far below a wavefront's width, so aerial_kernel's steps-across-lanes shape does not
// fit.  Bit-identical to cloud_aerial_pixel on one lane.  The geometry and the sun are kernel arguments: the call takes no slot of any ring.
// A lane reads its own two texels before it writes its own one: `out` may be the cloud frame.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "cloud_aerial_core.h"
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

}  // namespace

hipError_t launch_cloud_aerial(const CloudAerialGeom& g, const float4* d_trans, int tw, int th, const uint2* d_cloud, const uint2* d_depth, uint2* d_out,
                               hipStream_t s, int tlut) {
    const int grid = tile_grid(g.w, g.h);
    if (tlut == TLUT_BRUNETON) cloud_aerial_kernel<TLUT_BRUNETON><<<grid, 256, 0, s>>>(g, d_trans, tw, th, d_cloud, d_depth, d_out);
    else cloud_aerial_kernel<TLUT_REFERENCE><<<grid, 256, 0, s>>>(g, d_trans, tw, th, d_cloud, d_depth, d_out);
    return hipGetLastError();
}

}  // namespace csky
