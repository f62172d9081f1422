// cloud_aerial_core.h -- aerial perspective on a cloud frame (cloudsky.h csky_apply_cloud_aerial): the air between the observer
// and the cloud of every pixel of a hemisphere frame, the cloud placed at the mean distance its depth frame holds (depth_core.h).  Per pixel it
// is one column of the aerial-perspective volume (aerial_core.h; §14) with D = 1, S = n and far_km the pixel's own distance, composited the way
// the header tells a host to composite a surface: aerial_ray, the skip rule, sky_step, sky_accumulate and sky_output are used unchanged.  What
// is new here is only the pixel -> direction step (cloud_core.h pixel_dir, the cloud march's own) and the composite.
// Host+device like the other cores: cloud_aerial_pixel is the definition, what tests/cloud_aerial_host runs and what cloud_aerial.hip must equal
// bit for bit.  FP contraction off.  Units: km.
#pragma once
#include "csky_common.h"
#include "cloud_core.h"
#include "aerial_core.h"

namespace csky {
#pragma clang fp contract(off)

// What a call is made for, besides the transmittance table and the two images: a kernel argument.
struct CloudAerialGeom {
    int w, h;                          // pixels: the cloud frame's and the depth frame's
    int n;                             // steps per pixel
    float sun[3];                      // used as given, like AerialGeom::sun
};

CSKY_HD uint16_t half_of(const uint2& px, int c) { return (uint16_t)((c < 2 ? px.x : px.y) >> ((c & 1) * 16)); }

// A pixel that leaves as it came: no cloud (alpha is +0 or -0), or no distance (0, negative or NaN)
CSKY_HD bool cloud_aerial_passes(const uint2& c, const uint2& z) {
    return (half_of(c, 3) & 0x7fffu) == 0u || !(h2f(half_of(z, 0)) > 0.0f);
}

// The air in front of pixel (i, j), z its depth texel: the spectral state (L, Tr) behind the last of the n steps of the pixel's column.
template <int TLUT> CSKY_HD void cloud_aerial_column(const CloudAerialGeom& g, int i, int j, const uint2& z, const float4* trans, int tw, int th, F4& L, F4& Tr) {
    float ex, ey, ez;
    pixel_dir((float)g.w, (float)g.h, i, j, ex, ey, ez);
    const AerialRay a = aerial_ray(ex, ey, ez, g.sun, h2f(half_of(z, 0)), g.n);
    L = f4(0, 0, 0, 0); Tr = f4(1, 1, 1, 1);
    for (int s = 0; s < g.n; ++s)
        if (!aerial_skipped(a, s)) sky_accumulate(L, Tr, sky_step<TLUT>(a.r, s, trans, tw, th));
}

// The cloud texel c behind that air.
CSKY_HD uint2 cloud_aerial_composite(const uint2& c, const F4& L, const F4& Tr) {
    const F4 C = sky_output(L);
    const float tr = (((Tr.x + Tr.y) + Tr.z) + Tr.w) * 0.25f;                        // aerial_slice's a, before rounding
    const float ca = h2f(half_of(c, 3));
    const uint16_t r = f2h(h2f(half_of(c, 0)) * tr + ca * (C.x / 50.0f));
    const uint16_t gg = f2h(h2f(half_of(c, 1)) * tr + ca * (C.y / 50.0f));
    const uint16_t b = f2h(h2f(half_of(c, 2)) * tr + ca * (C.z / 50.0f));
    return pack_half4(r, gg, b, half_of(c, 3));
}

// Pixel (i, j) of a frame that does not pass: c the cloud texel, z the depth texel.
template <int TLUT> CSKY_HD uint2 cloud_aerial_pixel(const CloudAerialGeom& g, int i, int j, const uint2& c, const uint2& z, const float4* trans, int tw, int th) {
    F4 L, Tr;
    cloud_aerial_column<TLUT>(g, i, j, z, trans, tw, th, L, Tr);
    return cloud_aerial_composite(c, L, Tr);
}

}  // namespace csky
