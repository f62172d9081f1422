// radiance.hip -- gfx950 kernels of the sky's radiance cubemap (include/cloudsky.h csky_render_radiance*, csky_prefilter_cube; the maths:
// radiance_core.h).  Layer 0 is the compositor's own kernel (lut_kernels.hip composite_kernel, view_mode 2); this file holds the source-cube
// reduction, the bounding cones of the culling test and the GGX prefilter.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "radiance_core.h"

namespace csky {

// one thread per source texel: block mean of layer 0, direction, solid angle -> the block-major record table
__global__ __launch_bounds__(256) void radiance_source_kernel(const uint16_t* __restrict__ layer0, int n, int ns, float4* __restrict__ tab) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 6 * ns * ns) return;
    const int f = t / (ns * ns), j = (t / ns) % ns, i = t % ns;
    rad_source_texel(layer0, n, ns, f, i, j, tab);
}
hipError_t launch_radiance_source(const uint16_t* d_layer0, int n, int ns, float4* d_tab, hipStream_t s) {
    radiance_source_kernel<<<(6 * ns * ns + 255) / 256, 256, 0, s>>>(d_layer0, n, ns, d_tab);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void radiance_cones_kernel(int n, float4* __restrict__ cones) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < rad_block_count(n)) cones[b] = rad_block_cone(n, b);
}
hipError_t launch_radiance_cones(int n, float4* d_cones, hipStream_t s) {
    radiance_cones_kernel<<<(rad_block_count(n) + 255) / 256, 256, 0, s>>>(n, d_cones);
    return hipGetLastError();
}

struct RadFilterArgs {
    int n, ns, cull;
    RadLayer ly[RAD_MAX_LAYERS - 1];
};

// One workgroup = one 8x8 block of one output face, one receiver texel per lane; its RAD_WAVES waves take the source blocks
// wave, wave + RAD_WAVES, ... (records are wave-uniform: scalar loads from the read-only table) and wave 0 adds the partial sums in wave
// order.  Fixed order everywhere, no atomics: repeated calls give the same bytes.
template <int NL>
__global__ __launch_bounds__(64 * RAD_WAVES) void radiance_filter_kernel(RadFilterArgs A, const float4* __restrict__ tab, const float4* __restrict__ src_cones,
                                                                         const float4* __restrict__ out_cones, uint2* __restrict__ out) {
    __shared__ float4 red[RAD_WAVES - 1][64];
    const int ob = blockIdx.x, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int S = A.n, nbo = S / 8;
    const int f = ob / (nbo * nbo), by = (ob / nbo) % nbo, bx = ob % nbo;
    const int i = bx * 8 + (lane & 7), j = by * 8 + (lane >> 3);
    float nx, ny, nz;
    rad_texel_dir(f, i, j, S, nx, ny, nz);
    RadLayer ly[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) ly[l] = A.ly[l];
    float4 acc[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) acc[l] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 oc = out_cones[ob];
    const int per = rad_block_size(A.ns) * rad_block_size(A.ns), nsb = rad_block_count(A.ns);
    for (int sb = wave; sb < nsb; sb += RAD_WAVES) {
        if (A.cull && rad_cull(oc, src_cones[sb])) continue;
        const float4* rec = tab + (size_t)sb * per * 2;
#pragma unroll 4
        for (int t = 0; t < per; t++) rad_accumulate<NL>(nx, ny, nz, rec[2 * t], rec[2 * t + 1], ly, acc);
    }
    const size_t plane = (size_t)6 * S * S, px = ((size_t)f * S + j) * S + i;
#pragma unroll
    for (int l = 0; l < NL; l++) {
        if (wave > 0) red[wave - 1][lane] = acc[l];
        __syncthreads();
        if (wave == 0) {
            float4 s = acc[l];
            for (int w = 0; w < RAD_WAVES - 1; w++) { const float4 p = red[w][lane]; s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w; }
            out[l * plane + px] = make_uint2((uint32_t)f2h(s.x / s.w) | ((uint32_t)f2h(s.y / s.w) << 16), (uint32_t)f2h(s.z / s.w) | ((uint32_t)f2h(1.0f) << 16));
        }
        __syncthreads();
    }
}

template <int NL>
static void filter_launch(const RadFilterArgs& a, const float4* tab, const float4* sc, const float4* oc, uint2* out, hipStream_t s) {
    radiance_filter_kernel<NL><<<6 * (a.n / 8) * (a.n / 8), 64 * RAD_WAVES, 0, s>>>(a, tab, sc, oc, out);
}

hipError_t launch_radiance_filter(const float4* d_tab, const float4* d_src_cones, const float4* d_out_cones, int n, int ns, const RadLayer* ly, int nl, bool cull,
                                  uint2* d_out, hipStream_t s) {
    RadFilterArgs a;
    a.n = n; a.ns = ns; a.cull = cull ? 1 : 0;
    for (int l = 0; l < RAD_MAX_LAYERS - 1; l++) a.ly[l] = l < nl ? ly[l] : RadLayer{1.0f, 0.0f};
    switch (nl) {
        case 1: filter_launch<1>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        case 2: filter_launch<2>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        case 3: filter_launch<3>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        case 4: filter_launch<4>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        case 5: filter_launch<5>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        case 6: filter_launch<6>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        case 7: filter_launch<7>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        case 8: filter_launch<8>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        case 9: filter_launch<9>(a, d_tab, d_src_cones, d_out_cones, d_out, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace csky
