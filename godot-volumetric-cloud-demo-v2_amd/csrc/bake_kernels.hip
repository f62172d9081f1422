// bake_kernels.hip -- gfx950 kernels of csky_set_noise and the noise generators: everything that runs once per texture set.
//
//   shape_noise_kernel / detail_noise_kernel : the stand-in noise volumes, one voxel per lane (noise_core.h)
//   weather_noise_kernel                     : the generated weather map, one texel per lane (noise_core.h)
//   mip_level_kernel                         : 2x2x2 box mips of an 8-bit chain
//   bake_{shape,detail,weather}[32]_kernel   : the device texture layouts, one texel per lane (bake_core.h)
// Checked buffer by buffer against numpy in tests/test_gpu_bake.py (tests/bake_reference.py, oracle/noise_restatement.py), not against the host
// build of the same headers alone.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "noise_core.h"
#include "bake_core.h"
#pragma clang fp contract(off)   // for the code of this file, whatever the last header left (the cores state their own)

namespace csky {

// ------------------------------------------------------------------------------------------------ shape-noise bake
// The stand-in 128^3 RGBA shape volume, one voxel per lane (bit-identical to the host generator: noise_core.h).
__global__ __launch_bounds__(256) void shape_noise_kernel(uint32_t seed, int n, ShapeNoiseParams P, uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * n * n) return;
    const int x = (int)(i % n), y = (int)((i / n) % n), z = (int)(i / ((size_t)n * n));
    uint8_t o[4];
    shape_voxel(seed, n, x, y, z, P, o);
    out[i] = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
}
hipError_t launch_shape_noise(uint32_t seed, int n, const ShapeNoiseParams& P, uint32_t* d_out, hipStream_t s) {
    const size_t total = (size_t)n * n * n;
    shape_noise_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(seed, n, P, d_out);
    return hipGetLastError();
}

// the 32^3 RGB detail volume (noise_core.h::detail_voxel), one voxel per lane, 3 bytes each
__global__ __launch_bounds__(256) void detail_noise_kernel(uint32_t seed, int n, uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * n * n) return;
    const int x = (int)(i % n), y = (int)((i / n) % n), z = (int)(i / ((size_t)n * n));
    uint8_t o[3];
    detail_voxel(seed, n, x, y, z, o);
    out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}
hipError_t launch_detail_noise(uint32_t seed, int n, uint8_t* d_out, hipStream_t s) {
    const size_t total = (size_t)n * n * n;
    detail_noise_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(seed, n, d_out);
    return hipGetLastError();
}

// the 512 x 512 RGB weather map (noise_core.h::weather_texel), one texel per lane, 3 bytes each: 1024 workgroups, four per CU of the device
__global__ __launch_bounds__(256) void weather_noise_kernel(uint32_t seed, WeatherNoiseParams P, uint8_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= WEATHER_N * WEATHER_N) return;
    uint8_t o[3];
    weather_texel(seed, i % WEATHER_N, i / WEATHER_N, P, o);
    out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}
hipError_t launch_weather_noise(uint32_t seed, const WeatherNoiseParams& P, uint8_t* d_out, hipStream_t s) {
    weather_noise_kernel<<<(WEATHER_N * WEATHER_N + 255) / 256, 256, 0, s>>>(seed, P, d_out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ mip chains + texture bake on the device
// csky_set_noise uploads the three 8-bit level-0 textures (9.2 MB) and does everything else here: 2x2x2 box mips (Godot's
// mipmaps/generate=true), then one lane per texel of each device layout (bake_core.h: the same per-texel code as the host bake of
// tests/hostsim).  Replaces ~1.5 s of host loops + 78 MB of pageable uploads per csky_set_noise by < 1 ms of kernels.
__global__ __launch_bounds__(256) void mip_level_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int nd, int ch) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)nd * nd * nd * ch;
    if (i >= total) return;
    const int c = (int)(i % ch); const size_t t = i / ch;
    const int x = (int)(t % nd), y = (int)((t / nd) % nd), z = (int)(t / ((size_t)nd * nd));
    dst[i] = mip_texel(src, nd * 2, ch, x, y, z, c);
}
hipError_t launch_mip_chain(uint8_t* d_chain, int n, int ch, int levels, hipStream_t s) {
    for (int l = 1; l < levels; l++) {
        const int nd = n >> l;
        const size_t total = (size_t)nd * nd * nd * ch;
        mip_level_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(d_chain + chain_offset(n, l - 1, ch), d_chain + chain_offset(n, l, ch), nd, ch);
    }
    return hipGetLastError();
}
__device__ __forceinline__ void bake_tally(unsigned bad, unsigned long long* __restrict__ inexact) {
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(inexact, (unsigned long long)bad);
}
template <int N, int LEVELS> __device__ __forceinline__ bool level_of(size_t i, int& l, int& n, size_t& local) {
    size_t base = 0;
    for (l = 0; l < LEVELS; l++) { n = N >> l; const size_t cnt = (size_t)n * n * n; if (i < base + cnt) { local = i - base; return true; } base += cnt; }
    return false;
}
__global__ __launch_bounds__(256) void bake_shape_kernel(const uint8_t* __restrict__ chain, ShapeTexel* __restrict__ out, unsigned long long* __restrict__ inexact) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int l, n; size_t local; unsigned bad = 0;
    if (level_of<SHAPE_N, SHAPE_LEVELS>(i, l, n, local)) {
        const int x = (int)(local % n), y = (int)((local / n) % n), z = (int)(local / ((size_t)n * n));
        out[(i - local) + shape_cell_index(n, x, y, z)] = bake_shape_texel(chain + chain_offset(SHAPE_N, l, 4), n, x, y, z, bad);
    }
    bake_tally(bad, inexact);
}
__global__ __launch_bounds__(256) void bake_detail_kernel(const uint8_t* __restrict__ chain, uint4* __restrict__ out, uint16_t* __restrict__ out_h, unsigned long long* __restrict__ inexact) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int l, n; size_t local; unsigned bad = 0;
    if (level_of<DETAIL_N, DETAIL_LEVELS>(i, l, n, local)) {
        const uint8_t* src = chain + chain_offset(DETAIL_N, l, 3);
        const int x = (int)(local % n), y = (int)((local / n) % n), z = (int)(local / ((size_t)n * n));
        out[i] = bake_detail_texel(src, n, x, y, z, bad);
        out_h[i] = f2h((float)detail_numerator(src, n, x, y, z));                 // unpacked fp16 chain: source of the "lds" variant's LDS copy
    }
    bake_tally(bad, inexact);
}
// also the channel ranges of the map (exact height-window reject, bake.h::height_window): range[0] = min R, [1] = max R, [2] = max B
__global__ __launch_bounds__(256) void bake_weather_kernel(const uint8_t* __restrict__ rgb, uint4* __restrict__ out, unsigned long long* __restrict__ inexact, int* __restrict__ range) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned bad = 0;
    if (i < WEATHER_N * WEATHER_N) {
        out[i] = bake_weather_texel(rgb, i % WEATHER_N, i / WEATHER_N, bad);
        int r = rgb[3 * i], b = rgb[3 * i + 2], rmin = r, rmax = r, bmax = b;
        for (int off = 32; off > 0; off >>= 1) { rmin = min(rmin, __shfl_down(rmin, off)); rmax = max(rmax, __shfl_down(rmax, off)); bmax = max(bmax, __shfl_down(bmax, off)); }
        if ((threadIdx.x & 63) == 0) { atomicMin(&range[0], rmin); atomicMax(&range[1], rmax); atomicMax(&range[2], bmax); }
    }
    bake_tally(bad, inexact);
}
hipError_t launch_bake(const uint8_t* d_large_chain, const uint8_t* d_small_chain, const uint8_t* d_weather, ShapeTexel* d_shape, uint4* d_detail, uint16_t* d_detail_h,
                       uint4* d_weather_out, unsigned long long* d_inexact, int* d_range, hipStream_t s) {
    const size_t shape_total = chain_offset(SHAPE_N, SHAPE_LEVELS, 1), detail_total = chain_offset(DETAIL_N, DETAIL_LEVELS, 1);   // texels of all levels
    bake_shape_kernel<<<(unsigned)((shape_total + 255) / 256), 256, 0, s>>>(d_large_chain, d_shape, d_inexact);
    bake_detail_kernel<<<(unsigned)((detail_total + 255) / 256), 256, 0, s>>>(d_small_chain, d_detail, d_detail_h, d_inexact);
    bake_weather_kernel<<<(WEATHER_N * WEATHER_N + 255) / 256, 256, 0, s>>>(d_weather, d_weather_out, d_inexact, d_range);
    return hipGetLastError();
}
hipError_t launch_bake_weather(const uint8_t* d_weather, uint4* d_weather_out, unsigned long long* d_inexact, int* d_range, hipStream_t s) {
    bake_weather_kernel<<<(WEATHER_N * WEATHER_N + 255) / 256, 256, 0, s>>>(d_weather, d_weather_out, d_inexact, d_range);
    return hipGetLastError();
}

// exact cells (bake_core.h: fp32 coefficients), built only for textures with coefficients fp16 cannot hold (or on request)
__global__ __launch_bounds__(256) void bake_shape32_kernel(const uint8_t* __restrict__ chain, float4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int l, n; size_t local;
    if (level_of<SHAPE_N, SHAPE_LEVELS>(i, l, n, local)) {
        const int x = (int)(local % n), y = (int)((local / n) % n), z = (int)(local / ((size_t)n * n));
        float4 c[4];
        bake_shape_texel32(chain + chain_offset(SHAPE_N, l, 4), n, x, y, z, c);
        float4* o = out + 4 * ((i - local) + shape_cell_index(n, x, y, z));
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
    }
}
__global__ __launch_bounds__(256) void bake_detail32_kernel(const uint8_t* __restrict__ chain, float4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int l, n; size_t local;
    if (level_of<DETAIL_N, DETAIL_LEVELS>(i, l, n, local)) {
        const int x = (int)(local % n), y = (int)((local / n) % n), z = (int)(local / ((size_t)n * n));
        float4 c[2];
        bake_detail_texel32(chain + chain_offset(DETAIL_N, l, 3), n, x, y, z, c);
        out[2 * i] = c[0]; out[2 * i + 1] = c[1];
    }
}
__global__ __launch_bounds__(256) void bake_weather32_kernel(const uint8_t* __restrict__ rgb, float4* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < WEATHER_N * WEATHER_N) {
        float4 c[2];
        bake_weather_texel32(rgb, i % WEATHER_N, i / WEATHER_N, c);
        out[2 * i] = c[0]; out[2 * i + 1] = c[1];
    }
}
hipError_t launch_bake32(const uint8_t* d_large_chain, const uint8_t* d_small_chain, const uint8_t* d_weather, float4* d_shape32, float4* d_detail32, float4* d_weather32, hipStream_t s) {
    const size_t shape_total = chain_offset(SHAPE_N, SHAPE_LEVELS, 1), detail_total = chain_offset(DETAIL_N, DETAIL_LEVELS, 1);   // texels of all levels
    bake_shape32_kernel<<<(unsigned)((shape_total + 255) / 256), 256, 0, s>>>(d_large_chain, d_shape32);
    bake_detail32_kernel<<<(unsigned)((detail_total + 255) / 256), 256, 0, s>>>(d_small_chain, d_detail32);
    bake_weather32_kernel<<<(WEATHER_N * WEATHER_N + 255) / 256, 256, 0, s>>>(d_weather, d_weather32);
    return hipGetLastError();
}
hipError_t launch_bake_weather32(const uint8_t* d_weather, float4* d_weather32, hipStream_t s) {
    bake_weather32_kernel<<<(WEATHER_N * WEATHER_N + 255) / 256, 256, 0, s>>>(d_weather, d_weather32);
    return hipGetLastError();
}

}  // namespace csky
