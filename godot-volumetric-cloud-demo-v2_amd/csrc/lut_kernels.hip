// lut_kernels.hip -- gfx950 (CDNA4, wave64) kernels of everything that reads or writes the transmittance LUT, one instantiation per mapping of
// that table (template <int TLUT>, tlut_core.h), and the frame set-up that goes with them:
//
//   transmittance_kernel    : transmittance-lut.glsl, one texel per wavefront, 40 steps on 40 lanes   (16 384 wavefronts, once)
//   sky_lut_kernel          : sky-lut.glsl, one texel per half wavefront, 30 steps on 30 lanes       (20 000 texels, per sun change)
//   sky_lut_rows_kernel     : one rank's rows of that LUT
//   composite_kernel        : clouds.gdshader sky(), one pixel per lane
//   frame_setup_kernel      : the ray-invariant prologue of clouds.glsl march()          (1 lane, per frame)
//   frame_setup_taps_kernel : the same for a context without a whole sky LUT: it renders the <= 12 texels it filters with sky_texel
//
// The per-lane maths is lut_core.h, composite_core.h and cloud_core.h (frame_setup).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.h"
#include "cloud_core.h"
#include "lut_core.h"
#include "composite_core.h"
#pragma clang fp contract(off)   // for the code of this file, whatever the last header left (the cores state their own)

namespace csky {

// tlut (a run-time value of the context) -> the TLUT template argument: launch(std::integral_constant<int, TLUT>), written once per launcher
template <class Launch> static void with_tlut(int tlut, Launch&& launch) {
    if (tlut == TLUT_BRUNETON) launch(std::integral_constant<int, TLUT_BRUNETON>());
    else launch(std::integral_constant<int, TLUT_REFERENCE>());
}

// ------------------------------------------------------------------------------------------------ LUTs
// transmittance-lut.glsl: one texel per wavefront: lanes 0..39 evaluate the 40 optical-depth steps in parallel (each ~150 VALU with five
// correctly rounded transcendentals, independent of the others), park extinction * dt in LDS, then lane 0 replays the sum in the reference's
// order (T:186-192; bit-identical to the one-lane-per-texel form, 40x shorter critical path).  Round 1 had the GLSL's own dispatch shape here
// (8x8 groups, one texel per lane, a 40-step serial loop: 2 048 one-wave groups on 6 % of the chip).
// TLUT: the table's parametrization (tlut_core.h), one instantiation per mapping (here and in the sky-LUT, set-up and compositor kernels below).
template <int TLUT> __global__ __launch_bounds__(256) void transmittance_kernel(int w, int h, uint16_t* __restrict__ out_h, float4* __restrict__ out_f) {
    __shared__ float terms[4][TRANSMITTANCE_STEPS][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int texel = blockIdx.x * 4 + wave;
    const bool live = texel < w * h;                              // (T:159 tests `>`; the extra row/column would be an out-of-image store)
    const int px = live ? texel % w : 0, py = live ? texel / w : 0;
    const TransRay r = transmittance_ray<TLUT>(px, py, (float)w, (float)h);
    if (lane < TRANSMITTANCE_STEPS) {
        const F4 e = transmittance_step(r, lane);
        float* d = terms[wave][lane];
        d[0] = e.x; d[1] = e.y; d[2] = e.z; d[3] = e.w;
    }
    __syncthreads();
    if (lane == 0 && live) {
        F4 result = f4(0, 0, 0, 0);
        for (int i = 0; i < TRANSMITTANCE_STEPS; ++i) { const float* d = terms[wave][i]; result = result + f4(d[0], d[1], d[2], d[3]); }
        const F4 t = transmittance_finish(result);
        const uint16_t hx = f2h(t.x), hy = f2h(t.y), hz = f2h(t.z), hw = f2h(t.w);
        reinterpret_cast<uint2*>(out_h)[texel] = pack_half4(hx, hy, hz, hw);
        out_f[texel] = make_float4(h2f(hx), h2f(hy), h2f(hz), h2f(hw));
    }
}

struct Sun3 { float v[3]; explicit Sun3(const float s[3]) : v{s[0], s[1], s[2]} {} };   // the sun direction as a kernel argument
// sky-lut.glsl: one texel per HALF wavefront: lanes 0..29 evaluate the 30 in-scattering steps in parallel (each step is
// ~600 VALU with 20 LUT loads and 12 transcendentals and independent of the others), park source term + transmittance
// in LDS, then lane 0 of the half replays the front-to-back accumulation in the reference's order (bit-identical to the
// one-lane-per-texel form, 4x shorter critical path: this kernel sits on the critical path of every frame).
// One texel; store(px, py, hx, hy, hz, hw) takes the four fp16 values (lane 0 of the half wavefront, live texels only).
template <int TLUT, class Store> __device__ __forceinline__ void sky_texel(float (*steps)[8], int sub, bool live, int px, int py, int w, int h, const Sun3& sun,
                                                                 const float4* __restrict__ trans, int tw, int th, Store store) {
    const SkyRay r = sky_ray(px, py, (float)w, (float)h, sun.v);
    if (sub < IN_SCATTERING_STEPS) {
        const SkyStep s = sky_step<TLUT>(r, sub, trans, tw, th);
        float* d = steps[sub];
        d[0] = s.S_int.x; d[1] = s.S_int.y; d[2] = s.S_int.z; d[3] = s.S_int.w;
        d[4] = s.step_tr.x; d[5] = s.step_tr.y; d[6] = s.step_tr.z; d[7] = s.step_tr.w;
    }
    __syncthreads();
    if (sub == 0 && live) {
        F4 L = f4(0, 0, 0, 0), Tr = f4(1, 1, 1, 1);
        for (int i = 0; i < IN_SCATTERING_STEPS; ++i) {
            const float* d = steps[i];
            SkyStep s; s.S_int = f4(d[0], d[1], d[2], d[3]); s.step_tr = f4(d[4], d[5], d[6], d[7]);
            sky_accumulate(L, Tr, s);
        }
        const F4 c = sky_output(L);
        store(px, py, f2h(c.x), f2h(c.y), f2h(c.z), f2h(c.w));
    }
}
template <int TLUT> __global__ __launch_bounds__(256) void sky_lut_kernel(int w, int h, Sun3 sun, const float4* __restrict__ trans, int tw, int th,
                                                     uint16_t* __restrict__ out_h, float4* __restrict__ out_f) {
    __shared__ float steps[8][IN_SCATTERING_STEPS][8];
    const int half = threadIdx.x >> 5, sub = threadIdx.x & 31;
    const int texel = blockIdx.x * 8 + half;                      // rows 100..103 of the reference dispatch are discarded stores (S:281)
    const bool live = texel < w * h;
    const int px = live ? texel % w : 0, py = live ? texel / w : 0;
    sky_texel<TLUT>(steps[half], sub, live, px, py, w, h, sun, trans, tw, th, [=](int x, int y, uint16_t hx, uint16_t hy, uint16_t hz, uint16_t hw) {
        reinterpret_cast<uint2*>(out_h)[y * w + x] = pack_half4(hx, hy, hz, hw);
        out_f[y * w + x] = make_float4(h2f(hx), h2f(hy), h2f(hz), h2f(hw));
    });
}
// One rank's rows of the LUT when N ranks / devices split a frame: rows row0, row0 + row_stride, ... (n_rows of them).  out_f == nullptr
// (csky_render_sky_lut_rows_device): stored COMPACT and as RGBA16F only, straight into the buffer that travels to the gathering rank with the
// rank's bands.  out_f != nullptr (csky_multi_render_sky_lut): stored at the texel's own place in the whole LUT (half + float copies) of the
// handle's first device, over xGMI peer access, like the frame's bands.
template <int TLUT> __global__ __launch_bounds__(256) void sky_lut_rows_kernel(int w, int h, int row0, int row_stride, int n_rows, Sun3 sun, const float4* __restrict__ trans,
                                                          int tw, int th, uint2* __restrict__ out_h, float4* __restrict__ out_f) {
    __shared__ float steps[8][IN_SCATTERING_STEPS][8];
    const int half = threadIdx.x >> 5, sub = threadIdx.x & 31;
    const int t = blockIdx.x * 8 + half;
    const bool live = t < w * n_rows;
    const int px = live ? t % w : 0, py = live ? row0 + (t / w) * row_stride : 0;
    sky_texel<TLUT>(steps[half], sub, live, px, py, w, h, sun, trans, tw, th, [=](int x, int y, uint16_t hx, uint16_t hy, uint16_t hz, uint16_t hw) {
        if (out_f) { out_h[y * w + x] = pack_half4(hx, hy, hz, hw); out_f[y * w + x] = make_float4(h2f(hx), h2f(hy), h2f(hz), h2f(hw)); }
        else out_h[t] = pack_half4(hx, hy, hz, hw);
    });
}

hipError_t launch_transmittance(int w, int h, uint16_t* d_half, float4* d_float, hipStream_t s, int tlut) {
    with_tlut(tlut, [&](auto m) { transmittance_kernel<decltype(m)::value><<<(w * h + 3) / 4, 256, 0, s>>>(w, h, d_half, d_float); });
    return hipGetLastError();
}
hipError_t launch_sky_lut(int w, int h, const float sun[3], const float4* d_trans, int tw, int th, uint16_t* d_half, float4* d_float,
                          hipStream_t s, int tlut) {
    with_tlut(tlut, [&](auto m) { sky_lut_kernel<decltype(m)::value><<<(w * h + 7) / 8, 256, 0, s>>>(w, h, Sun3(sun), d_trans, tw, th, d_half, d_float); });
    return hipGetLastError();
}
hipError_t launch_sky_lut_rows(int w, int h, int row0, int row_stride, const float sun[3], const float4* d_trans, int tw, int th, uint2* d_rows, float4* d_whole_f,
                               hipStream_t s, int tlut) {
    const int n_rows = row0 < h ? (h - row0 + row_stride - 1) / row_stride : 0;
    if (n_rows) with_tlut(tlut, [&](auto m) {
        sky_lut_rows_kernel<decltype(m)::value><<<(w * n_rows + 7) / 8, 256, 0, s>>>(w, h, row0, row_stride, n_rows, Sun3(sun), d_trans, tw, th, d_rows, d_whole_f);
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ compositor
// clouds.gdshader sky() on an equirectangular panorama, one pixel per lane
template <int TLUT> __global__ __launch_bounds__(256) void composite_kernel(CompositeArgs A, uint2* __restrict__ out) {
    const int i = blockIdx.x * 32 + (threadIdx.x & 31), j = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (i >= A.out_w || j >= A.out_h) return;
    const C3 c = composite_pixel<TLUT>(A, i, j);
    out[(size_t)j * A.out_w + i] = pack_half4(f2h(c.x), f2h(c.y), f2h(c.z), f2h(1.0f));
}
hipError_t launch_composite(const CompositeArgs& a, uint2* d_out, hipStream_t s, int tlut) {
    with_tlut(tlut, [&](auto m) { composite_kernel<decltype(m)::value><<<dim3((a.out_w + 31) / 32, (a.out_h + 7) / 8), 256, 0, s>>>(a, d_out); });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ frame set-up
// what frame_setup leaves to the caller that knows the weather map and the context's switches, and the store
__device__ __forceinline__ void store_frame_consts(FrameConsts& fc, const SetupArgs& a, FrameConsts* __restrict__ out) {
    fc.ct_mode = a.ct_mode;
    if (!a.sat_skip) fc.sat_skip = 0;
    *out = fc;
}
__global__ __launch_bounds__(64) void frame_setup_kernel(CloudParams p, const float4* __restrict__ sky, int sw, int sh, SetupArgs a, FrameConsts* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        FrameConsts fc;
        frame_setup(p, sky, sw, sh, a.primary_steps, a.light_steps, a.early_eps, a.hf_lo, a.hf_hi, fc);
        store_frame_consts(fc, a, out);
    }
}
hipError_t launch_frame_setup(const CloudParams& p, const float4* d_sky, int sw, int sh, const SetupArgs& a, FrameConsts* d_fc, hipStream_t s) {
    frame_setup_kernel<<<1, 64, 0, s>>>(p, d_sky, sw, sh, a, d_fc);
    return hipGetLastError();
}
// The same for a context that holds no sky LUT of its own (one rank of an N-way frame split renders only its rows of it, straight into the
// gather buffer): the <= 12 texels the three taps of clouds.glsl:163-167 filter are rendered here first, one per half wavefront with the
// per-texel code of sky_lut_kernel (fp16-rounded like the stored LUT), parked in LDS, and lane 0 runs the set-up on them.  The cell
// arithmetic is sky_lut_cell's in both places, so every texel the set-up asks for is one rendered here: the constants are bit-identical to
// those filtered from a whole LUT.
template <int TLUT> __global__ __launch_bounds__(384) void frame_setup_taps_kernel(CloudParams p, Sun3 sun, SetupArgs a, const float4* __restrict__ trans, int tw, int th, int sw, int sh,
                                                              FrameConsts* __restrict__ out) {
    __shared__ float steps[12][IN_SCATTERING_STEPS][8];
    __shared__ float4 texel[12];
    const int k = threadIdx.x >> 5, sub = threadIdx.x & 31;      // texel k: corner k % 4 of tap k / 4
    float sx, sy, ax, ay; int x0, x1, y0, y1;
    frame_setup_tap_uv(p.LIGHT_DIRECTION, k >> 2, sx, sy);
    sky_lut_cell(sw, sh, sx, sy, x0, x1, y0, y1, ax, ay);
    sky_texel<TLUT>(steps[k], sub, true, (k & 1) ? x1 : x0, (k & 2) ? y1 : y0, sw, sh, sun, trans, tw, th, [&](int, int, uint16_t hx, uint16_t hy, uint16_t hz, uint16_t hw) {
        texel[k] = make_float4(h2f(hx), h2f(hy), h2f(hz), h2f(hw));
    });
    __syncthreads();
    if (threadIdx.x == 0) {
        FrameConsts fc;
        frame_setup_f(p, [&](int tap, int corner, int, int) { return texel[tap * 4 + corner]; }, sw, sh, a.primary_steps, a.light_steps, a.early_eps, a.hf_lo, a.hf_hi, fc);
        store_frame_consts(fc, a, out);
    }
}
hipError_t launch_frame_setup_taps(const CloudParams& p, const float sun[3], const float4* d_trans, int tw, int th, int sw, int sh, const SetupArgs& a, FrameConsts* d_fc,
                                   hipStream_t s, int tlut) {
    with_tlut(tlut, [&](auto m) { frame_setup_taps_kernel<decltype(m)::value><<<1, 384, 0, s>>>(p, Sun3(sun), a, d_trans, tw, th, sw, sh, d_fc); });
    return hipGetLastError();
}

}  // namespace csky
