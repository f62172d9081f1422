// primitives_core.h -- TEST HOOK: the march's arithmetic primitives, one element per lane, for csky_test_primitive (cloudsky_internal.h).
//
// The suite checks the per-lane cores on the host (tests/hostsim) and the kernels against the host build, but on the host every function below
// takes its `#else` branch: libm's sqrtf / floorf / fmaf, 1.0f / x, the software f2h.  On the device they are other instructions, several of them
// hand-written (v_sqrt_f32 + neighbour residuals, v_cvt_flr_i32_f32 + v_fract_f32, v_fma_mix_f32 with op_sel, v_cvt_f16_f32, raw v_rcp / v_exp /
// v_log).  prim_apply<OP> calls THE SAME inline functions the march calls (cloud_core.h, radiance_core.h; no copies), so that
//   primitives.hip        runs the device branches over arrays (tests/test_gpu_primitives.py: bit equality or an ulp gate against numpy), and
//   tests/hostsim         runs the host branches over the same arrays (tests/test_primitives_host.py: the definitions the comments appeal to).
// Arrays are 32-bit words (float or uint32 by op); prim_shape gives the words per element of each: 0 = the array is not used.
#pragma once
#include "cloud_core.h"
#include "radiance_core.h"

namespace csky {

enum PrimOp : int {
    PRIM_SQRT_EXACT = 0,   // in: x                      out: sqrt_exact(x)
    PRIM_SQRTF,            // in: x                      out: sqrtf(x) as Section A gets it from the compiler
    PRIM_DIV,              // in: a; b                   out: a / b as Section A gets it from the compiler
    PRIM_SPLIT_COORD,      // in: u                      out: i (int32); f
    PRIM_LERP_H,           // in: fp16 pair (uint32); f  out: lerp_h
    PRIM_LERP_H2,          // in: fp16 pair (uint32); f  out: lerp_h2
    PRIM_F2H_NORMAL,       // in: x                      out: the half's bits in a uint32
    PRIM_FAST_RCP, PRIM_FAST_EXP2, PRIM_FAST_LOG2, PRIM_FAST_EXP,   // in: x   out: f(x)
    PRIM_FAST_POW,         // in: x; y                   out: fast_pow(x, y)
    PRIM_RAD_RCP,          // in: x                      out: rad_rcp(x)
    PRIM_RAY,              // in: dx dy dz; steps (as a float)   out: Ray px py pz ss dx dy dz sx sy sz of ray_from_dir
    PRIM_PIXEL_DIR,        // in: i j (int32); tex_w tex_h       out: dx dy dz of pixel_dir
    PRIM_COUNT
};
struct PrimShape { int in[3], out[2]; };
CSKY_HD PrimShape prim_shape(int op) {
    switch (op) {
        case PRIM_DIV: case PRIM_LERP_H: case PRIM_LERP_H2: case PRIM_FAST_POW: return PrimShape{{1, 1, 0}, {1, 0}};
        case PRIM_SPLIT_COORD: return PrimShape{{1, 0, 0}, {1, 1}};
        case PRIM_RAY: return PrimShape{{3, 1, 0}, {10, 0}};
        case PRIM_PIXEL_DIR: return PrimShape{{2, 2, 0}, {3, 0}};
        default: return PrimShape{{1, 0, 0}, {1, 0}};
    }
}

CSKY_HD float prim_f(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
CSKY_HD uint32_t prim_u(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// the plain divide and square root of cloud_core.h's Section A (pixel_dir, intersect_sphere_cam, ray_from_dir), compiled as that section is
#pragma clang fp contract(off)
CSKY_HD float prim_div(float a, float b) { return a / b; }
CSKY_HD float prim_sqrtf(float x) { return sqrtf(x); }
#pragma clang fp contract(fast)

template <int OP>
CSKY_HD void prim_apply(const uint32_t* in0, const uint32_t* in1, const uint32_t* in2, uint32_t* out0, uint32_t* out1, size_t i) {
    (void)in1; (void)in2; (void)out1;
    if constexpr (OP == PRIM_SQRT_EXACT) out0[i] = prim_u(sqrt_exact(prim_f(in0[i])));
    else if constexpr (OP == PRIM_SQRTF) out0[i] = prim_u(prim_sqrtf(prim_f(in0[i])));
    else if constexpr (OP == PRIM_DIV) out0[i] = prim_u(prim_div(prim_f(in0[i]), prim_f(in1[i])));
    else if constexpr (OP == PRIM_SPLIT_COORD) { int k; float f; split_coord(prim_f(in0[i]), k, f); out0[i] = (uint32_t)k; out1[i] = prim_u(f); }
    else if constexpr (OP == PRIM_LERP_H) out0[i] = prim_u(lerp_h(in0[i], prim_f(in1[i])));
    else if constexpr (OP == PRIM_LERP_H2) out0[i] = prim_u(lerp_h2(in0[i], prim_f(in1[i])));
    else if constexpr (OP == PRIM_F2H_NORMAL) out0[i] = (uint32_t)f2h_normal(prim_f(in0[i]));
    else if constexpr (OP == PRIM_FAST_RCP) out0[i] = prim_u(fast_rcp(prim_f(in0[i])));
    else if constexpr (OP == PRIM_FAST_EXP2) out0[i] = prim_u(fast_exp2(prim_f(in0[i])));
    else if constexpr (OP == PRIM_FAST_LOG2) out0[i] = prim_u(fast_log2(prim_f(in0[i])));
    else if constexpr (OP == PRIM_FAST_EXP) out0[i] = prim_u(fast_exp(prim_f(in0[i])));
    else if constexpr (OP == PRIM_FAST_POW) out0[i] = prim_u(fast_pow(prim_f(in0[i]), prim_f(in1[i])));
    else if constexpr (OP == PRIM_RAD_RCP) out0[i] = prim_u(rad_rcp(prim_f(in0[i])));
    else if constexpr (OP == PRIM_RAY) {
        FrameConsts fc = {};
        fc.steps_f = prim_f(in1[i]);                               // the one field ray_from_dir reads
        const Ray r = ray_from_dir(fc, prim_f(in0[3 * i]), prim_f(in0[3 * i + 1]), prim_f(in0[3 * i + 2]));
        const float v[10] = {r.px, r.py, r.pz, r.ss, r.dx, r.dy, r.dz, r.sx, r.sy, r.sz};
        for (int k = 0; k < 10; k++) out0[10 * i + k] = prim_u(v[k]);
    } else {
        static_assert(OP == PRIM_PIXEL_DIR, "unknown primitive");
        float dx, dy, dz;
        pixel_dir(prim_f(in1[2 * i]), prim_f(in1[2 * i + 1]), (int)in0[2 * i], (int)in0[2 * i + 1], dx, dy, dz);
        out0[3 * i] = prim_u(dx); out0[3 * i + 1] = prim_u(dy); out0[3 * i + 2] = prim_u(dz);
    }
}

// run-time op -> prim_apply<op> over i in [begin, end): the host build's loop (the device launches one lane per element, primitives.hip)
template <int OP = 0>
CSKY_HD bool prim_apply_range(int op, const uint32_t* in0, const uint32_t* in1, const uint32_t* in2, uint32_t* out0, uint32_t* out1, size_t begin, size_t end) {
    if constexpr (OP < PRIM_COUNT) {
        if (op != OP) return prim_apply_range<OP + 1>(op, in0, in1, in2, out0, out1, begin, end);
        for (size_t i = begin; i < end; i++) prim_apply<OP>(in0, in1, in2, out0, out1, i);
        return true;
    } else {
        return false;
    }
}

}  // namespace csky
