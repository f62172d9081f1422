// primitives.hip -- TEST HOOKS (csky_test_primitive, csky_test_sqrt_shell): the march's arithmetic primitives over arrays, one element per lane.
// A translation unit of its own, built with the flags of every other one (Makefile CXXFLAGS), so that the product kernels' code cannot change with
// it: it includes the headers the march includes and calls their inline functions (primitives_core.h::prim_apply, cloud_core.h::sqrt_shell).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "primitives_core.h"
#pragma clang fp contract(off)   // for the code of this file, whatever the last header left (the cores state their own)

namespace csky {

template <int OP>
__global__ __launch_bounds__(256) void primitive_kernel(const uint32_t* __restrict__ in0, const uint32_t* __restrict__ in1, const uint32_t* __restrict__ in2,
                                                        uint32_t* __restrict__ out0, uint32_t* __restrict__ out1, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) prim_apply<OP>(in0, in1, in2, out0, out1, i);
}

template <int OP = 0>
static hipError_t launch_primitive_op(int op, const uint32_t* const in[3], uint32_t* const out[2], size_t n, hipStream_t s) {
    if constexpr (OP < PRIM_COUNT) {
        if (op != OP) return launch_primitive_op<OP + 1>(op, in, out, n, s);
        primitive_kernel<OP><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(in[0], in[1], in[2], out[0], out[1], n);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

hipError_t launch_primitive(int op, const uint32_t* const d_in[3], uint32_t* const d_out[2], size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return launch_primitive_op(op, d_in, d_out, n, s);
}

// test hook (csky_test_sqrt_shell): cloud_core.h::sqrt_shell over an array, for the exhaustive check against the host's sqrtf
__global__ __launch_bounds__(256) void sqrt_shell_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sqrt_shell(in[i]);
}
hipError_t launch_sqrt_shell(const float* d_in, float* d_out, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    sqrt_shell_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_in, d_out, n);
    return hipGetLastError();
}

}  // namespace csky
