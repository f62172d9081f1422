// order_kernels.hip -- what decides where and when a cloud launch's workgroups run, and what becomes of the bands they write.  None of it marches:
//
//   lpt_hist / lpt_scan / lpt_scatter_kernel, launch_lpt_order : the cost-feedback order (schedule mode 7)
//   static_order_kernel, launch_static_order                  : the static orders (modes 1, 2, 5), order_core.h::static_order_entry per workgroup
//   interleave_bands_kernel, launch_interleave_bands          : the band interleave of a gathered frame (N ranks split a frame)
//
// The kernels that consume an order are in cloud_kernels.hip; the host side is clouds_launch.cpp.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "order_core.h"
#pragma clang fp contract(off)   // for the code of this file, whatever the last header left (integer code today)

namespace csky {

// ---- cost-feedback schedule (clouds_launch.cpp, schedule mode 7) ------------------------------------------------------------
// Workgroups differ 10x in cost (in-cloud samples per tile) and a C3 frame is only ~4 waves of resident workgroups deep, so
// the order they start in decides the tail.  Every launch records a cost per workgroup (wg_cost: in-cloud samples + live rays);
// these three kernels turn it into the NEXT launch's order, heaviest first (longest-processing-time-first list scheduling;
// consecutive blocks land on consecutive XCDs, so each XCD also receives a descending sequence).  Counting sort on 1024 cost
// buckets; ties are placed in arrival order (the schedule may differ run to run, the frame cannot: every ray's arithmetic is
// independent of where and when its workgroup runs, tests/test_gpu_parity.py::test_variants_and_schedules_agree).
// (LPT_BUCKETS and lpt_bucket: order_core.h; bucket 0 = heaviest)
__global__ __launch_bounds__(256) void lpt_hist_kernel(const uint32_t* __restrict__ cost, int n, int shift, uint32_t* __restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&hist[lpt_bucket(cost[i], shift)], 1u);
}
__global__ __launch_bounds__(LPT_BUCKETS) void lpt_scan_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t sh[LPT_BUCKETS];                       // counts -> exclusive offsets; the histogram is left zeroed for the next launch
    const int t = threadIdx.x;
    const uint32_t own = hist[t];
    hist[t] = 0u;
    sh[t] = own;
    __syncthreads();
    for (int off = 1; off < LPT_BUCKETS; off <<= 1) {
        const uint32_t v = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    offsets[t] = sh[t] - own;
}
__global__ __launch_bounds__(256) void lpt_scatter_kernel(uint32_t* __restrict__ cost, int n, int shift, uint32_t* __restrict__ offsets,
                                                          uint32_t* __restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        order[atomicAdd(&offsets[lpt_bucket(cost[i], shift)], 1u)] = (uint32_t)i;
        cost[i] = 0u;                                          // the next launch accumulates into a clean array: no memset nodes per frame
    }
}
// d_cost[n] and d_scratch[2 * LPT_BUCKETS] must be zero before their first use (clouds_launch.cpp clears them at allocation); both are left zeroed
hipError_t launch_lpt_order(uint32_t* d_cost, int n, int shift, uint32_t* d_scratch, uint32_t* d_order, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    lpt_hist_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_cost, n, shift, d_scratch);
    lpt_scan_kernel<<<1, LPT_BUCKETS, 0, s>>>(d_scratch, d_scratch + LPT_BUCKETS);
    lpt_scatter_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_cost, n, shift, d_scratch + LPT_BUCKETS, d_order);
    return hipGetLastError();
}

// ---- static workgroup orders, generated on the device (clouds_launch.cpp::ensure_order) --------------------------------
// Physical workgroup b runs on XCD b % 8 (observed placement, used for speed only).  A "slab" is one 32 x 8 pixel workgroup
// footprint (bw x 8 for segmented launches); `grid` entries, 0xffffffff = idle padding.
// The entry of workgroup b in modes 1, 2 and 5 is order_core.h::static_order_entry, which the host tests walk too.
// Written by a kernel on the launch's own stream: no host table, no pageable copy, no device-wide synchronisation when the
// geometry changes (a 64-tile walk re-uses the table anyway: these orders depend on the launch geometry only).
__global__ __launch_bounds__(256) void static_order_kernel(int mode, int tiles_x, int slabs, int grid, uint32_t* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= grid) return;
    out[b] = static_order_entry(mode, tiles_x, slabs, b);
}
hipError_t launch_static_order(int mode, int tiles_x, int slabs, int grid, uint32_t* d_order, hipStream_t s) {
    if (grid <= 0) return hipSuccess;
    static_order_kernel<<<(grid + 255) / 256, 256, 0, s>>>(mode, tiles_x, slabs, grid, d_order);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ band interleave (gathering rank, N > 1)
// The gather leaves rank-major compact bands ([member][local band][rows]); the frame wants band k = member k % n, local band k / n.  A plain
// strided copy, deliberately on FEW workgroups: it is HBM-bound (32 MiB per 2048x1024 frame) beside marches that are not, so 48 workgroups
// streaming 16-byte chunks take it off the critical path instead of sweeping the whole chip for 15 us per frame (torch's permute + copy).
__global__ __launch_bounds__(256) void interleave_bands_kernel(const uint4* __restrict__ src, size_t member_stride16, int members, uint32_t band16, uint32_t total_bands,
                                                              uint4* __restrict__ dst) {
    const size_t total = (size_t)band16 * total_bands;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const uint32_t k = (uint32_t)(i / band16), c = (uint32_t)(i - (size_t)k * band16);
        dst[i] = src[(size_t)(k % members) * member_stride16 + (size_t)(k / members) * band16 + c];
    }
}
hipError_t launch_interleave_bands(const void* d_gathered, size_t member_stride_bytes, int members, size_t band_bytes, int total_bands, void* d_frame, hipStream_t s) {
    const size_t chunks = band_bytes / 16 * (size_t)total_bands;
    if (!chunks) return hipSuccess;
    const unsigned grid = (unsigned)(chunks / 256 + 1 < 48 ? chunks / 256 + 1 : 48);
    interleave_bands_kernel<<<grid, 256, 0, s>>>(reinterpret_cast<const uint4*>(d_gathered), member_stride_bytes / 16, members, (uint32_t)(band_bytes / 16), (uint32_t)total_bands,
                                                 reinterpret_cast<uint4*>(d_frame));
    return hipGetLastError();
}

}  // namespace csky
