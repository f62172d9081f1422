// order_core.h -- the index arithmetic of the launch orders: which workgroup footprint a physical workgroup renders.
//
// Shared, like lut_core.h and tlut_core.h, by the device (order_kernels.hip: static_order_kernel, the lpt_* kernels; cloud_kernels.hip: the pop loop of
// clouds_kernel_persistent), the host layer (clouds_launch.cpp: the grid of a static order, the bucket shift of the cost feedback) and
// tests/hostsim, which compiles it with g++ so that tests/test_launch_order.py checks every function here against a numpy restatement of
// what the orders MEAN, without a GPU.  No HIP, no state.
//
// A launch renders `nblocks = tiles_x * slabs` footprints, numbered row-major: logical = slab * tiles_x + bx.  An order is a table of
// `grid` entries, one per physical workgroup b, which runs on XCD b % 8 (observed placement, used for speed only); every logical number
// occurs exactly once, the other entries are ORDER_IDLE.
#pragma once
#include "csky_common.h"

namespace csky {

constexpr uint32_t ORDER_IDLE = 0xffffffffu;                  // an order entry without a footprint: the workgroup returns at once
constexpr int LPT_BUCKETS = 1024;                             // cost buckets of the feedback order's counting sort

// ---- static orders (modes 1, 2, 5) ---------------------------------------------------------------------------------------------
//   mode 2: natural order
//   mode 1: contiguous eighths of the launch per XCD
//   mode 5: slab ROWS dealt round-robin to the XCDs, every XCD walks its rows left to right: all XCDs see the same mix of
//           elevations and concurrently running workgroups are neighbours (shared cache lines)
// entries of the table = workgroups of the launch
CSKY_HD int static_order_grid(int mode, int tiles_x, int slabs) {
    const int nblocks = tiles_x * slabs;
    if (mode == 2) return nblocks;
    if (mode == 1) return ((nblocks + 7) >> 3) * 8;
    return ((slabs + 7) >> 3) * tiles_x * 8;
}
// the entry of physical workgroup b
CSKY_HD uint32_t static_order_entry(int mode, int tiles_x, int slabs, int b) {
    const int nblocks = tiles_x * slabs;
    uint32_t l = ORDER_IDLE;
    if (mode == 2) { if (b < nblocks) l = (uint32_t)b; }
    else if (mode == 1) { const int per = (nblocks + 7) >> 3, v = (b & 7) * per + (b >> 3); if ((b >> 3) < per && v < nblocks) l = (uint32_t)v; }
    else { const int x = b & 7, j = b >> 3, k = j / tiles_x, bx = j - k * tiles_x, i = 8 * k + x; if (i < slabs) l = (uint32_t)(i * tiles_x + bx); }
    return l;
}

// ---- cost-feedback order (mode 7) ----------------------------------------------------------------------------------------------
// bucket 0 = heaviest: the counting sort places the buckets in ascending order, so the heaviest workgroups start first
CSKY_HD int lpt_bucket(uint32_t cost, int shift) {
    const uint32_t b = cost >> shift;
    return LPT_BUCKETS - 1 - (int)(b > (uint32_t)(LPT_BUCKETS - 1) ? (uint32_t)(LPT_BUCKETS - 1) : b);
}
// the smallest shift that puts the largest cost of a workgroup, 4 wavefronts x 64 rays x (steps + 16), below LPT_BUCKETS
CSKY_HD int lpt_shift(int primary_steps) {
    int shift = 0;
    while ((((long long)256 * (primary_steps + 16)) >> shift) >= LPT_BUCKETS) shift++;
    return shift;
}

// ---- persistent form -----------------------------------------------------------------------------------------------------------
// The order of n_items entries is read as eight interleaved sequences: entry 8 j + y is the j-th of sequence y (XCD y's, the assignment
// the hardware's round-robin gives a plain launch).  Pop number j of sequence y -> the order index in `i`; false: the sequence is empty.
CSKY_HD bool persistent_pop_index(uint32_t j, uint32_t y, uint32_t n_items, uint32_t& i) {
    const uint32_t per_xcd = (n_items + 7u) >> 3;
    i = 8u * j + y;
    return j < per_xcd && i < n_items;
}

}  // namespace csky
