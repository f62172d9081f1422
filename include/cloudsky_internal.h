/*
 * cloudsky_internal.h -- the lab bench of libcloudsky.so: measurement, tuning and test entry points.
 *
 * Same library, same conventions as cloudsky.h, NOT part of the product surface: nothing here is needed to render, and some of it selects
 * kernels that are 2x slower than the default (kept for A/B).  Users: bench.py (kernel timing, the census), tests/ (texture read-back, the
 * exhaustive sqrt check, variants / schedules / segments as parity cases), tools/ (A/B scripts, the BC7 sensitivity study).  A Godot host
 * (gdext/cloudsky_gdextension.c) and a plain C client (tests/c_abi_check.c) compile against cloudsky.h alone.
 */
#ifndef CLOUDSKY_INTERNAL_H
#define CLOUDSKY_INTERNAL_H
#include "cloudsky.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement ---------------------------------------------------------------------------------
 * Times `iters` back-to-back launches of the cloud kernel alone with HIP events on the context's stream
 * (after `warmup` untimed launches) and returns the mean per-launch milliseconds.  Also fills the
 * sample counters of one launch (the kernel's own tallies).  The counters come from the FIRST, untimed launch, which is given the stats
 * buffer; the warm-up and timed launches are given none, like csky_render_clouds_device, and so run the kernel form that keeps no in-cloud
 * tally and stops marching a ray whose stored pixel is final.  The counts are exact (the full march's); the time is the headline path's. */
int csky_time_clouds(csky_ctx* ctx, const csky_cloud_params* p, int tile_w, const csky_bands* bands, int warmup,
                     int iters, float* mean_ms, csky_cloud_stats* stats);
int csky_get_cloud_stats(csky_ctx* ctx, csky_cloud_stats* stats); /* tallies of the last stats-enabled launch */
/* Per-launch timing of the cloud kernel inside the caller's own frame loop: while enabled, every csky_render_clouds* launch is
 * bracketed by a pair of HIP events recorded on the stream the kernel is launched on.  csky_get_kernel_ms waits for the launches
 * recorded since the last call (all of them: the event pool grows on demand), returns the sum of their durations and their
 * number, and resets. */
int csky_set_kernel_timing(csky_ctx* ctx, int enabled);
/* The multi-device handle's preconditions and, while csky_multi_set_timing is on, HIP-event timings of the LAST frame enqueued: per device the
 * march of its bands and (staged form) the peer copy of those bands into the first device's frame -- the "7 concurrent P2P copies" of SURVEY 8(e).
 * csky_multi_get_stats waits for the handle's work (csky_multi_sync).  march_ms / copy_ms: -1 = not measured; copy_ms 0 in the in-place form. */
#define CSKY_MULTI_STATS_MAX 16
typedef struct csky_multi_stats {
    int32_t n_devices, staged, all_peer, groups, frames_in_flight, timing;
    int32_t device_id[CSKY_MULTI_STATS_MAX];
    int32_t peer_access[CSKY_MULTI_STATS_MAX];   /* 1 = this device can store into the first device's memory (1 for the first device) */
    float march_ms[CSKY_MULTI_STATS_MAX];
    float copy_ms[CSKY_MULTI_STATS_MAX];
} csky_multi_stats;
int csky_multi_set_timing(csky_multi* m, int enabled);
int csky_multi_get_stats(csky_multi* m, csky_multi_stats* out);
int csky_get_kernel_ms(csky_ctx* ctx, float* total_ms, int* launches);
/* Kernel variant selector for A/B measurement (csky_variant_name lists them).  -1 = the default = the fastest measured
 * (CSKY_DEFAULT_VARIANT, "compact").  Unknown ids -> CSKY_ERR_INVALID. */
#define CSKY_DEFAULT_VARIANT 3
int csky_set_variant(csky_ctx* ctx, int variant);
/* The exact specialisations of the march, switched together: the height-window reject (density() provably 0 above/below the cloud
 * body for the bound weather map), the frame-wide cloud-type branch of the height gradient, and the saturation skip (whole-ray
 * "compact" marches leave out the light march of a ray whose stored RGBA16F pixel can no longer change: csrc/cloud_core.h
 * ray_saturated).  On by default; 0 disables all three (A/B measurement: identical frames and sample tallies). */
int csky_set_height_window(csky_ctx* ctx, int enabled);
int csky_variant_count(void);
/* Workgroup -> XCD schedule (tuning knob, results are identical): -1 = auto (see csrc/launch_policy.h for the launch-size policy);
 * 5 = slab rows round-robin over the XCDs; 1 = contiguous eighths; 2 = natural order (all three written on the device);
 * 7 = cost feedback: every launch records a cost per workgroup (in-cloud samples) and the next launch of the same geometry
 *     and view starts its workgroups heaviest first (the first launch runs in a static order);
 *     Only the ORDER comes from the previous launch; every sample is recomputed.
 * (0, 3, 4, 6 were azimuth-wedge / horizon-first orders of round 1; 8 / 9 the 'deadline' reorder and per-workgroup adaptive ray
 *  segments of round 2: all measured, no gain, removed -- docs/EXPERIMENTS.md section 5 keeps the numbers.) */
int csky_set_schedule(csky_ctx* ctx, int mode);
/* Ray segments: the primary march of every ray is cut into `segments` pieces marched by different wavefronts of one
 * workgroup and composited front to back (T and L are associative).  0 = auto (whole rays for large launches, 2 or 4
 * step ranges for one GPU's share of a split frame, 4 interleaved step sets for tile-sized launches such as the
 * reference's 96x96 temporal tiles), 1, 2, 4 (step ranges) or 5 (4 interleaved). */
int csky_set_segments(csky_ctx* ctx, int segments);
const char* csky_variant_name(int variant);

/* Test hook: read back what csky_set_noise built on the device.  which: 0 shape layout, 1 detail layout, 2 weather layout (csky_common.h),
 * 3 / 4 the 8-bit mip chains of the large / small volume, 5 the unpacked fp16 detail chain (one half per texel of all six levels, without the
 * allocation's 8-half pad), 6 / 7 / 8 the exact fp32 cells of shape / detail / weather (csrc/bake_core.h: 4 / 2 / 2 float4 per texel;
 * CSKY_ERR_STATE when the bound set has none: its textures fit fp16 and csky_set_exact_cells is 0), 9 what the context holds from the bake and
 * launches its kernels with, 24 bytes: uint64 inexact coefficients; int32 min R, max R, max B of the weather map; float detail LOD-5 value.
 * out may be NULL to query the size.  tests/test_gpu_bake.py compares all of them with tests/bake_reference.py. */
int csky_read_baked_texture(csky_ctx* ctx, int which, void* out, size_t capacity, size_t* bytes);
/* Test hook: the march's range-restricted exact square root (cloud_core.h::sqrt_shell, |p|^2 of sample positions) over an array, so that
 * a test can check it EXHAUSTIVELY against IEEE sqrtf on the range it is used on (all 30 067 floats in [3.597e13, 3.6097e13]). */
int csky_test_sqrt_shell(csky_ctx* ctx, const float* in, float* out, size_t n);
/* Test hook: one of the march's arithmetic primitives over arrays on the device, one element per lane, through the SAME inline functions the kernels
 * call (csrc/primitives_core.h, which also lists what every op reads and writes; csrc/primitives.hip, a translation unit of its own built with the
 * product's flags).  Arrays are 32-bit words, float or uint32 by op; an array the op does not use may be NULL; n <= 2^24; copies and the launch run
 * on the context's stream.  tests/test_gpu_primitives.py holds every op against numpy: bit equality for the exact ones, an ulp gate for the
 * hardware approximations.
 *    op  name          in0              in1            out0                                       out1
 *     0  sqrt_exact    x                               cloud_core.h::sqrt_exact
 *     1  sqrtf         x                               sqrtf(x) as Section A of cloud_core.h gets it
 *     2  div           a                b              a / b as Section A gets it (contraction off)
 *     3  split_coord   u                               i (int32)                                  f
 *     4  lerp_h        fp16 pair (u32)  f              a + f d
 *     5  lerp_h2       fp16 pair (u32)  f              lo + f (hi - lo), the two-step form
 *     6  f2h_normal    x                               the half's bits (uint32)
 *     7  fast_rcp   8  fast_exp2   9  fast_log2   10  fast_exp      x -> f(x)
 *    11  fast_pow      x                y              fast_pow(x, y)
 *    12  rad_rcp       x                               radiance_core.h::rad_rcp
 *    13  ray           [n][3] unit dir  steps (float)  [n][10] Ray px py pz ss dx dy dz sx sy sz of ray_from_dir
 *    14  pixel_dir     [n][2] i j (i32) [n][2] w h     [n][3] direction */
int csky_test_primitive(csky_ctx* ctx, int op, const void* in0, const void* in1, const void* in2, void* out0, void* out1, size_t n);
/* Test hooks of the launch orders (csrc/order_core.h; tests/test_gpu_launch_order.py compares both with the host's tables and with numpy).
 * csky_test_static_order: the table of workgroup order `mode` (1, 2 or 5) for a launch of tiles_x x slabs footprints, written by the kernel the
 * frame path runs, and in *grid its number of entries = the launch's workgroups.  table may be NULL to query the grid; capacity is in entries. */
int csky_test_static_order(csky_ctx* ctx, int mode, int tiles_x, int slabs, uint32_t* table, size_t capacity, int* grid);
/* csky_test_lpt_order: the cost-feedback sort over the caller's n costs with bucket shift `shift`, `rounds` times back to back on the same device
 * buffers, as consecutive frames run it: the costs are uploaded again before every round, the 2 * 1024 words of sort scratch are zeroed once, before
 * the first round.  Out: the order of the last round (n entries), the cost array as the kernels left it (n), the scratch words as left (2048). */
int csky_test_lpt_order(csky_ctx* ctx, const uint32_t* cost, int n, int shift, int rounds, uint32_t* order_out, uint32_t* cost_out, uint32_t* scratch_out);
/* Measurement hook of tools/isa_profile.py: one launch of the cloud kernel over `bands` with the statistics buffer bound, then the first n
 * (<= 256) 32-bit basic-block execution counters behind the kernel's own tallies.  The counters are written only by the CENSUS build of the
 * library (the product assembly with a counter per basic block, made by that tool); the product build leaves them zero. */
int csky_census_clouds(csky_ctx* ctx, const csky_cloud_params* p, int tile_w, const csky_bands* bands, uint32_t* counts, int n);

/* The other direction, on the GPU (bc7enc.hip, one block per lane): n_images images of w x h RGBA8 texels back to back -> per image
 * ceil(h/4) x ceil(w/4) blocks of 16 bytes, row-major (a 3-D texture is its slices: one image per slice, every mip level its own call, as the
 * importer stores them).  All eight modes (6; 0-3 for opaque blocks; 4, 5 and 7 for blocks whose alpha varies); principal-axis fit + least-squares refits, smallest
 * squared error wins.  It is NOT the engine's encoder (that one cannot be reproduced): textures passed through this and csky_decode_bc7 show the
 * SIZE of what compress/mode=2 does to a frame (tools/bc7_sensitivity.py), not the reference's exact texels. */
int csky_encode_bc7(csky_ctx* ctx, const uint8_t* rgba8, int w, int h, int n_images, uint8_t* blocks_out);
/* quality 0 = csky_encode_bc7; 1 = eight instead of four partitions fitted in full per multi-subset mode and, per subset, coordinate descent on the
 * stored end points (every channel of either end -2 .. +2 steps, indices searched again, until a sweep improves nothing): the second encoder of the
 * sensitivity study's error bar (profiles/r05/bc7_sensitivity.txt).  Frozen there: a sensitivity tool, not a product feature. */
int csky_encode_bc7_quality(csky_ctx* ctx, const uint8_t* rgba8, int w, int h, int n_images, int quality, uint8_t* blocks_out);

#ifdef __cplusplus
}
#endif
/* The switch and the launch counter of the sky LUT's reuse: declared in a header of their own, which every user of this one gets with it. */
#include "cloudsky_lut_hooks.h"
/* The A/B switch of the cloud shadow map's exact end, likewise. */
#include "cloudsky_shadow_hooks.h"
#endif /* CLOUDSKY_INTERNAL_H */
