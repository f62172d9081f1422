// kernels.h -- host-callable launchers of the gfx950 kernels, headed by the file that holds them.  Internal to libcloudsky.
#pragma once
#include <hip/hip_runtime_api.h>
#include "csky_common.h"
#include "composite_core.h"
#include "noise_core.h"

namespace csky {

// f(the texture set a launch marches on, as its own type): *t32, the exact fp32-coefficient cells, when there is one, else t.  A generic lambda
// instantiates its kernel once per type; every launcher that takes (t, t32) and runs the same kernel on either goes through here.
template <class F> inline void with_texset(const TexSet& t, const TexSet32* t32, F&& f) { if (t32) f(*t32); else f(t); }

// ------------------------------------------------------------------------------------------------ lut_kernels.hip
// transmittance-lut.glsl main(): writes the RGBA16F image and a float4 copy of the fp16-ROUNDED values
// (what a sampler would read back), so later kernels sample floats without per-tap half unpacking.
// `tlut` (here and below): the parametrization the table is written / read in, tlut_core.h (0 = the reference's, 1 = Bruneton's)
hipError_t launch_transmittance(int w, int h, uint16_t* d_half, float4* d_float, hipStream_t s, int tlut = 0);
// sky-lut.glsl main()
hipError_t launch_sky_lut(int w, int h, const float sun[3], const float4* d_trans, int tw, int th, uint16_t* d_half,
                          float4* d_float, hipStream_t s, int tlut = 0);
// rows row0, row0 + row_stride, ... of that LUT (one rank / device of an N-way frame split): d_whole_f == nullptr: compact RGBA16F into d_rows;
// otherwise at their own place in the whole LUT d_rows (RGBA16F) + d_whole_f (the float copy)
hipError_t launch_sky_lut_rows(int w, int h, int row0, int row_stride, const float sun[3], const float4* d_trans, int tw, int th, uint2* d_rows, float4* d_whole_f,
                               hipStream_t s, int tlut = 0);
// clouds.gdshader sky() on an equirectangular panorama (all pointers in `a` are device pointers)
hipError_t launch_composite(const CompositeArgs& a, uint2* d_out, hipStream_t s, int tlut = 0);
// What the frame set-up takes from its caller besides the push constants and the sky LUT (clouds_launch.cpp::clouds_dev fills it; a kernel argument)
struct SetupArgs {
    int primary_steps, light_steps;   // clouds.glsl:228, :186
    float early_eps, hf_lo, hf_hi;    // FrameConsts::early_eps; the height window of the exact reject (bake.h height_window)
    int ct_mode, sat_skip;            // FrameConsts::ct_mode; sat_skip 0: the saturation skip stays off whatever the constants allow
};
// per-frame constants of clouds.glsl:143-170 (one wave)
hipError_t launch_frame_setup(const CloudParams& p, const float4* d_sky, int sw, int sh, const SetupArgs& a, FrameConsts* d_fc, hipStream_t s);
// the same without a sky LUT in memory: renders the <= 12 texels the set-up filters itself (sw x sh LUT of the sun `sun`)
hipError_t launch_frame_setup_taps(const CloudParams& p, const float sun[3], const float4* d_trans, int tw, int th, int sw, int sh, const SetupArgs& a, FrameConsts* d_fc,
                                   hipStream_t s, int tlut = 0);

// ------------------------------------------------------------------------------------------------ bake_kernels.hip
// stand-in shape noise bake: n^3 RGBA8 voxels (little-endian u32 = r | g<<8 | b<<16 | a<<24)
hipError_t launch_shape_noise(uint32_t seed, int n, const ShapeNoiseParams& P, uint32_t* d_out, hipStream_t s);
// generated 32^3 RGB detail volume (noise_core.h::detail_voxel), 3 bytes per voxel
hipError_t launch_detail_noise(uint32_t seed, int n, uint8_t* d_out, hipStream_t s);
// generated 512 x 512 RGB8 weather map (noise_core.h::weather_texel), 3 bytes per texel, texel (x, y) at byte (y * 512 + x) * 3
hipError_t launch_weather_noise(uint32_t seed, const WeatherNoiseParams& P, uint8_t* d_out, hipStream_t s);
// 2x2x2 box mips of a device chain whose level 0 is filled (level l at chain_offset(n, l, ch))
hipError_t launch_mip_chain(uint8_t* d_chain, int n, int ch, int levels, hipStream_t s);
// the three device texture layouts from the 8-bit chains; *d_inexact += coefficients not exact in fp16; d_range = {min R, max R, max B} of the
// weather map (initialise to {255, 0, 0})
hipError_t launch_bake(const uint8_t* d_large_chain, const uint8_t* d_small_chain, const uint8_t* d_weather, ShapeTexel* d_shape, uint4* d_detail, uint16_t* d_detail_h,
                       uint4* d_weather_out, unsigned long long* d_inexact, int* d_range, hipStream_t s);
// exact cells (bake_core.h): fp32-coefficient layouts of the same three textures
hipError_t launch_bake32(const uint8_t* d_large_chain, const uint8_t* d_small_chain, const uint8_t* d_weather, float4* d_shape32, float4* d_detail32, float4* d_weather32, hipStream_t s);

// the weather map's share of the two above alone (csky_set_weather*): the same kernels, the same counters (its cells never add to *d_inexact)
hipError_t launch_bake_weather(const uint8_t* d_weather, uint4* d_weather_out, unsigned long long* d_inexact, int* d_range, hipStream_t s);
hipError_t launch_bake_weather32(const uint8_t* d_weather, float4* d_weather32, hipStream_t s);

// ------------------------------------------------------------------------------------------------ cloud_kernels.hip
// clouds.glsl main() over the rows described by `g`.  d_stats (may be null): [0] += in-cloud samples,
// [1] += rays above the horizon.  With neither d_stats nor d_wg_cost the whole-ray compact kernel (variant 3, seg 1, fp16-pair cells) runs without its
// in-cloud tally and stops marching a ray once its stored pixel is final (march_compact.h march_compact, TALLY = false); the frame is the same.
// census_lean: launch that form although d_stats is given (csky_census_clouds: the census build's block counters are the buffer's only writers then).
// seg = ray segments per ray (1, 2 or 4; variant 1 only): a workgroup covers 4/seg tiles of 8x8 pixels.
// d_order[grid]: physical workgroup -> workgroup-footprint id (0xffffffff = idle), see clouds_launch.cpp::clouds_dev.
hipError_t launch_clouds(int variant, int seg, const TexSet& t, const FrameConsts* d_fc, const RenderGeom& g, const uint32_t* d_order, int grid,
                         uint2* d_out, unsigned long long* d_stats, uint32_t* d_wg_cost, hipStream_t s, uint32_t* d_heads = nullptr, int resident = 0,
                         const TexSet32* t32 = nullptr, bool census_lean = false,    // t32: march on the exact fp32-coefficient cells (variant 3, seg 1 only)
                         int ct_mode = 0,    // the SetupArgs::ct_mode *d_fc was set up with: a persistent launch runs the march compiled for that mode (0: the generic one)
                         int resident_slim = 0);   // `resident` of the specialised persistent forms without a tally (0: `resident`)
// resident 256-thread workgroups per CU of the "compact" kernel (its launch bound): the size of a persistent launch
int cloud_resident_workgroups_per_cu();
// the same for the persistent forms with a compiled-in cloud-type mode and no tally, asked of the runtime for the current device (at most their launch bound)
int cloud_resident_workgroups_per_cu_slim();
int cloud_variant_count();
const char* cloud_variant_name(int v);

// ------------------------------------------------------------------------------------------------ order_kernels.hip
// next launch's workgroup order from this launch's per-workgroup costs, heaviest first.  d_cost[n] and d_scratch[2048] must be zero
// before their first use and are left zeroed (the cloud kernel accumulates the next costs into d_cost).
hipError_t launch_lpt_order(uint32_t* d_cost, int n, int shift, uint32_t* d_scratch, uint32_t* d_order, hipStream_t s);
// static workgroup orders 1, 2, 5 written on the device; grid = padded number of physical workgroups
hipError_t launch_static_order(int mode, int tiles_x, int slabs, int grid, uint32_t* d_order, hipStream_t s);
// frame band k (band_bytes each, total_bands of them) = member k % members, local band k / members of a gathered rank-major buffer
hipError_t launch_interleave_bands(const void* d_gathered, size_t member_stride_bytes, int members, size_t band_bytes, int total_bands, void* d_frame, hipStream_t s);

// ------------------------------------------------------------------------------------------------ cloud_kernels.hip, the direct march
// the direct march (rays_core.h): g.w x g.h RGBA16F texels into d_out, row pitch g.pitch_px pixels, for the directions of d_dirs ([h][w][3] floats),
// or for the view of g when d_dirs is null.  d_fc: the cloud frame's own frame constants (launch_frame_setup*).  t32: march on the exact
// fp32-coefficient cells.  A plain launch in natural order; g travels as a kernel argument.
struct RaysGeom;
hipError_t launch_clouds_rays(const TexSet& t, const TexSet32* t32, const FrameConsts* d_fc, const RaysGeom& g, const float* d_dirs, uint2* d_out, hipStream_t s);
// the temporal split of a view frame (view_update_core.h): the fresh pixels of g's phase over their sub-grid (no launch where the image has none), then
// every other pixel of the g.w x g.h image from d_prev (row pitch g.prev_pitch_px pixels; NULL exactly when g.has_history is 0) or, where that frame
// has none, by the march; no second launch for g.block 1.  The two launches write disjoint texels of d_out.  g travels as a kernel argument.
struct ViewUpdateGeom;
hipError_t launch_clouds_view_update(const TexSet& t, const TexSet32* t32, const FrameConsts* d_fc, const ViewUpdateGeom& g, const uint2* d_prev, uint2* d_out, hipStream_t s);
// the direct march from an observer's position (observer_core.h): launch_clouds_rays for the rays of g.g seen from g.o, each ray's first segment
// through the layer capped at g.max_dist.  g travels as a kernel argument.
struct ObserverGeom;
hipError_t launch_clouds_observer(const TexSet& t, const TexSet32* t32, const FrameConsts* d_fc, const ObserverGeom& g, const float* d_dirs, uint2* d_out, hipStream_t s);
// the same behind a per-pixel scene depth (scene_depth_core.h): each ray also ends at its pixel's texel of d_depth (g.og.g.h rows of g.og.g.w floats,
// g.depth_pitch floats apart, metres along the ray or, g.kind DEPTH_VIEW_Z and a view only, along the camera's forward axis).  d_depth does not
// overlap d_out.  g travels as a kernel argument.
struct SceneDepthGeom;
hipError_t launch_clouds_observer_depth(const TexSet& t, const TexSet32* t32, const FrameConsts* d_fc, const SceneDepthGeom& g, const float* d_dirs, const float* d_depth,
                                        uint2* d_out, hipStream_t s);

// ------------------------------------------------------------------------------------------------ shadow.hip
// the cloud shadow map (shadow_core.h): sc.w x sc.h halfs into d_out, row pitch sc.pitch_h halfs.  fc: shadow_frame_consts; both blocks travel as
// kernel arguments.  t32: march on the exact fp32-coefficient cells.
struct ShadowConsts;
hipError_t launch_cloud_shadow(const TexSet& t, const TexSet32* t32, const FrameConsts& fc, const ShadowConsts& sc, uint16_t* d_out, hipStream_t s);

// ------------------------------------------------------------------------------------------------ aerial.hip
// the aerial-perspective volume (aerial_core.h): g.d slices of g.h x g.w RGBA16F texels into d_out, tightly packed; g travels as a kernel argument
struct AerialGeom;
hipError_t launch_aerial(const AerialGeom& g, const float4* d_trans, int tw, int th, uint2* d_out, hipStream_t s, int tlut = 0);

// ------------------------------------------------------------------------------------------------ shafts.hip
// the same volume with the cloud shadow map m inside it (shafts_core.h): m.texels is a device pointer, read on s; g and m travel as kernel arguments
struct ShaftsMap;
hipError_t launch_shafts(const AerialGeom& g, const ShaftsMap& m, const float4* d_trans, int tw, int th, uint2* d_out, hipStream_t s, int tlut = 0);

// ------------------------------------------------------------------------------------------------ depth.hip
// the cloud depth frame (depth_core.h): dc.w x dc.h RGBA16F texels into d_out, row pitch dc.pitch_px pixels.  fc: depth_frame_consts; both blocks
// travel as kernel arguments.  t32: march on the exact fp32-coefficient cells.
struct DepthConsts;
hipError_t launch_cloud_depth(const TexSet& t, const TexSet32* t32, const FrameConsts& fc, const DepthConsts& dc, uint2* d_out, hipStream_t s);
// the depth frame of a ray frame (view_depth_core.h): the same texels for the directions of d_dirs ([h][w][3] floats, tightly packed), or for the
// view of g (g.w x g.h = dc.w x dc.h) when d_dirs is null.  All three blocks travel as kernel arguments.
hipError_t launch_cloud_depth_rays(const TexSet& t, const TexSet32* t32, const FrameConsts& fc, const DepthConsts& dc, const RaysGeom& g, const float* d_dirs,
                                   uint2* d_out, hipStream_t s);

// ------------------------------------------------------------------------------------------------ cloud_aerial.hip
// the air in front of a cloud frame (cloud_aerial_core.h): g.w x g.h RGBA16F texels of d_cloud, placed by d_depth, into d_out, all tightly packed;
// d_out may be d_cloud.  g travels as a kernel argument
struct CloudAerialGeom;
hipError_t launch_cloud_aerial(const CloudAerialGeom& g, const float4* d_trans, int tw, int th, const uint2* d_cloud, const uint2* d_depth, uint2* d_out,
                               hipStream_t s, int tlut = 0);
// the same step on a ray frame (view_depth_core.h): every pixel's direction from d_dirs ([h][w][3] floats, tightly packed), or from the view of rg
// (rg.w x rg.h = g.w x g.h) when d_dirs is null
hipError_t launch_cloud_aerial_rays(const CloudAerialGeom& g, const RaysGeom& rg, const float* d_dirs, const float4* d_trans, int tw, int th, const uint2* d_cloud,
                                    const uint2* d_depth, uint2* d_out, hipStream_t s, int tlut = 0);

// ------------------------------------------------------------------------------------------------ bc7enc.hip
// BC7 (BPTC) blocks of n_img images of w x h RGBA8 texels (what compress/mode=2 of the *.import files asks the importer for)
hipError_t launch_bc7_encode(const uint8_t* d_img, int w, int h, int n_img, int quality, uint4* d_blocks, hipStream_t s);

// ------------------------------------------------------------------------------------------------ radiance.hip
// radiance cubemap (radiance_core.h): source records of an ns x ns cube from the n x n layer 0 (RGBA16F, device), the bounding
// cones of the 8x8 blocks of an n x n cube, and nl >= 1 prefiltered layers (ly[0..nl)) written back to back from d_out
struct RadLayer;
hipError_t launch_radiance_source(const uint16_t* d_layer0, int n, int ns, float4* d_tab, hipStream_t s);
hipError_t launch_radiance_cones(int n, float4* d_cones, hipStream_t s);
hipError_t launch_radiance_filter(const float4* d_tab, const float4* d_src_cones, const float4* d_out_cones, int n, int ns, const RadLayer* ly, int nl, bool cull,
                                  uint2* d_out, hipStream_t s);

// ------------------------------------------------------------------------------------------------ primitives.hip
// test hook: primitive `op` (primitives_core.h PrimOp) over n elements, one per lane.  d_in / d_out: prim_shape(op) words per element each; an
// array the op does not use may be null.
hipError_t launch_primitive(int op, const uint32_t* const d_in[3], uint32_t* const d_out[2], size_t n, hipStream_t s);
// test hook: cloud_core.h::sqrt_shell over an array
hipError_t launch_sqrt_shell(const float* d_in, float* d_out, size_t n, hipStream_t s);

}  // namespace csky
