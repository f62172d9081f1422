// view_depth_host.cpp -- TEST TOOL ONLY.  Compiles the per-lane code of the depth frame and of the aerial step for view frames and ray frames
// (csrc/view_depth_core.h on depth_core.h, cloud_aerial_core.h and rays_core.h: what the lanes of depth_rays_kernel and cloud_aerial_rays_kernel
// run) for the HOST with g++, so that the `-m "not gpu"` suite can hold it to the hemisphere forms' host cores (tests/cloud_aerial_host) and to the
// numpy restatement of the definition without a GPU, and the GPU tests have a host core of the same rays to compare against.  It is NOT part of
// libcloudsky and is never a render fallback: the product has no CPU path.
#include <cstdint>
#include <cstring>
#include <cmath>
#include <vector>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/view_depth_core.h"
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/noise_set.h"

using namespace csky;

namespace {
// the view of a width x height image as the view forms' launches build it (api_depth.cpp, api_aerial.cpp)
RaysGeom view_geom(const float basis[9], float fov_y_degrees, int width, int height) { return rays_geom(basis, fov_y_degrees, width, height, (uint32_t)width); }
}  // namespace

extern "C" {

// The directions of a view as the view forms' lanes compute them: dirs [h][w][3].
void view_depth_host_view_dirs(const float basis[9], float fov_y_degrees, int width, int height, float* dirs) {
    const RaysGeom g = view_geom(basis, fov_y_degrees, width, height);
    for (int j = 0; j < height; j++) for (int i = 0; i < width; i++) {
        float* d = dirs + ((size_t)j * width + i) * 3;
        rays_view_dir(g, i, j, d[0], d[1], d[2]);
    }
}

// mip chains (level 0 first) -> baked fp16-pair layouts -> every texel of the depth frame of a width x height ray frame as depth_rays_kernel's lanes
// compute it (a wavefront of one lane).  dirs: [height][width][3] floats, or NULL for the view (basis, fov_y_degrees).  out_h: height rows of width
// texels of four halfs.  t0, ss (may be NULL): [height][width] floats, the ray's entry distance and step length (0 where the direction is not
// accepted).  incloud (may be NULL): [height][width], the in-cloud samples of every pixel.  taken (may be NULL): the lane-samples taken, summed over
// the frame.  Returns 0, or -1 for a size or step count out of range.
int view_depth_host_frame(const uint8_t* large_chain, const uint8_t* small_chain, const uint8_t* weather_rgb8, const float params[28], int width, int height,
                          int steps, int use_window, const float* dirs, const float basis[9], float fov_y_degrees, uint16_t* out_h, float* t0, float* ss,
                          uint32_t* incloud, uint64_t* taken) {
    if (steps < 1 || steps > 1024 || width < 1 || height < 1) return -1;
    std::vector<uint8_t> lc(large_chain, large_chain + RAW_SHAPE_CHAIN);
    std::vector<uint8_t> sc_(small_chain, small_chain + RAW_DETAIL_CHAIN);
    std::vector<ShapeTexel> shape; std::vector<uint4> detail, weather;
    uint32_t so[SHAPE_LEVELS], dof[DETAIL_LEVELS];
    bake_shape(lc, shape, so); bake_detail(sc_, detail, dof); bake_weather(weather_rgb8, weather);
    TexSet T;
    T.shape = shape.data(); T.detail = detail.data(); T.weather = weather.data(); T.sky = nullptr; T.sky_w = 0; T.sky_h = 0;
    T.detail_h = nullptr; T.detail_lds = nullptr;
    T.detail_lod5 = detail_lod5_value(sc_.data() + RAW_DETAIL_LOD5);
    CloudParams P; memcpy(&P, params, sizeof P);
    const ExactRejects rej = exact_rejects(weather_range(weather_rgb8), P.cloud_coverage, use_window != 0);   // like api_depth.cpp
    DepthConsts dc;
    dc.w = width; dc.h = height; dc.steps = steps; dc.pitch_px = (uint32_t)width;
    FrameConsts fc;
    depth_frame_consts(P, width, height, steps, rej.hf_lo, rej.hf_hi, rej.ct_mode, fc);
    RaysGeom g; memset(&g, 0, sizeof g);
    if (!dirs) g = view_geom(basis, fov_y_degrees, width, height);
    unsigned long long n = 0;
    for (int j = 0; j < height; j++) for (int i = 0; i < width; i++) {
        const size_t at = (size_t)j * width + i;
        float ex, ey, ez;
        if (dirs) { ex = dirs[at * 3]; ey = dirs[at * 3 + 1]; ez = dirs[at * 3 + 2]; }
        else rays_view_dir(g, i, j, ex, ey, ez);
        unsigned long long nin = 0;
        float a = 0.0f, b = 0.0f;
        const DepthTexel t = depth_dir(T, fc, dc, ex, ey, ez, true, &n, &nin, &a, &b);
        for (int c = 0; c < 4; c++) out_h[at * 4 + c] = t.h[c];
        if (t0) t0[at] = a;
        if (ss) ss[at] = b;
        if (incloud) incloud[at] = (uint32_t)nin;
    }
    if (taken) *taken = n;
    return 0;
}

// csky_apply_cloud_aerial_dirs / _view as cloud_aerial_rays_kernel's lanes compute it, from a tw x th transmittance LUT (RGBA16F) of `mapping`:
// cloud_h, depth_h and out_h are [height][width][4] halfs; out_h may be cloud_h.  dirs: [height][width][3] floats, or NULL for the view (basis,
// fov_y_degrees).  state (may be NULL): [height][width][8] floats, the spectral (L, Tr) in front of every pixel that does not pass (0 and 1 where it
// does).  worked (may be NULL): the number of pixels that did not pass.  Returns 0, or -1 for a size or step count out of range.
int view_depth_host_apply(int mapping, const uint16_t* trans_h, int tw, int th, int width, int height, int steps, const float sun[3], const float* dirs,
                          const float basis[9], float fov_y_degrees, const uint16_t* cloud_h, const uint16_t* depth_h, uint16_t* out_h, float* state,
                          uint64_t* worked) {
    if (width < 1 || height < 1 || steps < 1 || steps > 64) return -1;
    std::vector<float4> tf((size_t)tw * th);
    for (size_t i = 0; i < tf.size(); i++) tf[i] = float4{h2f(trans_h[4 * i]), h2f(trans_h[4 * i + 1]), h2f(trans_h[4 * i + 2]), h2f(trans_h[4 * i + 3])};
    CloudAerialGeom g;
    g.w = width; g.h = height; g.n = steps;
    for (int k = 0; k < 3; k++) g.sun[k] = sun[k];
    RaysGeom rg; memset(&rg, 0, sizeof rg);
    if (!dirs) rg = view_geom(basis, fov_y_degrees, width, height);
    uint64_t nw = 0;
    for (int j = 0; j < height; j++) for (int i = 0; i < width; i++) {
        const size_t px = (size_t)j * width + i, at = px * 4;
        float ex, ey, ez;
        if (dirs) { ex = dirs[px * 3]; ey = dirs[px * 3 + 1]; ez = dirs[px * 3 + 2]; }
        else rays_view_dir(rg, i, j, ex, ey, ez);
        uint2 c = pack_half4(cloud_h[at], cloud_h[at + 1], cloud_h[at + 2], cloud_h[at + 3]);
        const uint2 z = pack_half4(depth_h[at], depth_h[at + 1], depth_h[at + 2], depth_h[at + 3]);
        F4 L = f4(0, 0, 0, 0), Tr = f4(1, 1, 1, 1);
        if (!cloud_aerial_dir_passes(c, z, ex, ey, ez)) {
            nw++;
            c = mapping ? cloud_aerial_dir<TLUT_BRUNETON>(g, ex, ey, ez, c, z, tf.data(), tw, th) : cloud_aerial_dir<TLUT_REFERENCE>(g, ex, ey, ez, c, z, tf.data(), tw, th);
            if (state) {
                if (mapping) cloud_aerial_dir_column<TLUT_BRUNETON>(g, ex, ey, ez, z, tf.data(), tw, th, L, Tr);
                else cloud_aerial_dir_column<TLUT_REFERENCE>(g, ex, ey, ez, z, tf.data(), tw, th, L, Tr);
            }
        }
        if (state) { float* s = state + at * 2; s[0] = L.x; s[1] = L.y; s[2] = L.z; s[3] = L.w; s[4] = Tr.x; s[5] = Tr.y; s[6] = Tr.z; s[7] = Tr.w; }
        for (int k = 0; k < 4; k++) out_h[at + k] = half_of(c, k);
    }
    if (worked) *worked = nw;
    return 0;
}

}
