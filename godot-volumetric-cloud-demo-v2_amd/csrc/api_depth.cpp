// api_depth.cpp -- the cloud depth frame's C ABI (csky_render_cloud_depth / _device; depth_core.h, depth.hip), and the same frame for
// the rays of a camera view or of a caller's buffer of directions (csky_render_cloud_depth_dirs / _view and their _device forms; view_depth_core.h;
// DESIGN.md §18).
// The call reads the bound noise and the push-constant block and nothing else: no LUT, no slot of the cloud frames' constants ring (both constant
// blocks of a launch are computed here and travel as kernel arguments), no stream of its own; the blocking form works in the stage (host_stage.h).
#include <cmath>
#include <cstring>
#include "context.h"
#include "depth_core.h"
#include "view_depth_core.h"

using namespace csky;

namespace {

// The argument and state checks of both forms.  fn: the entry point's name for the error text.
int depth_check(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_depth_params* dp, size_t pitch_bytes) {
    if (!p || !dp) return fail(c, CSKY_ERR_INVALID, "%s: NULL argument", fn);
    if (dp->width < 1 || dp->width > 8192 || dp->height < 1 || dp->height > 8192) return fail(c, CSKY_ERR_INVALID, "%s: width and height must be in [1, 8192]", fn);
    if (dp->steps < 0 || dp->steps > 1024) return fail(c, CSKY_ERR_INVALID, "%s: steps must be in [1, 1024], or 0 for the context's primary step count", fn);
    CloudParams cp; memcpy(&cp, p, sizeof cp);
    const float read[] = {cp.cloud_pos[0], cp.cloud_pos[1], cp.detailed_pos[0], cp.detailed_pos[1], cp.weather_pos[0], cp.weather_pos[1], cp.time, cp.density, cp.cloud_coverage};
    for (float v : read) if (!std::isfinite(v)) return fail(c, CSKY_ERR_INVALID, "%s: a push-constant field the depth frame reads is not finite", fn);
    if (pitch_bytes < (size_t)dp->width * 8 || pitch_bytes % 8) return fail(c, CSKY_ERR_INVALID, "%s: row pitch must be a multiple of 8 and >= 8 * width", fn);
    if (!c->noise.st.have()) return fail(c, CSKY_ERR_STATE, "%s: csky_set_noise has not been called", fn);
    return CSKY_OK;
}

// The launch on stream s, for arguments depth_check has passed: the rays of `view`, or of d_dirs, or the frame's own when both are NULL.
int depth_launch(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_depth_params* dp, uint2* d_out, size_t pitch_bytes, hipStream_t s,
                 const csky_view* view = nullptr, const float* d_dirs = nullptr) {
    CloudParams cp; memcpy(&cp, p, sizeof cp);
    const ExactRejects rej = c->noise.st.rejects(cp.cloud_coverage, c->use_window);   // the height window and the cloud-type branch, as the cloud march gets them
    DepthConsts dc;
    dc.w = dp->width; dc.h = dp->height; dc.steps = dp->steps == 0 ? c->primary_steps : dp->steps; dc.pitch_px = (uint32_t)(pitch_bytes / 8);
    FrameConsts fc;
    depth_frame_consts(cp, dc.w, dc.h, dc.steps, rej.hf_lo, rej.hf_hi, rej.ct_mode, fc);
    TexSet32 t32;
    if (!view && !d_dirs) return launched(c, fn, launch_cloud_depth(texset(c), texset32_if(c, t32), fc, dc, d_out, s));
    const RaysGeom g = rays_geom(view ? view->basis : nullptr, view ? view->fov_y_degrees : 0.0f, dc.w, dc.h, dc.pitch_px);   // as csky_render_clouds_view's
    return launched(c, fn, launch_cloud_depth_rays(texset(c), texset32_if(c, t32), fc, dc, g, d_dirs, d_out, s));
}

// The argument and state checks of the four ray forms: depth_check on (w, h, steps) as a csky_depth_params, and the view's own.  dp receives them.
int depth_rays_check(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, bool is_view, int w, int h, int steps, size_t pitch_bytes,
                     csky_depth_params& dp) {
    if (is_view && !view) return fail(c, CSKY_ERR_INVALID, "%s: view is NULL", fn);
    dp.width = w; dp.height = h; dp.steps = steps;
    if (!p) return fail(c, CSKY_ERR_INVALID, "%s: params is NULL", fn);
    if (is_view) if (const int rc = view_check(c, fn, view)) return rc;
    return depth_check(c, fn, p, &dp, pitch_bytes);
}

// The blocking ray forms: dirs (NULL for a view) up, the frame down, on the context's stream.
int depth_rays_host(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, bool is_view, int w, int h, int steps, const float* dirs,
                    uint16_t* out) {
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    if (!is_view && !dirs) return fail(c, CSKY_ERR_INVALID, "%s: dirs_xyz is NULL", fn);
    csky_depth_params dp;
    int rc; if ((rc = depth_rays_check(c, fn, p, view, is_view, w, h, steps, (w >= 1 && w <= 8192) ? (size_t)w * 8 : 8, dp)) || (rc = bind(c))) return rc;
    const size_t n = (size_t)w * h, db = is_view ? 0 : n * 3 * sizeof(float);
    HostCall hc = host_call(c, fn, {db, n * 8});
    hc.up(0, dirs, db);
    hc.step([&] { return depth_launch(c, fn, p, &dp, hc.at<uint2>(1), (size_t)w * 8, c->stream, view, is_view ? nullptr : hc.at<float>(0)); });
    hc.down(out, 1, n * 8);
    return hc.finish();
}

}  // namespace

extern "C" {

int csky_render_cloud_depth_device(csky_ctx* c, const csky_cloud_params* p, const csky_depth_params* dp, void* d_out, size_t pitch, void* hip_stream) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_cloud_depth_device: ctx is NULL");
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "csky_render_cloud_depth_device: d_out is NULL");
    const char* fn = "csky_render_cloud_depth_device";
    int rc; if ((rc = depth_check(c, fn, p, dp, pitch)) || (rc = bind(c))) return rc;
    return depth_launch(c, fn, p, dp, static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream));
}

int csky_render_cloud_depth(csky_ctx* c, const csky_cloud_params* p, const csky_depth_params* dp, uint16_t* out) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_cloud_depth: ctx is NULL");
    const char* fn = "csky_render_cloud_depth";
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    int rc; if ((rc = depth_check(c, fn, p, dp, dp ? (size_t)dp->width * 8 : 0)) || (rc = bind(c))) return rc;
    const size_t nb = (size_t)dp->width * dp->height * 8;
    HostCall hc = host_call(c, fn, {nb});
    hc.step([&] { return depth_launch(c, fn, p, dp, hc.at<uint2>(0), (size_t)dp->width * 8, c->stream); });
    hc.down(out, 0, nb);
    return hc.finish();
}

int csky_render_cloud_depth_dirs(csky_ctx* c, const csky_cloud_params* p, int w, int h, int steps, const float* dirs, uint16_t* out) {
    const char* fn = "csky_render_cloud_depth_dirs";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return depth_rays_host(c, fn, p, nullptr, false, w, h, steps, dirs, out);
}

int csky_render_cloud_depth_view(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, int w, int h, int steps, uint16_t* out) {
    const char* fn = "csky_render_cloud_depth_view";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return depth_rays_host(c, fn, p, view, true, w, h, steps, nullptr, out);
}

int csky_render_cloud_depth_dirs_device(csky_ctx* c, const csky_cloud_params* p, int w, int h, int steps, const void* d_dirs, void* d_out, size_t pitch,
                                        void* hip_stream) {
    const char* fn = "csky_render_cloud_depth_dirs_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_dirs || !d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_dirs_xyz or d_out is NULL", fn);
    csky_depth_params dp;
    int rc; if ((rc = depth_rays_check(c, fn, p, nullptr, false, w, h, steps, pitch, dp)) || (rc = bind(c))) return rc;
    return depth_launch(c, fn, p, &dp, static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream), nullptr, static_cast<const float*>(d_dirs));
}

int csky_render_cloud_depth_view_device(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, int w, int h, int steps, void* d_out, size_t pitch,
                                        void* hip_stream) {
    const char* fn = "csky_render_cloud_depth_view_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    csky_depth_params dp;
    int rc; if ((rc = depth_rays_check(c, fn, p, view, true, w, h, steps, pitch, dp)) || (rc = bind(c))) return rc;
    return depth_launch(c, fn, p, &dp, static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream), view, nullptr);
}

}  // extern "C"
