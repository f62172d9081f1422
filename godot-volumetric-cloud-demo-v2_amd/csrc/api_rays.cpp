// api_rays.cpp -- the direct cloud march's C ABI (csky_render_clouds_dirs / _view and their _device forms; rays_core.h, cloud_kernels.hip
// clouds_rays_kernel), the same from an observer's position (the _from forms; observer_core.h, clouds_observer_kernel; §21), that behind a per-pixel scene depth (the
// _from_depth forms; scene_depth_core.h, clouds_observer_depth_kernel; §22) and the temporal split of a view frame (csky_render_clouds_view_update*; view_update_core.h).
// The call reads what a cloud frame reads (noise, sky LUT, the march settings) and writes none of it.  Its frame constants come from the cloud
// frame's own set-up kernel, enqueued on the context's stream into a block of the call's own: no slot of the frame ring, none of the ring's order,
// feedback or head state, no stream of its own.  The blocking forms work in the context's stage (host_stage.h).
#include <cmath>
#include <cstring>
#include "context.h"
#include "rays_core.h"
#include "observer_core.h"
#include "scene_depth_core.h"
#include "view_update_core.h"

using namespace csky;

namespace {

// The argument and state checks of all four forms.  fn: the entry point's name for the error text.  view: NULL for the dirs forms.
int rays_check(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, bool is_view, int w, int h, size_t pitch_bytes) {
    if (!p) return fail(c, CSKY_ERR_INVALID, "%s: params is NULL", fn);
    if (is_view && !view) return fail(c, CSKY_ERR_INVALID, "%s: view is NULL", fn);
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return fail(c, CSKY_ERR_INVALID, "%s: w and h must be in [1, 8192]", fn);
    if (pitch_bytes % 8 || pitch_bytes < (size_t)w * 8) return fail(c, CSKY_ERR_INVALID, "%s: row pitch must be a multiple of 8 and >= 8 * w", fn);
    if (is_view) if (const int rc = view_check(c, fn, view)) return rc;
    if (!c->noise.st.have()) return fail(c, CSKY_ERR_STATE, "render_clouds: csky_set_noise has not been called");
    if (c->lut.st.holds == SkyLutHolds::None) return fail(c, CSKY_ERR_STATE, "render_clouds: no sky LUT yet (call csky_render_sky_lut first; cloud_sky.gd:187,242)");
    return CSKY_OK;
}

// The frame constants of this call, by the cloud frame's set-up kernel (as clouds_launch.cpp frame_setup chooses it) on the context's stream into
// c->d_rays_fc; stream s waits for them.  The block's last reader, the march of the rays call before, is waited for first.
int rays_setup(csky_ctx* c, const CloudParams& cp, hipStream_t s) {
    int rc;
    if (!c->d_rays_fc && (rc = c->d_rays_fc.alloc(c, 1))) return rc;
    if (!c->ev_rays && (rc = c->ev_rays.create(c, hipEventDisableTiming))) return rc;
    if (c->rays_pending) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_rays, 0));
    const ExactRejects rej = c->noise.st.rejects(cp.cloud_coverage, c->use_window);
    const SetupArgs sa = {c->primary_steps, c->light_steps, c->early_eps, rej.hf_lo, rej.hf_hi, rej.ct_mode, c->use_window ? 1 : 0};
    const SkyLut& l = c->lut;
    if (l.st.own_taps())
        HIPCHK(c, launch_frame_setup_taps(cp, l.st.sun, c->d_trans_f, c->tw, c->th, l.st.w, l.st.h, sa, c->d_rays_fc, c->stream, c->tlut));
    else
        HIPCHK(c, launch_frame_setup(cp, l.cur_f(), l.aw, l.ah, sa, c->d_rays_fc, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_rays, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_rays, 0));
    return CSKY_OK;
}

// Set-up and the call's march on stream s, for arguments the checks have passed.  `launch(t, t32)` enqueues the march (one launch, or the update's
// two) on s with the frame constants in c->d_rays_fc and returns its hipError_t.
template <class F> int rays_run(csky_ctx* c, const char* fn, const csky_cloud_params* p, hipStream_t s, F launch) {
    CloudParams cp; memcpy(&cp, p, sizeof cp);
    // texture_size and update_position are not read by this path; the set-up kernel copies them into fields no lane of the rays kernels looks at.
    // Fixed values keep whatever the caller left there (NaNs included) out of every conversion.
    cp.texture_size[0] = cp.texture_size[1] = 1.0f; cp.update_position[0] = cp.update_position[1] = 0.0f;
    int rc; if ((rc = rays_setup(c, cp, s))) return rc;
    TexSet32 t32;
    const Event* kt = nullptr;                                  // timing pair of this call (csky_set_kernel_timing), as around a cloud frame's
    if (c->kt.on && (rc = c->kt.next_pair(c, kt))) return rc;
    if (kt) HIPCHK(c, hipEventRecord(kt[0], s));
    if ((rc = launched(c, fn, launch(texset(c), texset32_if(c, t32))))) return rc;
    if (kt) HIPCHK(c, hipEventRecord(kt[1], s));
    HIPCHK(c, hipEventRecord(c->ev_rays, s));                   // the next call's set-up overwrites the block this march reads
    c->rays_pending = true;
    return CSKY_OK;
}

// What the _from forms check beyond rays_check, before it (a bad observer is CSKY_ERR_INVALID whatever the context holds): observer_core.h's rule.
int observer_check(csky_ctx* c, const char* fn, const csky_observer* obs) {
    if (!obs) return fail(c, CSKY_ERR_INVALID, "%s: observer is NULL", fn);
    switch (observer_invalid(obs->position, obs->max_distance)) {
        case 0: return CSKY_OK;
        case 1: return fail(c, CSKY_ERR_INVALID, "%s: the observer's position is not finite", fn);
        case 2: return fail(c, CSKY_ERR_INVALID, "%s: the observer's position[0] and position[2] must be within 1e6 m", fn);
        case 3: return fail(c, CSKY_ERR_INVALID, "%s: the observer is under the ground", fn);
        case 4: return fail(c, CSKY_ERR_INVALID, "%s: the observer is more than 100 000 m above the ground", fn);
        default: return fail(c, CSKY_ERR_INVALID, "%s: max_distance must be > 0 (+inf: no cap)", fn);
    }
}

// The dirs and view forms' march.  d_dirs: NULL for the view forms.  obs: NULL for the reference's observer, else checked (the _from forms).
int rays_launch(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, int w, int h, const float* d_dirs, uint2* d_out, size_t pitch_bytes,
                hipStream_t s, const csky_observer* obs = nullptr) {
    const float* basis = view ? view->basis : nullptr;
    const float fov = view ? view->fov_y_degrees : 0.0f;
    if (obs) {
        const ObserverGeom g = observer_geom(basis, fov, w, h, (uint32_t)(pitch_bytes / 8), obs->position, obs->max_distance);
        return rays_run(c, fn, p, s, [&](const TexSet& t, const TexSet32* t32) { return launch_clouds_observer(t, t32, c->d_rays_fc, g, d_dirs, d_out, s); });
    }
    const RaysGeom g = rays_geom(basis, fov, w, h, (uint32_t)(pitch_bytes / 8));
    return rays_run(c, fn, p, s, [&](const TexSet& t, const TexSet32* t32) { return launch_clouds_rays(t, t32, c->d_rays_fc, g, d_dirs, d_out, s); });
}

// The blocking host forms: dirs (NULL for a view) up, the image down, on the context's stream.  from: a _from form, obs its observer.
int rays_host(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, bool is_view, int w, int h, const float* dirs, uint16_t* out,
              bool from = false, const csky_observer* obs = nullptr) {
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    if (!is_view && !dirs) return fail(c, CSKY_ERR_INVALID, "%s: dirs_xyz is NULL", fn);
    int rc; if (from && (rc = observer_check(c, fn, obs))) return rc;
    if ((rc = rays_check(c, fn, p, view, is_view, w, h, (w >= 1 && w <= 8192) ? (size_t)w * 8 : 8)) || (rc = bind(c))) return rc;
    const size_t n = (size_t)w * h, db = is_view ? 0 : n * 3 * sizeof(float);
    HostCall hc = host_call(c, fn, {db, n * 8});
    hc.up(0, dirs, db);
    hc.step([&] { return rays_launch(c, fn, p, view, w, h, is_view ? nullptr : hc.at<float>(0), hc.at<uint2>(1), (size_t)w * 8, c->stream, obs); });
    hc.down(out, 1, n * 8);
    return hc.finish();
}

// ---- the temporal split of a view frame (view_update_core.h)
// What the update forms check beyond rays_check, before it (a bad argument is CSKY_ERR_INVALID whatever the context holds).  prev / out: device
// pointers of the device form, host pointers of the host form; both are byte ranges of (h - 1) * pitch + 8 * w bytes.
int update_check(csky_ctx* c, const char* fn, const csky_view* prev_view, int w, int h, int block, int phase, const void* prev, size_t prev_pitch, const void* out, size_t pitch) {
    if (block < 1 || block > 8) return fail(c, CSKY_ERR_INVALID, "%s: block must be in [1, 8]", fn);
    if (phase < 0 || phase >= block * block) return fail(c, CSKY_ERR_INVALID, "%s: phase must be in [0, block * block)", fn);
    if (!prev) return CSKY_OK;                                  // no history: prev_view and prev_pitch are not read
    if (!prev_view) return fail(c, CSKY_ERR_INVALID, "%s: prev_view is NULL beside a previous frame", fn);
    if (const int rc = view_check(c, fn, prev_view)) return rc;
    if (w < 1 || w > 8192 || h < 1 || h > 8192) return CSKY_OK;   // rays_check refuses it
    if (prev_pitch % 8 || prev_pitch < (size_t)w * 8) return fail(c, CSKY_ERR_INVALID, "%s: the previous frame's row pitch must be a multiple of 8 and >= 8 * w", fn);
    if (pitch < (size_t)w * 8) return CSKY_OK;                  // likewise
    const uintptr_t a = (uintptr_t)prev, b = (uintptr_t)out;
    const size_t na = (size_t)(h - 1) * prev_pitch + (size_t)w * 8, nb = (size_t)(h - 1) * pitch + (size_t)w * 8;
    if (a < b + nb && b < a + na) return fail(c, CSKY_ERR_INVALID, "%s: the previous frame and out overlap", fn);
    return CSKY_OK;
}

// The update's two launches, one timing pair around both.  d_prev: NULL without history (prev_view is then not read).
int update_launch(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, const csky_view* prev_view, int w, int h, int block, int phase,
                  const uint2* d_prev, size_t prev_pitch, uint2* d_out, size_t pitch_bytes, hipStream_t s) {
    static_assert(sizeof(csky_view) == 10 * sizeof(float), "csky_view is ten floats");
    const ViewUpdateGeom g = view_update_geom(reinterpret_cast<const float*>(view), d_prev ? reinterpret_cast<const float*>(prev_view) : nullptr, w, h,
                                              (uint32_t)(pitch_bytes / 8), d_prev ? (uint32_t)(prev_pitch / 8) : 0u, block, phase);
    return rays_run(c, fn, p, s, [&](const TexSet& t, const TexSet32* t32) { return launch_clouds_view_update(t, t32, c->d_rays_fc, g, d_prev, d_out, s); });
}

// ---- the observer's march behind a per-pixel scene depth (scene_depth_core.h)
// What the _from_depth forms check beyond observer_check and rays_check, before them: scene_depth_core.h's rule.  out, pitch: the device forms' image (the
// overlap test); NULL for the host forms, whose depth is staged.
int depth_check(csky_ctx* c, const char* fn, const csky_scene_depth* depth, bool is_view, bool host_form, int w, int h, const void* out, size_t pitch) {
    if (!depth) return fail(c, CSKY_ERR_INVALID, "%s: depth is NULL", fn);
    switch (scene_depth_invalid((uintptr_t)depth->texels, depth->pitch_bytes, depth->kind, is_view, host_form, w, h, (uintptr_t)out, pitch)) {
        case 0: return CSKY_OK;
        case 1: return fail(c, CSKY_ERR_INVALID, "%s: depth->texels is NULL", fn);
        case 2: return fail(c, CSKY_ERR_INVALID, "%s: depth->kind must be CSKY_DEPTH_DISTANCE or CSKY_DEPTH_VIEW_Z", fn);
        case 3: return fail(c, CSKY_ERR_INVALID, "%s: CSKY_DEPTH_VIEW_Z needs a view: the dirs forms take CSKY_DEPTH_DISTANCE only", fn);
        case 4: return fail(c, CSKY_ERR_INVALID, "%s: the depth buffer's row pitch must be a multiple of 4 and >= 4 * w", fn);
        default: return fail(c, CSKY_ERR_INVALID, "%s: the depth buffer and out overlap", fn);
    }
}

// The march of a _from_depth form, for arguments the checks have passed.  d_dirs: NULL for the view forms.  d_depth, depth_pitch (bytes): on the device.
int depth_launch(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, int w, int h, const float* d_dirs, const csky_observer* obs, const float* d_depth,
                 size_t depth_pitch, int kind, uint2* d_out, size_t pitch_bytes, hipStream_t s) {
    const SceneDepthGeom g = scene_depth_geom(view ? view->basis : nullptr, view ? view->fov_y_degrees : 0.0f, w, h, (uint32_t)(pitch_bytes / 8), obs->position, obs->max_distance,
                                              (uint32_t)(depth_pitch / 4), kind);
    return rays_run(c, fn, p, s, [&](const TexSet& t, const TexSet32* t32) { return launch_clouds_observer_depth(t, t32, c->d_rays_fc, g, d_dirs, d_depth, d_out, s); });
}

// The blocking host forms: dirs (NULL for a view) and the depth buffer up, the image down, on the context's stream.  A pitched depth buffer goes up
// as it lies, its pitch with it.
int depth_host(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, bool is_view, int w, int h, const float* dirs, const csky_observer* obs,
               const csky_scene_depth* depth, uint16_t* out) {
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    if (!is_view && !dirs) return fail(c, CSKY_ERR_INVALID, "%s: dirs_xyz is NULL", fn);
    int rc;
    if ((rc = depth_check(c, fn, depth, is_view, true, w, h, nullptr, 0)) || (rc = observer_check(c, fn, obs)) ||
        (rc = rays_check(c, fn, p, view, is_view, w, h, (w >= 1 && w <= 8192) ? (size_t)w * 8 : 8)) || (rc = bind(c))) return rc;
    const size_t n = (size_t)w * h, db = is_view ? 0 : n * 3 * sizeof(float);
    const size_t dp = depth->pitch_bytes ? depth->pitch_bytes : (size_t)w * 4, zb = (size_t)(h - 1) * dp + (size_t)w * 4;
    HostCall hc = host_call(c, fn, {db, zb, n * 8});
    hc.up(0, dirs, db);
    hc.up(1, depth->texels, zb);
    hc.step([&] { return depth_launch(c, fn, p, view, w, h, is_view ? nullptr : hc.at<float>(0), obs, hc.at<float>(1), dp, depth->kind, hc.at<uint2>(2), (size_t)w * 8, c->stream); });
    hc.down(out, 2, n * 8);
    return hc.finish();
}

int depth_device(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, bool is_view, int w, int h, const void* d_dirs, const csky_observer* obs,
                 const csky_scene_depth* depth, void* d_out, size_t pitch, void* hip_stream) {
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    if (!is_view && !d_dirs) return fail(c, CSKY_ERR_INVALID, "%s: d_dirs_xyz is NULL", fn);
    int rc;
    if ((rc = depth_check(c, fn, depth, is_view, false, w, h, d_out, pitch)) || (rc = observer_check(c, fn, obs)) || (rc = rays_check(c, fn, p, view, is_view, w, h, pitch)) ||
        (rc = bind(c))) return rc;
    return depth_launch(c, fn, p, view, w, h, is_view ? nullptr : static_cast<const float*>(d_dirs), obs, static_cast<const float*>(depth->texels), depth->pitch_bytes,
                        depth->kind, static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream));
}

}  // namespace

extern "C" {

int csky_render_clouds_view_update(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_view* prev_view, int w, int h, int block, int phase,
                                   const uint16_t* prev, uint16_t* out) {
    const char* fn = "csky_render_clouds_view_update";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    const size_t tight = (w >= 1 && w <= 8192) ? (size_t)w * 8 : 8;
    int rc; if ((rc = update_check(c, fn, prev_view, w, h, block, phase, prev, tight, out, tight)) || (rc = rays_check(c, fn, p, view, true, w, h, tight)) || (rc = bind(c))) return rc;
    const size_t n = (size_t)w * h, pb = prev ? n * 8 : 0;
    HostCall hc = host_call(c, fn, {pb, n * 8});
    hc.up(0, prev, pb);
    hc.step([&] { return update_launch(c, fn, p, view, prev_view, w, h, block, phase, prev ? hc.at<uint2>(0) : nullptr, tight, hc.at<uint2>(1), tight, c->stream); });
    hc.down(out, 1, n * 8);
    return hc.finish();
}

int csky_render_clouds_view_update_device(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_view* prev_view, int w, int h, int block, int phase,
                                          const void* d_prev, size_t prev_pitch, void* d_out, size_t pitch, void* hip_stream) {
    const char* fn = "csky_render_clouds_view_update_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    int rc; if ((rc = update_check(c, fn, prev_view, w, h, block, phase, d_prev, prev_pitch, d_out, pitch)) || (rc = rays_check(c, fn, p, view, true, w, h, pitch)) || (rc = bind(c))) return rc;
    return update_launch(c, fn, p, view, prev_view, w, h, block, phase, static_cast<const uint2*>(d_prev), prev_pitch, static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream));
}

int csky_render_clouds_dirs(csky_ctx* c, const csky_cloud_params* p, int w, int h, const float* dirs, uint16_t* out) {
    const char* fn = "csky_render_clouds_dirs";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return rays_host(c, fn, p, nullptr, false, w, h, dirs, out);
}

int csky_render_clouds_view(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, int w, int h, uint16_t* out) {
    const char* fn = "csky_render_clouds_view";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return rays_host(c, fn, p, view, true, w, h, nullptr, out);
}

int csky_render_clouds_dirs_device(csky_ctx* c, const csky_cloud_params* p, int w, int h, const void* d_dirs, void* d_out, size_t pitch, void* hip_stream) {
    const char* fn = "csky_render_clouds_dirs_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_dirs || !d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_dirs_xyz or d_out is NULL", fn);
    int rc; if ((rc = rays_check(c, fn, p, nullptr, false, w, h, pitch)) || (rc = bind(c))) return rc;
    return rays_launch(c, fn, p, nullptr, w, h, static_cast<const float*>(d_dirs), static_cast<uint2*>(d_out), pitch,
                       stream_of(c, hip_stream));
}

int csky_render_clouds_view_device(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, int w, int h, void* d_out, size_t pitch, void* hip_stream) {
    const char* fn = "csky_render_clouds_view_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    int rc; if ((rc = rays_check(c, fn, p, view, true, w, h, pitch)) || (rc = bind(c))) return rc;
    return rays_launch(c, fn, p, view, w, h, nullptr, static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream));
}

// ---- the same from an observer's position (observer_core.h)
int csky_render_clouds_dirs_from(csky_ctx* c, const csky_cloud_params* p, int w, int h, const float* dirs, const csky_observer* obs, uint16_t* out) {
    const char* fn = "csky_render_clouds_dirs_from";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return rays_host(c, fn, p, nullptr, false, w, h, dirs, out, true, obs);
}

int csky_render_clouds_view_from(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_observer* obs, int w, int h, uint16_t* out) {
    const char* fn = "csky_render_clouds_view_from";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return rays_host(c, fn, p, view, true, w, h, nullptr, out, true, obs);
}

int csky_render_clouds_dirs_from_device(csky_ctx* c, const csky_cloud_params* p, int w, int h, const void* d_dirs, const csky_observer* obs, void* d_out, size_t pitch,
                                        void* hip_stream) {
    const char* fn = "csky_render_clouds_dirs_from_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_dirs || !d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_dirs_xyz or d_out is NULL", fn);
    int rc; if ((rc = observer_check(c, fn, obs)) || (rc = rays_check(c, fn, p, nullptr, false, w, h, pitch)) || (rc = bind(c))) return rc;
    return rays_launch(c, fn, p, nullptr, w, h, static_cast<const float*>(d_dirs), static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream), obs);
}

int csky_render_clouds_view_from_device(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_observer* obs, int w, int h, void* d_out, size_t pitch,
                                        void* hip_stream) {
    const char* fn = "csky_render_clouds_view_from_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    int rc; if ((rc = observer_check(c, fn, obs)) || (rc = rays_check(c, fn, p, view, true, w, h, pitch)) || (rc = bind(c))) return rc;
    return rays_launch(c, fn, p, view, w, h, nullptr, static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream), obs);
}

// ---- the same behind a per-pixel scene depth (scene_depth_core.h)
int csky_render_clouds_view_from_depth(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_observer* obs, int w, int h, const csky_scene_depth* depth,
                                       uint16_t* out) {
    const char* fn = "csky_render_clouds_view_from_depth";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return depth_host(c, fn, p, view, true, w, h, nullptr, obs, depth, out);
}

int csky_render_clouds_dirs_from_depth(csky_ctx* c, const csky_cloud_params* p, int w, int h, const float* dirs, const csky_observer* obs, const csky_scene_depth* depth,
                                       uint16_t* out) {
    const char* fn = "csky_render_clouds_dirs_from_depth";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return depth_host(c, fn, p, nullptr, false, w, h, dirs, obs, depth, out);
}

int csky_render_clouds_view_from_depth_device(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_observer* obs, int w, int h,
                                              const csky_scene_depth* depth, void* d_out, size_t pitch, void* hip_stream) {
    const char* fn = "csky_render_clouds_view_from_depth_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return depth_device(c, fn, p, view, true, w, h, nullptr, obs, depth, d_out, pitch, hip_stream);
}

int csky_render_clouds_dirs_from_depth_device(csky_ctx* c, const csky_cloud_params* p, int w, int h, const void* d_dirs, const csky_observer* obs,
                                              const csky_scene_depth* depth, void* d_out, size_t pitch, void* hip_stream) {
    const char* fn = "csky_render_clouds_dirs_from_depth_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return depth_device(c, fn, p, nullptr, false, w, h, d_dirs, obs, depth, d_out, pitch, hip_stream);
}

}  // extern "C"
