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

// The row pitch of a blocking form's image, whose rows are packed; for a width rays_check refuses, one that passes every check in front of it.
size_t tight_pitch(int w) { return (w >= 1 && w <= 8192) ? (size_t)w * 8 : 8; }

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

// What both update forms do before their work: the checks in the C ABI's order, then bind.
int update_begin(csky_ctx* c, const char* fn, bool host_form, const csky_cloud_params* p, const csky_view* view, const csky_view* prev_view, int w, int h, int block, int phase,
                 const void* prev, size_t prev_pitch, const void* out, size_t pitch) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!out) return fail(c, CSKY_ERR_INVALID, host_form ? "%s: out is NULL" : "%s: d_out is NULL", fn);
    int rc;
    if ((rc = update_check(c, fn, prev_view, w, h, block, phase, prev, prev_pitch, out, pitch)) || (rc = rays_check(c, fn, p, view, true, w, h, pitch))) return rc;
    return bind(c);
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

// ---- the twelve forms that are not an update: one description, one host path, one device path
// What an entry point says of its call.  `form` names the arguments the form has, so that a NULL one is an error; the pointer of an argument the form
// does not have is NULL.  dirs: on the host for a blocking form, on the device for a _device form.
enum : int { RAYS_VIEW = 1, RAYS_FROM = 2, RAYS_DEPTH = 4 };   // a view, not dirs; an observer; a scene depth behind that observer
struct RaysCall {
    const char* fn;
    int form;
    const csky_cloud_params* p;
    const csky_view* view;
    int w, h;
    const void* dirs;
    const csky_observer* obs;
    const csky_scene_depth* depth;
};

// The checks of a call, in the order the C ABI promises (a bad argument is CSKY_ERR_INVALID whatever the context holds), then bind.  out, pitch: the
// image of either path; a blocking form's depth buffer is staged, so it cannot overlap out.
int rays_call_check(csky_ctx* c, const RaysCall& k, bool host_form, const void* out, size_t pitch) {
    const bool is_view = k.form & RAYS_VIEW;
    if (!out) return fail(c, CSKY_ERR_INVALID, host_form ? "%s: out is NULL" : "%s: d_out is NULL", k.fn);
    if (!is_view && !k.dirs) return fail(c, CSKY_ERR_INVALID, host_form ? "%s: dirs_xyz is NULL" : "%s: d_dirs_xyz is NULL", k.fn);
    int rc;
    if ((k.form & RAYS_DEPTH) && (rc = depth_check(c, k.fn, k.depth, is_view, host_form, k.w, k.h, host_form ? nullptr : out, host_form ? 0 : pitch))) return rc;
    if ((k.form & RAYS_FROM) && (rc = observer_check(c, k.fn, k.obs))) return rc;
    if ((rc = rays_check(c, k.fn, k.p, k.view, is_view, k.w, k.h, pitch))) return rc;
    return bind(c);
}

// The march of a call the checks have passed, on stream s: the launcher of what the description holds.  d_dirs (NULL for a view), d_depth and its
// pitch in bytes (a _from_depth form's), d_out: on the device.
int rays_launch(csky_ctx* c, const RaysCall& k, const float* d_dirs, const float* d_depth, size_t depth_pitch, uint2* d_out, size_t pitch_bytes, hipStream_t s) {
    const float* basis = k.view ? k.view->basis : nullptr;
    const float fov = k.view ? k.view->fov_y_degrees : 0.0f;
    const uint32_t pitch_px = (uint32_t)(pitch_bytes / 8);
    return rays_run(c, k.fn, k.p, s, [&](const TexSet& t, const TexSet32* t32) {
        if (k.form & RAYS_DEPTH) return launch_clouds_observer_depth(t, t32, c->d_rays_fc, scene_depth_geom(basis, fov, k.w, k.h, pitch_px, k.obs->position, k.obs->max_distance,
                                                                                               (uint32_t)(depth_pitch / 4), k.depth->kind), d_dirs, d_depth, d_out, s);
        if (k.form & RAYS_FROM) return launch_clouds_observer(t, t32, c->d_rays_fc, observer_geom(basis, fov, k.w, k.h, pitch_px, k.obs->position, k.obs->max_distance), d_dirs, d_out, s);
        return launch_clouds_rays(t, t32, c->d_rays_fc, rays_geom(basis, fov, k.w, k.h, pitch_px), d_dirs, d_out, s);
    });
}

// The blocking forms: dirs and the depth buffer (where the form has them) up, the image down, on the context's stream.  A pitched depth buffer goes up
// as it lies, its pitch with it.
int rays_host(csky_ctx* c, const RaysCall& k, uint16_t* out) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", k.fn);
    if (const int rc = rays_call_check(c, k, true, out, tight_pitch(k.w))) return rc;
    const bool has_depth = k.form & RAYS_DEPTH;
    const size_t n = (size_t)k.w * k.h, db = (k.form & RAYS_VIEW) ? 0 : n * 3 * sizeof(float);
    const size_t dp = !has_depth ? 0 : k.depth->pitch_bytes ? k.depth->pitch_bytes : (size_t)k.w * 4, zb = has_depth ? (size_t)(k.h - 1) * dp + (size_t)k.w * 4 : 0;
    HostCall hc = host_call(c, k.fn, {db, zb, n * 8});            // a region of 0 bytes takes nothing
    hc.up(0, k.dirs, db);
    hc.up(1, has_depth ? k.depth->texels : nullptr, zb);
    hc.step([&] { return rays_launch(c, k, db ? hc.at<float>(0) : nullptr, hc.at<float>(1), dp, hc.at<uint2>(2), (size_t)k.w * 8, c->stream); });
    hc.down(out, 2, n * 8);
    return hc.finish();
}

// The _device forms: the caller's pointers, pitch and stream.
int rays_device(csky_ctx* c, const RaysCall& k, void* d_out, size_t pitch, void* hip_stream) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", k.fn);
    if (const int rc = rays_call_check(c, k, false, d_out, pitch)) return rc;
    const bool has_depth = k.form & RAYS_DEPTH;
    return rays_launch(c, k, static_cast<const float*>(k.dirs), has_depth ? static_cast<const float*>(k.depth->texels) : nullptr, has_depth ? k.depth->pitch_bytes : 0,
                       static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream));
}

}  // namespace

extern "C" {

int csky_render_clouds_view_update(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_view* prev_view, int w, int h, int block, int phase,
                                   const uint16_t* prev, uint16_t* out) {
    const char* fn = "csky_render_clouds_view_update";
    const size_t tight = tight_pitch(w);
    if (const int rc = update_begin(c, fn, true, p, view, prev_view, w, h, block, phase, prev, tight, out, tight)) return rc;
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
    if (const int rc = update_begin(c, fn, false, p, view, prev_view, w, h, block, phase, d_prev, prev_pitch, d_out, pitch)) return rc;
    return update_launch(c, fn, p, view, prev_view, w, h, block, phase, static_cast<const uint2*>(d_prev), prev_pitch, static_cast<uint2*>(d_out), pitch, stream_of(c, hip_stream));
}

// RaysCall: {fn, form, params, view, w, h, dirs, observer, depth}
int csky_render_clouds_dirs(csky_ctx* c, const csky_cloud_params* p, int w, int h, const float* dirs, uint16_t* out) {
    return rays_host(c, {"csky_render_clouds_dirs", 0, p, nullptr, w, h, dirs, nullptr, nullptr}, out);
}

int csky_render_clouds_view(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, int w, int h, uint16_t* out) {
    return rays_host(c, {"csky_render_clouds_view", RAYS_VIEW, p, view, w, h, nullptr, nullptr, nullptr}, out);
}

int csky_render_clouds_dirs_device(csky_ctx* c, const csky_cloud_params* p, int w, int h, const void* d_dirs, void* d_out, size_t pitch, void* hip_stream) {
    return rays_device(c, {"csky_render_clouds_dirs_device", 0, p, nullptr, w, h, d_dirs, nullptr, nullptr}, d_out, pitch, hip_stream);
}

int csky_render_clouds_view_device(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, int w, int h, void* d_out, size_t pitch, void* hip_stream) {
    return rays_device(c, {"csky_render_clouds_view_device", RAYS_VIEW, p, view, w, h, nullptr, nullptr, nullptr}, d_out, pitch, hip_stream);
}

// ---- the same from an observer's position (observer_core.h)
int csky_render_clouds_dirs_from(csky_ctx* c, const csky_cloud_params* p, int w, int h, const float* dirs, const csky_observer* obs, uint16_t* out) {
    return rays_host(c, {"csky_render_clouds_dirs_from", RAYS_FROM, p, nullptr, w, h, dirs, obs, nullptr}, out);
}

int csky_render_clouds_view_from(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_observer* obs, int w, int h, uint16_t* out) {
    return rays_host(c, {"csky_render_clouds_view_from", RAYS_VIEW | RAYS_FROM, p, view, w, h, nullptr, obs, nullptr}, out);
}

int csky_render_clouds_dirs_from_device(csky_ctx* c, const csky_cloud_params* p, int w, int h, const void* d_dirs, const csky_observer* obs, void* d_out, size_t pitch,
                                        void* hip_stream) {
    return rays_device(c, {"csky_render_clouds_dirs_from_device", RAYS_FROM, p, nullptr, w, h, d_dirs, obs, nullptr}, d_out, pitch, hip_stream);
}

int csky_render_clouds_view_from_device(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_observer* obs, int w, int h, void* d_out, size_t pitch,
                                        void* hip_stream) {
    return rays_device(c, {"csky_render_clouds_view_from_device", RAYS_VIEW | RAYS_FROM, p, view, w, h, nullptr, obs, nullptr}, d_out, pitch, hip_stream);
}

// ---- the same behind a per-pixel scene depth (scene_depth_core.h)
int csky_render_clouds_view_from_depth(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_observer* obs, int w, int h, const csky_scene_depth* depth,
                                       uint16_t* out) {
    return rays_host(c, {"csky_render_clouds_view_from_depth", RAYS_VIEW | RAYS_FROM | RAYS_DEPTH, p, view, w, h, nullptr, obs, depth}, out);
}

int csky_render_clouds_dirs_from_depth(csky_ctx* c, const csky_cloud_params* p, int w, int h, const float* dirs, const csky_observer* obs, const csky_scene_depth* depth,
                                       uint16_t* out) {
    return rays_host(c, {"csky_render_clouds_dirs_from_depth", RAYS_FROM | RAYS_DEPTH, p, nullptr, w, h, dirs, obs, depth}, out);
}

int csky_render_clouds_view_from_depth_device(csky_ctx* c, const csky_cloud_params* p, const csky_view* view, const csky_observer* obs, int w, int h,
                                              const csky_scene_depth* depth, void* d_out, size_t pitch, void* hip_stream) {
    return rays_device(c, {"csky_render_clouds_view_from_depth_device", RAYS_VIEW | RAYS_FROM | RAYS_DEPTH, p, view, w, h, nullptr, obs, depth}, d_out, pitch, hip_stream);
}

int csky_render_clouds_dirs_from_depth_device(csky_ctx* c, const csky_cloud_params* p, int w, int h, const void* d_dirs, const csky_observer* obs,
                                              const csky_scene_depth* depth, void* d_out, size_t pitch, void* hip_stream) {
    return rays_device(c, {"csky_render_clouds_dirs_from_depth_device", RAYS_FROM | RAYS_DEPTH, p, nullptr, w, h, d_dirs, obs, depth}, d_out, pitch, hip_stream);
}

}  // extern "C"
