// api_rays.cpp -- the direct cloud march's C ABI (csky_render_clouds_dirs / _view and their _device forms; rays_core.h, cloud_kernels.hip
// clouds_rays_kernel).
// The call reads what a cloud frame reads (noise, sky LUT, the march settings) and writes none of it.  Its frame constants come from the cloud
// frame's own set-up kernel, enqueued on the context's stream into a block of the call's own: no slot of the frame ring, none of the ring's order,
// feedback or head state, no stream of its own.  The blocking forms work in the context's stage (host_stage.h).
#include <cmath>
#include <cstring>
#include "context.h"
#include "rays_core.h"

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

// Set-up and launch on stream s, for arguments rays_check has passed.  d_dirs: NULL for the view forms.
int rays_launch(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, int w, int h, const float* d_dirs, uint2* d_out, size_t pitch_bytes,
                hipStream_t s) {
    CloudParams cp; memcpy(&cp, p, sizeof cp);
    // texture_size and update_position are not read by this path; the set-up kernel copies them into fields no lane of the rays kernel looks at.
    // Fixed values keep whatever the caller left there (NaNs included) out of every conversion.
    cp.texture_size[0] = cp.texture_size[1] = 1.0f; cp.update_position[0] = cp.update_position[1] = 0.0f;
    int rc; if ((rc = rays_setup(c, cp, s))) return rc;
    const RaysGeom g = rays_geom(view ? view->basis : nullptr, view ? view->fov_y_degrees : 0.0f, w, h, (uint32_t)(pitch_bytes / 8));
    TexSet32 t32;
    const Event* kt = nullptr;                                  // timing pair of this launch (csky_set_kernel_timing), as around a cloud frame's
    if (c->kt.on && (rc = c->kt.next_pair(c, kt))) return rc;
    if (kt) HIPCHK(c, hipEventRecord(kt[0], s));
    if ((rc = launched(c, fn, launch_clouds_rays(texset(c), texset32_if(c, t32), c->d_rays_fc, g, d_dirs, d_out, s)))) return rc;
    if (kt) HIPCHK(c, hipEventRecord(kt[1], s));
    HIPCHK(c, hipEventRecord(c->ev_rays, s));                   // the next call's set-up overwrites the block this march reads
    c->rays_pending = true;
    return CSKY_OK;
}

// The blocking host forms: dirs (NULL for a view) up, the image down, on the context's stream.
int rays_host(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_view* view, bool is_view, int w, int h, const float* dirs, uint16_t* out) {
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    if (!is_view && !dirs) return fail(c, CSKY_ERR_INVALID, "%s: dirs_xyz is NULL", fn);
    int rc; if ((rc = rays_check(c, fn, p, view, is_view, w, h, (w >= 1 && w <= 8192) ? (size_t)w * 8 : 8)) || (rc = bind(c))) return rc;
    const size_t n = (size_t)w * h, db = is_view ? 0 : n * 3 * sizeof(float);
    HostCall hc = host_call(c, fn, {db, n * 8});
    hc.up(0, dirs, db);
    hc.step([&] { return rays_launch(c, fn, p, view, w, h, is_view ? nullptr : hc.at<float>(0), hc.at<uint2>(1), (size_t)w * 8, c->stream); });
    hc.down(out, 1, n * 8);
    return hc.finish();
}

}  // namespace

extern "C" {

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

}  // extern "C"
