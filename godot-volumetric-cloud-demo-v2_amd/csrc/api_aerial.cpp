// api_aerial.cpp -- the aerial-perspective volume's C ABI (csky_render_aerial_perspective / _device; aerial_core.h, aerial.hip).
// The call reads the context's transmittance table and nothing else of it: no noise, no sky LUT, no cloud frame, no slot of any ring (geometry and sun
// travel as kernel arguments), no stream of its own.
#include <cmath>
#include "context.h"
#include "aerial_core.h"

using namespace csky;

namespace {

// The argument and state checks of both forms, and the kernel's argument block with the defaults filled in.  fn: the entry point's name for the error text.
int aerial_check(csky_ctx* c, const char* fn, const csky_aerial_params* ap, const csky_view* view, AerialGeom& g) {
    if (!ap) return fail(c, CSKY_ERR_INVALID, "%s: params is NULL", fn);
    g.w = ap->width ? ap->width : 32; g.h = ap->height ? ap->height : 32; g.d = ap->depth ? ap->depth : 32;
    g.s = ap->steps_per_slice ? ap->steps_per_slice : 2;
    g.far_km = ap->far_km == 0.0f ? 32.0f : ap->far_km;
    if (g.w < 1 || g.w > 512 || g.h < 1 || g.h > 512) return fail(c, CSKY_ERR_INVALID, "%s: width and height must be in [1, 512], or 0 for 32", fn);
    if (g.d < 1 || g.d > 256) return fail(c, CSKY_ERR_INVALID, "%s: depth must be in [1, 256], or 0 for 32", fn);
    if (g.s < 1 || g.s > 16) return fail(c, CSKY_ERR_INVALID, "%s: steps_per_slice must be in [1, 16], or 0 for 2", fn);
    if (!std::isfinite(g.far_km) || !(g.far_km > 0.0f) || !(g.far_km <= 2000.0f)) return fail(c, CSKY_ERR_INVALID, "%s: far_km must be finite and in (0, 2000], or 0 for 32", fn);
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(ap->sun_direction[k])) return fail(c, CSKY_ERR_INVALID, "%s: sun_direction is not finite", fn);
        g.sun[k] = ap->sun_direction[k];
    }
    g.view_mode = 0; g.tan_half_fov_y = 1.0f; g.aspect = 1.0f;
    for (int k = 0; k < 9; k++) g.cam[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    if (view) {
        for (int k = 0; k < 9; k++) if (!std::isfinite(view->basis[k])) return fail(c, CSKY_ERR_INVALID, "%s: the view's basis is not finite", fn);
        if (!(view->fov_y_degrees > 0.0f && view->fov_y_degrees < 180.0f)) return fail(c, CSKY_ERR_INVALID, "%s: fov_y_degrees must be in (0, 180)", fn);
        if (!std::isfinite(ap->aspect) || ap->aspect < 0.0f) return fail(c, CSKY_ERR_INVALID, "%s: aspect must be finite and > 0, or 0 for width / height", fn);
        g.view_mode = 1;
        for (int k = 0; k < 9; k++) g.cam[k] = view->basis[k];
        g.tan_half_fov_y = tan_half_fov(view->fov_y_degrees);
        g.aspect = ap->aspect == 0.0f ? (float)g.w / (float)g.h : ap->aspect;
    }
    if (!c->have_trans) return fail(c, CSKY_ERR_STATE, "%s: the transmittance LUT has not been rendered (csky_render_transmittance)", fn);
    return CSKY_OK;
}

// The launch on stream s, behind whatever the context's stream has done to the table.
int aerial_launch(csky_ctx* c, const char* fn, const AerialGeom& g, uint2* d_out, hipStream_t s) {
    HIPCHK(c, hipEventRecord(c->ev_aerial, c->stream));          // the LUT may have been rendered there
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_aerial, 0));
    const hipError_t e = launch_aerial(g, c->d_trans_f, c->tw, c->th, d_out, s, c->tlut);
    if (e != hipSuccess) return fail(c, CSKY_ERR_HIP, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
    return CSKY_OK;
}

}  // namespace

extern "C" {

int csky_render_aerial_perspective_device(csky_ctx* c, const csky_aerial_params* ap, const csky_view* view, void* d_out, void* hip_stream) {
    const char* fn = "csky_render_aerial_perspective_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    AerialGeom g;
    int rc; if ((rc = aerial_check(c, fn, ap, view, g)) || (rc = bind(c))) return rc;
    return aerial_launch(c, fn, g, static_cast<uint2*>(d_out), hip_stream ? (hipStream_t)hip_stream : (hipStream_t)c->stream);
}

int csky_render_aerial_perspective(csky_ctx* c, const csky_aerial_params* ap, const csky_view* view, uint16_t* out) {
    const char* fn = "csky_render_aerial_perspective";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    AerialGeom g;
    int rc; if ((rc = aerial_check(c, fn, ap, view, g)) || (rc = bind(c))) return rc;
    const size_t n = (size_t)g.d * g.h * g.w;
    if ((rc = c->d_aerial.grow(c, n))) return rc;               // nothing of an earlier call is in flight: this form blocks
    if ((rc = aerial_launch(c, fn, g, c->d_aerial, c->stream))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->d_aerial, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

}  // extern "C"
