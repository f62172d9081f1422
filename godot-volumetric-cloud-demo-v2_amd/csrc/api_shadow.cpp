// api_shadow.cpp -- the cloud shadow map's C ABI (csky_render_cloud_shadow / _device; shadow_core.h, shadow.hip).
// The call reads the bound noise and the push-constant block and nothing else: no LUT, no slot of the cloud frames' constants ring (both constant
// blocks of a launch are computed here and travel as kernel arguments), no stream of its own; the blocking form works in the stage (host_stage.h).
#include <cmath>
#include <cstring>
#include "context.h"
#include "shadow_core.h"

using namespace csky;

namespace {

// The argument and state checks of both forms.  fn: the entry point's name for the error text.
int shadow_check(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_shadow_params* sp, size_t pitch_bytes) {
    if (!p || !sp) return fail(c, CSKY_ERR_INVALID, "%s: NULL argument", fn);
    if (sp->width < 1 || sp->width > 8192 || sp->height < 1 || sp->height > 8192) return fail(c, CSKY_ERR_INVALID, "%s: width and height must be in [1, 8192]", fn);
    if (sp->steps < 0 || sp->steps > 1024) return fail(c, CSKY_ERR_INVALID, "%s: steps must be in [1, 1024], or 0 for 64", fn);
    for (int k = 0; k < 2; k++) {
        if (!std::isfinite(sp->center[k]) || !std::isfinite(sp->extent[k]) || !(sp->extent[k] > 0.0f) || !(std::fabs(sp->center[k]) + 0.5f * sp->extent[k] <= 1.0e6f))
            return fail(c, CSKY_ERR_INVALID, "%s: center and extent must be finite, extent > 0 and |center| + extent / 2 <= 1e6 m", fn);
    }
    CloudParams cp; memcpy(&cp, p, sizeof cp);
    const float read[] = {cp.cloud_pos[0], cp.cloud_pos[1], cp.detailed_pos[0], cp.detailed_pos[1], cp.weather_pos[0], cp.weather_pos[1],
                          cp.LIGHT_DIRECTION[0], cp.LIGHT_DIRECTION[1], cp.LIGHT_DIRECTION[2], cp.time, cp.density, cp.cloud_coverage};
    for (float v : read) if (!std::isfinite(v)) return fail(c, CSKY_ERR_INVALID, "%s: a push-constant field the shadow map reads is not finite", fn);
    if (pitch_bytes < (size_t)sp->width * 2 || pitch_bytes % 2) return fail(c, CSKY_ERR_INVALID, "%s: row pitch must be even and >= 2 * width", fn);
    if (!c->noise.st.have()) return fail(c, CSKY_ERR_STATE, "%s: csky_set_noise has not been called", fn);
    return CSKY_OK;
}

// The launch on stream s, for arguments shadow_check has passed.
int shadow_launch(csky_ctx* c, const char* fn, const csky_cloud_params* p, const csky_shadow_params* sp, uint16_t* d_out, size_t pitch_bytes, hipStream_t s) {
    CloudParams cp; memcpy(&cp, p, sizeof cp);
    const ExactRejects rej = c->noise.st.rejects(cp.cloud_coverage, c->use_window);   // the height window and the cloud-type branch, as the cloud march gets them
    ShadowConsts sc;
    sc.w = sp->width; sc.h = sp->height; sc.cx = sp->center[0]; sc.cz = sp->center[1]; sc.ex = sp->extent[0]; sc.ez = sp->extent[1];
    sc.steps = sp->steps == 0 ? 64 : sp->steps; sc.exact_end = c->shadow_exact_end ? 1 : 0; sc.pitch_h = (uint32_t)(pitch_bytes / 2);
    FrameConsts fc;
    shadow_frame_consts(cp, sc.steps, rej.hf_lo, rej.hf_hi, rej.ct_mode, fc);
    sc.night = fc.ldir[1] > 0.0f ? 0 : 1;               // l.y <= 0; a zero LIGHT_DIRECTION (no direction: l is NaN) counts as night too
    TexSet32 t32;
    return launched(c, fn, launch_cloud_shadow(texset(c), texset32_if(c, t32), fc, sc, d_out, s));
}

}  // namespace

extern "C" {

int csky_render_cloud_shadow_device(csky_ctx* c, const csky_cloud_params* p, const csky_shadow_params* sp, void* d_out, size_t pitch, void* hip_stream) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_cloud_shadow_device: ctx is NULL");
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "csky_render_cloud_shadow_device: d_out is NULL");
    const char* fn = "csky_render_cloud_shadow_device";
    int rc; if ((rc = shadow_check(c, fn, p, sp, pitch)) || (rc = bind(c))) return rc;
    return shadow_launch(c, fn, p, sp, static_cast<uint16_t*>(d_out), pitch, stream_of(c, hip_stream));
}

int csky_render_cloud_shadow(csky_ctx* c, const csky_cloud_params* p, const csky_shadow_params* sp, uint16_t* out) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_cloud_shadow: ctx is NULL");
    const char* fn = "csky_render_cloud_shadow";
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    int rc; if ((rc = shadow_check(c, fn, p, sp, sp ? (size_t)sp->width * 2 : 0)) || (rc = bind(c))) return rc;
    const size_t nb = (size_t)sp->width * sp->height * 2;
    HostCall hc = host_call(c, fn, {nb});
    hc.step([&] { return shadow_launch(c, fn, p, sp, hc.at<uint16_t>(0), (size_t)sp->width * 2, c->stream); });
    hc.down(out, 0, nb);
    return hc.finish();
}

int csky_set_shadow_exact_end(csky_ctx* c, int enabled) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_shadow_exact_end: ctx is NULL");
    c->shadow_exact_end = enabled != 0; return CSKY_OK;
}

}  // extern "C"
