// api_aerial.cpp -- the aerial-perspective volume's C ABI (csky_render_aerial_perspective / _device; aerial_core.h, aerial.hip), and
// the same volume with a cloud shadow map inside it (csky_render_aerial_perspective_shadowed / _device, csky_aerial_shadow_rect; shafts_core.h,
// shafts.hip), and the air in front of a cloud frame (csky_apply_cloud_aerial / _device; cloud_aerial_core.h, cloud_aerial.hip;
// DESIGN.md §16), which reads the caller's two images besides, and that step on a view frame or a ray frame (csky_apply_cloud_aerial_dirs / _view and
// their _device forms; view_depth_core.h).
// The call reads the context's transmittance table and nothing else of it: no noise, no sky LUT, no cloud frame, no slot of any ring (geometry and sun
// travel as kernel arguments), no stream of its own.  The blocking forms work in the context's stage (host_stage.h).
#include <cmath>
#include "context.h"
#include "aerial_core.h"
#include "shafts_core.h"
#include "cloud_aerial_core.h"
#include "view_depth_core.h"

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
        if (const int rc = view_check(c, fn, view)) return rc;
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
    return launched(c, fn, launch_aerial(g, c->d_trans_f, c->tw, c->th, d_out, s, c->tlut));
}

// The shadowed forms' own arguments: the map's geometry (of sp only width, height, center and extent are read) and its pitch; m gets everything
// but the pointer and the sun.
int shafts_check(csky_ctx* c, const char* fn, const csky_shadow_params* sp, const void* map, size_t pitch_bytes, ShaftsMap& m) {
    if (!sp) return fail(c, CSKY_ERR_INVALID, "%s: the shadow map's params are NULL", fn);
    if (!map) return fail(c, CSKY_ERR_INVALID, "%s: the shadow map is NULL", fn);
    if (sp->width < 1 || sp->width > 8192 || sp->height < 1 || sp->height > 8192) return fail(c, CSKY_ERR_INVALID, "%s: the shadow map's width and height must be in [1, 8192]", fn);
    for (int k = 0; k < 2; k++)
        if (!std::isfinite(sp->center[k]) || !std::isfinite(sp->extent[k]) || !(sp->extent[k] > 0.0f))
            return fail(c, CSKY_ERR_INVALID, "%s: the shadow map's center and extent must be finite, extent > 0", fn);
    if (pitch_bytes < (size_t)sp->width * 2 || pitch_bytes % 2) return fail(c, CSKY_ERR_INVALID, "%s: the shadow map's row pitch must be even and >= 2 * width", fn);
    m.texels = nullptr; m.pitch_h = (uint32_t)(pitch_bytes / 2); m.w = sp->width; m.h = sp->height;
    m.cx = sp->center[0]; m.cz = sp->center[1]; m.ex = sp->extent[0]; m.ez = sp->extent[1];
    m.lx = m.ly = m.lz = 0.0f;
    return CSKY_OK;
}

// The shadowed launch on stream s, behind whatever the context's stream has done to the table; the map is read on s.  g.sun, which aerial_check
// has found finite, gives the map its sun.
int shafts_launch(csky_ctx* c, const char* fn, const AerialGeom& g, ShaftsMap m, uint2* d_out, hipStream_t s) {
    float l[3];
    shafts_sun(g.sun, l);
    m.lx = l[0]; m.ly = l[1]; m.lz = l[2];
    HIPCHK(c, hipEventRecord(c->ev_aerial, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_aerial, 0));
    return launched(c, fn, launch_shafts(g, m, c->d_trans_f, c->tw, c->th, d_out, s, c->tlut));
}

// csky_apply_cloud_aerial*: the argument and state checks of both forms, and the kernel's argument block with the default filled in.
int cloud_aerial_check(csky_ctx* c, const char* fn, const csky_cloud_aerial_params* ap, CloudAerialGeom& g) {
    if (!ap) return fail(c, CSKY_ERR_INVALID, "%s: params is NULL", fn);
    if (ap->width < 1 || ap->width > 8192 || ap->height < 1 || ap->height > 8192) return fail(c, CSKY_ERR_INVALID, "%s: width and height must be in [1, 8192]", fn);
    if (ap->steps < 0 || ap->steps > 64) return fail(c, CSKY_ERR_INVALID, "%s: steps must be in [1, 64], or 0 for 16", fn);
    g.w = ap->width; g.h = ap->height; g.n = ap->steps ? ap->steps : 16;
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(ap->sun_direction[k])) return fail(c, CSKY_ERR_INVALID, "%s: sun_direction is not finite", fn);
        g.sun[k] = ap->sun_direction[k];
    }
    if (!c->have_trans) return fail(c, CSKY_ERR_STATE, "%s: the transmittance LUT has not been rendered (csky_render_transmittance)", fn);
    return CSKY_OK;
}

// The launch on stream s, behind whatever the context's stream has done to the table; both images are read on s.
int cloud_aerial_launch(csky_ctx* c, const char* fn, const CloudAerialGeom& g, const uint2* d_cloud, const uint2* d_depth, uint2* d_out, hipStream_t s) {
    HIPCHK(c, hipEventRecord(c->ev_aerial, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_aerial, 0));
    return launched(c, fn, launch_cloud_aerial(g, c->d_trans_f, c->tw, c->th, d_cloud, d_depth, d_out, s, c->tlut));
}

// The ray forms' launch: the directions of d_dirs, or of `view` when d_dirs is NULL (read on s like the images).
int cloud_aerial_rays_launch(csky_ctx* c, const char* fn, const CloudAerialGeom& g, const csky_view* view, const float* d_dirs, const uint2* d_cloud,
                             const uint2* d_depth, uint2* d_out, hipStream_t s) {
    const RaysGeom rg = rays_geom(view ? view->basis : nullptr, view ? view->fov_y_degrees : 0.0f, g.w, g.h, (uint32_t)g.w);   // as csky_render_clouds_view's
    HIPCHK(c, hipEventRecord(c->ev_aerial, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_aerial, 0));
    return launched(c, fn, launch_cloud_aerial_rays(g, rg, d_dirs, c->d_trans_f, c->tw, c->th, d_cloud, d_depth, d_out, s, c->tlut));
}

// The ray forms' checks: cloud_aerial_check, and the view's own.
int cloud_aerial_rays_check(csky_ctx* c, const char* fn, const csky_cloud_aerial_params* ap, const csky_view* view, bool is_view, CloudAerialGeom& g) {
    if (is_view && !view) return fail(c, CSKY_ERR_INVALID, "%s: view is NULL", fn);
    if (!ap) return fail(c, CSKY_ERR_INVALID, "%s: params is NULL", fn);
    if (is_view) if (const int rc = view_check(c, fn, view)) return rc;
    return cloud_aerial_check(c, fn, ap, g);
}

// The blocking ray forms: the two images and dirs (NULL for a view) up, the cloud frame, corrected in place, down.
int cloud_aerial_rays_host(csky_ctx* c, const char* fn, const csky_cloud_aerial_params* ap, const csky_view* view, bool is_view, const float* dirs,
                           const uint16_t* cloud, const uint16_t* depth, uint16_t* out) {
    if (!cloud || !depth || !out) return fail(c, CSKY_ERR_INVALID, "%s: cloud, depth or out is NULL", fn);
    if (!is_view && !dirs) return fail(c, CSKY_ERR_INVALID, "%s: dirs_xyz is NULL", fn);
    CloudAerialGeom g;
    int rc; if ((rc = cloud_aerial_rays_check(c, fn, ap, view, is_view, g)) || (rc = bind(c))) return rc;
    const size_t n = (size_t)g.w * g.h, nb = n * 8, db = is_view ? 0 : n * 3 * sizeof(float);
    HostCall hc = host_call(c, fn, {nb, nb, db});
    hc.up(0, cloud, nb);
    hc.up(1, depth, nb);
    hc.up(2, dirs, db);
    hc.step([&] { return cloud_aerial_rays_launch(c, fn, g, view, is_view ? nullptr : hc.at<float>(2), hc.at<uint2>(0), hc.at<uint2>(1), hc.at<uint2>(0), c->stream); });
    hc.down(out, 0, nb);
    return hc.finish();
}

}  // namespace

extern "C" {

int csky_apply_cloud_aerial_dirs(csky_ctx* c, const csky_cloud_aerial_params* ap, const float* dirs, const uint16_t* cloud, const uint16_t* depth, uint16_t* out) {
    const char* fn = "csky_apply_cloud_aerial_dirs";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return cloud_aerial_rays_host(c, fn, ap, nullptr, false, dirs, cloud, depth, out);
}

int csky_apply_cloud_aerial_view(csky_ctx* c, const csky_cloud_aerial_params* ap, const csky_view* view, const uint16_t* cloud, const uint16_t* depth, uint16_t* out) {
    const char* fn = "csky_apply_cloud_aerial_view";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    return cloud_aerial_rays_host(c, fn, ap, view, true, nullptr, cloud, depth, out);
}

int csky_apply_cloud_aerial_dirs_device(csky_ctx* c, const csky_cloud_aerial_params* ap, const void* d_dirs, const void* d_cloud, const void* d_depth, void* d_out,
                                        void* hip_stream) {
    const char* fn = "csky_apply_cloud_aerial_dirs_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_dirs || !d_cloud || !d_depth || !d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_dirs_xyz, d_cloud, d_depth or d_out is NULL", fn);
    CloudAerialGeom g;
    int rc; if ((rc = cloud_aerial_rays_check(c, fn, ap, nullptr, false, g)) || (rc = bind(c))) return rc;
    return cloud_aerial_rays_launch(c, fn, g, nullptr, static_cast<const float*>(d_dirs), static_cast<const uint2*>(d_cloud), static_cast<const uint2*>(d_depth),
                                    static_cast<uint2*>(d_out), stream_of(c, hip_stream));
}

int csky_apply_cloud_aerial_view_device(csky_ctx* c, const csky_cloud_aerial_params* ap, const csky_view* view, const void* d_cloud, const void* d_depth, void* d_out,
                                        void* hip_stream) {
    const char* fn = "csky_apply_cloud_aerial_view_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_cloud || !d_depth || !d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_cloud, d_depth or d_out is NULL", fn);
    CloudAerialGeom g;
    int rc; if ((rc = cloud_aerial_rays_check(c, fn, ap, view, true, g)) || (rc = bind(c))) return rc;
    return cloud_aerial_rays_launch(c, fn, g, view, nullptr, static_cast<const uint2*>(d_cloud), static_cast<const uint2*>(d_depth), static_cast<uint2*>(d_out),
                                    stream_of(c, hip_stream));
}

int csky_apply_cloud_aerial_device(csky_ctx* c, const csky_cloud_aerial_params* ap, const void* d_cloud, const void* d_depth, void* d_out, void* hip_stream) {
    const char* fn = "csky_apply_cloud_aerial_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_cloud || !d_depth || !d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_cloud, d_depth or d_out is NULL", fn);
    CloudAerialGeom g;
    int rc; if ((rc = cloud_aerial_check(c, fn, ap, g)) || (rc = bind(c))) return rc;
    return cloud_aerial_launch(c, fn, g, static_cast<const uint2*>(d_cloud), static_cast<const uint2*>(d_depth), static_cast<uint2*>(d_out),
                               stream_of(c, hip_stream));
}

int csky_apply_cloud_aerial(csky_ctx* c, const csky_cloud_aerial_params* ap, const uint16_t* cloud, const uint16_t* depth, uint16_t* out) {
    const char* fn = "csky_apply_cloud_aerial";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!cloud || !depth || !out) return fail(c, CSKY_ERR_INVALID, "%s: cloud, depth or out is NULL", fn);
    CloudAerialGeom g;
    int rc; if ((rc = cloud_aerial_check(c, fn, ap, g)) || (rc = bind(c))) return rc;
    const size_t nb = (size_t)g.w * g.h * 8;
    HostCall hc = host_call(c, fn, {nb, nb});                                   // the cloud frame, corrected in place, then the depth frame
    hc.up(0, cloud, nb);
    hc.up(1, depth, nb);
    hc.step([&] { return cloud_aerial_launch(c, fn, g, hc.at<uint2>(0), hc.at<uint2>(1), hc.at<uint2>(0), c->stream); });
    hc.down(out, 0, nb);
    return hc.finish();
}

int csky_render_aerial_perspective_device(csky_ctx* c, const csky_aerial_params* ap, const csky_view* view, void* d_out, void* hip_stream) {
    const char* fn = "csky_render_aerial_perspective_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    AerialGeom g;
    int rc; if ((rc = aerial_check(c, fn, ap, view, g)) || (rc = bind(c))) return rc;
    return aerial_launch(c, fn, g, static_cast<uint2*>(d_out), stream_of(c, hip_stream));
}

int csky_render_aerial_perspective(csky_ctx* c, const csky_aerial_params* ap, const csky_view* view, uint16_t* out) {
    const char* fn = "csky_render_aerial_perspective";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    AerialGeom g;
    int rc; if ((rc = aerial_check(c, fn, ap, view, g)) || (rc = bind(c))) return rc;
    const size_t nb = (size_t)g.d * g.h * g.w * 8;
    HostCall hc = host_call(c, fn, {nb});
    hc.step([&] { return aerial_launch(c, fn, g, hc.at<uint2>(0), c->stream); });
    hc.down(out, 0, nb);
    return hc.finish();
}

int csky_render_aerial_perspective_shadowed_device(csky_ctx* c, const csky_aerial_params* ap, const csky_view* view, const csky_shadow_params* sp,
                                                   const void* d_map, size_t pitch, void* d_out, void* hip_stream) {
    const char* fn = "csky_render_aerial_perspective_shadowed_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    AerialGeom g; ShaftsMap m;
    int rc; if ((rc = shafts_check(c, fn, sp, d_map, pitch, m)) || (rc = aerial_check(c, fn, ap, view, g)) || (rc = bind(c))) return rc;
    m.texels = static_cast<const uint16_t*>(d_map);
    return shafts_launch(c, fn, g, m, static_cast<uint2*>(d_out), stream_of(c, hip_stream));
}

int csky_render_aerial_perspective_shadowed(csky_ctx* c, const csky_aerial_params* ap, const csky_view* view, const csky_shadow_params* sp,
                                            const uint16_t* map, uint16_t* out) {
    const char* fn = "csky_render_aerial_perspective_shadowed";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    AerialGeom g; ShaftsMap m;
    int rc; if ((rc = shafts_check(c, fn, sp, map, sp ? (size_t)sp->width * 2 : 0, m)) || (rc = aerial_check(c, fn, ap, view, g)) || (rc = bind(c))) return rc;
    const size_t nb = (size_t)g.d * g.h * g.w * 8, mb = (size_t)m.w * m.h * 2;
    HostCall hc = host_call(c, fn, {mb, nb});                                   // the caller's map, then the volume
    hc.up(0, map, mb);
    hc.step([&] { m.texels = hc.at<uint16_t>(0); return shafts_launch(c, fn, g, m, hc.at<uint2>(1), c->stream); });
    hc.down(out, 1, nb);
    return hc.finish();
}

int csky_aerial_shadow_rect(const csky_aerial_params* ap, float center[2], float extent[2]) {
    const char* fn = "csky_aerial_shadow_rect";
    if (!ap || !center || !extent) return fail(nullptr, CSKY_ERR_INVALID, "%s: NULL argument", fn);
    const float far_km = ap->far_km == 0.0f ? 32.0f : ap->far_km;
    if (!std::isfinite(far_km) || !(far_km > 0.0f) || !(far_km <= 2000.0f)) return fail(nullptr, CSKY_ERR_INVALID, "%s: far_km must be finite and in (0, 2000], or 0 for 32", fn);
    for (int k = 0; k < 3; k++) if (!std::isfinite(ap->sun_direction[k])) return fail(nullptr, CSKY_ERR_INVALID, "%s: sun_direction is not finite", fn);
    float ce[2], ex[2];
    if (!shafts_rect(ap->sun_direction, far_km * 1000.0f, ce, ex)) return fail(nullptr, CSKY_ERR_INVALID, "%s: the sun is not above the horizon: no shadow map applies", fn);
    for (int k = 0; k < 2; k++)
        if (!(std::fabs(ce[k]) + 0.5f * ex[k] <= 1.0e6f)) return fail(nullptr, CSKY_ERR_INVALID, "%s: the sun is too low: the rectangle leaves the 1e6 m range of csky_shadow_params", fn);
    for (int k = 0; k < 2; k++) { center[k] = ce[k]; extent[k] = ex[k]; }
    return CSKY_OK;
}

}  // extern "C"
