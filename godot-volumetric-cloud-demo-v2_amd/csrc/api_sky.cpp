// api_sky.cpp -- the sky's C ABI: the compositor (csky_composite_sky / _view: clouds.gdshader sky() on a panorama or a camera view) and the
// radiance cubemap (csky_render_radiance*, csky_prefilter_cube: the same sky() evaluated into a cube map (layer 0) and GGX-prefiltered into
// roughness layers, radiance_core.h, radiance.hip).  The blocking forms work in the context's stage (host_stage.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "context.h"
#include "radiance_core.h"
#include "rays_core.h"

using namespace csky;

namespace {

// the compositor's arguments for the panorama (view_mode 0) from the caller's parameters and DEVICE copies of its four images
CompositeArgs composite_args(const csky_ctx* c, const csky_composite_params* p, const void* cloud_from, const void* cloud_to, const void* sky_from,
                             const void* sky_to) {
    CompositeArgs a;
    a.cloud_from = static_cast<const uint16_t*>(cloud_from); a.cloud_to = static_cast<const uint16_t*>(cloud_to); a.cw = p->cloud_w; a.ch = p->cloud_h;
    a.sky_from = static_cast<const uint16_t*>(sky_from); a.sky_to = static_cast<const uint16_t*>(sky_to); a.sw = p->sky_w; a.sh = p->sky_h;
    a.trans = c->d_trans_f; a.tw = c->tw; a.th = c->th;
    a.blend_amount = p->blend_amount; a.sun_disk_scale = p->sun_disk_scale;
    a.sun[0] = p->light_direction[0]; a.sun[1] = p->light_direction[1]; a.sun[2] = p->light_direction[2];
    a.out_w = p->out_w; a.out_h = p->out_h;
    a.view_mode = 0; a.tan_half_fov_y = 1.0f; a.aspect = 1.0f; a.cloud_mode = 0;
    for (int k = 0; k < 9; k++) a.cam[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    return a;
}
int composite_impl(csky_ctx* c, const csky_composite_params* p, const csky_view* view, const uint16_t* cloud_from, const uint16_t* cloud_to,
                   const uint16_t* sky_from, const uint16_t* sky_to, uint16_t* out, int cloud_mode = 0) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_composite_sky: ctx is NULL");
    if (!p || !cloud_from || !cloud_to || !sky_from || !sky_to || !out) return fail(c, CSKY_ERR_INVALID, "csky_composite_sky: NULL argument");
    if (p->out_w < 1 || p->out_h < 1 || p->cloud_w < 1 || p->cloud_h < 1 || p->sky_w < 1 || p->sky_h < 1 || p->out_w > 16384 || p->out_h > 16384)
        return fail(c, CSKY_ERR_INVALID, "csky_composite_sky: bad image size");
    if (cloud_mode == 1 && (p->cloud_w != p->out_w || p->cloud_h != p->out_h))
        return fail(c, CSKY_ERR_INVALID, "csky_composite_view_frames: cloud_w x cloud_h must equal out_w x out_h (the cloud images are view frames)");
    int rc; if ((rc = bind(c))) return rc;
    if ((rc = ensure_default_trans(c))) return rc;            // source_transmittance, clouds_material.tres
    const size_t cb = (size_t)p->cloud_w * p->cloud_h * 8, sb = (size_t)p->sky_w * p->sky_h * 8, ob = (size_t)p->out_w * p->out_h * 8;
    HostCall hc = host_call(c, "csky_composite_sky", {cb, cb, sb, sb, ob});
    hc.up(0, cloud_from, cb); hc.up(1, cloud_to, cb); hc.up(2, sky_from, sb); hc.up(3, sky_to, sb);
    hc.step([&] {
        CompositeArgs a = composite_args(c, p, hc.at<void>(0), hc.at<void>(1), hc.at<void>(2), hc.at<void>(3));
        if (view) {
            composite_view_args(a, view->basis, view->fov_y_degrees, p->out_w, p->out_h);   // rays_core.h: the view march's projection is this one
            a.cloud_mode = cloud_mode;
        }
        const hipError_t e = launch_composite(a, hc.at<uint2>(4), c->stream, c->tlut);
        return e == hipSuccess ? CSKY_OK : fail(c, CSKY_ERR_HIP, "csky_composite_sky: %s", hipGetErrorString(e));
    });
    hc.down(out, 4, ob);
    return hc.finish();
}

// ---- radiance cubemap
int rad_args(csky_ctx* c, const char* fn, const csky_radiance_params* rp, int first, int n, int& S, int& L, int& Ss) {
    if (!rp) return fail(c, CSKY_ERR_INVALID, "%s: NULL argument", fn);
    S = rp->face_size; L = rp->layers; Ss = rp->source_size == 0 ? std::min(S, 64) : rp->source_size;
    if (S < 8 || S > 512 || (S & (S - 1))) return fail(c, CSKY_ERR_INVALID, "%s: face_size %d is not a power of two in [8, 512]", fn, S);
    if (L < 1 || L > RAD_MAX_LAYERS) return fail(c, CSKY_ERR_INVALID, "%s: layers %d not in [1, %d]", fn, L, RAD_MAX_LAYERS);
    if (Ss < 1 || Ss > S || (Ss & (Ss - 1))) return fail(c, CSKY_ERR_INVALID, "%s: source_size %d is not 0 or a power of two <= face_size", fn, rp->source_size);
    if (first < 0 || n < 1 || first >= L || n > L - first) return fail(c, CSKY_ERR_INVALID, "%s: layer range [%d, %d + %d) not within [0, %d)", fn, first, first, n, L);
    return CSKY_OK;
}
// table storage and the block cones of an (S, Ss) geometry (the cones depend on the geometry alone: rebuilt when it changes)
int rad_prepare(csky_ctx* c, csky_ctx::RadSet& r, int S, int Ss, hipStream_t s) {
    int rc;
    if ((rc = r.tab.grow(c, (size_t)12 * Ss * Ss))) return rc;
    if (r.cones_ss != Ss || r.src_cones.count() < (size_t)rad_block_count(Ss)) {
        r.cones_ss = 0;
        if ((rc = r.src_cones.grow(c, (size_t)rad_block_count(Ss)))) return rc;
        HIPCHK(c, launch_radiance_cones(Ss, r.src_cones, s));
        r.cones_ss = Ss;
    }
    if (r.cones_s != S || r.out_cones.count() < (size_t)rad_block_count(S)) {
        r.cones_s = 0;
        if ((rc = r.out_cones.grow(c, (size_t)rad_block_count(S)))) return rc;
        HIPCHK(c, launch_radiance_cones(S, r.out_cones, s));
        r.cones_s = S;
    }
    return CSKY_OK;
}
// layers [lo, hi) (lo >= 1) from the set's table into d_lo (= layer lo)
int rad_filter(csky_ctx* c, const csky_ctx::RadSet& r, int S, int L, int Ss, int lo, int hi, uint2* d_lo, hipStream_t s) {
    if (lo >= hi) return CSKY_OK;
    RadLayer ly[RAD_MAX_LAYERS - 1];
    for (int k = lo; k < hi; k++) ly[k - lo] = rad_layer(k, L);
    const char* cull = getenv("CSKY_RADIANCE_CULL");                  // A/B switch: 0 = every source block of every receiver block
    HIPCHK(c, launch_radiance_filter(r.tab, r.src_cones, r.out_cones, S, Ss, ly, hi - lo, !(cull && cull[0] == '0'), d_lo, s));
    return CSKY_OK;
}
// layers [first, first + n) into d_first (= layer `first` of the caller's array); first == 0 renders the faces and takes the snapshot
int radiance_dev(csky_ctx* c, const char* fn, const csky_composite_params* p, int S, int L, int Ss, const void* cloud_from, const void* cloud_to,
                 const void* sky_from, const void* sky_to, int first, int n, uint2* d_first, hipStream_t s) {
    int rc;
    const size_t plane = (size_t)6 * S * S;
    if (first == 0) {
        if ((rc = ensure_default_trans(c))) return rc;                                    // source_transmittance, clouds_material.tres
        HIPCHK(c, hipEventRecord(c->ev_rad, c->stream));                                  // the LUT may have been rendered there
        HIPCHK(c, hipStreamWaitEvent(s, c->ev_rad, 0));
        c->rad.valid = false;
        CompositeArgs a = composite_args(c, p, cloud_from, cloud_to, sky_from, sky_to);
        a.out_w = S; a.out_h = 6 * S; a.view_mode = 2;
        HIPCHK(c, launch_composite(a, d_first, s, c->tlut));
        if ((rc = rad_prepare(c, c->rad, S, Ss, s))) return rc;
        HIPCHK(c, launch_radiance_source(reinterpret_cast<const uint16_t*>(d_first), S, Ss, c->rad.tab, s));
        c->rad.S = S; c->rad.L = L; c->rad.Ss = Ss; c->rad.valid = true;
    } else if (!c->rad.valid) {
        return fail(c, CSKY_ERR_STATE, "%s: layer %d requested before a call that renders layer 0", fn, first);
    } else if (c->rad.S != S || c->rad.L != L || c->rad.Ss != Ss) {
        return fail(c, CSKY_ERR_STATE, "%s: the snapshot is of (face_size, layers, source_size) = (%d, %d, %d), this call asks for (%d, %d, %d): render layer 0 again",
                    fn, c->rad.S, c->rad.L, c->rad.Ss, S, L, Ss);
    }
    const int lo = std::max(first, 1);
    return rad_filter(c, c->rad, S, L, Ss, lo, first + n, d_first + (size_t)(lo - first) * plane, s);
}
int rad_sky_args(csky_ctx* c, const char* fn, const csky_composite_params* p, int S, const void* cf, const void* ct, const void* sf, const void* st) {
    if (!p || !cf || !ct || !sf || !st) return fail(c, CSKY_ERR_INVALID, "%s: NULL sky argument (a call that renders layer 0 needs all of them)", fn);
    if (p->out_w != S || p->out_h != S) return fail(c, CSKY_ERR_INVALID, "%s: sky out_w x out_h must be face_size x face_size", fn);
    if (p->cloud_w < 1 || p->cloud_h < 1 || p->sky_w < 1 || p->sky_h < 1 || p->cloud_w > 16384 || p->cloud_h > 16384 || p->sky_w > 16384 || p->sky_h > 16384)
        return fail(c, CSKY_ERR_INVALID, "%s: bad image size", fn);
    return CSKY_OK;
}

}  // namespace

extern "C" {

int csky_composite_sky(csky_ctx* c, const csky_composite_params* p, const uint16_t* cloud_from, const uint16_t* cloud_to, const uint16_t* sky_from,
                       const uint16_t* sky_to, uint16_t* out) {
    return composite_impl(c, p, nullptr, cloud_from, cloud_to, sky_from, sky_to, out);
}
int csky_composite_view(csky_ctx* c, const csky_composite_params* p, const csky_view* view, const uint16_t* cloud_from, const uint16_t* cloud_to,
                        const uint16_t* sky_from, const uint16_t* sky_to, uint16_t* out) {
    if (!view) return fail(c, CSKY_ERR_INVALID, "csky_composite_view: view is NULL");
    if (!(view->fov_y_degrees > 0.0f && view->fov_y_degrees < 180.0f)) return fail(c, CSKY_ERR_INVALID, "csky_composite_view: fov_y_degrees must be in (0, 180)");
    return composite_impl(c, p, view, cloud_from, cloud_to, sky_from, sky_to, out);
}
int csky_composite_view_frames(csky_ctx* c, const csky_composite_params* p, const csky_view* view, const uint16_t* cloud_from, const uint16_t* cloud_to,
                               const uint16_t* sky_from, const uint16_t* sky_to, uint16_t* out) {
    if (!view) return fail(c, CSKY_ERR_INVALID, "csky_composite_view_frames: view is NULL");
    if (!(view->fov_y_degrees > 0.0f && view->fov_y_degrees < 180.0f)) return fail(c, CSKY_ERR_INVALID, "csky_composite_view_frames: fov_y_degrees must be in (0, 180)");
    return composite_impl(c, p, view, cloud_from, cloud_to, sky_from, sky_to, out, 1);
}

int csky_render_radiance_device(csky_ctx* c, const csky_composite_params* p, const csky_radiance_params* rp, const void* d_cloud_from, const void* d_cloud_to,
                                const void* d_sky_from, const void* d_sky_to, int first_layer, int n_layers, void* d_out, void* hip_stream) {
    static const char* fn = "csky_render_radiance_device";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    int S, L, Ss, rc;
    if ((rc = rad_args(c, fn, rp, first_layer, n_layers, S, L, Ss))) return rc;
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "%s: d_out is NULL", fn);
    if (first_layer == 0 && (rc = rad_sky_args(c, fn, p, S, d_cloud_from, d_cloud_to, d_sky_from, d_sky_to))) return rc;
    if ((rc = bind(c))) return rc;
    return radiance_dev(c, fn, p, S, L, Ss, d_cloud_from, d_cloud_to, d_sky_from, d_sky_to, first_layer, n_layers,
                        static_cast<uint2*>(d_out) + (size_t)first_layer * 6 * S * S, stream_of(c, hip_stream));
}
int csky_render_radiance(csky_ctx* c, const csky_composite_params* p, const csky_radiance_params* rp, const uint16_t* cloud_from, const uint16_t* cloud_to,
                         const uint16_t* sky_from, const uint16_t* sky_to, int first_layer, int n_layers, uint16_t* out) {
    static const char* fn = "csky_render_radiance";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    int S, L, Ss, rc;
    if ((rc = rad_args(c, fn, rp, first_layer, n_layers, S, L, Ss))) return rc;
    if (!out) return fail(c, CSKY_ERR_INVALID, "%s: out is NULL", fn);
    if (first_layer == 0 && (rc = rad_sky_args(c, fn, p, S, cloud_from, cloud_to, sky_from, sky_to))) return rc;
    if ((rc = bind(c))) return rc;
    const size_t cb = first_layer == 0 ? (size_t)p->cloud_w * p->cloud_h * 8 : 0, sb = first_layer == 0 ? (size_t)p->sky_w * p->sky_h * 8 : 0;
    const size_t ob = (size_t)n_layers * 6 * S * S * 8;
    HostCall hc = host_call(c, fn, {cb, cb, sb, sb, ob});                             // the inputs are 0 bytes, and not uploaded, unless layer 0 is rendered
    hc.up(0, cloud_from, cb); hc.up(1, cloud_to, cb); hc.up(2, sky_from, sb); hc.up(3, sky_to, sb);
    hc.step([&] { return radiance_dev(c, fn, p, S, L, Ss, hc.at<void>(0), hc.at<void>(1), hc.at<void>(2), hc.at<void>(3), first_layer, n_layers, hc.at<uint2>(4), c->stream); });
    hc.down(out + (size_t)first_layer * 6 * S * S * 4, 4, ob);
    return hc.finish();
}
int csky_prefilter_cube(csky_ctx* c, const uint16_t* cube, int face_size, int layers, int source_size, int first_layer, int n_layers, uint16_t* out) {
    static const char* fn = "csky_prefilter_cube";
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "%s: ctx is NULL", fn);
    const csky_radiance_params rp = {face_size, layers, source_size};
    int S, L, Ss, rc;
    if ((rc = rad_args(c, fn, &rp, first_layer, n_layers, S, L, Ss))) return rc;
    if (!cube || !out) return fail(c, CSKY_ERR_INVALID, "%s: NULL argument", fn);
    if ((rc = bind(c))) return rc;
    const size_t plane = (size_t)6 * S * S, lb = plane * 8;
    const int lo = std::max(first_layer, 1), hi = first_layer + n_layers;
    const size_t ob = lb * (size_t)(hi - lo);                         // layers [lo, hi): none when only layer 0 is asked for
    HostCall hc = host_call(c, fn, {lb, ob});
    hc.up(0, cube, lb);
    if (ob) hc.step([&] {
        if (const int r = rad_prepare(c, c->rad_pf, S, Ss, c->stream)) return r;
        HIPCHK(c, launch_radiance_source(hc.at<uint16_t>(0), S, Ss, c->rad_pf.tab, c->stream));
        return rad_filter(c, c->rad_pf, S, L, Ss, lo, hi, hc.at<uint2>(1), c->stream);
    });
    hc.down(out + (size_t)lo * plane * 4, 1, ob);
    if ((rc = hc.finish())) return rc;
    if (first_layer == 0) memcpy(out, cube, lb);                      // layer 0 is the input
    return CSKY_OK;
}

}  // extern "C"
