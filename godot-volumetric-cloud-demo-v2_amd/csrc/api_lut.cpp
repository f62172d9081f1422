// api_lut.cpp -- the LUTs' C ABI: the transmittance table and its mapping, the sky LUT in its whole and rows form, the rows cache, the read-backs
// and copies out.  What a context holds as its sky LUT is csky_ctx::lut (context.h); it changes through the transitions of sky_lut_reuse.h alone.
// Mirrors sky_lut.gd (`render_lut`) and transmittance_lut.gd (`_initialize_compute_code`).
#include "context.h"
#include "lut_core.h"

using namespace csky;

namespace {

int ensure_trans(csky_ctx* c, int w, int h) {
    if (c->d_trans_h && c->tw == w && c->th == h) return CSKY_OK;
    int rc; if ((rc = c->d_trans_h.alloc(c, (size_t)w * h * 4))) return rc;
    if ((rc = c->d_trans_f.alloc(c, (size_t)w * h))) return rc;
    c->tw = w; c->th = h; c->have_trans = false; return CSKY_OK;
}

bool event_done(hipEvent_t ev) {
    if (hipEventQuery(ev) == hipSuccess) return true;
    (void)hipGetLastError();                                   // hipErrorNotReady is an answer, not a failure to resurface later
    return false;
}

}  // namespace

namespace csky {

// (the event protocol: context.h, above RowsCache)
int RowsCache::fill(csky_ctx* c, const void* d_rows, size_t px, hipStream_t s) {
    int rc;
    if (!ev_fill) {
        if ((rc = ev_fill.create(c, hipEventDisableTiming))) return rc;
        for (Event& ev : ev_read) if ((rc = ev.create(c, hipEventDisableTiming))) return rc;
    }
    const bool regrow = d.count() < px;
    for (int k = 0; k < RING; k++) {
        if (!read_pending[k]) continue;
        if (regrow) HIPCHK(c, hipEventSynchronize(ev_read[k]));
        else if (!event_done(ev_read[k])) HIPCHK(c, hipStreamWaitEvent(s, ev_read[k], 0));
        read_pending[k] = false;
    }
    if (!fill_done) {
        if (regrow) HIPCHK(c, hipEventSynchronize(ev_fill));
        else if (!event_done(ev_fill)) HIPCHK(c, hipStreamWaitEvent(s, ev_fill, 0));
    }
    if (regrow && (rc = d.alloc(c, px))) return rc;
    HIPCHK(c, hipMemcpyAsync(d, d_rows, px * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(ev_fill, s));
    fill_done = false;
    return CSKY_OK;
}
int RowsCache::read(csky_ctx* c, void* d_rows_out, size_t px, hipStream_t s) {
    if (!fill_done) {
        if (event_done(ev_fill)) fill_done = true;
        else HIPCHK(c, hipStreamWaitEvent(s, ev_fill, 0));
    }
    const int k = read_cur;
    if (read_pending[k] && !event_done(ev_read[k])) HIPCHK(c, hipStreamWaitEvent(s, ev_read[k], 0));
    HIPCHK(c, hipMemcpyAsync(d_rows_out, d, px * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipEventRecord(ev_read[k], s));
    read_pending[k] = true; read_cur = (k + 1) % RING;
    return CSKY_OK;
}

int ensure_sky(csky_ctx* c, int w, int h) {
    SkyLut& l = c->lut;
    if (l.aw == w && l.ah == h) return CSKY_OK;
    l.drop(); l.aw = l.ah = 0;                                  // whatever the slots held goes, BEFORE they do: a failure below leaves a context that holds nothing
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));  // a size change is rare: drain the context's stream (every reader of the LUT runs there), rebuild both slots
    for (int k = 0; k < 2; k++) {
        int rc; if ((rc = l.ring_h[k].alloc(c, (size_t)w * h * 4))) return rc;
        if ((rc = l.ring_f[k].alloc(c, (size_t)w * h))) return rc;
    }
    l.cur = 0; l.aw = w; l.ah = h; return CSKY_OK;
}

int render_trans_dev(csky_ctx* c, int w, int h, hipStream_t s) {
    c->lut.st.table_replaced();
    int rc; if ((rc = ensure_trans(c, w, h))) return rc;
    HIPCHK(c, launch_transmittance(w, h, c->d_trans_h, c->d_trans_f, s, c->tlut));
    c->have_trans = true; return CSKY_OK;
}

int ensure_default_trans(csky_ctx* c) { return c->have_trans ? CSKY_OK : render_trans_dev(c, 256, 64, c->stream); }

int lut_size(csky_ctx* c, const char* fn, const float texture_size[2], int& w, int& h) {
    w = (int)texture_size[0]; h = (int)texture_size[1];
    if (w < 1 || h < 1 || w > 8192 || h > 8192) return fail(c, CSKY_ERR_INVALID, "%s: texture_size out of range", fn);
    return CSKY_OK;
}

}  // namespace csky

extern "C" {

int csky_set_transmittance_mapping(csky_ctx* c, int mapping) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_transmittance_mapping: ctx is NULL");
    if (mapping != CSKY_TLUT_REFERENCE && mapping != CSKY_TLUT_BRUNETON) return fail(c, CSKY_ERR_INVALID, "csky_set_transmittance_mapping: CSKY_TLUT_REFERENCE (0) or CSKY_TLUT_BRUNETON (1)");
    if (mapping == c->tlut) return CSKY_OK;
    int rc; if ((rc = bind(c))) return rc;
    HIPCHK(c, hipDeviceSynchronize());                         // readers of the old table may be in flight, on caller streams too (csky_render_transmittance)
    // everything rendered through the old table goes: the table itself (re-rendered on demand), the sky LUT and the radiance snapshot
    c->tlut = mapping; c->have_trans = false; c->rad.valid = false;
    c->lut.drop(); c->lut.st.table_replaced();
    return CSKY_OK;
}
int csky_get_transmittance_mapping(const csky_ctx* c) { return c ? c->tlut : CSKY_ERR_INVALID; }
int csky_set_sky_lut_reuse(csky_ctx* c, int enabled) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_set_sky_lut_reuse: ctx is NULL");
    if (enabled != 0 && enabled != 1) return fail(c, CSKY_ERR_INVALID, "csky_set_sky_lut_reuse: 0 (a launch per call) or 1 (reuse, the default)");
    c->lut.st.set_reuse(enabled != 0);
    return CSKY_OK;
}
int64_t csky_sky_lut_launches(const csky_ctx* c) { return c ? (int64_t)c->lut.launches : (int64_t)CSKY_ERR_INVALID; }
int csky_transmittance_uv(int mapping, int w, int h, float r_km, float mu, float uv[2], int* hits_ground) {
    if (!uv) return fail(nullptr, CSKY_ERR_INVALID, "csky_transmittance_uv: uv is NULL");
    if (mapping == CSKY_TLUT_REFERENCE) {                      // transmittance_from_lut (sky-lut.glsl:137-142); the table stores every ray
        if (w < 1 || h < 1) return fail(nullptr, CSKY_ERR_INVALID, "csky_transmittance_uv: empty table");
        uv[0] = sat(mu * 0.5f + 0.5f); uv[1] = sat((r_km - EARTH_RADIUS) / ATMOSPHERE_THICKNESS);
        if (hits_ground) *hits_ground = 0;
        return CSKY_OK;
    }
    if (mapping != CSKY_TLUT_BRUNETON) return fail(nullptr, CSKY_ERR_INVALID, "csky_transmittance_uv: CSKY_TLUT_REFERENCE (0) or CSKY_TLUT_BRUNETON (1)");
    if (w < 2 || h < 2) return fail(nullptr, CSKY_ERR_INVALID, "csky_transmittance_uv: CSKY_TLUT_BRUNETON needs a table of at least 2 x 2");
    const bool hit = tlut_uv(w, h, r_km, mu, uv[0], uv[1]);
    if (hits_ground) *hits_ground = hit ? 1 : 0;
    return CSKY_OK;
}

int csky_render_transmittance(csky_ctx* c, const csky_transmittance_params* p, uint16_t* out) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_transmittance: ctx is NULL");
    if (!p) return fail(c, CSKY_ERR_INVALID, "csky_render_transmittance: params is NULL");
    int w, h, rc; if ((rc = lut_size(c, "csky_render_transmittance", p->texture_size, w, h))) return rc;
    if (c->tlut == CSKY_TLUT_BRUNETON && (w < 2 || h < 2)) return fail(c, CSKY_ERR_INVALID, "csky_render_transmittance: CSKY_TLUT_BRUNETON needs a table of at least 2 x 2 (texel centres sit on the ends of both ranges)");
    if ((rc = bind(c))) return rc;
    // sky LUTs in flight read the old transmittance LUT: whole ones and the set-ups' own texels on the prologue stream, a rank's rows
    // (csky_render_sky_lut_rows_device) on CALLER streams; the LUT is rendered once at load (transmittance_lut.gd:15-18), so wait for the device
    HIPCHK(c, hipDeviceSynchronize());
    if ((rc = render_trans_dev(c, w, h, c->stream))) return rc;
    if (out) HIPCHK(c, hipMemcpyAsync(out, c->d_trans_h, (size_t)w * h * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_render_sky_lut_device(csky_ctx* c, const csky_sky_params* p, void* hip_stream) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_sky_lut: ctx is NULL");
    if (!p) return fail(c, CSKY_ERR_INVALID, "csky_render_sky_lut: params is NULL");
    int w, h, rc; if ((rc = lut_size(c, "csky_render_sky_lut", p->texture_size, w, h))) return rc;
    if ((rc = bind(c))) return rc;
    (void)hip_stream;   // the LUT has no inputs of the caller's: it is rendered on the context's stream and its consumers are ordered by events
    if ((rc = ensure_default_trans(c))) return rc;
    if ((rc = ensure_sky(c, w, h))) return rc;
    // The LUT is a function of the sun, its size and the transmittance table alone, and a host refreshes it every pass whether the sun moved or not
    // (cloud_sky.gd:187 against sun.gd:17): the same request as the one the current slot was rendered from launches nothing and leaves the ring where
    // it is.  Every consumer (the frame set-ups, the copies out) runs on `stream`, behind the launch that filled the slot.
    SkyLut& l = c->lut;
    const SkyLutKey req = sky_lut_key(p->sun_direction, w, h, c->tlut, l.st.trans_gen);
    if (sky_lut_whole_hit(l.st.sky_key, req, sky_lut_state(c))) return CSKY_OK;
    l.st.touch();                                              // (the key is set again below, once the launch went through)
    const int k = l.render_slot();
    HIPCHK(c, launch_sky_lut(w, h, p->sun_direction, c->d_trans_f, c->tw, c->th, l.ring_h[k], l.ring_f[k], c->stream, c->tlut));
    l.launches++;
    l.publish(k); l.st.became_whole(req);
    return CSKY_OK;
}
int csky_render_sky_lut_rows_device(csky_ctx* c, const csky_sky_params* p, int first_row, int row_stride, void* d_rows_out, size_t capacity_bytes, void* hip_stream) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_render_sky_lut_rows_device: ctx is NULL");
    if (!p || !d_rows_out) return fail(c, CSKY_ERR_INVALID, "csky_render_sky_lut_rows_device: NULL argument");
    int w, h, rc; if ((rc = lut_size(c, "csky_render_sky_lut_rows_device", p->texture_size, w, h))) return rc;
    if (first_row < 0 || row_stride < 1 || first_row >= row_stride) return fail(c, CSKY_ERR_INVALID, "csky_render_sky_lut_rows_device: need 0 <= first_row < row_stride");
    const int n_rows = first_row < h ? (h - first_row + row_stride - 1) / row_stride : 0;
    if (capacity_bytes < (size_t)n_rows * w * 8) return fail(c, CSKY_ERR_INVALID, "csky_render_sky_lut_rows_device: %zu bytes given, %d rows of %d bytes needed", capacity_bytes, n_rows, w * 8);
    if ((rc = bind(c))) return rc;
    if (!c->have_trans) {                                       // (rendered on the context's stream: the caller's stream reads it)
        if ((rc = ensure_default_trans(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    // the rows have no consumer inside the library: they are rendered on the CALLER's stream, in order with the bands they travel with.
    // (Round 5 measured them on a side stream BESIDE the march that follows, joined behind it: a 1/8 share one frame at a time 0.409 -> 0.460 ms, eight
    // in flight 0.241 -> 0.244: two more cross-stream hops cost more than the rows they take off the critical path; profiles/r05/rows_overlap_ab.txt.)
    hipStream_t s = stream_of(c, hip_stream);
    // The caller's buffer differs from frame to frame, so the rows of an unchanged request cannot simply stay where they are: the context keeps a
    // copy of the last rows it rendered, and the same request again is one device copy of them on the caller's stream instead of the kernel.
    // A request that differs renders into the caller's buffer as ever and leaves its copy behind (a sun that moves every frame pays that copy alone).
    SkyLutHeld& st = c->lut.st;
    const size_t px = (size_t)n_rows * w;
    const SkyLutKey req = sky_lut_key(p->sun_direction, w, h, c->tlut, st.trans_gen, first_row, row_stride);
    st.touch();                                                 // the ring's whole LUT, if any, is no longer what the set-ups use (on a hit of the cache too: a csky_multi handle's reuse asks the epoch)
    if (px && sky_lut_rows_hit(st.rows_key, req, st.reuse)) {
        if ((rc = c->rows_cache.read(c, d_rows_out, px, s))) { st.rows_key.valid = false; return rc; }
    } else {
        st.rows_key.valid = false;
        HIPCHK(c, launch_sky_lut_rows(w, h, first_row, row_stride, p->sun_direction, c->d_trans_f, c->tw, c->th, reinterpret_cast<uint2*>(d_rows_out), nullptr, s, c->tlut));
        if (px) c->lut.launches++;
        if (px && st.reuse) {
            if ((rc = c->rows_cache.fill(c, d_rows_out, px, s))) return rc;
            st.rows_key = req;
        }
    }
    st.became_rows(p->sun_direction, w, h); c->lut.writers.clear();
    return CSKY_OK;
}

int csky_render_sky_lut(csky_ctx* c, const csky_sky_params* p, uint16_t* out) {
    int rc = csky_render_sky_lut_device(c, p, nullptr);
    if (rc) return rc;
    if (out) HIPCHK(c, hipMemcpyAsync(out, c->lut.cur_h(), (size_t)c->lut.aw * c->lut.ah * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CSKY_OK;
}

int csky_read_transmittance(csky_ctx* c, uint16_t* out, int* w, int* h) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_read_transmittance: ctx is NULL");
    if (!c->have_trans) return fail(c, CSKY_ERR_STATE, "csky_read_transmittance: LUT not rendered yet");
    int rc; if ((rc = bind(c))) return rc;
    if (w) *w = c->tw; if (h) *h = c->th;
    if (out) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipMemcpy(out, c->d_trans_h, (size_t)c->tw * c->th * 8, hipMemcpyDeviceToHost)); }
    return CSKY_OK;
}
int csky_read_sky_lut(csky_ctx* c, uint16_t* out, int* w, int* h) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_read_sky_lut: ctx is NULL");
    const SkyLut& l = c->lut;
    if (l.st.holds == SkyLutHolds::None) return fail(c, CSKY_ERR_STATE, "csky_read_sky_lut: LUT not rendered yet");
    if (!l.st.in_memory()) return fail(c, CSKY_ERR_STATE, "csky_read_sky_lut: the last LUT went to the caller as rows (csky_render_sky_lut_rows_device), this context holds none");
    int rc; if ((rc = bind(c))) return rc;
    if (w) *w = l.aw; if (h) *h = l.ah;
    if (out) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (hipEvent_t ev : l.writers) HIPCHK(c, hipEventSynchronize(ev));            // rows written by the other devices of a csky_multi handle
        HIPCHK(c, hipMemcpy(out, l.cur_h(), (size_t)l.aw * l.ah * 8, hipMemcpyDeviceToHost));
    }
    return CSKY_OK;
}

int csky_copy_sky_lut_device(csky_ctx* c, void* d_out, void* hip_stream) {
    if (!c) return fail(nullptr, CSKY_ERR_INVALID, "csky_copy_sky_lut_device: ctx is NULL");
    if (!d_out) return fail(c, CSKY_ERR_INVALID, "csky_copy_sky_lut_device: d_out is NULL");
    const SkyLut& l = c->lut;
    if (l.st.holds == SkyLutHolds::None) return fail(c, CSKY_ERR_STATE, "csky_copy_sky_lut_device: LUT not rendered yet");
    if (!l.st.in_memory()) return fail(c, CSKY_ERR_STATE, "csky_copy_sky_lut_device: the last LUT went to the caller as rows (csky_render_sky_lut_rows_device), this context holds none");
    int rc; if ((rc = bind(c))) return rc;
    hipStream_t s = stream_of(c, hip_stream);
    // the copy runs on the context's stream right behind the LUT's render (a later render goes to the other ring slot and, like every
    // writer of a slot, is queued behind this reader on the same stream); the caller's stream then waits for it
    for (hipEvent_t ev : l.writers) HIPCHK(c, hipStreamWaitEvent(c->stream, ev, 0));   // rows written by the other devices of a csky_multi handle
    HIPCHK(c, hipMemcpyAsync(d_out, l.cur_h(), (size_t)l.aw * l.ah * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_copy, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s, c->ev_copy, 0));
    return CSKY_OK;
}

}  // extern "C"
