// api_multi.cpp -- multi-GPU: n contexts, one frame on the first device written by peer stores (csky_multi_*, cloudsky.h).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>
#include "context.h"

using namespace csky;

constexpr int MULTI_SLOTS = 8;            // frames in flight over all groups (csky_multi_set_frames_in_flight x csky_multi_set_groups)
// What the handle holds per device.  The owners (owners.h) are released with that device current, after it has been waited for (csky_multi_destroy);
// the context is destroyed after them.  An empty Dev is safe to destroy, so csky_multi_create may bail at any point.
struct Dev {
    csky_ctx* ctx = nullptr;              // csky_destroy'ed by csky_multi_destroy
    Stream side[RING];                    // [frame in flight]: the march streams of the devices behind the first (whose march runs on the consumer's stream);
                                          // never the context's own stream: the frame prologue runs there, beside the march (context.h)
    Event done[MULTI_SLOTS];              // [frame slot]: its march (and staged copy) of that frame has finished
    DevBuf<uint2> stage[RING];            // [per-device frame slot]: compact band buffer on that device (staged form), in pixels, grow-only
    Event lut;                            // its rows of the sky LUT have been stored into the first device's LUT (csky_multi_render_sky_lut)
    // preconditions + instrumentation (round 6): peer access to the first device, and timing events of the LAST frame enqueued (csky_multi_set_timing)
    Event tm[3];                          // [0] before the march, [1] after it, [2] after the staged copy
    int peer_ok = 1;                      // 1 = hipDeviceCanAccessPeer(device, first) and it was enabled (1 for the first device itself)
    int tm_valid = 0;                     // 0 none, 1 march only, 2 march + copy
};
struct csky_multi {
    std::vector<Dev> dev;
    // on the first device:
    Event ev_begin[MULTI_SLOTS];          // the consumer stream's position when the frame was requested
    Event ev_lut_begin;                   // on its prologue stream: the readers of the LUT slot about to be rewritten are behind this
    SkyLutKey lut_key;                    // what csky_multi_render_sky_lut rendered last (sky_lut_reuse.h), and every device's LUT epoch as that call left it:
    std::vector<unsigned long long> lut_epoch;   // the same request again, with no device's LUT state touched since, renders nothing
    DevBuf<uint2> d_frame;                // host-buffer form: internal frame, in pixels, grow-only
    int fif = 1, groups = 1;              // frames in flight PER GROUP, frame groups (csky_multi_set_groups)
    unsigned long long frame_no = 0;
    bool staged = false;                  // CSKY_MULTI_STAGED=1 / csky_multi_set_staged: local band buffer + peer copy instead of in-place peer stores
    bool all_peer = true;                 // false: some device has no peer access -> staged copies (the runtime bounces them) + the whole LUT on the first device
    bool timing = false;
    char err[512] = {0};
    char warn[512] = {0};
};
namespace {
int mfail(csky_multi* m, int code, const char* fmt, ...) {
    char* dst = m ? m->err : g_err;
    va_list ap; va_start(ap, fmt); vsnprintf(dst, 512, fmt, ap); va_end(ap);
    return code;
}
int mpass(csky_multi* m, int i, int rc) {      // propagate a per-device error text
    if (rc) snprintf(m->err, sizeof m->err, "device %d (index %d): %s", m->dev[i].ctx->device, i, m->dev[i].ctx->err);
    return rc;
}
}  // namespace

extern "C" {

int csky_multi_create(csky_multi** out, const int* device_ids, int n) {
    if (!out) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_create: out is NULL");
    *out = nullptr;
    if (!device_ids || n < 1 || n > 64) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_create: need 1..64 device ids");
    csky_multi* m = new (std::nothrow) csky_multi();
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_create: out of host memory");
    for (int i = 0; i < n; i++) {
        csky_ctx* c = nullptr;
        const int rc = csky_create(&c, device_ids[i]);
        if (rc) { csky_multi_destroy(m); return rc; }           // g_err already holds csky_create's text
        m->dev.emplace_back().ctx = c;
    }
    // a step that fails leaves its text in the context it was made for: it goes to the caller's thread, and the half-built handle goes
    auto bail = [&](int rc, const csky_ctx* c) { mfail(nullptr, rc, "csky_multi_create: %s", c->err); csky_multi_destroy(m); return rc; };
    const int d0 = device_ids[0];
    for (int i = 0; i < n; i++) {
        const int di = device_ids[i];
        Dev& d = m->dev[i];
        int rc; if ((rc = bind(d.ctx))) return bail(rc, d.ctx);
        for (Event& ev : d.done) if ((rc = ev.create(d.ctx, hipEventDisableTiming))) return bail(rc, d.ctx);
        for (Stream& st : d.side) if ((rc = st.create(d.ctx, hipStreamNonBlocking))) return bail(rc, d.ctx);
        if ((rc = d.lut.create(d.ctx, hipEventDisableTiming))) return bail(rc, d.ctx);
        int ok = 1;
        if (di != d0) {                                          // the march on device di stores into the frame on d0: xGMI peer access
            int can = 0;
            hipError_t e = hipDeviceCanAccessPeer(&can, di, d0);
            if (e != hipSuccess) return bail(fail(d.ctx, CSKY_ERR_HIP, "hipDeviceCanAccessPeer: %s", hipGetErrorString(e)), d.ctx);
            if (can) {
                e = hipDeviceEnablePeerAccess(d0, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
                (void)hipGetLastError();
            }
            ok = can;
        }
        // test hook: pretend device INDEX i (> 0) has no peer access -- also when it IS the first device's GPU, which is all a single-GPU box can offer
        if (const char* fk = getenv("CSKY_MULTI_FAKE_NO_PEER")) if (i > 0 && atoi(fk) == i) ok = 0;
        d.peer_ok = ok;
        if (!ok) {
            // No peer access between this device and the first one (no xGMI / PCIe P2P route, IOMMU policy, a container without the devices' links): the
            // in-place form cannot work for it.  Not fatal: the whole handle falls back to the STAGED form -- every device renders into a local band
            // buffer and hipMemcpy2DAsync moves the bands (the runtime bounces them through host memory where it must) -- and the first device renders the
            // whole sky LUT itself.  Slower; the caller is told (csky_multi_last_warning), and csky_multi_get_stats says which devices.
            const size_t at = strlen(m->warn);
            snprintf(m->warn + at, sizeof m->warn - at, "%sdevice %d (index %d) has no peer access to device %d", at ? "; " : "csky_multi_create: ", di, i, d0);
            m->all_peer = false;
        }
    }
    if (!m->all_peer) {
        const size_t at = strlen(m->warn);
        snprintf(m->warn + at, sizeof m->warn - at, ": falling back to staged band copies and a whole sky LUT on the first device (slower than in-place xGMI stores)");
        m->staged = true;
    }
    csky_ctx* const c0 = m->dev[0].ctx;
    if (const int rc = bind(c0)) return bail(rc, c0);
    for (Event& ev : m->ev_begin) if (const int rc = ev.create(c0, hipEventDisableTiming)) return bail(rc, c0);
    if (const int rc = m->ev_lut_begin.create(c0, hipEventDisableTiming)) return bail(rc, c0);
    if (const char* se = getenv("CSKY_MULTI_STAGED")) m->staged = (atoi(se) != 0) || !m->all_peer;   // A/B switch for the driver's 8-GPU node (never off without peer access)
    *out = m;
    return CSKY_OK;
}

void csky_multi_destroy(csky_multi* m) {
    if (!m) return;
    for (Dev& d : m->dev) {
        (void)hipSetDevice(d.ctx->device);
        (void)hipDeviceSynchronize();
        Dev gone(std::move(d));                                 // its events, buffers and streams die here, with the device current; d keeps the context alone
    }
    if (!m->dev.empty()) {
        csky_ctx* const c0 = m->dev[0].ctx;
        (void)hipSetDevice(c0->device);
        for (Event& ev : m->ev_begin) ev.reset();
        m->ev_lut_begin.reset(); m->d_frame.reset();
        c0->lut.writers.clear();
    }
    for (Dev& d : m->dev) csky_destroy(d.ctx);
    delete m;
}

int csky_multi_device_count(const csky_multi* m) { return m ? (int)m->dev.size() : 0; }
csky_ctx* csky_multi_ctx(csky_multi* m, int i) { return (m && i >= 0 && i < (int)m->dev.size()) ? m->dev[i].ctx : nullptr; }
const char* csky_multi_last_error(const csky_multi* m) { return m ? m->err : g_err; }
const char* csky_multi_last_warning(const csky_multi* m) { return m ? m->warn : ""; }
int csky_multi_set_timing(csky_multi* m, int enabled) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_timing: handle is NULL");
    const int rc = csky_multi_sync(m); if (rc) return rc;
    if (enabled)
        for (size_t i = 0; i < m->dev.size(); i++) {
            Dev& d = m->dev[i];
            if ((hipSetDevice(d.ctx->device)) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_set_timing: hipSetDevice failed");
            for (Event& ev : d.tm) if (!ev) { const int rc = ev.create(d.ctx, hipEventDefault); if (rc) return mpass(m, (int)i, rc); }
        }
    m->timing = enabled != 0;
    for (Dev& d : m->dev) d.tm_valid = 0;
    return CSKY_OK;
}
int csky_multi_get_stats(csky_multi* m, csky_multi_stats* out) {
    if (!m || !out) return mfail(m, CSKY_ERR_INVALID, "csky_multi_get_stats: NULL argument");
    memset(out, 0, sizeof *out);
    const int rc = csky_multi_sync(m); if (rc) return rc;       // the events of the last frame must have completed
    const int n = (int)m->dev.size();
    out->n_devices = n; out->staged = m->staged ? 1 : 0; out->all_peer = m->all_peer ? 1 : 0; out->groups = m->groups; out->frames_in_flight = m->fif;
    out->timing = m->timing ? 1 : 0;
    for (int i = 0; i < n && i < CSKY_MULTI_STATS_MAX; i++) {
        const Dev& d = m->dev[i];
        out->device_id[i] = d.ctx->device; out->peer_access[i] = d.peer_ok;
        out->march_ms[i] = out->copy_ms[i] = -1.0f;
        if (d.tm_valid >= 1) {
            if (hipSetDevice(d.ctx->device) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_get_stats: hipSetDevice failed");
            float ms = 0.0f;
            // (the first device's share runs on the CALLER's consumer stream, which csky_multi_sync does not own: wait for the timing events themselves)
            if (hipEventSynchronize(d.tm[d.tm_valid >= 2 ? 2 : 1]) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_get_stats: hipEventSynchronize failed");
            if (hipEventElapsedTime(&ms, d.tm[0], d.tm[1]) == hipSuccess) out->march_ms[i] = ms; else (void)hipGetLastError();
            if (d.tm_valid >= 2) { if (hipEventElapsedTime(&ms, d.tm[1], d.tm[2]) == hipSuccess) out->copy_ms[i] = ms; else (void)hipGetLastError(); }
            else out->copy_ms[i] = 0.0f;                         // in-place form: the stores ARE the march
        }
    }
    return CSKY_OK;
}

int csky_multi_set_noise(csky_multi* m, const uint8_t* large, const uint8_t* small, const uint8_t* weather) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_noise: handle is NULL");
    for (size_t i = 0; i < m->dev.size(); i++) { const int rc = csky_set_noise(m->dev[i].ctx, large, small, weather); if (rc) return mpass(m, (int)i, rc); }
    return CSKY_OK;
}
int csky_multi_set_noise_mips(csky_multi* m, const uint8_t* large_chain, const uint8_t* small_chain, const uint8_t* weather) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_noise_mips: handle is NULL");
    for (size_t i = 0; i < m->dev.size(); i++) { const int rc = csky_set_noise_mips(m->dev[i].ctx, large_chain, small_chain, weather); if (rc) return mpass(m, (int)i, rc); }
    return CSKY_OK;
}
int csky_multi_set_march(csky_multi* m, int primary_steps, int light_steps) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_march: handle is NULL");
    for (size_t i = 0; i < m->dev.size(); i++) { const int rc = csky_set_march(m->dev[i].ctx, primary_steps, light_steps); if (rc) return mpass(m, (int)i, rc); }
    return CSKY_OK;
}
int csky_multi_set_transmittance_mapping(csky_multi* m, int mapping) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_transmittance_mapping: handle is NULL");
    if (mapping != CSKY_TLUT_REFERENCE && mapping != CSKY_TLUT_BRUNETON) return mfail(m, CSKY_ERR_INVALID, "csky_multi_set_transmittance_mapping: CSKY_TLUT_REFERENCE (0) or CSKY_TLUT_BRUNETON (1)");
    for (size_t i = 0; i < m->dev.size(); i++) { const int rc = csky_set_transmittance_mapping(m->dev[i].ctx, mapping); if (rc) return mpass(m, (int)i, rc); }
    return CSKY_OK;
}
int csky_multi_set_frames_in_flight(csky_multi* m, int frames) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_frames_in_flight: handle is NULL");
    if (frames < 1 || frames > RING) return mfail(m, CSKY_ERR_INVALID, "csky_multi_set_frames_in_flight: 1 .. 8 per frame group (the per-device rings are eight deep)");
    if (frames * m->groups > MULTI_SLOTS) return mfail(m, CSKY_ERR_INVALID, "csky_multi_set_frames_in_flight: frames x groups must be <= %d", MULTI_SLOTS);
    for (size_t i = 0; i < m->dev.size(); i++) { const int rc = csky_set_frames_in_flight(m->dev[i].ctx, frames); if (rc) return mpass(m, (int)i, rc); }
    m->fif = frames;
    return CSKY_OK;
}
int csky_multi_set_groups(csky_multi* m, int groups) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_groups: handle is NULL");
    const int n = (int)m->dev.size();
    if (groups < 1 || groups > n || n % groups) return mfail(m, CSKY_ERR_INVALID, "csky_multi_set_groups: the group count must divide the %d devices", n);
    if (groups * m->fif > MULTI_SLOTS) return mfail(m, CSKY_ERR_INVALID, "csky_multi_set_groups: frames in flight x groups must be <= %d", MULTI_SLOTS);
    const int rc = csky_multi_sync(m); if (rc) return rc;       // frames of the old partition may be in flight
    m->groups = groups; m->frame_no = 0;
    return CSKY_OK;
}
int csky_multi_set_staged(csky_multi* m, int staged) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_staged: handle is NULL");
    const int rc = csky_multi_sync(m); if (rc) return rc;
    if (!staged && !m->all_peer) return mfail(m, CSKY_ERR_STATE, "csky_multi_set_staged: the in-place form needs peer access from every device to the first (%s)", m->warn);
    m->staged = staged != 0;
    return CSKY_OK;
}
int csky_multi_render_sky_lut(csky_multi* m, const csky_sky_params* p) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_render_sky_lut: handle is NULL");
    if (!p) return mfail(m, CSKY_ERR_INVALID, "csky_multi_render_sky_lut: params is NULL");
    int w, h, rc;
    if ((rc = lut_size(nullptr, "csky_multi_render_sky_lut", p->texture_size, w, h))) return mfail(m, rc, "%s", g_err);
    // sky_lut.gd:43-52 renders the LUT once per frame (cloud_sky.gd:187); n devices rendering n whole copies would each spend 33 us of a chip on it,
    // 12 % of a 1/8 frame share.  Device i renders rows i, i + n, ... and stores them, like its bands, straight into the LUT on the first device
    // (the copy a consumer reads: csky_read_sky_lut / csky_copy_sky_lut_device on csky_multi_ctx(m, 0) wait for every writer).  No device's frame
    // set-up reads that copy: each renders the <= 12 texels it filters itself (frame_setup_taps_kernel), for the sun recorded here -- on EVERY
    // device, whatever the group layout (a caller with a static sun renders the LUT once and then frames on all groups).
    const int n = (int)m->dev.size();
    csky_ctx* c0 = m->dev[0].ctx;
    // A static sun (the case above) asks for the LUT the handle rendered last: no device renders its rows again, every device keeps the sun it
    // recorded, and the first context's writers stay the events of the call that stored the rows.  Anything that touched a device's LUT
    // state since (a context's own LUT calls, a new transmittance table or mapping) moved its epoch: then the handle renders.
    if (c0->lut.st.reuse && sky_lut_same_key(m->lut_key, sky_lut_key(p->sun_direction, w, h, c0->tlut, c0->lut.st.trans_gen)) && m->lut_epoch.size() == (size_t)n) {
        bool same = true;
        for (int i = 0; i < n; i++) same = same && m->dev[i].ctx->lut.st.epoch == m->lut_epoch[i];
        if (same) return CSKY_OK;
    }
    m->lut_key.valid = false;
    for (int i = 0; i < n; i++) m->dev[i].ctx->lut.st.touch();   // (the first context's ring slot is about to hold rows of several devices)
    if (c0->lut.aw && (c0->lut.aw != w || c0->lut.ah != h))   // a size change re-allocates the first device's LUT slots: no device may still be storing rows into them
        for (int i = 0; i < n; i++) { if ((rc = bind(m->dev[i].ctx))) return mpass(m, i, rc); if (hipStreamSynchronize(m->dev[i].ctx->stream) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_sky_lut: hipStreamSynchronize failed"); }
    if ((rc = bind(c0))) return mpass(m, 0, rc);
    if ((rc = ensure_sky(c0, w, h))) return mpass(m, 0, rc);
    const int k = c0->lut.render_slot();
    // the readers of slot k (device copies of the LUT before last) sit on the first device's prologue stream: every writer queues behind them
    if (hipEventRecord(m->ev_lut_begin, c0->stream) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_sky_lut: hipEventRecord failed");
    for (int i = 0; i < n; i++) {
        csky_ctx* c = m->dev[i].ctx;
        if ((rc = bind(c))) return mpass(m, i, rc);
        if ((rc = ensure_default_trans(c))) return mpass(m, i, rc);
        hipError_t e = i ? hipStreamWaitEvent(c->stream, m->ev_lut_begin, 0) : hipSuccess;
        // rows i, i + n, ... stored into the first device's LUT -- or, when some device cannot reach that memory, every row by the first device itself
        if (e == hipSuccess && (m->all_peer || i == 0)) {
            if ((m->all_peer ? i : 0) < h) c->lut.launches++;
            e = launch_sky_lut_rows(w, h, m->all_peer ? i : 0, m->all_peer ? n : 1, p->sun_direction, c->d_trans_f, c->tw, c->th, reinterpret_cast<uint2*>(c0->lut.ring_h[k].get()), c0->lut.ring_f[k], c->stream, c->tlut);
        }
        if (e == hipSuccess) e = hipEventRecord(m->dev[i].lut, c->stream);
        if (e != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_sky_lut: device index %d: %s", i, hipGetErrorString(e));
        if (i) { c->lut.st.became_rows(p->sun_direction, w, h); c->lut.writers.clear(); }
    }
    c0->lut.publish(k); c0->lut.st.became_shared(p->sun_direction, w, h);
    for (int i = 1; i < n; i++) c0->lut.writers.push_back(m->dev[i].lut);   // (its own rows are on its prologue stream, ahead of any reader)
    m->lut_key = sky_lut_key(p->sun_direction, w, h, c0->tlut, c0->lut.st.trans_gen);
    m->lut_epoch.resize(n);
    for (int i = 0; i < n; i++) m->lut_epoch[i] = m->dev[i].ctx->lut.st.epoch;
    return CSKY_OK;
}

int csky_multi_render_clouds_device(csky_multi* m, const csky_cloud_params* p, int tile_w, int tile_h, void* d_out, size_t pitch, void* hip_stream) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_render_clouds_device: handle is NULL");
    if (!d_out || !p) return mfail(m, CSKY_ERR_INVALID, "csky_multi_render_clouds_device: NULL argument");
    if (tile_w < 1 || tile_h < 8 || (tile_h & 7)) return mfail(m, CSKY_ERR_INVALID, "csky_multi_render_clouds_device: tile_h must be a positive multiple of 8 (bands are 8 rows)");
    if (pitch % 8 || pitch < (size_t)tile_w * 8) return mfail(m, CSKY_ERR_INVALID, "csky_multi_render_clouds_device: row pitch must be a multiple of 8 and >= tile_w*8");
    const int n_all = (int)m->dev.size(), total = tile_h / 8;
    // Frame groups (csky_multi_set_groups): consecutive frames go to the G groups in turn; the n/G devices of a group split the frame's bands.
    // Slot = frame number mod (groups x frames in flight): its events, and on every device of the group the stream / ring position
    // slot / groups of that device's frames in flight.
    const int G = m->groups, per = n_all / G, slots = G * m->fif;
    const int slot = (int)(m->frame_no % (unsigned long long)slots), grp = slot % G, dslot = slot / G;   // (frame_no advances only when the frame was enqueued: a failed call must not shift the slot / group rotation)
    csky_ctx* c0 = m->dev[0].ctx;
    int rc; if ((rc = bind(c0))) return mpass(m, 0, rc);
    hipStream_t consumer = stream_of(c0, hip_stream);
    // no device may store into the frame before the consumer's earlier work on it (reads of the previous frame) is done
    if (hipEventRecord(m->ev_begin[slot], consumer) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds_device: hipEventRecord failed");
    for (int k = 0; k < per; k++) {
        const int i = grp * per + k;
        Dev& d = m->dev[i];
        csky_ctx* c = d.ctx;
        if ((rc = bind(c))) return mpass(m, i, rc);
        const int nb = k < total ? (total - k + per - 1) / per : 0;
        if (nb == 0) continue;
        hipStream_t s = (i == 0) ? consumer : d.side[dslot];
        if (i != 0 && hipStreamWaitEvent(s, m->ev_begin[slot], 0) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds_device: hipStreamWaitEvent failed");
        const csky_bands b = {8, k, per, nb};
        const bool tmg = m->timing && d.tm[0];
        if (tmg) { d.tm_valid = 0; if (hipEventRecord(d.tm[0], s) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds_device: hipEventRecord failed"); }
        if (m->staged && i != 0) {
            // Fallback for nodes where fine-grained remote stores from inside the march stall: the device renders its bands into a compact local
            // buffer and one strided peer copy (a band = 8 rows, n bands apart in the frame) moves them over xGMI behind the march.
            const size_t need = (size_t)nb * 8 * tile_w;
            if (d.stage[dslot].count() < need) {
                if (hipStreamSynchronize(s) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds_device: hipStreamSynchronize failed");
                if ((rc = d.stage[dslot].alloc(c, need))) return mpass(m, i, rc);
            }
            uint2* st = d.stage[dslot];
            if ((rc = clouds_dev(c, p, tile_w, &b, st, (size_t)tile_w * 8, s, nullptr, true, /*out_full=*/false))) return mpass(m, i, rc);
            if (tmg && hipEventRecord(d.tm[1], s) == hipSuccess) d.tm_valid = 1;
            const size_t band_bytes = (size_t)8 * tile_w * 8;
            char* dst0 = (char*)d_out + (size_t)k * 8 * pitch;
            hipError_t e;
            if (pitch == (size_t)tile_w * 8) e = hipMemcpy2DAsync(dst0, (size_t)per * 8 * pitch, st, band_bytes, band_bytes, nb, hipMemcpyDeviceToDevice, s);
            else {
                e = hipSuccess;
                for (int bnd = 0; bnd < nb && e == hipSuccess; bnd++)
                    e = hipMemcpy2DAsync(dst0 + (size_t)bnd * per * 8 * pitch, pitch, (char*)st + (size_t)bnd * band_bytes, (size_t)tile_w * 8, (size_t)tile_w * 8, 8, hipMemcpyDeviceToDevice, s);
            }
            if (e != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds_device: peer copy failed: %s", hipGetErrorString(e));
            if (tmg && d.tm_valid == 1 && hipEventRecord(d.tm[2], s) == hipSuccess) d.tm_valid = 2;
        } else {
            if ((rc = clouds_dev(c, p, tile_w, &b, (uint2*)d_out, pitch, s, nullptr, true, /*out_full=*/true))) return mpass(m, i, rc);
            if (tmg && hipEventRecord(d.tm[1], s) == hipSuccess) d.tm_valid = 1;
        }
        if (i != 0 && hipEventRecord(d.done[slot], s) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds_device: hipEventRecord failed");
    }
    if ((rc = bind(c0))) return mpass(m, 0, rc);
    for (int k = 0; k < per; k++) {
        const int i = grp * per + k;
        if (i == 0 || k >= total) continue;
        if (hipStreamWaitEvent(consumer, m->dev[i].done[slot], 0) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds_device: hipStreamWaitEvent failed");
    }
    m->frame_no++;
    return CSKY_OK;
}

int csky_multi_render_clouds(csky_multi* m, const csky_cloud_params* p, int tile_w, int tile_h, uint16_t* out, size_t pitch) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_render_clouds: handle is NULL");
    if (tile_w < 1 || tile_h < 8 || (tile_h & 7)) return mfail(m, CSKY_ERR_INVALID, "csky_multi_render_clouds: tile_h must be a positive multiple of 8 (bands are 8 rows; the single-device csky_render_clouds takes ragged tiles)");
    if (out && pitch < (size_t)tile_w * 8) return mfail(m, CSKY_ERR_INVALID, "csky_multi_render_clouds: row_pitch_bytes < tile_w*8");
    csky_ctx* c0 = m->dev[0].ctx;
    int rc; if ((rc = bind(c0))) return mpass(m, 0, rc);
    const size_t px = (size_t)tile_w * tile_h;
    if (m->d_frame.count() < px) {
        if (hipStreamSynchronize(c0->stream) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds: hipStreamSynchronize failed");
        if ((rc = m->d_frame.alloc(c0, px))) return mpass(m, 0, rc);
    }
    if ((rc = csky_multi_render_clouds_device(m, p, tile_w, tile_h, m->d_frame, (size_t)tile_w * 8, nullptr))) return rc;
    if ((rc = bind(c0))) return mpass(m, 0, rc);
    if (out && hipMemcpy2DAsync(out, pitch, m->d_frame, (size_t)tile_w * 8, (size_t)tile_w * 8, tile_h, hipMemcpyDeviceToHost, c0->stream) != hipSuccess)
        return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds: copy to host failed");
    if (hipStreamSynchronize(c0->stream) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_render_clouds: hipStreamSynchronize failed");
    return CSKY_OK;
}

// asynchronous host form over the multi-device handle: the first context's pinned ring and streams serve as consumer streams
int csky_multi_set_host_ring(csky_multi* m, int slots) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_set_host_ring: handle is NULL");
    if (slots < 1 || slots > HOST_RING || slots > m->groups * RING || slots % m->groups) return mfail(m, CSKY_ERR_INVALID, "csky_multi_set_host_ring: 1 .. 8 frames, a multiple of the group count, at most 8 per group");
    csky_ctx* c0 = m->dev[0].ctx;
    for (auto& hs : c0->hring) if (hs.busy) return mfail(m, CSKY_ERR_STATE, "csky_multi_set_host_ring: collect the outstanding tickets first");
    const int rc = csky_multi_set_frames_in_flight(m, slots / m->groups); if (rc) return rc;
    c0->hslots = slots;
    return CSKY_OK;
}
int csky_multi_submit_clouds(csky_multi* m, const csky_cloud_params* p, int tile_w, int tile_h, int64_t* ticket) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_submit_clouds: handle is NULL");
    if (!ticket || !p) return mfail(m, CSKY_ERR_INVALID, "csky_multi_submit_clouds: NULL argument");
    if (tile_w < 1 || tile_h < 8 || (tile_h & 7) || tile_w > 16384 || tile_h > 16384) return mfail(m, CSKY_ERR_INVALID, "csky_multi_submit_clouds: tile_h must be a positive multiple of 8, sizes <= 16384");
    csky_ctx* c0 = m->dev[0].ctx;
    if (c0->hslots != m->groups * m->fif) { const int rc = csky_multi_set_host_ring(m, m->groups * m->fif); if (rc) return rc; }
    int rc; if ((rc = bind(c0))) return mpass(m, 0, rc);
    csky_ctx::HostSlot& hs = c0->hring[c0->next_ticket % c0->hslots];
    if (hs.busy) return mfail(m, CSKY_ERR_STATE, "csky_multi_submit_clouds: %d frames are already in flight; collect ticket %lld first", c0->hslots, hs.ticket);
    const size_t px = (size_t)tile_w * tile_h;
    if ((rc = host_slot_prepare(c0, hs, px))) return mpass(m, 0, rc);
    if ((rc = csky_multi_render_clouds_device(m, p, tile_w, tile_h, hs.d, (size_t)tile_w * 8, hs.s))) return rc;
    if ((rc = bind(c0))) return mpass(m, 0, rc);
    if (hipMemcpyAsync(hs.h, hs.d, px * 8, hipMemcpyDeviceToHost, hs.s) != hipSuccess || hipEventRecord(hs.done, hs.s) != hipSuccess)
        return mfail(m, CSKY_ERR_HIP, "csky_multi_submit_clouds: copy to the pinned frame failed");
    hs.busy = true; hs.ticket = c0->next_ticket; hs.w = tile_w; hs.hh = tile_h;
    *ticket = c0->next_ticket++;
    return CSKY_OK;
}
int csky_multi_collect(csky_multi* m, int64_t ticket, const uint16_t** frame, size_t* bytes) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_collect: handle is NULL");
    return mpass(m, 0, csky_collect(m->dev[0].ctx, ticket, frame, bytes));
}

int csky_multi_sync(csky_multi* m) {
    if (!m) return mfail(nullptr, CSKY_ERR_INVALID, "csky_multi_sync: handle is NULL");
    for (size_t i = 0; i < m->dev.size(); i++) {
        const int rc = csky_sync(m->dev[i].ctx); if (rc) return mpass(m, (int)i, rc);
        for (int k = 0; k < RING; k++)                         // the march streams of a device's frames in flight
            if (hipStreamSynchronize(m->dev[i].side[k]) != hipSuccess) return mfail(m, CSKY_ERR_HIP, "csky_multi_sync: hipStreamSynchronize failed on device index %d", (int)i);
    }
    return CSKY_OK;
}

}  // extern "C"
