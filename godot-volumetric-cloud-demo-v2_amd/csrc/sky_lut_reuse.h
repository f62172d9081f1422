// sky_lut_reuse.h -- when a sky-LUT call may hand back what the context already holds instead of launching sky_lut_kernel again.
// The LUT is a pure function of the sun direction, its size, the transmittance table and that table's mapping (lut_core.h), none of them a
// per-frame input: a host that refreshes the LUT every pass (cloud_sky.gd:187) with a sun that only moves when the user moves it (sun.gd:17)
// asks for the same bytes again and again.  The decision is a pure function of (stored key, request, context flags), kept free of HIP so that
// tests/lut_reuse_host checks its whole table with g++; api.cpp and api_multi.cpp call nothing else to decide.
#pragma once
#include <cstring>

namespace csky {

// What the texels of a rendered LUT (whole: first_row 0, row_stride 1; a rank's rows: first_row :: row_stride) depend on.
struct SkyLutKey {
    bool valid = false;                    // false: nothing is stored (never rendered, or a call since then may have changed what the slot holds)
    float sun[3] = {0.0f, 0.0f, 0.0f};     // compared BITWISE: -0.0 is not 0.0 (atan2 tells them apart), a NaN equals itself
    int w = 0, h = 0;
    int tlut = 0;                          // the transmittance LUT's mapping (CSKY_TLUT_*)
    unsigned long long trans_gen = 0;      // the context's count of transmittance-table renders and mapping changes
    int first_row = 0, row_stride = 1;
};

inline SkyLutKey sky_lut_key(const float sun[3], int w, int h, int tlut, unsigned long long trans_gen, int first_row = 0, int row_stride = 1) {
    SkyLutKey k; k.valid = true; memcpy(k.sun, sun, sizeof k.sun);
    k.w = w; k.h = h; k.tlut = tlut; k.trans_gen = trans_gen; k.first_row = first_row; k.row_stride = row_stride;
    return k;
}

inline bool sky_lut_same_key(const SkyLutKey& stored, const SkyLutKey& req) {
    return stored.valid && req.valid && memcmp(stored.sun, req.sun, sizeof stored.sun) == 0 && stored.w == req.w && stored.h == req.h &&
           stored.tlut == req.tlut && stored.trans_gen == req.trans_gen && stored.first_row == req.first_row && stored.row_stride == req.row_stride;
}

// The context's side of the decision (context.h): the switch of csky_set_sky_lut_reuse, and whether ring slot sky_cur still is a whole LUT this
// context rendered alone.
struct SkyLutState {
    bool reuse = true;
    bool have_sky = false, sky_in_memory = false, sky_partial = false;
    bool no_writers = true;                // lut_writers is empty: no other device of a csky_multi handle stored rows into the slot
};

// csky_render_sky_lut_device: a hit launches nothing and leaves the ring where it is.
inline bool sky_lut_whole_hit(const SkyLutKey& stored, const SkyLutKey& req, const SkyLutState& s) {
    return s.reuse && s.have_sky && s.sky_in_memory && !s.sky_partial && s.no_writers && sky_lut_same_key(stored, req);
}

// csky_render_sky_lut_rows_device: the rows live in a cache of the context's own, whatever the ring holds; a hit copies them to the caller.
inline bool sky_lut_rows_hit(const SkyLutKey& stored, const SkyLutKey& req, bool reuse) { return reuse && sky_lut_same_key(stored, req); }

}  // namespace csky
