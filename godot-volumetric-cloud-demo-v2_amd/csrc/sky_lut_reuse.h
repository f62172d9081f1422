// sky_lut_reuse.h -- when a sky-LUT call may hand back what the context already holds instead of launching sky_lut_kernel again.
// The LUT is a pure function of the sun direction, its size, the transmittance table and that table's mapping (lut_core.h), none of them a
// per-frame input: a host that refreshes the LUT every pass (cloud_sky.gd:187) with a sun that only moves when the user moves it (sun.gd:17)
// asks for the same bytes again and again.  The decision is a pure function of (stored key, request, context flags), kept free of HIP so that
// tests/lut_reuse_host checks its whole table with g++; api_lut.cpp and api_multi.cpp call nothing else to decide.
// Below the decision: what a context holds as its sky LUT (SkyLutHeld) and the transitions that change it, free of HIP for the same reason
// (tests/lut_reuse_host/lut_transitions_host.cpp walks them).  api_lut.cpp, api_multi.cpp and clouds_launch.cpp change the state through them alone.
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

// The context's side of the decision (context.h): the switch of csky_set_sky_lut_reuse, and whether the current ring slot still is a whole LUT this
// context rendered alone.
struct SkyLutState {
    bool reuse = true;
    bool have_sky = false, sky_in_memory = false, sky_partial = false;
    bool no_writers = true;                // the list of writers is empty: no other device of a csky_multi handle stored rows into the slot
};

// csky_render_sky_lut_device: a hit launches nothing and leaves the ring where it is.
inline bool sky_lut_whole_hit(const SkyLutKey& stored, const SkyLutKey& req, const SkyLutState& s) {
    return s.reuse && s.have_sky && s.sky_in_memory && !s.sky_partial && s.no_writers && sky_lut_same_key(stored, req);
}

// csky_render_sky_lut_rows_device: the rows live in a cache of the context's own, whatever the ring holds; a hit copies them to the caller.
inline bool sky_lut_rows_hit(const SkyLutKey& stored, const SkyLutKey& req, bool reuse) { return reuse && sky_lut_same_key(stored, req); }

// What a context holds as its sky LUT.
enum class SkyLutHolds {
    None,      // nothing usable: clouds, read and copy answer CSKY_ERR_STATE "not rendered yet"
    Whole,     // the current ring slot holds a whole LUT this context rendered alone: frame set-ups filter it from memory.  The one state a whole-form hit needs
    Rows,      // the LUT exists only as the rows a caller received (one rank of an N-way frame split): frame set-ups render their own taps for the
               // recorded sun and size; read and copy answer CSKY_ERR_STATE "went to the caller as rows"
    Shared,    // the current ring slot holds a whole LUT written row by row by the devices of a csky_multi handle: frame set-ups render their own taps
               // (they never read the memory copy), read and copy wait for the writers first
};

struct SkyLutHeld {
    SkyLutHolds holds = SkyLutHolds::None;
    float sun[3] = {0.0f, 1.0f, 0.0f}; int w = 0, h = 0;   // of a Rows or Shared LUT: what the set-ups' own taps are rendered for
    SkyLutKey sky_key;                     // what the current ring slot was rendered from by csky_render_sky_lut_device (a Whole LUT)
    SkyLutKey rows_key;                    // what the rows cache holds (csky_render_sky_lut_rows_device)
    unsigned long long trans_gen = 0;      // counts what replaces the transmittance table: a render of it, a mapping change
    unsigned long long epoch = 0;          // moves with every call that may change this state, so that a csky_multi handle can tell that none happened
                                           // since its own last render.  Only ever compared for equality
    bool reuse = true;                     // csky_set_sky_lut_reuse

    // The transitions.  None of them touches the ring or a buffer: the caller has done, or is about to do, what the name says.
    // the caller is about to change what the current slot holds, or the context's LUT state
    void touch() { sky_key.valid = false; epoch++; }
    // every LUT rendered through the old table is another table's.  What the context holds stays: a whole LUT rendered through the old table is still readable
    void table_replaced() { trans_gen++; rows_key.valid = false; touch(); }
    void drop() { holds = SkyLutHolds::None; touch(); }
    // (the touch comes BEFORE the launch: a launch that fails leaves no key)
    void became_whole(const SkyLutKey& key) { holds = SkyLutHolds::Whole; sky_key = key; }
    void became_rows(const float s[3], int w_, int h_) { holds = SkyLutHolds::Rows; memcpy(sun, s, sizeof sun); w = w_; h = h_; }
    void became_shared(const float s[3], int w_, int h_) { holds = SkyLutHolds::Shared; memcpy(sun, s, sizeof sun); w = w_; h = h_; }
    void set_reuse(bool on) { reuse = on; rows_key.valid = false; touch(); }

    bool own_taps() const { return holds == SkyLutHolds::Rows || holds == SkyLutHolds::Shared; }      // frame set-ups render the texels they filter themselves
    bool in_memory() const { return holds == SkyLutHolds::Whole || holds == SkyLutHolds::Shared; }    // read and copy have a whole LUT to hand out
};

// no_writers: the context's list of other devices' writer events is empty (context.h)
inline SkyLutState sky_lut_state(const SkyLutHeld& s, bool no_writers) {
    SkyLutState f; f.reuse = s.reuse; f.have_sky = s.holds != SkyLutHolds::None; f.sky_in_memory = s.in_memory(); f.sky_partial = s.own_taps(); f.no_writers = no_writers;
    return f;
}

}  // namespace csky
