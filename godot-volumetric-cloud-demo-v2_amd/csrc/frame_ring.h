// frame_ring.h -- what one slot of the per-frame ring (context.h, FrameRing) remembers about its two cached workgroup orders, and the steps that
// change it.  A slot's static order table is a function of (tiles_x, slabs, mode, grid); the order a cost-feedback launch derives from the costs
// of the launch before it belongs to one view of one tile.  Both caches are decided by named keys with named fields, so that a field taken for
// another one (the order key once held tile_w where it needed tiles_x) is a compile-time name and a CPU test, not a GPU run.
// Free of HIP, like sky_lut_reuse.h: tests/frame_ring_host builds this header alone with g++ and walks it against a model; context.h and
// clouds_launch.cpp change the state through it alone.
#pragma once

namespace csky {

// Everything a static order table (order_kernels.hip::static_order_kernel) is a function of.  tiles_x counts workgroup FOOTPRINTS per row, not pixels:
// in mode 1 a 33-pixel-wide launch of one slab has a grid of 8 both as whole rays (2 footprints) and as two segments (3 footprints), and a key that
// could not tell them apart handed the second form the first one's table, one footprint short.
struct OrderKey {
    bool valid = false;                    // false: no table is recorded (never written, or re-allocated since)
    int tiles_x = 0, slabs = 0, mode = 0, grid = 0;
};

inline OrderKey order_key(int tiles_x, int slabs, int mode, int grid) {
    OrderKey k; k.valid = true; k.tiles_x = tiles_x; k.slabs = slabs; k.mode = mode; k.grid = grid;
    return k;
}

inline bool same_order_key(const OrderKey& stored, const OrderKey& req) {
    return stored.valid && req.valid && stored.tiles_x == req.tiles_x && stored.slabs == req.slabs && stored.mode == req.mode && stored.grid == req.grid;
}

// What a slot knows about its order table.  None of the steps touches the table: the caller has done what the name says.
struct OrderTableState {
    OrderKey key;
    // the table can be used as it is: it exists and was written for this request
    bool hit(bool allocated, const OrderKey& req) const { return allocated && same_order_key(key, req); }
    void written(const OrderKey& k) { key = k; }           // the kernel that writes the table for k was enqueued
    void forget() { key = OrderKey(); }                    // the table was re-allocated
    int grid() const { return key.grid; }                  // of the table last written
};

// What the costs a feedback launch records, and the order derived from them, belong to: one view of one tile -- the launch geometry AND the place in the
// texture (a tile walk never reuses them) -- marched in one form.
struct FeedbackKey {
    bool valid = false;
    int tile_w = 0, band_rows = 0, first_band = 0, band_stride = 0, n_bands = 0;
    long long texture_w = 0, texture_h = 0, update_x = 0, update_y = 0;   // the float parameters, truncated toward zero
    int modes = 0;                         // mode * 16 + static_mode
    int seg = 0;
};

inline FeedbackKey feedback_key(int tile_w, int band_rows, int first_band, int band_stride, int n_bands, const float texture_size[2], const float update_position[2],
                                int mode, int static_mode, int seg) {
    FeedbackKey k; k.valid = true;
    k.tile_w = tile_w; k.band_rows = band_rows; k.first_band = first_band; k.band_stride = band_stride; k.n_bands = n_bands;
    k.texture_w = (long long)texture_size[0]; k.texture_h = (long long)texture_size[1];
    k.update_x = (long long)update_position[0]; k.update_y = (long long)update_position[1];
    k.modes = mode * 16 + static_mode; k.seg = seg;
    return k;
}

inline bool same_feedback_key(const FeedbackKey& a, const FeedbackKey& b) {
    return a.valid && b.valid && a.tile_w == b.tile_w && a.band_rows == b.band_rows && a.first_band == b.first_band && a.band_stride == b.band_stride &&
           a.n_bands == b.n_bands && a.texture_w == b.texture_w && a.texture_h == b.texture_h && a.update_x == b.update_x && a.update_y == b.update_y &&
           a.modes == b.modes && a.seg == b.seg;
}

// A slot's cost feedback: whether the order buffer of the slot holds the order derived from the last feedback launch with `key`.  A launch that is
// not a feedback launch takes none of the steps and leaves the state as it is.
struct FeedbackState {
    bool valid = false;
    FeedbackKey key;
    // a feedback launch begins with this key: may it run in the order the previous one left?  Another key's order is dropped and the key stored
    bool begin(const FeedbackKey& k) {
        if (!same_feedback_key(key, k)) { valid = false; key = k; }
        return valid;
    }
    void sort_enqueued() { valid = true; }                 // only now: a launch that fails before its sort leaves no order
    void forget() { *this = FeedbackState(); }             // the buffers were re-allocated
};

}  // namespace csky
