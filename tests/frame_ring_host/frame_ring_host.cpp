// TEST TOOL ONLY: the keys and the per-slot state of csrc/frame_ring.h (OrderKey, OrderTableState, FeedbackKey, FeedbackState) on the CPU, built with
// g++: the header uses nothing of HIP.  Reads one command per line from standard input; numbers are integers, a float travels as its fp32 bit pattern.
//   an order key     O = tiles_x slabs mode grid
//   a feedback key   F = tile_w band_rows first_band band_stride n_bands  texture_size[0] [1]  update_position[0] [1] (bit patterns)  mode static_mode seg
//   omatch O O | fmatch F F                  print "match 0|1": same_order_key / same_feedback_key of the two keys, each built by order_key / feedback_key
//   odefault O | fdefault F                  print "match a b c": a default key against itself, against the given key, and the given key against a default one
//   reset                                    a fresh slot: no table allocated, default states
//   oreq O                                   the order table of the slot for this key: answers hit 0|1; on a miss the table is (allocated and) written and the key recorded
//   oforget                                  the slot forgets its order key (the table stays allocated)
//   fbegin F                                 a feedback launch begins with this key: answers whether the previous order may be used
//   fsort                                    the sort was enqueued
//   fforget                                  the feedback state is forgotten
// After reset and after every step it prints one line:
//   answer (0 where the step has none)  allocated  order key: valid tiles_x slabs mode grid  OrderTableState::grid()
//   feedback: valid  key valid  tile_w band_rows first_band band_stride n_bands texture_w texture_h update_x update_y modes seg
// tests/test_frame_ring_host.py writes the commands and holds the model.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/frame_ring.h"

namespace {
bool numbers(long long* v, int n) {
    for (int i = 0; i < n; i++) if (scanf("%lld", &v[i]) != 1) return false;
    return true;
}
float as_float(long long bits) { const uint32_t b = (uint32_t)bits; float f; memcpy(&f, &b, 4); return f; }
csky::OrderKey okey(const long long* v) { return csky::order_key((int)v[0], (int)v[1], (int)v[2], (int)v[3]); }
csky::FeedbackKey fkey(const long long* v) {
    const float ts[2] = {as_float(v[5]), as_float(v[6])}, up[2] = {as_float(v[7]), as_float(v[8])};
    return csky::feedback_key((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], ts, up, (int)v[9], (int)v[10], (int)v[11]);
}
}  // namespace

int main() {
    csky::OrderTableState ord; csky::FeedbackState fb; bool allocated = false;
    char cmd[16];
    long long v[24];
    while (scanf("%15s", cmd) == 1) {
        int answer = 0;
        if (!strcmp(cmd, "omatch")) { if (!numbers(v, 8)) return 2; printf("match %d\n", csky::same_order_key(okey(v), okey(v + 4)) ? 1 : 0); continue; }
        else if (!strcmp(cmd, "fmatch")) { if (!numbers(v, 24)) return 2; printf("match %d\n", csky::same_feedback_key(fkey(v), fkey(v + 12)) ? 1 : 0); continue; }
        else if (!strcmp(cmd, "odefault")) {
            if (!numbers(v, 4)) return 2;
            const csky::OrderKey d;
            printf("match %d %d %d\n", csky::same_order_key(d, d) ? 1 : 0, csky::same_order_key(d, okey(v)) ? 1 : 0, csky::same_order_key(okey(v), d) ? 1 : 0);
            continue;
        }
        else if (!strcmp(cmd, "fdefault")) {
            if (!numbers(v, 12)) return 2;
            const csky::FeedbackKey d;
            printf("match %d %d %d\n", csky::same_feedback_key(d, d) ? 1 : 0, csky::same_feedback_key(d, fkey(v)) ? 1 : 0, csky::same_feedback_key(fkey(v), d) ? 1 : 0);
            continue;
        }
        else if (!strcmp(cmd, "reset")) { ord = csky::OrderTableState(); fb = csky::FeedbackState(); allocated = false; }
        else if (!strcmp(cmd, "oreq")) {
            if (!numbers(v, 4)) return 2;
            const csky::OrderKey k = okey(v);
            answer = ord.hit(allocated, k) ? 1 : 0;
            if (!answer) { allocated = true; ord.written(k); }
        }
        else if (!strcmp(cmd, "oforget")) ord.forget();
        else if (!strcmp(cmd, "fbegin")) { if (!numbers(v, 12)) return 2; answer = fb.begin(fkey(v)) ? 1 : 0; }
        else if (!strcmp(cmd, "fsort")) fb.sort_enqueued();
        else if (!strcmp(cmd, "fforget")) fb.forget();
        else return 2;
        const csky::OrderKey& o = ord.key; const csky::FeedbackKey& f = fb.key;
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %lld %d %d\n", answer, allocated ? 1 : 0, o.valid ? 1 : 0, o.tiles_x, o.slabs, o.mode, o.grid, ord.grid(),
               fb.valid ? 1 : 0, f.valid ? 1 : 0, f.tile_w, f.band_rows, f.first_band, f.band_stride, f.n_bands, f.texture_w, f.texture_h, f.update_x, f.update_y, f.modes, f.seg);
    }
    return 0;
}
