// TEST TOOL ONLY: what a context holds as its sky LUT and the transitions that change it (csrc/sky_lut_reuse.h, SkyLutHeld) on the CPU, built with
// g++: the header uses nothing of HIP.  Reads one command per line from standard input; numbers are unsigned integers, a sun travels as its three
// fp32 bit patterns:
//   reset                                    a fresh state (and no_writers = 1)
//   touch | table | drop                     the transitions without arguments ("table": the transmittance table was replaced)
//   whole  s0 s1 s2 w h tlut gen             became whole, with the key of that whole-form request
//   rows   s0 s1 s2 w h                      became rows
//   shared s0 s1 s2 w h                      became shared
//   reuse  v                                 the reuse switch
//   cached s0 s1 s2 w h tlut gen first stride    NOT a transition: stores a rows key, as the rows form does behind a fill of its cache
//   nw v                                     NOT a transition: what the context's list of writers says from here on (no_writers)
//   hit s0 s1 s2 w h tlut gen                prints "hit 1" or "hit 0": sky_lut_whole_hit of that request against the state, through sky_lut_state
// After reset, every transition and cached it prints the state on one line:
//   holds (0 None, 1 Whole, 2 Rows, 3 Shared)  sky_key.valid  rows_key.valid  trans_gen  epoch moved (by this command; 0 after reset)
//   sun bits x 3  w  h  then sky_lut_state's  reuse  have_sky  sky_in_memory  sky_partial  no_writers
// tests/test_sky_lut_transitions_host.py writes the commands and holds the model.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/sky_lut_reuse.h"

namespace {
bool numbers(unsigned long long* v, int n) {
    for (int i = 0; i < n; i++) if (scanf("%llu", &v[i]) != 1) return false;
    return true;
}
void sun_of(const unsigned long long* v, float sun[3]) {
    for (int i = 0; i < 3; i++) { const uint32_t b = (uint32_t)v[i]; memcpy(&sun[i], &b, 4); }
}
}  // namespace

int main() {
    csky::SkyLutHeld st;
    bool no_writers = true;
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        unsigned long long epoch0 = st.epoch;
        unsigned long long v[9]; float sun[3];
        if (!strcmp(cmd, "reset")) { st = csky::SkyLutHeld(); no_writers = true; epoch0 = st.epoch; }
        else if (!strcmp(cmd, "touch")) st.touch();
        else if (!strcmp(cmd, "table")) st.table_replaced();
        else if (!strcmp(cmd, "drop")) st.drop();
        else if (!strcmp(cmd, "whole")) { if (!numbers(v, 7)) return 2; sun_of(v, sun); st.became_whole(csky::sky_lut_key(sun, (int)v[3], (int)v[4], (int)v[5], v[6])); }
        else if (!strcmp(cmd, "rows")) { if (!numbers(v, 5)) return 2; sun_of(v, sun); st.became_rows(sun, (int)v[3], (int)v[4]); }
        else if (!strcmp(cmd, "shared")) { if (!numbers(v, 5)) return 2; sun_of(v, sun); st.became_shared(sun, (int)v[3], (int)v[4]); }
        else if (!strcmp(cmd, "reuse")) { if (!numbers(v, 1)) return 2; st.set_reuse(v[0] != 0); }
        else if (!strcmp(cmd, "cached")) { if (!numbers(v, 9)) return 2; sun_of(v, sun); st.rows_key = csky::sky_lut_key(sun, (int)v[3], (int)v[4], (int)v[5], v[6], (int)v[7], (int)v[8]); }
        else if (!strcmp(cmd, "nw")) { if (!numbers(v, 1)) return 2; no_writers = v[0] != 0; continue; }
        else if (!strcmp(cmd, "hit")) {
            if (!numbers(v, 7)) return 2;
            sun_of(v, sun);
            printf("hit %d\n", csky::sky_lut_whole_hit(st.sky_key, csky::sky_lut_key(sun, (int)v[3], (int)v[4], (int)v[5], v[6]), csky::sky_lut_state(st, no_writers)) ? 1 : 0);
            continue;
        }
        else return 2;
        uint32_t b[3]; memcpy(b, st.sun, sizeof b);
        const csky::SkyLutState f = csky::sky_lut_state(st, no_writers);
        printf("%d %d %d %llu %d %u %u %u %d %d %d %d %d %d %d\n", (int)st.holds, st.sky_key.valid ? 1 : 0, st.rows_key.valid ? 1 : 0, st.trans_gen, st.epoch != epoch0 ? 1 : 0,
               b[0], b[1], b[2], st.w, st.h, f.reuse ? 1 : 0, f.have_sky ? 1 : 0, f.sky_in_memory ? 1 : 0, f.sky_partial ? 1 : 0, f.no_writers ? 1 : 0);
    }
    return 0;
}
