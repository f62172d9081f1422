// weather_set_host.cpp -- TEST TOOL ONLY.  NoiseHeld (csrc/noise_set.h) with its weather-only step, compiled for the host with g++.  Reads one step per
// line from stdin and prints the state after it, for tests/test_weather_set_host.py to walk against a model.  Floats travel as their bit patterns.
//   reset | request_exact M | begin_rebind | bound INEXACT RMIN RMAX BMAX LOD5 | ready | reweathered RMIN RMAX BMAX | rejects COVERAGE USE_WINDOW
//       -> have cell32 inexact lod5 rmin rmax bmax answer lo hi ct_mode   (answer: what bound or reweathered returned; lo hi ct_mode: what rejects returned)
//   window COVERAGE RMIN RMAX BMAX  -> lo hi                              bake.h height_window called directly: the reference of the walk
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/noise_set.h"

using namespace csky;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float unbits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main() {
    NoiseHeld st;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd; in >> cmd;
        int answer = 0; ExactRejects rej = {0.0f, 0.0f, 0};
        if (cmd == "reset") st = NoiseHeld();
        else if (cmd == "request_exact") { int m; in >> m; st.request_exact(m); }
        else if (cmd == "begin_rebind") st.begin_rebind();
        else if (cmd == "bound") { unsigned long long n; WeatherRange w; uint32_t l; in >> n >> w.rmin >> w.rmax >> w.bmax >> l; answer = st.bound(n, w, unbits(l)); }
        else if (cmd == "ready") st.ready();
        else if (cmd == "reweathered") { WeatherRange w; in >> w.rmin >> w.rmax >> w.bmax; answer = st.reweathered(w); }
        else if (cmd == "rejects") { uint32_t c; int win; in >> c >> win; rej = st.rejects(unbits(c), win != 0); }
        else if (cmd == "window") {
            uint32_t c; int rmin, rmax, bmax; in >> c >> rmin >> rmax >> bmax;
            float lo, hi; height_window((double)unbits(c), rmin / 255.0, rmax / 255.0, bmax / 255.0, lo, hi);
            printf("%u %u\n", bits(lo), bits(hi));
            continue;
        } else { fprintf(stderr, "unknown step: %s\n", line.c_str()); return 2; }
        if (!in) { fprintf(stderr, "bad arguments: %s\n", line.c_str()); return 2; }
        const WeatherRange w = st.range();
        printf("%d %d %llu %u %d %d %d %d %u %u %d\n", (int)st.have(), (int)st.cell32(), st.inexact(), bits(st.detail_lod5()), w.rmin, w.rmax, w.bmax, answer,
               bits(rej.hf_lo), bits(rej.hf_hi), rej.ct_mode);
    }
    return 0;
}
