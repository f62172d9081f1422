// noise_set_host.cpp -- TEST TOOL ONLY.  What a context knows about its bound noise set (csrc/noise_set.h: NoiseHeld and the values it derives),
// compiled for the host with g++, which is what keeps the header free of HIP.  Reads one step per line from stdin and prints the state after it,
// for tests/test_noise_set_host.py to walk against a model.  Floats travel as their bit patterns.
//   reset | request_exact M | begin_rebind | bound INEXACT RMIN RMAX BMAX LOD5 | ready | rejects COVERAGE USE_WINDOW
//       -> have cell32 inexact lod5 answer lo hi ct_mode     (answer: what bound returned; lo hi ct_mode: what rejects returned; 0 otherwise)
//   window COVERAGE RMIN RMAX BMAX  -> lo hi                 bake.h height_window called directly: the reference of the walk
//   ctmodes                         -> 65536 lines, rmin-major: ct_mode of the range (rmin, rmax, 255) with the window on
//   weather_range FILE              -> rmin rmax bmax        of 512 x 512 RGB8 texels
//   lod5 R G B                      -> detail_lod5_value
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
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
        else if (cmd == "rejects") { uint32_t c; int win; in >> c >> win; rej = st.rejects(unbits(c), win != 0); }
        else if (cmd == "window") {
            uint32_t c; int rmin, rmax, bmax; in >> c >> rmin >> rmax >> bmax;
            float lo, hi; height_window((double)unbits(c), rmin / 255.0, rmax / 255.0, bmax / 255.0, lo, hi);
            printf("%u %u\n", bits(lo), bits(hi));
            continue;
        } else if (cmd == "ctmodes") {
            for (int rmin = 0; rmin < 256; rmin++) for (int rmax = 0; rmax < 256; rmax++) {
                const WeatherRange w = {rmin, rmax, 255};
                printf("%d\n", exact_rejects(w, 2.0f, true).ct_mode);   // (a coverage above 1 has no window to bisect for)
            }
            continue;
        } else if (cmd == "weather_range") {
            std::string path; in >> path;
            std::vector<uint8_t> rgb(RAW_WEATHER);
            FILE* f = fopen(path.c_str(), "rb");
            if (!f || fread(rgb.data(), 1, rgb.size(), f) != rgb.size()) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
            fclose(f);
            const WeatherRange w = weather_range(rgb.data());
            printf("%d %d %d\n", w.rmin, w.rmax, w.bmax);
            continue;
        } else if (cmd == "lod5") {
            int r, g, b; in >> r >> g >> b;
            const uint8_t t5[3] = {(uint8_t)r, (uint8_t)g, (uint8_t)b};
            printf("%u\n", bits(detail_lod5_value(t5)));
            continue;
        } else { fprintf(stderr, "unknown step: %s\n", line.c_str()); return 2; }
        if (!in) { fprintf(stderr, "bad arguments: %s\n", line.c_str()); return 2; }
        printf("%d %d %llu %u %d %u %u %d\n", (int)st.have(), (int)st.cell32(), st.inexact(), bits(st.detail_lod5()), answer, bits(rej.hf_lo), bits(rej.hf_hi), rej.ct_mode);
    }
    return 0;
}
