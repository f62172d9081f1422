// weather_asan.cpp -- TEST TOOL ONLY.  Calls csky_check_weather_params and csky_generate_weather (the host generator of the weather map) with the
// defaults, a tweaked block and every kind of parameter the check refuses, in a program of its own built with -fsanitize=address,undefined
// (tests/test_weather_asan.py runs it on the CPU).  The output buffer is exactly 512 * 512 * 3 bytes on the heap: one byte beyond it is a report.
// Prints "weather asan ok <FNV-1a of the default map>" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../../include/cloudsky.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static uint32_t fnv(const std::vector<uint8_t>& v) { uint32_t h = 2166136261u; for (uint8_t b : v) { h ^= b; h *= 16777619u; } return h; }

int main() {
    const size_t bytes = (size_t)512 * 512 * 3;
    std::vector<uint8_t> out(bytes, 0xA5), untouched(bytes, 0xA5);
    csky_weather_params d; csky_weather_default_params(&d);
    csky_weather_default_params(nullptr);
    EXPECT(csky_check_weather_params(&d) == CSKY_OK);
    EXPECT(csky_check_weather_params(nullptr) == CSKY_ERR_INVALID);
    EXPECT(csky_generate_weather(1, nullptr, nullptr) == CSKY_ERR_INVALID);

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<csky_weather_params> bad;
    auto with = [&](auto set) { csky_weather_params p = d; set(p); bad.push_back(p); };
    with([](csky_weather_params& p) { p.coverage_freq = 0; });
    with([](csky_weather_params& p) { p.coverage_freq = -3; });
    with([](csky_weather_params& p) { p.type_freq = 0; });
    with([](csky_weather_params& p) { p.type_freq = std::numeric_limits<int32_t>::min(); });
    with([](csky_weather_params& p) { p.coverage_freq = 1 << 30; });
    with([](csky_weather_params& p) { p.type_freq = std::numeric_limits<int32_t>::max(); });
    with([](csky_weather_params& p) { p.coverage_octaves = 0; });
    with([](csky_weather_params& p) { p.coverage_octaves = 31; });
    with([](csky_weather_params& p) { p.coverage_octaves = 33; });
    with([](csky_weather_params& p) { p.type_octaves = -1; });
    with([](csky_weather_params& p) { p.type_octaves = 64; });
    with([&](csky_weather_params& p) { p.phase = nan; });
    with([&](csky_weather_params& p) { p.phase = inf; });
    with([](csky_weather_params& p) { p.phase = 1025.0f; });
    with([](csky_weather_params& p) { p.phase = -3e38f; });
    with([&](csky_weather_params& p) { p.coverage_gain = nan; });
    with([&](csky_weather_params& p) { p.dilate = -inf; });
    with([&](csky_weather_params& p) { p.coverage_centre = inf; });
    with([&](csky_weather_params& p) { p.coverage_contrast = nan; });
    with([&](csky_weather_params& p) { p.coverage_offset = -inf; });
    with([](csky_weather_params& p) { p.coverage_floor = -0.01f; });
    with([](csky_weather_params& p) { p.coverage_floor = 1.01f; });
    with([&](csky_weather_params& p) { p.type_mean = nan; });
    with([&](csky_weather_params& p) { p.type_spread = inf; });
    for (const csky_weather_params& p : bad) {
        EXPECT(csky_check_weather_params(&p) == CSKY_ERR_INVALID);
        EXPECT(csky_generate_weather(1, &p, out.data()) == CSKY_ERR_INVALID);
        EXPECT(out == untouched);
        EXPECT(strstr(csky_assets_last_error(), "weather parameters") != nullptr);
    }

    // what the check accepts runs clean: the defaults (as NULL and as a block), the ends of the bounds, a tweaked block
    EXPECT(csky_generate_weather(1, nullptr, out.data()) == CSKY_OK);
    const uint32_t h = fnv(out);
    std::vector<uint8_t> again(bytes, 0);
    EXPECT(csky_generate_weather(1, &d, again.data()) == CSKY_OK);
    EXPECT(out == again);
    csky_weather_params e = d;
    e.coverage_freq = 64; e.coverage_octaves = 8; e.type_freq = 64; e.type_octaves = 8; e.phase = -1024.0f; e.coverage_gain = 16.0f; e.dilate = 1.0f;
    e.coverage_centre = -4.0f; e.coverage_contrast = 64.0f; e.coverage_offset = 4.0f; e.coverage_floor = 1.0f; e.type_mean = -4.0f; e.type_spread = -16.0f;
    EXPECT(csky_check_weather_params(&e) == CSKY_OK);
    EXPECT(csky_generate_weather(0xFFFFFFFFu, &e, again.data()) == CSKY_OK);
    e = d; e.coverage_freq = 3; e.coverage_octaves = 4; e.type_freq = 5; e.type_octaves = 2; e.coverage_floor = 0.2f; e.phase = 0.375f;
    EXPECT(csky_generate_weather(7, &e, again.data()) == CSKY_OK);
    EXPECT(again != out);
    if (failures) return 1;
    printf("weather asan ok %08x\n", h);
    return 0;
}
