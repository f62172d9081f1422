"""numpy-fp32 restatement of the weather-map generator (csrc/noise_core.h weather_texel; the definition: include/cloudsky.h), on the
noise primitives of oracle/noise_restatement.py: array arithmetic written from the formula, every operation IEEE single precision in the formula's
order, so the host generator and the HIP kernel must agree with it to the byte.  Test infrastructure: the product never imports it."""
import numpy as np

from oracle.noise_restatement import F, _clamp01, _unorm8, perlin_fbm, worley_fbm

N = 512

# csky_weather_default_params, restated (tests/test_weather_generator.py compares with the library's)
DEFAULTS = dict(coverage_freq=2, coverage_octaves=5, type_freq=6, type_octaves=3, phase=0.0, coverage_gain=0.9, dilate=0.55, coverage_centre=0.38,
                coverage_contrast=2.0, coverage_offset=0.06, coverage_floor=0.07, type_mean=0.748, type_spread=0.32)


def weather_block(seed, x, y, **knobs):
    """uint8 [..., 3]: the texels at integer coordinates x, y (arrays of one shape; any integers: 512 lies one period beyond 0)."""
    unknown = set(knobs) - set(DEFAULTS)
    assert not unknown, unknown
    P = dict(DEFAULTS, **knobs)
    with np.errstate(over="ignore"):
        u = (np.asarray(x).astype(F) + F(0.5)) / F(N)
        v = (np.asarray(y).astype(F) + F(0.5)) / F(N)
        phase = F(P["phase"])
        w = np.full(u.shape, F(phase - np.floor(phase)), F)
        s = (seed * 307) & 0xFFFFFFFF
        wf = worley_fbm(u, v, w, P["coverage_freq"], (s + 19) & 0xFFFFFFFF)
        pf = perlin_fbm(u, v, w, P["coverage_freq"], P["coverage_octaves"], (s + 5) & 0xFFFFFFFF)
        p01 = _clamp01(pf * F(P["coverage_gain"]) + F(0.5))
        nmin = wf * F(P["dilate"])
        pw = nmin + ((p01 - F(0.0)) / (F(1.0) - F(0.0))) * (F(1.0) - nmin)
        b = _clamp01((pw - F(P["coverage_centre"])) * F(P["coverage_contrast"]) + F(P["coverage_offset"]))
        floor = F(P["coverage_floor"])
        b = floor + (F(1.0) - floor) * b
        tf = perlin_fbm(u, v, w, P["type_freq"], P["type_octaves"], (s + 41) & 0xFFFFFFFF)
        r = _clamp01(F(P["type_mean"]) + tf * F(P["type_spread"]))
        return np.stack([_unorm8(r), np.zeros(u.shape, np.uint8), _unorm8(b)], -1)


def weather_map(seed=1, **knobs):
    """the whole [512, 512, 3] map, row 0 first"""
    yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return weather_block(seed, xx, yy, **knobs)
