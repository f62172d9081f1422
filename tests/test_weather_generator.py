"""The weather-map generator on the host (csky_generate_weather, csrc/noise_core.h weather_texel), no GPU:
  W1  the whole 512 x 512 map equals the numpy restatement (tests/weather_reference.py) byte for byte: seeds 1 and 7, the defaults and a tweaked block;
  W2  it tiles in x and y, has period 1 in phase, and evolves smoothly in phase;
  W3  the default map at seed 1 meets the calibration conditions, measured against the shipped weather.bmp itself;
  W4  csky_check_weather_params is the one rule of what the generators refuse, and a refused call writes nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import weather_reference as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWEAKED = dict(coverage_freq=3, coverage_octaves=4, type_freq=5, type_octaves=2, coverage_floor=0.2, phase=0.375)
BLOCKS = {"defaults": {}, "tweaked": TWEAKED}


@pytest.fixture(scope="module")
def reference_maps():
    """computed once, shared, never written to"""
    maps = {(seed, name): WR.weather_map(seed, **knobs) for seed in (1, 7) for name, knobs in BLOCKS.items()}
    for m in maps.values():
        m.setflags(write=False)
    return maps


def test_the_restated_defaults_are_the_librarys(pkg):
    d = pkg.assets.weather_default_params()
    assert set(d) == set(WR.DEFAULTS)
    for k, v in WR.DEFAULTS.items():
        assert d[k] == (v if isinstance(v, int) else float(np.float32(v))), k


@pytest.mark.parametrize("seed", [1, 7])
@pytest.mark.parametrize("block", sorted(BLOCKS))
def test_w1_the_host_generator_equals_the_restatement(pkg, reference_maps, seed, block):
    got = pkg.assets.generate_weather(seed, **BLOCKS[block])
    want = reference_maps[(seed, block)]
    assert got.shape == (512, 512, 3) and got.dtype == np.uint8
    assert (got[..., 1] == 0).all()
    differ = int((got != want).sum())
    assert differ == 0, "%d bytes differ" % differ
    assert got[..., 0].std() > 5 and got[..., 2].std() > 5        # a map, not a constant


def test_w2_the_map_tiles_in_x_and_y(reference_maps):
    k = np.arange(512)
    for seed, block in reference_maps:
        m, knobs = reference_maps[(seed, block)], BLOCKS[block]
        assert (WR.weather_block(seed, np.full(512, 512), k, **knobs) == m[:, 0]).all(), (seed, block)       # x = 512 is x = 0
        assert (WR.weather_block(seed, k, np.full(512, 512), **knobs) == m[0, :]).all(), (seed, block)       # y = 512 is y = 0
    m = reference_maps[(1, "defaults")].astype(np.int32)
    # ... and is continuous across the seam: the step from texel 511 to texel 0 is no larger than the largest step inside the map
    for axis in (0, 1):
        inside = np.abs(np.diff(m, axis=axis)).max()
        seam = np.abs(np.take(m, 0, axis=axis) - np.take(m, 511, axis=axis)).max()
        assert seam <= inside, (axis, seam, inside)


@pytest.mark.parametrize("phase", [0.0, 0.375, -0.25, 2.5])
def test_w2_phase_has_period_one(pkg, phase):
    a, b = pkg.assets.generate_weather(7, phase=phase), pkg.assets.generate_weather(7, phase=phase + 1.0)
    assert (a == b).all()
    assert (a != pkg.assets.generate_weather(7, phase=phase + 0.5)).any()


def test_w2_the_map_evolves_smoothly_in_phase(pkg):
    b = lambda p: pkg.assets.generate_weather(1, phase=p)[..., 2].astype(np.float64)
    at = b(0.5)
    near, far = np.abs(b(0.5 + 1.0 / 256) - at).mean(), np.abs(b(0.75) - at).mean()
    print("mean |dB|: %.4f over 1/256 of a period, %.4f over 1/4" % (near, far))
    assert 0 < near < far


def test_w3_the_default_map_is_calibrated_on_the_shipped_one(pkg, noise, tmp_path):
    asset = noise[2]
    g = pkg.assets.generate_weather(1)
    r, b = g[..., 0], g[..., 2]
    print("generated: R [%d, %d] mean %.4f std %.4f; B [%d, %d] mean %.4f std %.4f" %
          (r.min(), r.max(), r.mean() / 255, r.std() / 255, b.min(), b.max(), b.mean() / 255, b.std() / 255))
    assert r.min() >= 128                                         # the shipped map's cloud-type mode, so the same specialised march
    assert b.min() >= 1 and b.max() == 255
    for c in (0, 2):
        assert abs(g[..., c].mean() - asset[..., c].mean()) / 255 <= 0.05, c
    # weather_range (csrc/noise_set.h, what a bind reads back) of the map is its own min and max
    tool = os.path.join(ROOT, "tests", "noise_set_host")
    subprocess.check_call(["make", "-C", tool, "-s"])
    path = tmp_path / "weather.rgb8"
    path.write_bytes(g.tobytes())
    out = subprocess.run([os.path.join(tool, "noise_set_host")], input="weather_range %s\n" % path, stdout=subprocess.PIPE, universal_newlines=True, check=True)
    assert tuple(int(x) for x in out.stdout.split()) == (int(r.min()), int(r.max()), int(b.max()))


NAN, INF = float("nan"), float("inf")
REFUSED = [dict(coverage_freq=0), dict(coverage_freq=-3), dict(type_freq=0), dict(type_freq=-1), dict(coverage_freq=1 << 30), dict(type_freq=65),
           dict(coverage_octaves=0), dict(coverage_octaves=31), dict(coverage_octaves=33), dict(type_octaves=-1), dict(type_octaves=40),
           dict(phase=NAN), dict(phase=INF), dict(phase=1025.0), dict(phase=-1e9), dict(coverage_gain=NAN), dict(coverage_gain=0.0), dict(dilate=-INF),
           dict(dilate=1.5), dict(coverage_centre=INF), dict(coverage_contrast=NAN), dict(coverage_contrast=0.0), dict(coverage_offset=-INF),
           dict(coverage_floor=-0.01), dict(coverage_floor=1.01), dict(coverage_floor=NAN), dict(type_mean=NAN), dict(type_spread=INF), dict(type_spread=1e30)]


def test_w4_the_check_accepts_the_defaults_and_the_ends_of_its_bounds(pkg):
    L = pkg.lib()
    ok = lambda **k: L.csky_check_weather_params(C.byref(pkg._lib.weather_params(**k)))
    assert ok() == 0 and L.csky_check_weather_params(None) == pkg._lib.ERR_INVALID
    for k in (dict(coverage_freq=64, coverage_octaves=8), dict(type_freq=1, type_octaves=1), dict(phase=1024.0), dict(phase=-1024.0), dict(coverage_floor=0.0),
              dict(coverage_floor=1.0), dict(dilate=0.0), dict(dilate=1.0), TWEAKED):
        assert ok(**k) == 0, k


@pytest.mark.parametrize("knobs", REFUSED, ids=lambda k: "%s=%s" % next(iter(k.items())))
def test_w4_what_the_check_refuses_the_generator_refuses_and_writes_nothing(pkg, knobs):
    L = pkg.lib()
    p = pkg._lib.weather_params(**knobs)
    assert L.csky_check_weather_params(C.byref(p)) == pkg._lib.ERR_INVALID
    assert b"weather parameters" in L.csky_assets_last_error()
    out = np.full((512, 512, 3), 0xA5, np.uint8)
    assert L.csky_generate_weather(1, C.byref(p), out.ctypes.data_as(C.c_void_p)) == pkg._lib.ERR_INVALID
    assert (out == 0xA5).all()
    with pytest.raises(pkg.CloudSkyError):
        pkg.assets.generate_weather(1, **knobs)


def test_w4_a_null_output_and_an_unknown_knob(pkg):
    assert pkg.lib().csky_generate_weather(1, None, None) == pkg._lib.ERR_INVALID
    with pytest.raises(TypeError):
        pkg.assets.generate_weather(1, coverage=3)
