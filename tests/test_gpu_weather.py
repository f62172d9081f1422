"""The weather-only rebind and the weather generator on the GPU (csky_set_weather, csky_set_weather_device, csky_set_weather_generated,
csky_generate_weather_device), held to the old path byte for byte: after a weather call a context is indistinguishable from one
that has only ever bound that set with csky_set_noise.

What is compared (capture()): TILE of the 2048 x 1024 frame through the default launch and through whole rays, each with its in-cloud count; a
64 x 36 view; a 64 x 36 view from `above_down` (tests/observers.py); a 32 x 32 cloud shadow map; a 64 x 32 depth frame; the baked weather cells
(csky_read_baked_texture 2, and 8 on exact cells) and what the context holds from the bake (9).  The maps: the shipped one and `stratus` of
tests/test_gpu_noise_rebind.py (R halved, B capped at 200: another cloud-type mode, another height window at the same coverage).  The fresh
contexts' captures are made once and shared."""
import ctypes as C

import numpy as np
import pytest

import observers as OB
from conftest import norm

pytestmark = pytest.mark.gpu

SUN = (1, 1, 0)
TILE = (512, 352, 64, 32)        # x, y, width, height inside the 2048 x 1024 frame: in cloud under both weather maps (asserted in capture)
TWEAKED = dict(coverage_freq=3, coverage_octaves=4, type_freq=5, type_octaves=2, coverage_floor=0.2, phase=0.375)


def stratus_of(weather):
    s = weather.copy(); s[..., 0] //= 2; s[..., 2] = np.minimum(s[..., 2], 200)
    assert s[..., 0].max() <= 127 and s[..., 2].max() != weather[..., 2].max() and weather[..., 0].min() >= 128
    return s


def u16(a):
    return np.ascontiguousarray(a).view(np.uint16).copy()


def with_luts(ctx):
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(norm(SUN), 200, 100)


def capture(ctx, oracle, exact=False, tile_only=False, in_cloud=True):
    """name -> bytes (or an integer) of everything a weather map can change"""
    p = oracle.default_params(2048, 1024, SUN)
    p[2], p[3] = TILE[0], TILE[1]
    out = {}
    for name, seg in (("tile", 0), ("tile whole rays", 1)):
        ctx.set_segments(seg)
        out[name] = u16(ctx.render_clouds(p, TILE[2], TILE[3]))
        out[name + " in-cloud"] = int(ctx.cloud_stats()["incloud_samples"])
        assert out[name + " in-cloud"] > 0 or not in_cloud     # an all-sky tile would compare equal whatever the context holds (a generated map promises no cloud there)
    ctx.set_segments(0)
    out["cells"] = ctx.read_baked_texture(2)
    out["held"] = ctx.read_baked_texture(9)
    if exact:
        out["cells32"] = ctx.read_baked_texture(8)
    if tile_only:
        return out
    pv = oracle.default_params(64, 36, SUN)
    pos, cap, basis, fov, w, h = OB.observer("ground")
    out["view"] = u16(ctx.render_clouds_view(pv, basis, fov, w, h))
    pos, cap, basis, fov, w, h = OB.observer("above_down")
    out["view from above_down"] = u16(ctx.render_clouds_view_from(pv, basis, fov, w, h, pos, cap))
    assert (w, h) == (64, 36) and (out["view"][..., 3] != 0).any() and (out["view from above_down"][..., 3] != 0).any()
    out["shadow"] = u16(ctx.render_cloud_shadow(p, 32, 32))
    out["depth"] = u16(ctx.render_cloud_depth(oracle.default_params(64, 32, SUN), 64, 32))
    return out


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        if isinstance(want[k], int):
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k, int((got[k] != want[k]).sum()))


class Fresh:
    """Contexts that have only ever bound one set, and their captures, made on first use and kept for the module."""

    def __init__(self, pkg, noise, oracle):
        self.pkg, self.oracle, self.made, self.captures = pkg, oracle, [], {}
        large, small, weather = noise
        rng = np.random.default_rng(5)
        self.large = {"shipped": large, "white": rng.integers(0, 256, large.shape, dtype=np.uint8)}
        self.small = small
        self.maps = {"shipped": weather, "stratus": stratus_of(weather)}

    def context(self, weather, exact=False, shape="shipped"):
        ctx = self.pkg.Context(0)
        self.made.append(ctx)
        if exact:
            ctx.set_exact_cells(1)
        ctx.set_noise(self.large[shape], self.small, weather if isinstance(weather, np.ndarray) else self.maps[weather])
        with_luts(ctx)
        return ctx

    def capture(self, name, exact=False, shape="shipped", tile_only=False):
        key = (name, exact, shape, tile_only)
        if key not in self.captures:
            ctx = self.context(name, exact, shape)
            self.captures[key] = capture(ctx, self.oracle, exact or shape == "white", tile_only)
            ctx.close()
        return self.captures[key]

    def close(self):
        for c in self.made:
            c.close()


@pytest.fixture(scope="module")
def fresh(pkg, noise, oracle):
    if pkg.lib().csky_device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible (libcloudsky has no CPU fallback)")
    f = Fresh(pkg, noise, oracle)
    yield f
    f.close()


# ---------------------------------------------------------------------------------------------------------------- G1, G2
@pytest.mark.parametrize("exact", [False, True], ids=["fp16-cells", "exact-cells"])
def test_g1_g2_every_weather_rebind_renders_like_a_fresh_context(fresh, oracle, exact):
    a, b = fresh.capture("shipped", exact), fresh.capture("stratus", exact)
    for k in ("tile", "tile whole rays", "view", "view from above_down", "shadow", "depth", "cells", "held"):
        assert (a[k] != b[k]).any(), k                           # the two maps differ in everything compared
    ctx = fresh.context("shipped", exact)
    warning, inexact = ctx.last_warning(), ctx.noise_inexact_coeffs()
    assert inexact == 0
    assert_same(capture(ctx, oracle, exact), a, "after set_noise(shipped)")
    for name in ("stratus", "shipped", "stratus"):
        ctx.set_weather(fresh.maps[name])
        assert_same(capture(ctx, oracle, exact), fresh.capture(name, exact), "after set_weather(%s)" % name)
        assert ctx.last_warning() == warning and ctx.noise_inexact_coeffs() == inexact
    if not exact:
        with pytest.raises(fresh.pkg.CloudSkyError) as e:        # no exact cells were built behind the context's back
            ctx.read_baked_texture(8)
        assert e.value.code == fresh.pkg._lib.ERR_STATE
        # csky_set_exact_cells still waits for the next csky_set_noise*: a weather call is not one
        ctx.set_exact_cells(1)
        ctx.set_weather(fresh.maps["shipped"])
        assert_same(capture(ctx, oracle), a, "a request for exact cells before set_weather")
        with pytest.raises(fresh.pkg.CloudSkyError):
            ctx.read_baked_texture(8)
    ctx.close()


def test_g2_textures_with_inexact_coefficients_stay_on_exact_cells(fresh, oracle):
    want = fresh.capture("stratus", shape="white", tile_only=True)
    ctx = fresh.context("shipped", shape="white")
    warning, inexact = ctx.last_warning(), ctx.noise_inexact_coeffs()
    assert inexact > 0 and "exact fp32 cells" in warning
    ctx.set_weather(fresh.maps["stratus"])
    assert ctx.noise_inexact_coeffs() == inexact and ctx.last_warning() == warning
    assert_same(capture(ctx, oracle, True, tile_only=True), want, "white-noise shape, after set_weather(stratus)")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- G3
def test_g3_the_device_form_gives_the_same_bytes_and_only_reads_its_input(fresh, oracle):
    import torch
    ctx = fresh.context("shipped")
    t = torch.from_numpy(fresh.maps["stratus"]).cuda()
    ctx.set_weather(t)
    assert_same(capture(ctx, oracle), fresh.capture("stratus"), "after set_weather(device tensor)")
    assert (t.cpu().numpy() == fresh.maps["stratus"]).all()
    with pytest.raises(ValueError):
        ctx.set_weather(t.cpu())
    with pytest.raises(ValueError):
        ctx.set_weather(t[:, :, :2])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- G4
@pytest.mark.parametrize("seed", [1, 7])
@pytest.mark.parametrize("block", ["defaults", "tweaked"])
def test_g4_the_kernel_generates_the_host_generators_bytes_and_binds_them(fresh, oracle, seed, block):
    knobs = TWEAKED if block == "tweaked" else {}
    host = fresh.pkg.assets.generate_weather(seed, **knobs)
    ctx = fresh.context("shipped")
    dev = ctx.generate_weather(seed, device=True, **knobs)
    differ = int((dev != host).sum())
    assert differ == 0, "%d bytes differ" % differ
    assert host[..., 2].std() > 5
    shape_chain = ctx.read_baked_texture(3)
    ctx.set_weather(host)
    want = capture(ctx, oracle, in_cloud=False)
    ctx.set_weather(fresh.maps["stratus"])                       # so that nothing of the host map's bind is left to compare equal
    ctx.set_weather_generated(seed, **knobs)
    assert_same(capture(ctx, oracle, in_cloud=False), want, "after set_weather_generated")
    assert (ctx.read_baked_texture(3) == shape_chain).all()
    held = ctx.read_baked_texture(9).view(np.int32)
    assert tuple(held[2:5]) == (int(host[..., 0].min()), int(host[..., 0].max()), int(host[..., 2].max()))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- G5
def test_g5_a_frame_submitted_before_the_call_is_of_the_old_map(fresh, oracle):
    a, b = fresh.capture("shipped"), fresh.capture("stratus")
    p = oracle.default_params(2048, 1024, SUN)
    p[2], p[3] = TILE[0], TILE[1]
    ctx = fresh.context("shipped")
    ctx.set_host_ring(2)
    ticket = ctx.submit_clouds(p, TILE[2], TILE[3])
    ctx.set_weather(fresh.maps["stratus"])
    assert (u16(ctx.collect(ticket)) == a["tile"]).all()
    assert (u16(ctx.collect(ctx.submit_clouds(p, TILE[2], TILE[3]))) == b["tile"]).all()
    assert (u16(ctx.render_clouds(p, TILE[2], TILE[3])) == b["tile"]).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- G6
def test_g6_the_luts_and_the_sky_luts_reuse_state_are_untouched(fresh, oracle):
    ctx = fresh.context("shipped")
    p = oracle.default_params(2048, 1024, SUN)
    p[2], p[3] = TILE[0], TILE[1]
    ctx.render_clouds(p, TILE[2], TILE[3])
    trans, sky, launches = u16(ctx.read_transmittance()), u16(ctx.read_sky_lut()), ctx.sky_lut_launches()
    assert launches >= 1
    ctx.set_weather(fresh.maps["stratus"])
    ctx.set_weather_generated(3)
    assert (u16(ctx.read_transmittance()) == trans).all() and (u16(ctx.read_sky_lut()) == sky).all()
    assert ctx.sky_lut_launches() == launches
    again = u16(ctx.render_sky_lut(norm(SUN), 200, 100))         # the same sun: reused, not re-rendered
    assert (again == sky).all() and ctx.sky_lut_launches() == launches
    ctx.set_weather(fresh.maps["stratus"])
    assert (u16(ctx.render_clouds(p, TILE[2], TILE[3])) == fresh.capture("stratus")["tile"]).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- G7
def test_g7_errors_of_every_entry_point(fresh, oracle):
    import torch
    pkg = fresh.pkg
    L, E = pkg.lib(), pkg._lib
    w = np.ascontiguousarray(fresh.maps["stratus"])
    t = torch.from_numpy(w).cuda()
    hp, dp = w.ctypes.data_as(C.c_void_p), C.c_void_p(t.data_ptr())
    good, bad = E.weather_params(), E.weather_params(coverage_freq=0)
    out = np.full((512, 512, 3), 0xA5, np.uint8)
    op = out.ctypes.data_as(C.c_void_p)
    # NULL context
    assert L.csky_set_weather(None, hp) == E.ERR_INVALID and L.csky_set_weather_device(None, dp) == E.ERR_INVALID
    assert L.csky_set_weather_generated(None, 1, C.byref(good)) == E.ERR_INVALID and L.csky_generate_weather_device(None, 1, C.byref(good), op) == E.ERR_INVALID
    # before any bind: STATE; arguments are judged first
    ctx = pkg.Context(0)
    fresh.made.append(ctx)
    h = ctx._h
    assert L.csky_set_weather(h, hp) == E.ERR_STATE and L.csky_set_weather_device(h, dp) == E.ERR_STATE
    assert L.csky_set_weather_generated(h, 1, C.byref(good)) == E.ERR_STATE and L.csky_set_weather_generated(h, 1, None) == E.ERR_STATE
    assert L.csky_set_weather(h, None) == E.ERR_INVALID and L.csky_set_weather_device(h, None) == E.ERR_INVALID
    assert L.csky_set_weather_generated(h, 1, C.byref(bad)) == E.ERR_INVALID
    assert L.csky_generate_weather_device(h, 1, C.byref(bad), op) == E.ERR_INVALID and L.csky_generate_weather_device(h, 1, C.byref(good), None) == E.ERR_INVALID
    assert (out == 0xA5).all()
    assert L.csky_generate_weather_device(h, 1, None, op) == 0 and (out == pkg.assets.generate_weather(1)).all()    # the generator alone needs no bound set
    ctx.close()
    # a refused call leaves the bound set bound and rendering as before
    ctx = fresh.context("shipped")
    h = ctx._h
    assert L.csky_set_weather(h, None) == E.ERR_INVALID and L.csky_set_weather_device(h, None) == E.ERR_INVALID
    assert L.csky_set_weather_generated(h, 1, C.byref(bad)) == E.ERR_INVALID
    for knobs in (dict(phase=float("nan")), dict(coverage_floor=1.5), dict(type_octaves=40)):
        with pytest.raises(pkg.CloudSkyError) as e:
            ctx.set_weather_generated(1, **knobs)
        assert e.value.code == E.ERR_INVALID and "weather parameters" in str(e.value)
    assert_same(capture(ctx, oracle, tile_only=True), fresh.capture("shipped", tile_only=True), "after refused calls")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- G8
@pytest.mark.parametrize("device_buffers", [False, True], ids=["host-buffers", "device-buffers"])
def test_g8_cloud_sky_set_weather_gives_the_bytes_of_the_c_calls(fresh, oracle, noise, device_buffers):
    import torch
    sky = fresh.pkg.CloudSky(0, texture_size=64, noise=noise, device_buffers=device_buffers)
    try:
        with_luts(sky.ctx)
        stratus = fresh.maps["stratus"]
        sky.set_weather(torch.from_numpy(stratus).cuda() if device_buffers else stratus)
        assert_same(capture(sky.ctx, oracle, tile_only=True), fresh.capture("stratus", tile_only=True), "CloudSky.set_weather(map)")
        ctx = fresh.context("shipped")
        ctx.set_weather_generated(3)
        want = capture(ctx, oracle, tile_only=True, in_cloud=False)
        ctx.close()
        sky.set_weather(seed=3)
        assert_same(capture(sky.ctx, oracle, tile_only=True, in_cloud=False), want, "CloudSky.set_weather(seed=3)")
        sky.set_weather(seed=3, phase=0.5)
        assert (sky.ctx.read_baked_texture(2) != want["cells"]).any()
        with pytest.raises(ValueError):
            sky.set_weather()
    finally:
        sky.close()
