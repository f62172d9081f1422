"""The cloud shadow map on the GPU (csky_render_cloud_shadow / _device; csrc/shadow.hip) against the numpy restatement of its definition
(tests/shadow_reference.py, which calls the oracle per sample), at the project's gate for values rendered from the shipped assets: every texel
within 2 fp16 ulp, 99.9 % within 1, largest difference 2e-3.  Then what a launch may touch: its W x H halfs and nothing else, no state of the
cloud frames, the same bytes whatever the exact end does.  Tests 9 and 10: the scene sweep of shadow_reference.SCENES (12 scenes, suns from the
zenith down to a third of a degree over the rectangles csky_aerial_shadow_rect hands out, ordinary, chord and miss texels) on every context of the
scene's weather map, and two of its low-sun scenes device form against host form; 21 tests in all."""
import ctypes as C

import numpy as np
import pytest

import shadow_reference as SR
from conftest import norm

pytestmark = pytest.mark.gpu

GUARD = 4                           # guard rows before and after the map
PAD = 14                            # bytes of padding behind each row: the pitch is even and no multiple of 4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.fixture(scope="module")
def fresh_ctx(pkg, noise):
    """noise set, no LUT ever rendered"""
    ctx = pkg.Context(0)
    ctx.set_noise(*noise)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def exact_ctx(pkg, noise):
    """exact-cells mode: the march on TexSet32"""
    ctx = pkg.Context(0)
    ctx.set_exact_cells(1)
    ctx.set_noise(*noise)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", ["A", "B"])
def test_scenes_match_reference(gpu_ctx, fresh_ctx, exact_ctx, oracle, otex, name):
    """Test 5."""
    p = SR.scene(oracle, name)
    ref, _ = SR.shadow_map(oracle, otex, p, **SR.SCENE_SIZE)
    if name == "A":                                              # preconditions on the REFERENCE: a blank map cannot pass
        assert (bits(ref) == 0x3C00).mean() >= 0.30 and (ref.astype(np.float32) < 0.9).mean() >= 0.40
    else:
        assert (bits(ref) == 0).mean() >= 0.25 and (bits(ref) == 0x3C00).mean() >= 0.02
    s = SR.SCENE_SIZE
    args = (p, s["width"], s["height"], s["center"], s["extent"], s["steps"])
    m = gpu_ctx.render_cloud_shadow(*args)
    SR.assert_gate(m, ref, "GPU, scene " + name)
    assert fresh_ctx.sky_lut_launches() == 0                     # no LUT on this context
    f = fresh_ctx.render_cloud_shadow(*args)
    assert fresh_ctx.sky_lut_launches() == 0
    SR.assert_gate(f, ref, "GPU, no LUT, scene " + name)
    assert (bits(f) == bits(m)).all()
    e = exact_ctx.render_cloud_shadow(*args)
    SR.assert_gate(e, ref, "GPU, exact cells, scene " + name)


def poisoned_render(ctx, p, W, H, center, extent, N, runs=3):
    """The device form into a tensor of 0xFFFF halfs (a NaN no map contains) with GUARD rows before and after and PAD bytes behind each row: nothing
    of the poison is left inside the map, none is lost outside it, and the bytes are the host form's.  Returns the host form's map."""
    import torch
    host = ctx.render_cloud_shadow(p, W, H, center, extent, N)
    assert not (bits(host) == 0xFFFF).any()
    pitch = 2 * W + PAD
    s = torch.cuda.Stream()
    for run in range(runs):
        with torch.cuda.stream(s):
            t = torch.empty((H + 2 * GUARD, pitch // 2), dtype=torch.int16, device="cuda")
            t.fill_(-1)
            share = t[GUARD:GUARD + H, :W]
            assert share.stride(0) * 2 == pitch
            out = ctx.render_cloud_shadow(p, W, H, center, extent, N, out=share, stream=s.cuda_stream)
            assert out is share
            got = t.cpu().numpy().view(np.uint16)
        inside = np.zeros(got.shape, bool)
        inside[GUARD:GUARD + H, :W] = True
        assert not (got[inside] == 0xFFFF).any(), (run, np.argwhere(inside & (got == 0xFFFF))[:4])
        assert (got[~inside] == 0xFFFF).all(), (run, np.argwhere(~inside & (got != 0xFFFF))[:4])
        assert (got[GUARD:GUARD + H, :W] == bits(host)).all(), run
    return host


@pytest.mark.parametrize("size", [(64, 64, 32, (0.0, 0.0), (16384.0, 16384.0)), (37, 21, 17, (1000.0, -3000.0), (9000.0, 9000.0))], ids=["64x64", "37x21"])
def test_write_coverage(gpu_ctx, oracle, size):
    """Test 6: the device form into a tensor of 0xFFFF halfs (a NaN no map contains) with guard rows and row padding."""
    W, H, N, center, extent = size
    host = poisoned_render(gpu_ctx, SR.scene(oracle, "A"), W, H, center, extent, N)
    assert len(np.unique(bits(host))) > 8


def test_isolation(gpu_ctx, oracle):
    """Test 7: a shadow call leaves the cloud frames alone, repeats itself, and does not depend on the exact end."""
    sun = norm((1, 1, 0))
    gpu_ctx.render_transmittance(256, 64)
    gpu_ctx.render_sky_lut(sun, 200, 100)
    pc = oracle.default_params(64, 32, (1, 1, 0))
    before = gpu_ctx.render_clouds(pc, 64, 32)
    pb = SR.scene(oracle, "B")
    s = SR.SCENE_SIZE
    args = (pb, s["width"], s["height"], s["center"], s["extent"], s["steps"])
    one = gpu_ctx.render_cloud_shadow(*args)
    after = gpu_ctx.render_clouds(pc, 64, 32)
    assert (bits(before) == bits(after)).all() and bits(before).any()
    two = gpu_ctx.render_cloud_shadow(*args)
    assert (bits(one) == bits(two)).all()
    assert (bits(one) == 0).mean() >= 0.25                       # the exact end has something to fire on
    try:
        gpu_ctx.set_shadow_exact_end(False)
        off = gpu_ctx.render_cloud_shadow(*args)
    finally:
        gpu_ctx.set_shadow_exact_end(True)
    assert (bits(one) == bits(off)).all()
    again = gpu_ctx.render_clouds(pc, 64, 32)
    assert (bits(before) == bits(again)).all()


def test_error_paths(pkg, gpu_ctx, oracle):
    """Test 8, first half: every CSKY_ERR_INVALID and CSKY_ERR_STATE case of the header."""
    import torch
    L, lib = pkg.lib(), pkg._lib
    h = gpu_ctx._h
    p = lib.cloud_params(SR.scene(oracle, "A"))
    out = np.zeros((16, 16), np.uint16)
    optr = out.ctypes.data_as(C.c_void_p)
    d = torch.zeros((16, 32), dtype=torch.int16, device="cuda")
    dptr = C.c_void_p(d.data_ptr())

    def sp(width=16, height=16, center=(0.0, 0.0), extent=(4096.0, 4096.0), steps=8):
        return lib.ShadowParams(width, height, (C.c_float * 2)(*center), (C.c_float * 2)(*extent), steps)

    def host(ctx=h, params=p, s=None, o=optr):
        return L.csky_render_cloud_shadow(ctx, C.byref(params) if params is not None else None, C.byref(s) if s is not None else None, o)

    def dev(ctx=h, params=p, s=None, o=dptr, pitch=64):
        return L.csky_render_cloud_shadow_device(ctx, C.byref(params) if params is not None else None, C.byref(s) if s is not None else None, o, pitch, None)

    assert host(s=sp()) == lib.OK and dev(s=sp()) == lib.OK
    assert dev(s=sp(), pitch=32) == lib.OK and dev(s=sp(), pitch=34) == lib.OK
    torch.cuda.synchronize()
    INV = lib.ERR_INVALID
    # NULL pointers
    assert host(ctx=None, s=sp()) == INV and host(params=None, s=sp()) == INV and host(s=None) == INV and host(s=sp(), o=None) == INV
    assert dev(ctx=None, s=sp()) == INV and dev(params=None, s=sp()) == INV and dev(s=None) == INV and dev(s=sp(), o=None) == INV
    # sizes, steps, extents
    for bad in (sp(width=0), sp(width=8193), sp(height=0), sp(height=8193), sp(width=-1), sp(steps=-1), sp(steps=1025), sp(extent=(0.0, 4096.0)),
                sp(extent=(4096.0, -1.0)), sp(center=(999000.0, 0.0), extent=(4096.0, 4096.0)), sp(center=(0.0, -1.0e6), extent=(4096.0, 2.0)),
                sp(extent=(2.1e6, 4096.0))):
        assert host(s=bad) == INV and dev(s=bad, pitch=2 * 8193) == INV, (bad.width, bad.height, bad.steps, list(bad.center), list(bad.extent))
    assert host(s=sp(steps=0)) == lib.OK and host(s=sp(steps=1)) == lib.OK and host(s=sp(steps=1024)) == lib.OK
    assert host(s=sp(center=(997952.0, 0.0), extent=(4096.0, 4096.0))) == lib.OK          # |center| + extent / 2 == 1e6
    up = float(np.nextafter(np.float32(997952.0), np.float32(np.inf)))                     # the next float up: 1e6 + 2^-4 is a float, and refused
    assert np.float32(up) + np.float32(2048.0) == np.nextafter(np.float32(1.0e6), np.float32(np.inf))
    for bad in (sp(center=(up, 0.0), extent=(4096.0, 4096.0)), sp(center=(0.0, -up), extent=(4096.0, 4096.0))):
        assert host(s=bad) == INV and dev(s=bad) == INV
    assert host(s=sp(center=(0.0, -997952.0), extent=(4096.0, 4096.0))) == lib.OK
    # non-finite floats: the map's own and every field of the block that is read
    for bad in (sp(center=(float("nan"), 0.0)), sp(center=(0.0, float("inf"))), sp(extent=(float("inf"), 4096.0)), sp(extent=(4096.0, float("nan")))):
        assert host(s=bad) == INV and dev(s=bad) == INV
    for k in (4, 5, 6, 7, 8, 9, 16, 17, 18, 23, 25, 26):
        for v in (float("nan"), float("-inf")):
            q = lib.cloud_params(SR.scene(oracle, "A"))
            q.f[k] = v
            assert host(params=q, s=sp()) == INV and dev(params=q, s=sp()) == INV, (k, v)
    q = lib.cloud_params(SR.scene(oracle, "A"))
    for k in (0, 1, 2, 3, 10, 11, 12, 13, 14, 15, 19, 20, 21, 22, 24, 27):                 # the fields that are not read may hold anything
        q.f[k] = float("nan")
    a, b = np.zeros((16, 16), np.uint16), np.zeros((16, 16), np.uint16)
    assert host(params=q, s=sp(), o=a.ctypes.data_as(C.c_void_p)) == lib.OK and host(s=sp(), o=b.ctypes.data_as(C.c_void_p)) == lib.OK
    assert (a == b).all()
    # pitch
    assert dev(s=sp(), pitch=30) == INV and dev(s=sp(), pitch=33) == INV and dev(s=sp(), pitch=0) == INV
    assert b"pitch" in L.csky_last_error(h)
    # no noise
    bare = pkg.Context(0)
    try:
        assert host(ctx=bare._h, s=sp()) == lib.ERR_STATE and dev(ctx=bare._h, s=sp()) == lib.ERR_STATE
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.render_cloud_shadow(SR.scene(oracle, "A"), 16, 16)
        assert e.value.code == lib.ERR_STATE
    finally:
        bare.close()
    assert L.csky_set_shadow_exact_end(None, 1) == INV
    torch.cuda.synchronize()


def test_python_mirror(pkg, noise):
    """Test 8, second half: CloudSky.cloud_shadow_map is Context.render_cloud_shadow fed the block _fill_push_constant() packs."""
    for device_buffers in (False, True):
        sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=device_buffers)
        try:
            sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
            sky.update_sky()
            m = sky.cloud_shadow_map(size=64, steps=32)
            if device_buffers:
                import torch
                assert isinstance(m, torch.Tensor) and m.dtype == torch.float16 and m.is_cuda
                m = m.cpu().numpy()
            assert m.shape == (64, 64) and m.dtype == np.float16
            direct = sky.ctx.render_cloud_shadow(sky._fill_push_constant(), 64, 64, (0.0, 0.0), (16384.0, 16384.0), 32)
            assert (bits(m) == bits(direct)).all()
            v = m.astype(np.float32)
            assert np.isfinite(v).all() and v.min() >= 0.0 and v.max() <= 1.0 and len(np.unique(bits(m))) > 16
            r = sky.cloud_shadow_map(size=(40, 24), extent=(8192.0, 4096.0), center=(100.0, -200.0), steps=16)
            r = r.cpu().numpy() if device_buffers else r
            assert r.shape == (24, 40)
            assert (bits(r) == bits(sky.ctx.render_cloud_shadow(sky._fill_push_constant(), 40, 24, (100.0, -200.0), (8192.0, 4096.0), 16))).all()
        finally:
            sky.close()


# ---------------------------------------------------------------------------------------------------------------- the scene sweep (shadow_reference.SCENES)
@pytest.fixture(scope="module")
def sweep_ctxs(pkg, noise, gpu_ctx, fresh_ctx, exact_ctx):
    """weather name -> the contexts a scene of that weather runs on (the white-noise weather map: exact-cells mode, the mixed cloud-type branch)"""
    large, small, weather = noise
    stratus, white = pkg.Context(0), pkg.Context(0)
    stratus.set_noise(large, small, SR.weather_map(weather, "stratus"))
    white.set_exact_cells(1)
    white.set_noise(large, small, SR.weather_map(weather, "white"))
    yield {"shipped": {"": gpu_ctx, ", no LUT": fresh_ctx, ", exact cells": exact_ctx}, "stratus": {", stratus": stratus}, "white": {", exact cells, white-noise weather": white}}
    stratus.close()
    white.close()


@pytest.fixture(scope="module")
def sweep_otex(oracle, noise, otex):
    large, small, weather = noise
    cache = {"shipped": otex}

    def get(which):
        if which not in cache:
            cache[which] = oracle.OracleTextures(large, small, SR.weather_map(weather, which))
        return cache[which]
    return get


@pytest.mark.parametrize("name", list(SR.SCENES))
def test_sweep_matches_reference(sweep_ctxs, sweep_otex, oracle, name):
    """Test 9: every scene of the sweep through the C ABI at the gate over all its texels, no NaN anywhere; suns down to a third of a degree, the
    helper's rectangles, ordinary, chord and miss texels (cloudsky.h) in one wavefront's tile, step counts that end between the wave votes."""
    from test_shadow_host import sweep_preconditions
    sc = SR.SCENES[name]
    p, size = SR.sweep_scene(oracle, name)
    n = size["steps"] or 64
    kind = SR.texel_kinds(p, size["width"], size["height"], size["center"], size["extent"])
    ref, _ = SR.shadow_map(oracle, sweep_otex(sc["weather"]), p, **dict(size, steps=n))
    sweep_preconditions(name, ref, kind)
    args = (p, size["width"], size["height"], size["center"], size["extent"], size["steps"])     # steps as the table has it: 0 = 64
    first = None
    for what, ctx in sweep_ctxs[sc["weather"]].items():
        m = ctx.render_cloud_shadow(*args)
        SR.assert_gate(m, ref, "GPU%s, sweep %s" % (what, name))
        assert (bits(m)[kind == SR.MISS] == 0x3C00).all()
        if what == ", no LUT":
            assert (bits(m) == bits(first)).all() and ctx.sky_lut_launches() == 0
        first = m if first is None else first
    if sc["mixed"] and sc["weather"] == "shipped":                # chord lanes and ordinary lanes share a wave vote: the bytes do not depend on the exits
        ctx = sweep_ctxs["shipped"][""]
        try:
            ctx.set_shadow_exact_end(False)
            ctx.set_height_window(0)
            plain = ctx.render_cloud_shadow(*args)
        finally:
            ctx.set_shadow_exact_end(True)
            ctx.set_height_window(1)
        assert (bits(plain) == bits(first)).all()


@pytest.mark.parametrize("name", ["deg1.1", "deg0.66-z"])
def test_sweep_write_coverage(gpu_ctx, oracle, name):
    """Test 10: two low-sun scenes, device form against host form, in test 6's poisoned, pitched and guarded tensor."""
    p, size = SR.sweep_scene(oracle, name)
    assert SR.SCENES[name]["kinds"][1] > 0
    host = poisoned_render(gpu_ctx, p, size["width"], size["height"], size["center"], size["extent"], size["steps"], runs=2)
    assert np.isfinite(host.astype(np.float32)).all() and len(np.unique(bits(host))) > 8
