"""The shadowed aerial-perspective volume on the GPU (csky_render_aerial_perspective_shadowed / _device; csrc/shafts.hip) through the C ABI: against
the host-compiled core (tests/shafts_host: the definition the kernel must equal) and the numpy restatement of the contract
(tests/shafts_reference.py) at the volume's gate, every half within 1 fp16 ulp; then what ties it to the plain volume, the chunk boundaries of the
kernel, what a launch may touch, what state it needs and leaves, every error path, CloudSky's pair of launches, and the chain rectangle -> map ->
volume at suns about one degree up, where the map has chord texels (include/cloudsky.h).  The host core and the
restatement are given the GPU's own transmittance table: the volume kernel alone is compared."""
import ctypes as C

import numpy as np
import pytest

import aerial_reference as AR
import shadow_reference as SHR
import shafts_reference as SR
from test_aerial_host import CASES, SUNS, case_view
from test_shafts_host import (C4, LOW_MAP, LOW_SUNS, LOW_VIEWS, LOW_VOLUME, M, M_CENTER, M_EXTENT, low_sun_map_args, low_sun_reference, shafts_host,  # noqa: F401
                              shafts_volume)                                             # (shafts_host: the module-scoped fixture)

pytestmark = pytest.mark.gpu
GUARD = 64                          # halfs of guard before and after the volume (a multiple of 4: texels are stored whole)
ONES = np.ones_like(M)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.fixture(scope="module")
def ctxs(pkg):
    """One context per mapping with a transmittance table and nothing else: no noise, no sky LUT."""
    if pkg.lib().csky_device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible (libcloudsky has no CPU fallback)")
    out = {}
    for m in (0, 1):
        out[m] = pkg.Context(0)
        out[m].set_transmittance_mapping(m)
        out[m].render_transmittance(256, 64)
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def tables(ctxs):
    return {m: ctxs[m].read_transmittance() for m in (0, 1)}


def gpu_shafts(ctx, W, H, D, S, far, sun, shadow=M, center=M_CENTER, extent=M_EXTENT, view=None, aspect=0.0, **kw):
    return ctx.render_aerial_perspective_shadowed(sun, shadow, center, extent, W, H, D, far, S, view, aspect, **kw)


def device_map(shadow, pitch_h=None):
    """The map on the GPU as a [h, w] view of 2-byte elements; pitch_h > w: rows of pitch_h halfs whose padding is NaN halfs."""
    import torch
    m = bits(np.asarray(shadow, np.float16)).view(np.int16)
    if pitch_h is None:
        return torch.from_numpy(m.copy()).cuda()
    padded = np.full((m.shape[0], pitch_h), 0x7E00, np.uint16).view(np.int16)
    padded[:, :m.shape[1]] = m
    return torch.from_numpy(padded).cuda()[:, :m.shape[1]]


# ---------------------------------------------------------------------------------------------------------------- G1. the cases of the host tests
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_cases_match_host_core_and_restatement(ctxs, tables, shafts_host, case, mapping):  # noqa: F811
    W, H, D, S, far = CASES[case][:5]
    view, aspect = case_view(case)
    for sun in SUNS:
        got = gpu_shafts(ctxs[mapping], W, H, D, S, far, SUNS[sun], view=view, aspect=aspect)
        assert got.shape == (D, H, W, 4) and np.isfinite(got.astype(np.float32)).all()
        core, st = shafts_volume(shafts_host, mapping, tables[mapping], W, H, D, S, far, SUNS[sun], M, M_CENTER, M_EXTENT, view, aspect, state=True)
        ref = SR.volume(W, H, D, S, far, SUNS[sun], tables[mapping], M, M_CENTER, M_EXTENT, mapping, view, aspect)
        assert not ref["near"].any()
        if sun != "degm2":                                         # a volume the map does not reach cannot pass
            assert (ref["s"][ref["take"]] < 1).mean() >= 0.04
        what = "%s %s mapping %d" % (case, sun, mapping)
        d_core, _ = AR.gate(got, core, what=what + ", GPU vs host core")
        d_ref, cancel = AR.gate(got, ref["out"], st[..., :4], ref["L"], what=what + ", GPU vs restatement")
        print("%s: %d of %d halves differ from the host core, %d from the restatement (%d let through as cancellation)" % (what, d_core, got.size, d_ref, cancel))
    assert ctxs[mapping].sky_lut_launches() == 0                    # no sky LUT was needed or made


@pytest.mark.parametrize("mapping", [0, 1])
def test_height_rule(ctxs, tables, shafts_host, mapping):  # noqa: F811
    c = C4
    got = gpu_shafts(ctxs[mapping], c["W"], c["H"], c["D"], c["S"], c["far"], c["sun"], c["shadow"], c["center"], c["extent"])
    core, st = shafts_volume(shafts_host, mapping, tables[mapping], c["W"], c["H"], c["D"], c["S"], c["far"], c["sun"], c["shadow"], c["center"], c["extent"], state=True)
    ref = SR.volume(c["W"], c["H"], c["D"], c["S"], c["far"], c["sun"], tables[mapping], c["shadow"], c["center"], c["extent"], mapping)
    h = ref["h"][ref["take"]]
    assert min((h <= 1500).mean(), ((h > 1500) & (h < 4000)).mean(), (h >= 4000).mean()) >= 0.20
    d_core, _ = AR.gate(got, core, what="height rule mapping %d, GPU vs host core" % mapping)
    d_ref, cancel = AR.gate(got, ref["out"], st[..., :4], ref["L"], what="height rule mapping %d, GPU vs restatement" % mapping)
    print("height rule mapping %d: %d of %d halves differ from the host core, %d from the restatement (%d let through as cancellation)" % (mapping, d_core, got.size, d_ref, cancel))


# ---------------------------------------------------------------------------------------------------------------- G1b. rectangle -> map -> volume at sunrise
@pytest.mark.parametrize("sun", list(LOW_SUNS))
def test_low_sun_chain(pkg, gpu_ctx, ctxs, tables, shafts_host, oracle, sun):  # noqa: F811
    """The chain the product runs, at suns 1.1 and 0.66 degrees up: a 64 x 16 map rendered on the GPU over the helper's rectangle (it has chord
    texels: cloudsky.h) inside a 13 x 7 x 8 volume, through the panorama and a camera view.  Every half is finite; the volume meets the gates of G1
    against the host core and the restatement fed the same map; alpha is the plain volume's."""
    p, l, center, extent, kind = low_sun_map_args(oracle, sun)
    want = pkg.aerial_shadow_rect(l, LOW_VOLUME["far"])
    assert np.allclose(want[0], center, rtol=1e-6, atol=0) and np.allclose(want[1], extent, rtol=1e-6, atol=0)
    shadow = gpu_ctx.render_cloud_shadow(p, LOW_MAP["width"], LOW_MAP["height"], center, extent, LOW_MAP["steps"])
    assert np.isfinite(shadow.astype(np.float32)).all() and len(np.unique(bits(shadow)[kind == SHR.CHORD])) > 2
    v = LOW_VOLUME
    for view in LOW_VIEWS:
        ref, n_chord, n_tapped = low_sun_reference(tables[0], 0, l, shadow, center, extent, kind, view)
        vw, aspect = case_view(view)
        aspect = 0.0 if vw is None else aspect
        got = gpu_shafts(ctxs[0], v["W"], v["H"], v["D"], v["S"], v["far"], l, shadow, center, extent, view=vw, aspect=aspect)
        assert got.shape == (v["D"], v["H"], v["W"], 4) and np.isfinite(got.astype(np.float32)).all()
        core, st = shafts_volume(shafts_host, 0, tables[0], v["W"], v["H"], v["D"], v["S"], v["far"], l, shadow, center, extent, vw, aspect, state=True)
        what = "low sun %s %s" % (sun, view)
        d_core, _ = AR.gate(got, core, what=what + ", GPU vs host core")
        d_ref, cancel = AR.gate(got, ref["out"], st[..., :4], ref["L"], what=what + ", GPU vs restatement")
        print("%s: %d of %d tapped steps project into a chord texel; %d of %d halves differ from the host core, %d from the restatement (%d let through as cancellation)"
              % (what, n_chord, n_tapped, d_core, got.size, d_ref, cancel))
        plain = ctxs[0].render_aerial_perspective(l, v["W"], v["H"], v["D"], v["far"], v["S"], vw, aspect)
        assert (bits(got[..., 3]) == bits(plain[..., 3])).all() and (bits(got[..., :3]) != bits(plain[..., :3])).any()


# ---------------------------------------------------------------------------------------------------------------- G2. the ties to the plain volume
@pytest.mark.parametrize("mapping", [0, 1])
def test_ties_to_the_plain_volume(ctxs, mapping):
    import torch
    ctx = ctxs[mapping]
    for case in CASES:
        W, H, D, S, far = CASES[case][:5]
        view, aspect = case_view(case)
        for sun in SUNS:
            plain = ctx.render_aerial_perspective(SUNS[sun], W, H, D, far, S, view, aspect)

            def dev(shadow):
                out = torch.empty((D, H, W, 4), dtype=torch.float16, device="cuda")
                gpu_shafts(ctx, W, H, D, S, far, SUNS[sun], device_map(shadow), view=view, aspect=aspect, out=out)
                ctx.sync()
                return out.cpu().numpy()
            assert (bits(dev(ONES)) == bits(plain)).all(), (case, sun)                # a map of all 1.0
            with_m = dev(M)
            assert (bits(with_m[..., 3]) == bits(plain[..., 3])).all(), (case, sun)  # alpha never sees the map
            if sun == "degm2":
                assert (bits(with_m) == bits(plain)).all(), case                      # the sun is down: the map is not read
            else:
                assert (AR.ulp_dist(with_m[..., :3], plain[..., :3]) > 8).mean() >= 0.15, (case, sun)
    zero = ctx.render_aerial_perspective((0.0, 0.0, 0.0), 13, 7, 5, 40.0, 3)
    assert (bits(gpu_shafts(ctx, 13, 7, 5, 3, 40.0, (0.0, 0.0, 0.0))) == bits(zero)).all()   # no direction at all


# ---------------------------------------------------------------------------------------------------------------- G3. chunk ends
@pytest.mark.parametrize("DS", [(21, 3), (16, 4), (13, 5), (192, 1), (32, 16)], ids=["n63", "n64", "n65", "n192", "n512"])
def test_chunk_boundaries(ctxs, tables, shafts_host, DS):  # noqa: F811
    """9 x 5 columns of the down-looking camera (columns stop inside the reach: later chunks start beyond t_stop) with step counts on both sides
    of a chunk end; D = 192, S = 1 has 64 slice ends in every chunk."""
    D, S = DS
    view, aspect = case_view("down")
    got = gpu_shafts(ctxs[0], 9, 5, D, S, 64.0, SUNS["deg45"], view=view, aspect=aspect)
    core = shafts_volume(shafts_host, 0, tables[0], 9, 5, D, S, 64.0, SUNS["deg45"], M, M_CENTER, M_EXTENT, view, aspect)
    differ, _ = AR.gate(got, core, what="n = %d, GPU vs host core" % (D * S))
    print("n = %d: %d of %d halves differ from the host core" % (D * S, differ, got.size))
    plain = ctxs[0].render_aerial_perspective(SUNS["deg45"], 9, 5, D, 64.0, S, view, aspect)
    assert (bits(got[..., 3]) == bits(plain[..., 3])).all() and (AR.ulp_dist(got[..., :3], plain[..., :3]) > 8).mean() >= 0.15
    assert (bits(got)[-1] == bits(got)[D // 2]).all(-1).mean() >= 0.25      # columns that stopped in the first half: their later chunks evaluated nothing


def test_split_identity_on_the_device(ctxs):
    view, aspect = case_view("down")
    for m in (0, 1):
        fine = bits(gpu_shafts(ctxs[m], 13, 7, 16, 2, 64.0, SUNS["deg45"], view=view, aspect=aspect))
        coarse = bits(gpu_shafts(ctxs[m], 13, 7, 8, 4, 64.0, SUNS["deg45"], view=view, aspect=aspect))
        assert (coarse == fine[1::2]).all()


# ---------------------------------------------------------------------------------------------------------------- G4. write coverage
@pytest.mark.parametrize("size", [(13, 7, 5), (1, 1, 1)], ids=["13x7x5", "1x1x1"])
def test_write_coverage(ctxs, size):
    """The device form into a buffer of 0xFFFF halfs (a NaN no volume contains) with guard regions before and after; the map tight, pitched with NaN
    halfs in its padding, and a single texel; on a caller's stream and on NULL (the context's own stream); the host form gives the same bytes."""
    import torch
    W, H, D = size
    ctx = ctxs[0]
    view, aspect = case_view("down")
    n = D * H * W * 4
    one = np.full((1, 1), 0.5, np.float16)
    maps = {"tight": (M, device_map(M)), "pitched": (M, device_map(M, M.shape[1] + 7)), "1x1": (one, device_map(one))}
    assert maps["pitched"][1].stride(0) == M.shape[1] + 7
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for name, (host_map, dev_map) in maps.items():
        host = gpu_shafts(ctx, W, H, D, 3, 64.0, SUNS["demo"], host_map, view=view, aspect=aspect)
        assert not (bits(host) == 0xFFFF).any() and np.isfinite(host.astype(np.float32)).all()
        for stream in (s, None):
            t = torch.empty(n + 2 * GUARD, dtype=torch.int16, device="cuda")
            t.fill_(-1)
            torch.cuda.synchronize()
            share = t[GUARD:GUARD + n].view(D, H, W, 4)
            out = gpu_shafts(ctx, W, H, D, 3, 64.0, SUNS["demo"], dev_map, view=view, aspect=aspect, out=share, stream=stream.cuda_stream if stream else None)
            assert out is share
            if stream:
                stream.synchronize()
            else:
                ctx.sync()
            got = t.cpu().numpy().view(np.uint16)
            assert not (got[GUARD:GUARD + n] == 0xFFFF).any(), name
            assert (got[:GUARD] == 0xFFFF).all() and (got[GUARD + n:] == 0xFFFF).all(), name
            assert (got[GUARD:GUARD + n] == bits(host).reshape(-1)).all(), name
    if size == (13, 7, 5):
        plain = ctx.render_aerial_perspective(SUNS["demo"], W, H, D, 64.0, 3, view, aspect)
        assert (bits(gpu_shafts(ctx, W, H, D, 3, 64.0, SUNS["demo"], view=view, aspect=aspect)) != bits(plain)).any()


# ---------------------------------------------------------------------------------------------------------------- G5. state, isolation, errors
def test_state_and_isolation(pkg, gpu_ctx, ctxs, oracle):
    lib = pkg._lib
    bare = pkg.Context(0)
    try:
        with pytest.raises(pkg.CloudSkyError) as e:                 # no table
            gpu_shafts(bare, 4, 4, 2, 2, 32.0, SUNS["demo"])
        assert e.value.code == lib.ERR_STATE
        bare.render_transmittance(256, 64)                          # a table, no noise, no sky LUT: renders
        v0 = gpu_shafts(bare, 13, 7, 5, 3, 40.0, SUNS["demo"])
        assert bare.sky_lut_launches() == 0 and (bits(v0) == bits(gpu_shafts(ctxs[0], 13, 7, 5, 3, 40.0, SUNS["demo"]))).all()
        bare.set_transmittance_mapping(1)                           # the table goes with the mapping
        with pytest.raises(pkg.CloudSkyError) as e:
            gpu_shafts(bare, 13, 7, 5, 3, 40.0, SUNS["demo"])
        assert e.value.code == lib.ERR_STATE
        bare.render_transmittance(256, 64)
        v1 = gpu_shafts(bare, 13, 7, 5, 3, 40.0, SUNS["demo"])
        assert (bits(v1) == bits(gpu_shafts(ctxs[1], 13, 7, 5, 3, 40.0, SUNS["demo"]))).all() and (bits(v1) != bits(v0)).any()
    finally:
        bare.close()
    gpu_ctx.render_transmittance(256, 64)
    gpu_ctx.render_sky_lut(SUNS["deg45"], 200, 100)
    pc = oracle.default_params(160, 80, (1, 1, 0))
    frame, lut, launches = gpu_ctx.render_clouds(pc, 160, 80), gpu_ctx.read_sky_lut(), gpu_ctx.sky_lut_launches()
    assert bits(frame).any()
    v = gpu_shafts(gpu_ctx, 13, 7, 5, 3, 40.0, SUNS["demo"])
    assert (bits(v) == bits(v0)).all()
    assert gpu_ctx.sky_lut_launches() == launches
    assert (bits(gpu_ctx.read_sky_lut()) == bits(lut)).all()
    assert (bits(gpu_ctx.render_clouds(pc, 160, 80)) == bits(frame)).all()
    assert gpu_ctx.sky_lut_launches() == launches


def test_error_paths(pkg, ctxs):
    import torch
    L, lib = pkg.lib(), pkg._lib
    h = ctxs[0]._h
    INV, nan, inf = lib.ERR_INVALID, float("nan"), float("inf")
    out = np.zeros((8, 4, 4, 4), np.uint16)
    optr = out.ctypes.data_as(C.c_void_p)
    d = torch.zeros(8 * 4 * 4 * 4, dtype=torch.int16, device="cuda")
    dptr = C.c_void_p(d.data_ptr())
    mh = bits(M)
    mptr = mh.ctypes.data_as(C.c_void_p)
    dm = device_map(M)
    dmptr = C.c_void_p(dm.data_ptr())
    p = lib.AerialParams(4, 4, 8, 2, 32.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0))

    def sp(width=24, height=16, center=M_CENTER, extent=M_EXTENT, steps=0):
        return lib.ShadowParams(width, height, (C.c_float * 2)(*center), (C.c_float * 2)(*extent), steps)

    def both(s, ap=p, ctx=h, o=True, m=True, pitch=48):
        sa, pa = (C.byref(s) if s is not None else None), (C.byref(ap) if ap is not None else None)
        return (L.csky_render_aerial_perspective_shadowed(ctx, pa, None, sa, mptr if m else None, optr if o else None),
                L.csky_render_aerial_perspective_shadowed_device(ctx, pa, None, sa, dmptr if m else None, pitch, dptr if o else None, None))

    assert both(sp()) == (lib.OK, lib.OK)
    assert both(sp(steps=-5)) == (lib.OK, lib.OK) and both(sp(steps=100000)) == (lib.OK, lib.OK)   # steps is not read
    # NULL pointers
    assert both(sp(), ctx=None) == (INV, INV) and both(None) == (INV, INV) and both(sp(), ap=None) == (INV, INV)
    assert both(sp(), o=False) == (INV, INV) and both(sp(), m=False) == (INV, INV)
    # the map's size
    for bad in (sp(width=0), sp(width=-1), sp(width=8193), sp(height=0), sp(height=-1), sp(height=8193)):
        assert both(bad, pitch=2 * 8193) == (INV, INV), (bad.width, bad.height)
    # its rectangle
    for k in range(2):
        for v in (nan, inf, -inf):
            c = list(M_CENTER)
            c[k] = v
            assert both(sp(center=c)) == (INV, INV), (k, v)
        for v in (nan, inf, 0.0, -1.0):
            e = list(M_EXTENT)
            e[k] = v
            assert both(sp(extent=e)) == (INV, INV), (k, v)
    assert b"extent" in L.csky_last_error(h)
    # the pitch (the device form's alone)
    for pitch in (0, 46, 47, 49):
        assert both(sp(), pitch=pitch)[1] == INV, pitch
    assert b"pitch" in L.csky_last_error(h)
    # the volume's own arguments are still checked
    for bad in (lib.AerialParams(513, 4, 8, 2, 32.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0)), lib.AerialParams(4, 4, 257, 2, 32.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0)),
                lib.AerialParams(4, 4, 8, 17, 32.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0)), lib.AerialParams(4, 4, 8, 2, -1.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0)),
                lib.AerialParams(4, 4, 8, 2, 32.0, 0.0, (C.c_float * 3)(0.6, nan, 0.0))):
        assert both(sp(), ap=bad) == (INV, INV)
    # the ends of the ranges: a single texel, and the largest map's dimensions (one row, one column)
    ctxs[0].sync()
    torch.cuda.synchronize()
    wide = torch.ones((1, 8192), dtype=torch.float16, device="cuda")
    tall = torch.ones((8192, 1), dtype=torch.float16, device="cuda")
    plain = ctxs[0].render_aerial_perspective((0.6, 0.8, 0.0), 4, 4, 8, 32.0, 2)
    for t in (wide, tall):
        got = ctxs[0].render_aerial_perspective_shadowed((0.6, 0.8, 0.0), t, (0.0, 0.0), (1.0e5, 1.0e5), 4, 4, 8, 32.0, 2)
        ctxs[0].sync()
        assert (bits(got.cpu().numpy()) == bits(plain)).all()
    # the Python mirror's own checks
    with pytest.raises(ValueError):
        ctxs[0].render_aerial_perspective_shadowed((0.6, 0.8, 0.0), M.astype(np.float32), M_CENTER, M_EXTENT, 4, 4, 8)
    with pytest.raises(ValueError):
        ctxs[0].render_aerial_perspective_shadowed((0.6, 0.8, 0.0), M, M_CENTER, M_EXTENT, 4, 4, 8, out=np.zeros((8, 4, 4, 3), np.float16))


# ---------------------------------------------------------------------------------------------------------------- G6. end to end
def test_cloud_sky_light_shafts(pkg, noise):
    """CloudSky.aerial_perspective(cloud_shadows=True): the shadow map and the volume back to back on the march stream equal the host form fed
    the same map and the helper's rectangle; against the plain volume the rgb changes and alpha does not."""
    import torch
    sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=True)
    try:
        sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
        sky.update_sky()
        sun = np.asarray(sky.frame_data.LIGHT_DIRECTION, np.float32)
        v = sky.aerial_perspective(cloud_shadows=True, shadow_size=64)
        assert isinstance(v, torch.Tensor) and v.dtype == torch.float16 and v.is_cuda and tuple(v.shape) == (32, 32, 32, 4)
        v = v.cpu().numpy()
        center, extent = pkg.aerial_shadow_rect(sun, 32.0)
        shadow = sky.cloud_shadow_map(64, extent, center).cpu().numpy()
        assert shadow.shape == (64, 64) and (shadow.astype(np.float32) < 0.9).mean() >= 0.02 and (bits(shadow) == 0x3C00).mean() >= 0.02   # clouds, and gaps
        host = sky.ctx.render_aerial_perspective_shadowed(sun, shadow, center, extent)
        assert (bits(v) == bits(host)).all()
        plain = sky.aerial_perspective().cpu().numpy()
        assert (bits(plain) == bits(sky.aerial_perspective(cloud_shadows=False).cpu().numpy())).all()
        assert (bits(v[..., :3]) != bits(plain[..., :3])).any()
        assert (bits(v[..., 3]) == bits(plain[..., 3])).all()
        assert (v[..., :3].astype(np.float32).sum() < plain[..., :3].astype(np.float32).sum())       # shadows remove light
        r = sky.aerial_perspective(13, 7, 5, far_km=40.0, steps_per_slice=3, view=(AR.camera_basis(30.0, -30.0), 70.0), cloud_shadows=True, shadow_size=(48, 32)).cpu().numpy()
        c2, e2 = pkg.aerial_shadow_rect(sun, 40.0)
        s2 = sky.cloud_shadow_map((48, 32), e2, c2).cpu().numpy()
        assert (bits(r) == bits(sky.ctx.render_aerial_perspective_shadowed(sun, s2, c2, e2, 13, 7, 5, 40.0, 3, (AR.camera_basis(30.0, -30.0), 70.0)))).all()
        # a sun about 1 degree up: the helper's rectangle reaches 260 km out, where the map has chord texels (cloudsky.h); nothing is NaN
        sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.012, 0.3))
        sky.update_sky()
        low = np.asarray(sky.frame_data.LIGHT_DIRECTION, np.float32)
        assert 0.5 < np.degrees(np.arcsin(low[1] / np.linalg.norm(low))) < 1.5
        lv = sky.aerial_perspective(cloud_shadows=True, shadow_size=64).cpu().numpy()
        assert np.isfinite(lv.astype(np.float32)).all()
        c3, e3 = pkg.aerial_shadow_rect(low, 32.0)
        s3 = sky.cloud_shadow_map(64, e3, c3).cpu().numpy()
        assert np.isfinite(s3.astype(np.float32)).all()
        assert (bits(lv) == bits(sky.ctx.render_aerial_perspective_shadowed(low, s3, c3, e3))).all()
        assert (bits(lv[..., 3]) == bits(sky.aerial_perspective().cpu().numpy()[..., 3])).all()
        # a sun under the horizon: the plain volume
        sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, -0.05, 0.3))
        sky.update_sky()
        assert sky.frame_data.LIGHT_DIRECTION[1] < 0
        night = sky.aerial_perspective(cloud_shadows=True, shadow_size=64).cpu().numpy()
        assert (bits(night) == bits(sky.aerial_perspective().cpu().numpy())).all()
    finally:
        sky.close()
    host_sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=False)
    try:
        host_sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
        host_sky.update_sky()
        hv = host_sky.aerial_perspective(cloud_shadows=True, shadow_size=64)
        assert isinstance(hv, np.ndarray) and (bits(hv) == bits(v)).all()
    finally:
        host_sky.close()
