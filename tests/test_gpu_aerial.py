"""The aerial-perspective volume on the GPU (csky_render_aerial_perspective / _device; csrc/aerial.hip) through the C ABI: against the host-compiled
core (tests/aerial_host: the definition the kernel must equal) and the numpy restatement of the contract (tests/aerial_reference.py) at the sky-LUT
gate, every half within 1 fp16 ulp; then the chunk boundaries of the kernel, what a launch may touch, what state it needs and leaves, every error
path, and the Python mirror.  The host core and the restatement are given the GPU's own transmittance table: the volume kernel alone is compared."""
import ctypes as C

import numpy as np
import pytest

import aerial_reference as AR
from test_aerial_host import CASES, SUNS, aerial_host, case_view, host_volume  # noqa: F401  (aerial_host: the module-scoped fixture)

pytestmark = pytest.mark.gpu
GUARD = 64                          # halfs of guard before and after the volume (a multiple of 4: texels are stored whole)


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


def gpu_volume(ctx, W, H, D, S, far, sun, view=None, aspect=0.0):
    return ctx.render_aerial_perspective(sun, W, H, D, far, S, view, aspect)


# ---------------------------------------------------------------------------------------------------------------- 4. the cases of the host test
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_cases_match_host_core_and_restatement(ctxs, tables, aerial_host, case, mapping):  # noqa: F811
    W, H, D, S, far = CASES[case][:5]
    view, aspect = case_view(case)
    assert ctxs[mapping].sky_lut_launches() == 0
    for sun in SUNS:
        got = gpu_volume(ctxs[mapping], W, H, D, S, far, SUNS[sun], view, aspect)
        assert got.shape == (D, H, W, 4) and np.isfinite(got.astype(np.float32)).all()
        core, st = host_volume(aerial_host, mapping, tables[mapping], W, H, D, S, far, SUNS[sun], view, aspect, state=True)
        ref = AR.volume(W, H, D, S, far, SUNS[sun], tables[mapping], mapping, view, aspect)
        assert not ref["near"].any()
        a = ref["out"][D - 1][..., 3].astype(np.float32)
        assert a.max() - a.min() >= 0.2                            # a blank volume cannot pass
        what = "%s %s mapping %d" % (case, sun, mapping)
        d_core, _ = AR.gate(got, core, what=what + ", GPU vs host core")
        d_ref, _ = AR.gate(got, ref["out"], what=what + ", GPU vs restatement")
        print("%s: %d of %d halves differ from the host core, %d from the restatement" % (what, d_core, got.size, d_ref))
    assert ctxs[mapping].sky_lut_launches() == 0                    # no sky LUT was needed or made


# ---------------------------------------------------------------------------------------------------------------- 5. chunk boundaries
@pytest.mark.parametrize("DS", [(21, 3), (16, 4), (13, 5), (24, 3), (192, 1), (32, 16)], ids=["n63", "n64", "n65", "n72", "n192", "n512"])
def test_chunk_boundaries(ctxs, tables, aerial_host, DS):  # noqa: F811
    """9 x 5 columns of the down-looking camera (columns stop inside the reach: later chunks start beyond t_stop) with step counts on both sides
    of a chunk end; D = 192, S = 1 has 64 slice ends in every chunk."""
    D, S = DS
    view, aspect = case_view("down")
    got = gpu_volume(ctxs[0], 9, 5, D, S, 64.0, SUNS["deg45"], view, aspect)
    core = host_volume(aerial_host, 0, tables[0], 9, 5, D, S, 64.0, SUNS["deg45"], view, aspect)
    differ, _ = AR.gate(got, core, what="n = %d, GPU vs host core" % (D * S))
    print("n = %d: %d of %d halves differ from the host core" % (D * S, differ, got.size))
    a = got[..., 3].astype(np.float32)
    assert (np.diff(a, axis=0) <= 0).all() and a[-1].max() - a[-1].min() >= 0.2
    assert (bits(got)[-1] == bits(got)[D // 2]).all(-1).mean() >= 0.25      # columns that stopped in the first half: their later chunks evaluated nothing


def test_split_identity_on_the_device(ctxs):
    view, aspect = case_view("down")
    for m in (0, 1):
        fine = bits(gpu_volume(ctxs[m], 13, 7, 16, 2, 64.0, SUNS["deg45"], view, aspect))
        coarse = bits(gpu_volume(ctxs[m], 13, 7, 8, 4, 64.0, SUNS["deg45"], view, aspect))
        assert (coarse == fine[1::2]).all()
        long_f = bits(gpu_volume(ctxs[m], 9, 5, 64, 2, 64.0, SUNS["demo"], view, aspect))      # the same across a chunk end: n = 128
        long_c = bits(gpu_volume(ctxs[m], 9, 5, 32, 4, 64.0, SUNS["demo"], view, aspect))
        assert (long_c == long_f[1::2]).all()


# ---------------------------------------------------------------------------------------------------------------- 6. write coverage
@pytest.mark.parametrize("size", [(13, 7, 5), (1, 1, 1)], ids=["13x7x5", "1x1x1"])
def test_write_coverage(ctxs, size):
    """The device form into a buffer of 0xFFFF halfs (a NaN no volume contains) with guard regions before and after; on a caller's stream and on
    NULL (the context's own stream); the host form gives the same bytes."""
    import torch
    W, H, D = size
    ctx = ctxs[0]
    view, aspect = case_view("up")
    n = D * H * W * 4
    host = ctx.render_aerial_perspective(SUNS["demo"], W, H, D, 40.0, 3, view, aspect)
    assert not (bits(host) == 0xFFFF).any()
    s = torch.cuda.Stream()
    for run in range(3):
        stream = s if run != 1 else None                            # the second launch goes to the NULL stream
        t = torch.empty(n + 2 * GUARD, dtype=torch.int16, device="cuda")
        t.fill_(-1)
        torch.cuda.synchronize()
        share = t[GUARD:GUARD + n].view(D, H, W, 4)
        out = ctx.render_aerial_perspective(SUNS["demo"], W, H, D, 40.0, 3, view, aspect, out=share, stream=stream.cuda_stream if stream else None)
        assert out is share
        if stream:
            stream.synchronize()
        else:
            ctx.sync()
        got = t.cpu().numpy().view(np.uint16)
        assert not (got[GUARD:GUARD + n] == 0xFFFF).any(), run
        assert (got[:GUARD] == 0xFFFF).all() and (got[GUARD + n:] == 0xFFFF).all(), run
        assert (got[GUARD:GUARD + n] == bits(host).reshape(-1)).all(), run


# ---------------------------------------------------------------------------------------------------------------- 7. state and isolation
def test_state_and_isolation(pkg, gpu_ctx, ctxs, oracle):
    lib = pkg._lib
    bare = pkg.Context(0)
    try:
        with pytest.raises(pkg.CloudSkyError) as e:                 # no table
            bare.render_aerial_perspective(SUNS["demo"], 4, 4, 2)
        assert e.value.code == lib.ERR_STATE
        # a table, no noise, no sky LUT: renders, and what it renders is what the session's context (noise, LUTs, frames) renders
        bare.render_transmittance(256, 64)
        v0 = bare.render_aerial_perspective(SUNS["demo"], 13, 7, 5, 40.0, 3)
        assert bare.sky_lut_launches() == 0
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.read_sky_lut()
        assert e.value.code == lib.ERR_STATE
        # the mapping 0 -> 1 -> 0: the table goes with each switch (CSKY_ERR_STATE until it is rendered again), the mapping-0 bytes come back
        bare.set_transmittance_mapping(1)
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.render_aerial_perspective(SUNS["demo"], 13, 7, 5, 40.0, 3)
        assert e.value.code == lib.ERR_STATE
        bare.render_transmittance(256, 64)
        v1 = bare.render_aerial_perspective(SUNS["demo"], 13, 7, 5, 40.0, 3)
        assert (bits(v1) == bits(ctxs[1].render_aerial_perspective(SUNS["demo"], 13, 7, 5, 40.0, 3))).all() and (bits(v1) != bits(v0)).any()
        bare.set_transmittance_mapping(0)
        bare.render_transmittance(256, 64)
        assert (bits(bare.render_aerial_perspective(SUNS["demo"], 13, 7, 5, 40.0, 3)) == bits(v0)).all()
    finally:
        bare.close()
    gpu_ctx.render_transmittance(256, 64)
    gpu_ctx.render_sky_lut(SUNS["deg45"], 200, 100)
    pc = oracle.default_params(160, 80, (1, 1, 0))
    frame, lut, launches = gpu_ctx.render_clouds(pc, 160, 80), gpu_ctx.read_sky_lut(), gpu_ctx.sky_lut_launches()
    assert bits(frame).any()
    v = gpu_ctx.render_aerial_perspective(SUNS["demo"], 13, 7, 5, 40.0, 3)
    assert (bits(v) == bits(v0)).all()
    assert gpu_ctx.sky_lut_launches() == launches
    assert (bits(gpu_ctx.read_sky_lut()) == bits(lut)).all()
    assert (bits(gpu_ctx.render_clouds(pc, 160, 80)) == bits(frame)).all()
    assert gpu_ctx.sky_lut_launches() == launches


# ---------------------------------------------------------------------------------------------------------------- 8. error paths
def test_error_paths(pkg, ctxs):
    import torch
    L, lib = pkg.lib(), pkg._lib
    h = ctxs[0]._h
    INV, nan, inf = lib.ERR_INVALID, float("nan"), float("inf")
    out = np.zeros((8, 4, 4, 4), np.uint16)
    optr = out.ctypes.data_as(C.c_void_p)
    d = torch.zeros(8 * 4 * 4 * 4, dtype=torch.int16, device="cuda")
    dptr = C.c_void_p(d.data_ptr())
    basis = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]

    def ap(width=4, height=4, depth=8, steps=2, far=32.0, aspect=0.0, sun=(0.6, 0.8, 0.0)):
        return lib.AerialParams(width, height, depth, steps, far, aspect, (C.c_float * 3)(*sun))

    def vw(b=basis, fov=70.0):
        return lib.View((C.c_float * 9)(*b), fov)

    def both(p, v=None, ctx=h, o=True):
        pa, va = (C.byref(p) if p is not None else None), (C.byref(v) if v is not None else None)
        return (L.csky_render_aerial_perspective(ctx, pa, va, optr if o else None), L.csky_render_aerial_perspective_device(ctx, pa, va, dptr if o else None, None))

    assert both(ap()) == (lib.OK, lib.OK) and both(ap(), vw()) == (lib.OK, lib.OK)
    assert both(ap(0, 0, 0, 0, 0.0), o=False) == (INV, INV)
    # NULL pointers
    assert both(ap(), ctx=None) == (INV, INV) and both(None) == (INV, INV) and both(ap(), o=False) == (INV, INV)
    # sizes
    for bad in (ap(width=-1), ap(width=513), ap(height=-1), ap(height=513), ap(depth=-1), ap(depth=257), ap(steps=-1), ap(steps=17)):
        assert both(bad) == (INV, INV), (bad.width, bad.height, bad.depth, bad.steps_per_slice)
    # far_km
    for far in (-1.0, 2000.5, nan, inf, -inf):
        assert both(ap(far=far)) == (INV, INV), far
    assert b"far_km" in L.csky_last_error(h)
    # the sun
    for k in range(3):
        for v in (nan, inf):
            s = [0.6, 0.8, 0.0]
            s[k] = v
            assert both(ap(sun=s)) == (INV, INV) and both(ap(sun=s), vw()) == (INV, INV), (k, v)
    # the view: basis, fov, aspect
    for k in range(9):
        b = list(basis)
        b[k] = nan
        assert both(ap(), vw(b=b)) == (INV, INV), k
        b[k] = -inf
        assert both(ap(), vw(b=b)) == (INV, INV), k
    for fov in (0.0, -10.0, 180.0, 200.0, nan, inf):
        assert both(ap(), vw(fov=fov)) == (INV, INV), fov
    for aspect in (-1.0, nan, inf):
        assert both(ap(aspect=aspect), vw()) == (INV, INV), aspect
    assert both(ap(aspect=nan)) == (lib.OK, lib.OK)                 # without a view the aspect is not read
    # the ends of the ranges, and the defaults of zero fields
    small = lib.AerialParams(1, 1, 1, 1, 2000.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0))
    assert both(small, vw(fov=179.0)) == (lib.OK, lib.OK)
    ctxs[0].sync()
    torch.cuda.synchronize()
    dflt = np.zeros((32, 32, 32, 4), np.uint16)
    assert L.csky_render_aerial_perspective(h, C.byref(ap(0, 0, 0, 0, 0.0)), None, dflt.ctypes.data_as(C.c_void_p)) == lib.OK
    assert (dflt == bits(ctxs[0].render_aerial_perspective((0.6, 0.8, 0.0), 32, 32, 32, 32.0, 2))).all()
    with pytest.raises(ValueError):
        ctxs[0].render_aerial_perspective((0.6, 0.8, 0.0), 4, 4, 8, out=np.zeros((8, 4, 4, 3), np.float16))


# ---------------------------------------------------------------------------------------------------------------- 9. the Python mirror
def test_python_mirror(pkg, noise):
    """CloudSky.aerial_perspective is Context.render_aerial_perspective fed the sun update_sky() hands the sky LUT."""
    basis = AR.camera_basis(30.0, 10.0)
    for device_buffers in (False, True):
        sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=device_buffers)
        try:
            sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
            sky.update_sky()
            sun = np.asarray(sky.frame_data.LIGHT_DIRECTION, np.float32)
            v = sky.aerial_perspective()
            if device_buffers:
                import torch
                assert isinstance(v, torch.Tensor) and v.dtype == torch.float16 and v.is_cuda
                v = v.cpu().numpy()
            assert v.shape == (32, 32, 32, 4) and v.dtype == np.float16
            assert (bits(v) == bits(sky.ctx.render_aerial_perspective(sun, 32, 32, 32, 32.0, 2))).all()
            f = v.astype(np.float32)
            assert np.isfinite(f).all() and f[..., 3].max() <= 1.0 and f[..., 3].min() > 0.0 and len(np.unique(bits(v))) > 64
            r = sky.aerial_perspective(13, 7, 5, far_km=40.0, steps_per_slice=3, view=(basis, 70.0))
            r = r.cpu().numpy() if device_buffers else r
            assert r.shape == (5, 7, 13, 4)
            assert (bits(r) == bits(sky.ctx.render_aerial_perspective(sun, 13, 7, 5, 40.0, 3, (basis, 70.0)))).all()
            assert (bits(r) == bits(AR.volume(13, 7, 5, 3, 40.0, sun, sky.ctx.read_transmittance(), 0, (basis, 70.0))["out"])).mean() > 0.9
        finally:
            sky.close()
