"""The cloud depth frame (csky_render_cloud_depth / _device; csrc/depth.hip) and the aerial perspective on a cloud frame (csky_apply_cloud_aerial /
_device; csrc/cloud_aerial.hip) on the GPU through the C ABI, against their host-compiled cores (tests/cloud_aerial_host: the per-lane code the
kernels instantiate).  The depth frame: front and back bit-equal wherever both sides see the same in-cloud samples, the mean distance at the
project's gate for values rendered from the shipped assets (shadow_reference.GATE).  The apply step: the host core is given the GPU's own
transmittance table and must be met bit for bit.  Then what a launch may touch, what state it needs and leaves, every error path, and the Python
mirror."""
import ctypes as C

import numpy as np
import pytest

import cloud_depth_reference as CR
import shadow_reference as SR
from conftest import norm, ulp_diff
from test_aerial_host import SUNS
from test_cloud_aerial_host import DEPTHS, H, W, ca_host, chains, golden_cloud, host_apply, host_depth, synthetic_depth  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu
GUARD = 3                           # guard rows before and after an image


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


def depth_gate(got, core, what):
    """A GPU depth frame against the host core's: the gates of the host test, the in-cloud sample set judged by front and back."""
    o, r = bits(got), bits(core)
    hit = r.any(-1)
    same = (o[..., 1:3] == r[..., 1:3]).all(-1)
    differ = int((~same).sum())
    print("%s: front / back differ from the host core in %d of %d in-cloud pixels; %d of %d halves differ in all" % (what, differ, int(hit.sum()), int((o != r).sum()), o.size))
    assert hit.mean() >= 0.40 and (~hit).mean() >= 0.20 and differ <= 0.005 * hit.sum()
    assert not o[same & ~hit].any()
    a = core[..., 3].astype(np.float32)
    thick = same & hit & (a >= float(CR.THIN))
    SR.assert_gate(got[..., 0][thick], core[..., 0][thick], what + ", mean distance")
    SR.assert_gate(got[..., 3][same & hit], core[..., 3][same & hit], what + ", alpha")
    g = got.astype(np.float32)
    nz = o.any(-1)
    assert (g[nz][:, 1] <= g[nz][:, 0]).all() and (g[nz][:, 0] <= g[nz][:, 2]).all()


# ---------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("name", ["A", "B"])
def test_depth_scenes_match_host_core(gpu_ctx, fresh_ctx, exact_ctx, ca_host, chains, oracle, name):  # noqa: F811
    p = SR.scene(oracle, name)
    N = CR.STEPS[name]
    core = host_depth(ca_host, chains, p, W, H, N)["out"]
    got = gpu_ctx.render_cloud_depth(p, W, H, N)
    assert got.shape == (H, W, 4) and got.dtype == np.float16 and np.isfinite(got.astype(np.float32)).all()
    depth_gate(got, core, "GPU, scene " + name)
    assert fresh_ctx.sky_lut_launches() == 0                     # no LUT on this context
    f = fresh_ctx.render_cloud_depth(p, W, H, N)
    assert fresh_ctx.sky_lut_launches() == 0
    assert (bits(f) == bits(got)).all()
    depth_gate(exact_ctx.render_cloud_depth(p, W, H, N), core, "GPU, exact cells, scene " + name)
    if name == "A":                                              # steps = 0: the context's primary step count, 128 unless changed
        assert (bits(fresh_ctx.render_cloud_depth(p, W, H)) == bits(got)).all()
    q = np.array(p, np.float32)                                  # the fields that are not read may hold anything
    for k in (0, 1, 2, 3, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 24, 27):
        q[k] = np.nan
    assert (bits(gpu_ctx.render_cloud_depth(q, W, H, N)) == bits(got)).all()


# ---------------------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("steps", [1, 16, 17, 64])
def test_apply_is_the_host_core(ctxs, tables, ca_host, golden_cloud, steps, mapping):  # noqa: F811
    total = 0
    for depth, sun in (("ramp", "deg45"), (10.0, "demo"), (65.0, "degm2")):
        z = synthetic_depth(depth, golden_cloud)
        core = host_apply(ca_host, mapping, tables[mapping], golden_cloud, z, SUNS[sun], steps)
        got = ctxs[mapping].apply_cloud_aerial(SUNS[sun], golden_cloud, z, steps)
        worked = ~CR.passes(golden_cloud, z)
        assert worked.mean() >= 0.40 and (ulp_diff(core[..., :3], golden_cloud[..., :3])[worked] > 8).mean() >= 0.50
        differ = int((bits(got) != bits(core)).sum())
        total += differ
        print("apply n = %d, mapping %d, %s km, %s: %d of %d halves differ from the host core" % (steps, mapping, depth, sun, differ, got.size))
        assert (bits(got)[..., 3] == bits(golden_cloud)[..., 3]).all()
    assert total == 0
    assert ctxs[mapping].sky_lut_launches() == 0


# ---------------------------------------------------------------------------------------------------------------- G3
@pytest.mark.parametrize("size", [(37, 21, 0), (37, 21, 24), (1, 1, 0), (1, 1, 24)], ids=["37x21", "37x21-pitched", "1x1", "1x1-pitched"])
def test_depth_write_coverage(gpu_ctx, oracle, size):
    """The device form into a tensor of 0xFFFF halfs (a NaN no frame contains) with guard rows and row padding."""
    import torch
    w, h, pad = size
    p = SR.scene(oracle, "A")
    host = gpu_ctx.render_cloud_depth(p, w, h, 17)
    assert not (bits(host) == 0xFFFF).any()
    if w > 1:
        assert len(np.unique(bits(host))) > 8
    pitch_h = (8 * w + pad) // 2
    s = torch.cuda.Stream()
    for stream in (s.cuda_stream, None):
        with torch.cuda.stream(s):
            t = torch.empty((h + 2 * GUARD, pitch_h), dtype=torch.int16, device="cuda")
            t.fill_(-1)
            s.synchronize()                                      # the NULL form runs on the context's own stream
            share = t[GUARD:GUARD + h, :4 * w].unflatten(1, (w, 4))
            assert share.stride(0) * 2 == 8 * w + pad or h == 1
            out = gpu_ctx.render_cloud_depth(p, w, h, 17, out=share, stream=stream)
            assert out is share
            if stream is None:
                gpu_ctx.sync()
            got = t.cpu().numpy().view(np.uint16)
        inside = np.zeros(got.shape, bool)
        inside[GUARD:GUARD + h, :4 * w] = True
        assert not (got[inside] == 0xFFFF).any()
        assert (got[~inside] == 0xFFFF).all(), np.argwhere(~inside & (got != 0xFFFF))[:4]
        assert (got[GUARD:GUARD + h, :4 * w].reshape(h, w, 4) == bits(host)).all()


def test_apply_write_coverage(ctxs, oracle, gpu_ctx):
    """37 x 21, out of place and in place, on the caller's stream and on the context's own: the W x H texels and nothing else."""
    import torch
    w, h = 37, 21
    cloud = gpu_ctx.render_cloud_depth(SR.scene(oracle, "A"), w, h, 17)            # any image with clear and cloudy pixels: (km, km, km, alpha)
    z = cloud.copy()
    host = ctxs[0].apply_cloud_aerial(SUNS["deg45"], cloud, z, 5)
    assert not (bits(host) == 0xFFFF).any() and (bits(host) != bits(cloud)).mean() >= 0.2
    s = torch.cuda.Stream()
    for stream in (s.cuda_stream, None):
        for in_place in (False, True):
            with torch.cuda.stream(s):
                t = torch.empty((h + 2 * GUARD, w, 4), dtype=torch.int16, device="cuda")
                t.fill_(-1)
                c = torch.from_numpy(bits(cloud).view(np.int16).copy()).cuda()
                d = torch.from_numpy(bits(z).view(np.int16).copy()).cuda()
                share = t[GUARD:GUARD + h]
                if in_place:
                    share.copy_(c)
                s.synchronize()
                out = ctxs[0].apply_cloud_aerial(SUNS["deg45"], share if in_place else c, d, 5, out=share, stream=stream)
                assert out is share
                if stream is None:
                    ctxs[0].sync()
                got = t.cpu().numpy().view(np.uint16)
                assert (c.cpu().numpy().view(np.uint16) == bits(cloud)).all() and (d.cpu().numpy().view(np.uint16) == bits(z)).all()
            assert (got[:GUARD] == 0xFFFF).all() and (got[GUARD + h:] == 0xFFFF).all()
            assert (got[GUARD:GUARD + h] == bits(host)).all(), (stream, in_place)


# ---------------------------------------------------------------------------------------------------------------- G4
def test_isolation(gpu_ctx, oracle):
    """Both calls leave a cloud frame and the sky LUT as they were, and repeat themselves."""
    sun = norm((1, 1, 0))
    gpu_ctx.render_transmittance(256, 64)
    lut = gpu_ctx.render_sky_lut(sun, 200, 100).copy()
    pc = oracle.default_params(64, 32, (1, 1, 0))
    before = gpu_ctx.render_clouds(pc, 64, 32).copy()
    pb = SR.scene(oracle, "B")
    z = gpu_ctx.render_cloud_depth(pb, 64, 32, 30).copy()
    one = gpu_ctx.apply_cloud_aerial(sun, before, z, 16).copy()
    after = gpu_ctx.render_clouds(pc, 64, 32)
    assert (bits(before) == bits(after)).all() and bits(before).any()
    assert (bits(gpu_ctx.read_sky_lut()) == bits(lut)).all()
    assert (bits(gpu_ctx.render_cloud_depth(pb, 64, 32, 30)) == bits(z)).all()
    assert (bits(gpu_ctx.apply_cloud_aerial(sun, before, z, 16)) == bits(one)).all()
    assert (bits(one) != bits(before)).any() and (bits(one)[..., 3] == bits(before)[..., 3]).all()


def test_error_paths(pkg, gpu_ctx, ctxs, oracle, noise):
    """Every CSKY_ERR_INVALID and CSKY_ERR_STATE case of the header."""
    import torch
    L, lib = pkg.lib(), pkg._lib
    h = gpu_ctx._h
    INV, STATE, OK = lib.ERR_INVALID, lib.ERR_STATE, lib.OK
    nan, inf = float("nan"), float("inf")
    p = lib.cloud_params(SR.scene(oracle, "A"))
    out = np.zeros((16, 16, 4), np.uint16)
    optr = out.ctypes.data_as(C.c_void_p)
    d = torch.zeros((16, 32, 4), dtype=torch.int16, device="cuda")
    dptr = C.c_void_p(d.data_ptr())

    def dp(width=16, height=16, steps=8):
        return lib.DepthParams(width, height, steps)

    def ref(x):
        return C.byref(x) if x is not None else None

    def host(ctx=h, params=p, s=None, o=optr):
        return L.csky_render_cloud_depth(ctx, ref(params), ref(s), o)

    def dev(ctx=h, params=p, s=None, o=dptr, pitch=128):
        return L.csky_render_cloud_depth_device(ctx, ref(params), ref(s), o, pitch, None)

    assert host(s=dp()) == OK and dev(s=dp()) == OK and dev(s=dp(), pitch=136) == OK and dev(s=dp(), pitch=256) == OK
    gpu_ctx.sync()
    assert host(ctx=None, s=dp()) == INV and host(params=None, s=dp()) == INV and host(s=None) == INV and host(s=dp(), o=None) == INV
    assert dev(ctx=None, s=dp()) == INV and dev(params=None, s=dp()) == INV and dev(s=None) == INV and dev(s=dp(), o=None) == INV
    for bad in (dp(width=0), dp(width=8193), dp(height=0), dp(height=8193), dp(width=-1), dp(steps=-1), dp(steps=1025)):
        assert host(s=bad) == INV and dev(s=bad, pitch=8 * 8193) == INV, (bad.width, bad.height, bad.steps)
    assert host(s=dp(steps=0)) == OK and host(s=dp(steps=1)) == OK and host(s=dp(steps=1024)) == OK
    for k in (4, 5, 6, 7, 8, 9, 23, 25, 26):                      # every field of the block that is read
        for v in (nan, -inf):
            q = lib.cloud_params(SR.scene(oracle, "A"))
            q.f[k] = v
            assert host(params=q, s=dp()) == INV and dev(params=q, s=dp()) == INV, (k, v)
    assert dev(s=dp(), pitch=120) == INV and dev(s=dp(), pitch=132) == INV and dev(s=dp(), pitch=0) == INV
    assert b"pitch" in L.csky_last_error(h)
    bare = pkg.Context(0)
    try:
        assert host(ctx=bare._h, s=dp()) == STATE and dev(ctx=bare._h, s=dp()) == STATE
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.render_cloud_depth(SR.scene(oracle, "A"), 16, 16)
        assert e.value.code == STATE
    finally:
        bare.close()

    # ---- the apply call
    a = ctxs[0]._h
    cloud, depth, res = np.zeros((16, 16, 4), np.uint16), np.zeros((16, 16, 4), np.uint16), np.zeros((16, 16, 4), np.uint16)
    cp, zp, rp = (x.ctypes.data_as(C.c_void_p) for x in (cloud, depth, res))
    dc, dz, dr = (torch.zeros((16, 16, 4), dtype=torch.int16, device="cuda") for _ in range(3))
    dcp, dzp, drp = (C.c_void_p(t.data_ptr()) for t in (dc, dz, dr))

    def ap(width=16, height=16, steps=4, sun=(0.6, 0.8, 0.0)):
        return lib.CloudAerialParams(width, height, steps, (C.c_float * 3)(*sun))

    def ahost(ctx=a, s=None, c=cp, z=zp, o=rp):
        return L.csky_apply_cloud_aerial(ctx, ref(s), c, z, o)

    def adev(ctx=a, s=None, c=dcp, z=dzp, o=drp):
        return L.csky_apply_cloud_aerial_device(ctx, ref(s), c, z, o, None)

    assert ahost(s=ap()) == OK and adev(s=ap()) == OK and ahost(s=ap(steps=0)) == OK and ahost(s=ap(steps=1)) == OK and ahost(s=ap(steps=64)) == OK
    ctxs[0].sync()
    assert ahost(ctx=None, s=ap()) == INV and ahost(s=None) == INV and ahost(s=ap(), c=None) == INV and ahost(s=ap(), z=None) == INV and ahost(s=ap(), o=None) == INV
    assert adev(ctx=None, s=ap()) == INV and adev(s=None) == INV and adev(s=ap(), c=None) == INV and adev(s=ap(), z=None) == INV and adev(s=ap(), o=None) == INV
    for bad in (ap(width=0), ap(width=8193), ap(height=0), ap(height=8193), ap(height=-1), ap(steps=-1), ap(steps=65), ap(sun=(nan, 0.8, 0.0)), ap(sun=(0.6, inf, 0.0)),
                ap(sun=(0.6, 0.8, -inf))):
        assert ahost(s=bad) == INV and adev(s=bad) == INV, (bad.width, bad.height, bad.steps, list(bad.sun_direction))
    bare = pkg.Context(0)
    try:
        bare.set_noise(*noise)                                    # the noise is not what the call needs
        assert ahost(ctx=bare._h, s=ap()) == STATE and adev(ctx=bare._h, s=ap()) == STATE
        bare.render_transmittance(256, 64)
        assert ahost(ctx=bare._h, s=ap()) == OK
        bare.set_transmittance_mapping(1)                         # the table goes with the switch
        assert ahost(ctx=bare._h, s=ap()) == STATE and adev(ctx=bare._h, s=ap()) == STATE
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.apply_cloud_aerial((0.6, 0.8, 0.0), cloud.view(np.float16), depth.view(np.float16))
        assert e.value.code == STATE
        bare.render_transmittance(256, 64)
        assert ahost(ctx=bare._h, s=ap()) == OK
    finally:
        bare.close()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- G5
def test_python_mirror(pkg, noise):
    """CloudSky.aerial_clouds with the shipped assets: the host forms fed the read-back frame and depth frame; alpha untouched."""
    import torch
    for device_buffers in (True, False):
        sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=device_buffers)
        try:
            sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
            frame = sky.update_sky()
            z = sky.cloud_depth()
            out = sky.aerial_clouds()
            if device_buffers:
                assert all(isinstance(t, torch.Tensor) and t.dtype == torch.float16 and t.is_cuda for t in (z, out))
                frame, z, out = frame.cpu().numpy(), z.cpu().numpy(), out.cpu().numpy()
            assert z.shape == (64, 128, 4) and out.shape == (64, 128, 4) and out.dtype == np.float16
            zh = sky.ctx.render_cloud_depth(sky._fill_push_constant(), 128, 64)
            assert (bits(z) == bits(zh)).all()
            direct = sky.ctx.apply_cloud_aerial(sky.frame_data.LIGHT_DIRECTION, frame, zh, 16)
            assert (bits(out) == bits(direct)).all()
            assert (bits(out)[..., 3] == bits(frame)[..., 3]).all()
            d = ulp_diff(z[..., 3], frame[..., 3])
            print("device_buffers=%s: depth alpha vs the frame's: %d of %d halves differ, worst %d ulp" % (device_buffers, int((d > 0).sum()), d.size, int(d.max())))
            assert d.max() <= 1 and (frame[..., 3] > 0).mean() >= 0.3
            assert (ulp_diff(out[..., :3], frame[..., :3])[frame[..., 3] > 0] > 8).mean() >= 0.5
            given = sky.aerial_clouds(frame=sky.last_frame, steps=5)
            given = given.cpu().numpy() if device_buffers else given
            assert (bits(given) == bits(sky.ctx.apply_cloud_aerial(sky.frame_data.LIGHT_DIRECTION, frame, zh, 5))).all()
            other = sky.aerial_clouds(frame=frame if device_buffers else torch.from_numpy(frame.copy()).cuda(), steps=5)    # a frame of the other kind is moved
            assert isinstance(other, torch.Tensor) == device_buffers
            assert (bits(other.cpu().numpy() if device_buffers else other) == bits(given)).all()
            for bad in (frame.tolist(), frame.astype(np.float32), frame[:, :64]):
                with pytest.raises(ValueError):
                    sky.aerial_clouds(frame=bad)
        finally:
            sky.close()
