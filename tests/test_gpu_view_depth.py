"""The depth frame and the aerial step for view frames and ray frames (csky_render_cloud_depth_dirs / _view, csky_apply_cloud_aerial_dirs / _view and
their _device forms; csrc/view_depth_core.h, depth.hip depth_rays_kernel, cloud_aerial.hip cloud_aerial_rays_kernel) on the GPU through the C ABI.
Fed the hemisphere grid's own directions the dirs forms must return the bytes of csky_render_cloud_depth and csky_apply_cloud_aerial; a camera view
is held to the host core of the same rays (tests/view_depth_host) with the gates of the hemisphere forms (tests/test_gpu_cloud_aerial.py).  Then what
a launch may touch, what state it needs and leaves, every error path, and the Python mirror.  No gate of its own: every one is "0 halves differ" or
one the hemisphere forms already apply."""
import ctypes as C

import numpy as np
import pytest

import cloud_depth_reference as CR
import clouds_rays_reference as RR
import shadow_reference as SR
from conftest import ulp_diff
from test_clouds_rays_host import grid, host_view_dirs, rays_host  # noqa: F401  (module-scoped fixtures)
from test_gpu_cloud_aerial import GUARD, bits, ctxs, depth_gate, fresh_ctx, tables  # noqa: F401
from test_gpu_clouds_rays import BASIS, MARCH, V, exact_ctx, view_frame, whole_ctx, with_lut  # noqa: F401
from test_view_depth_host import chains, vd_apply, vd_depth, vd_host  # noqa: F401

pytestmark = pytest.mark.gpu
W, H = CR.SIZE["width"], CR.SIZE["height"]
FOV, VW, VH = V["fov"], V["width"], V["height"]


def sun_of(p):
    return np.asarray(p[16:19], np.float32)


# ---------------------------------------------------------------------------------------------------------------- VG1
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("exact", [False, True], ids=["fp16-cells", "exact-cells"])
def test_grid_directions_give_the_bytes_of_the_hemisphere_forms(whole_ctx, exact_ctx, ctxs, rays_host, oracle, name, exact):  # noqa: F811
    import torch
    ctx = exact_ctx if exact else whole_ctx
    p = SR.scene(oracle, name)
    N, ls = MARCH[name]
    assert N == CR.STEPS[name]
    d, _ = grid(rays_host, W, H, N)
    ctx.set_march(N, ls)
    try:
        with_lut(ctx, p)
        frame = ctx.render_clouds(p, W, H).copy()                  # the cloud frame the depth frame belongs to
    finally:
        ctx.set_march(128, 6)
    ref = ctx.render_cloud_depth(p, W, H, N)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dd = torch.from_numpy(d).cuda()
        out = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
        s.synchronize()
        got = ctx.render_cloud_depth_dirs(p, dd, N, out=out, stream=s.cuda_stream)
        assert got is out
        got = out.cpu().numpy()
    differ = int((bits(got) != bits(ref)).sum())
    cloudy = float((frame[..., 3] > 0).mean())
    print("scene %s, %s: %d of %d halves differ from csky_render_cloud_depth; alpha > 0 in %.1f %% of the pixels" % (name, "exact" if exact else "fp16", differ, got.size,
                                                                                                           100.0 * cloudy))
    assert cloudy >= 0.40 and (ref[..., 3] > 0).mean() >= 0.40
    assert differ == 0
    assert (bits(ctx.render_cloud_depth_dirs(p, d, N)) == bits(ref)).all()          # the host form
    for mapping in (0, 1):
        want = ctxs[mapping].apply_cloud_aerial(sun_of(p), frame, ref, 16)
        with torch.cuda.stream(s):
            c, z = torch.from_numpy(frame).cuda(), torch.from_numpy(got).cuda()
            s.synchronize()
            res = ctxs[mapping].apply_cloud_aerial_dirs(sun_of(p), dd, c, z, 16, stream=s.cuda_stream).cpu().numpy()
        differ = int((bits(res) != bits(want)).sum())
        print("scene %s, mapping %d: %d of %d halves differ from csky_apply_cloud_aerial" % (name, mapping, differ, res.size))
        assert (bits(want) != bits(frame)).any(-1).mean() >= 0.40   # the air does something
        assert differ == 0
        assert (bits(ctxs[mapping].apply_cloud_aerial_dirs(sun_of(p), d, frame, ref, 16)) == bits(want)).all()   # the host form


# ---------------------------------------------------------------------------------------------------------------- VG2
def test_view_matches_the_host_core_and_the_dirs_form(whole_ctx, ctxs, tables, view_frame, vd_host, rays_host, chains):  # noqa: F811
    """The 64 x 36 view of the view tests (fov 70, pitched up 25 degrees, yawed 40), scene A.  On the CPU the host core's depth frame is not zero in
    57.4 % of its pixels and zero in 42.6 % (tests/test_view_depth_host.py prints both): depth_gate's two preconditions hold."""
    p, cv = view_frame
    core = vd_depth(vd_host, chains, p, VW, VH, 128, view=(BASIS, FOV))["out"]
    got = whole_ctx.render_cloud_depth_view(p, BASIS, FOV, VW, VH, 128)
    assert got.shape == (VH, VW, 4) and got.dtype == np.float16 and np.isfinite(got.astype(np.float32)).all()
    depth_gate(got, core, "GPU, view")
    assert (bits(whole_ctx.render_cloud_depth_view(p, BASIS, FOV, VW, VH)) == bits(got)).all()      # steps = 0: the context's 128
    d = host_view_dirs(rays_host, BASIS, FOV, VW, VH)
    assert (bits(whole_ctx.render_cloud_depth_dirs(p, d, 128)) == bits(got)).all()
    a = ulp_diff(got[..., 3], cv[..., 3])
    print("view depth alpha against the view frame's: %d of %d halves differ, worst %d fp16 ulp" % (int((a > 0).sum()), a.size, int(a.max())))
    assert a.max() <= 1
    worked = ~CR.passes(cv, got) & RR.accept(d)
    assert worked.mean() >= 0.40
    total = 0
    for mapping in (0, 1):
        for steps in (16, 5):
            want, n = vd_apply(vd_host, mapping, tables[mapping], cv, got, sun_of(p), steps, view=(BASIS, FOV))
            assert n == int(worked.sum())
            res = ctxs[mapping].apply_cloud_aerial_view(sun_of(p), BASIS, FOV, cv, got, steps)
            moved = (ulp_diff(want[..., :3], cv[..., :3])[worked] > 8).mean()
            differ = int((bits(res) != bits(want)).sum())
            total += differ
            print("apply view n = %d, mapping %d: %d of %d halves differ from the host core; %.1f %% of the worked rgb halves move by more than 8 ulp"
                  % (steps, mapping, differ, res.size, 100.0 * moved))
            assert moved >= 0.50                                  # a copy cannot pass
            assert (bits(res)[..., 3] == bits(cv)[..., 3]).all() and (bits(res)[~worked] == bits(cv)[~worked]).all()
            assert (bits(ctxs[mapping].apply_cloud_aerial_dirs(sun_of(p), d, cv, got, steps)) == bits(res)).all()
    assert total == 0
    assert ctxs[0].sky_lut_launches() == 0 and ctxs[1].sky_lut_launches() == 0


# ---------------------------------------------------------------------------------------------------------------- VG3
@pytest.mark.parametrize("size", [(37, 21, 0), (37, 21, 24), (1, 1, 0), (1, 1, 24)], ids=["37x21", "37x21-pitched", "1x1", "1x1-pitched"])
@pytest.mark.parametrize("form", ["view", "dirs"])
def test_depth_write_coverage(whole_ctx, view_frame, rays_host, size, form):  # noqa: F811
    """The device forms into a tensor of 0xFFFF halfs (a NaN no frame contains) with guard rows and row padding."""
    import torch
    w, h, pad = size
    p, _ = view_frame
    d = host_view_dirs(rays_host, BASIS, FOV, w, h)
    host = whole_ctx.render_cloud_depth_view(p, BASIS, FOV, w, h, 17) if form == "view" else whole_ctx.render_cloud_depth_dirs(p, d, 17)
    assert not (bits(host) == 0xFFFF).any()
    if w > 1:
        assert len(np.unique(bits(host))) > 8
    else:
        assert d[0, 0, 1] > 0                                      # the single ray looks up
    pitch_h = (8 * w + pad) // 2
    s = torch.cuda.Stream()
    for stream in (s.cuda_stream, None):
        with torch.cuda.stream(s):
            t = torch.empty((h + 2 * GUARD, pitch_h), dtype=torch.int16, device="cuda")
            t.fill_(-1)
            dd = torch.from_numpy(d).cuda()
            s.synchronize()                                      # the NULL form runs on the context's own stream
            share = t[GUARD:GUARD + h, :4 * w].unflatten(1, (w, 4))
            assert share.stride(0) * 2 == 8 * w + pad or h == 1
            if form == "view":
                out = whole_ctx.render_cloud_depth_view(p, BASIS, FOV, w, h, 17, out=share, stream=stream)
            else:
                out = whole_ctx.render_cloud_depth_dirs(p, dd, 17, out=share, stream=stream)
            assert out is share
            if stream is None:
                whole_ctx.sync()
            got = t.cpu().numpy().view(np.uint16)
        inside = np.zeros(got.shape, bool)
        inside[GUARD:GUARD + h, :4 * w] = True
        assert not (got[inside] == 0xFFFF).any()
        assert (got[~inside] == 0xFFFF).all(), np.argwhere(~inside & (got != 0xFFFF))[:4]
        assert (got[GUARD:GUARD + h, :4 * w].reshape(h, w, 4) == bits(host)).all()


@pytest.mark.parametrize("size", [(37, 21), (1, 1)], ids=["37x21", "1x1"])
@pytest.mark.parametrize("form", ["view", "dirs"])
def test_apply_write_coverage(whole_ctx, ctxs, view_frame, rays_host, size, form):  # noqa: F811
    """Out of place and in place, on the caller's stream and on the context's own: the W x H texels and nothing else."""
    import torch
    w, h = size
    p, _ = view_frame
    d = host_view_dirs(rays_host, BASIS, FOV, w, h)
    cloud = whole_ctx.render_clouds_view(p, BASIS, FOV, w, h).copy()
    z = whole_ctx.render_cloud_depth_view(p, BASIS, FOV, w, h).copy()
    sun = sun_of(p)

    def call(c, zz, **kw):
        if form == "view":
            return ctxs[0].apply_cloud_aerial_view(sun, BASIS, FOV, c, zz, 5, **kw)
        return ctxs[0].apply_cloud_aerial_dirs(sun, kw.pop("dirs", d), c, zz, 5, **kw)
    host = call(cloud, z)
    assert not (bits(host) == 0xFFFF).any() and (bits(host)[..., 3] == bits(cloud)[..., 3]).all()
    if w > 1:
        assert (bits(host) != bits(cloud)).any(-1).mean() >= 0.2
    else:
        assert (bits(host) != bits(cloud)).any() or bits(cloud)[0, 0, 3] == 0
    s = torch.cuda.Stream()
    for stream in (s.cuda_stream, None):
        for in_place in (False, True):
            with torch.cuda.stream(s):
                t = torch.empty((h + 2 * GUARD, w, 4), dtype=torch.int16, device="cuda")
                t.fill_(-1)
                c = torch.from_numpy(bits(cloud).view(np.int16).copy()).cuda()
                dz = torch.from_numpy(bits(z).view(np.int16).copy()).cuda()
                dd = torch.from_numpy(d).cuda()
                share = t[GUARD:GUARD + h]
                if in_place:
                    share.copy_(c)
                s.synchronize()
                kw = dict(out=share, stream=stream)
                if form == "dirs":
                    kw["dirs"] = dd
                out = call(share if in_place else c, dz, **kw)
                assert out is share
                if stream is None:
                    ctxs[0].sync()
                got = t.cpu().numpy().view(np.uint16)
                assert (c.cpu().numpy().view(np.uint16) == bits(cloud)).all() and (dz.cpu().numpy().view(np.uint16) == bits(z)).all()
                assert (dd.cpu().numpy().view(np.uint32) == d.view(np.uint32)).all()
            assert (got[:GUARD] == 0xFFFF).all() and (got[GUARD + h:] == 0xFFFF).all()
            assert (got[GUARD:GUARD + h] == bits(host)).all(), (stream, in_place)


# ---------------------------------------------------------------------------------------------------------------- VG4
def test_cloud_frames_and_luts_are_what_they_were(pkg, noise, oracle, fresh_ctx):  # noqa: F811
    """Two frames in flight on two streams: three cloud frames with a depth-view and an aerial-view call before, between and after them are the
    frames without; so are the sky LUT, the transmittance table and a view frame."""
    import torch
    ctx = pkg.Context(0)
    try:
        ctx.set_noise(*noise)
        ctx.set_frames_in_flight(2)
        pa = SR.scene(oracle, "A")
        with_lut(ctx, pa)
        lut, tr = ctx.read_sky_lut().copy(), ctx.read_transmittance().copy()
        blocks = []
        for k in range(3):
            q = oracle.default_params(128, 64, (1, 1, 0))
            q[4:6] = (0.5 * k, -0.25 * k)
            q[23] = 3.0 * k
            blocks.append(q)
        pb = SR.scene(oracle, "B")
        view_before = ctx.render_clouds_view(pb, BASIS, FOV, VW, VH).copy()
        cv = torch.from_numpy(view_before).cuda()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]

        def run(with_calls):
            frames = [torch.zeros((64, 128, 4), dtype=torch.float16, device="cuda") for _ in blocks]
            n = len(blocks) + 1 if with_calls else 0
            depths = [torch.zeros((VH, VW, 4), dtype=torch.float16, device="cuda") for _ in range(n)]
            aired = [torch.zeros((VH, VW, 4), dtype=torch.float16, device="cuda") for _ in range(n)]
            torch.cuda.synchronize()

            def calls(k, stream):
                ctx.render_cloud_depth_view(pb, BASIS, FOV, VW, VH, out=depths[k], stream=stream)
                ctx.apply_cloud_aerial_view(sun_of(pb), BASIS, FOV, cv, depths[k], 16, out=aired[k], stream=stream)
            for k, q in enumerate(blocks):
                s = streams[k % 2]
                if with_calls:                                   # on the stream of the frame still in flight, beside the one about to start
                    calls(k, streams[(k + 1) % 2].cuda_stream)
                ctx.render_clouds_device(q, 128, (8, 0, 1, 8), frames[k].data_ptr(), 128 * 8, s.cuda_stream)
            if with_calls:
                calls(len(blocks), streams[1].cuda_stream)
            torch.cuda.synchronize()
            return [f.cpu().numpy() for f in frames], [x.cpu().numpy() for x in depths], [x.cpu().numpy() for x in aired]
        plain, _, _ = run(False)
        mixed, depths, aired = run(True)
        again, _, _ = run(False)
        for a, b, c in zip(plain, mixed, again):
            assert bits(a).any() and (bits(a) == bits(b)).all() and (bits(a) == bits(c)).all()
        assert len(depths) == 4 and all((bits(x) == bits(depths[0])).all() for x in depths) and (depths[0][..., 3] > 0).any()
        assert all((bits(x) == bits(aired[0])).all() for x in aired) and (bits(aired[0]) != bits(view_before)).any()
        assert (bits(depths[0]) == bits(ctx.render_cloud_depth_view(pb, BASIS, FOV, VW, VH))).all()
        assert (bits(aired[0]) == bits(ctx.apply_cloud_aerial_view(sun_of(pb), BASIS, FOV, view_before, depths[0], 16))).all()
        assert (bits(ctx.render_clouds_view(pb, BASIS, FOV, VW, VH)) == bits(view_before)).all() and bits(view_before).any()
        assert (bits(ctx.read_sky_lut()) == bits(lut)).all() and (bits(ctx.read_transmittance()) == bits(tr)).all()
        # no LUT is needed and none is rendered: a context that never had one
        n0 = fresh_ctx.sky_lut_launches()
        assert n0 == 0
        f = fresh_ctx.render_cloud_depth_view(pb, BASIS, FOV, VW, VH)
        assert fresh_ctx.sky_lut_launches() == 0 and (bits(f) == bits(depths[0])).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- VG5
def test_error_paths(pkg, whole_ctx, ctxs, view_frame, noise):  # noqa: F811
    """Every CSKY_ERR_INVALID and CSKY_ERR_STATE case of the header, by return code."""
    import torch
    L, lib = pkg.lib(), pkg._lib
    h = whole_ctx._h
    INV, STATE, OK = lib.ERR_INVALID, lib.ERR_STATE, lib.OK
    nan, inf = float("nan"), float("inf")
    p = lib.cloud_params(view_frame[0])
    out = np.zeros((16, 16, 4), np.uint16)
    optr = out.ctypes.data_as(C.c_void_p)
    dirs = np.zeros((16, 16, 3), np.float32)
    dirs[..., 1] = 1.0
    hd = dirs.ctypes.data_as(C.c_void_p)
    d = torch.zeros((16, 32, 4), dtype=torch.int16, device="cuda")
    dptr = C.c_void_p(d.data_ptr())
    dd = torch.from_numpy(dirs).cuda()
    ddp = C.c_void_p(dd.data_ptr())

    def view(basis=RR.column_major(BASIS), fov=70.0):
        return lib.View((C.c_float * 9)(*[float(x) for x in basis]), fov)

    def ref(x):
        return C.byref(x) if x is not None else None

    def vhost(ctx=h, params=p, v=None, w=16, hh=16, n=8, o=optr):
        return L.csky_render_cloud_depth_view(ctx, ref(params), ref(v), w, hh, n, o)

    def vdev(ctx=h, params=p, v=None, w=16, hh=16, n=8, o=dptr, pitch=128):
        return L.csky_render_cloud_depth_view_device(ctx, ref(params), ref(v), w, hh, n, o, pitch, None)

    def dhost(ctx=h, params=p, w=16, hh=16, n=8, di=hd, o=optr):
        return L.csky_render_cloud_depth_dirs(ctx, ref(params), w, hh, n, di, o)

    def ddev(ctx=h, params=p, w=16, hh=16, n=8, di=ddp, o=dptr, pitch=128):
        return L.csky_render_cloud_depth_dirs_device(ctx, ref(params), w, hh, n, di, o, pitch, None)

    assert vhost(v=view()) == OK and vdev(v=view()) == OK and vdev(v=view(), pitch=136) == OK and dhost() == OK and ddev() == OK and ddev(pitch=256) == OK
    whole_ctx.sync()
    assert vhost(ctx=None, v=view()) == INV and vhost(params=None, v=view()) == INV and vhost(v=None) == INV and vhost(v=view(), o=None) == INV
    assert vdev(ctx=None, v=view()) == INV and vdev(params=None, v=view()) == INV and vdev(v=None) == INV and vdev(v=view(), o=None) == INV
    assert dhost(ctx=None) == INV and dhost(params=None) == INV and dhost(di=None) == INV and dhost(o=None) == INV
    assert ddev(ctx=None) == INV and ddev(params=None) == INV and ddev(di=None) == INV and ddev(o=None) == INV
    for w, hh in ((0, 16), (8193, 16), (16, 0), (16, 8193), (-1, 16), (16, -1)):
        assert vhost(v=view(), w=w, hh=hh) == INV and vdev(v=view(), w=w, hh=hh, pitch=8 * 8193) == INV and dhost(w=w, hh=hh) == INV and ddev(w=w, hh=hh, pitch=8 * 8193) == INV, (w, hh)
    for n in (-1, 1025):
        assert vhost(v=view(), n=n) == INV and vdev(v=view(), n=n) == INV and dhost(n=n) == INV and ddev(n=n) == INV, n
    for n in (0, 1, 1024):
        assert vhost(v=view(), n=n) == OK and dhost(n=n) == OK, n
    for pitch in (120, 132, 0):
        assert vdev(v=view(), pitch=pitch) == INV and ddev(pitch=pitch) == INV, pitch
    assert b"pitch" in L.csky_last_error(h)
    for k in (4, 5, 6, 7, 8, 9, 23, 25, 26):                      # every field of the block that is read
        for v in (nan, -inf):
            q = lib.cloud_params(view_frame[0])
            q.f[k] = v
            assert vhost(params=q, v=view()) == INV and vdev(params=q, v=view()) == INV and dhost(params=q) == INV and ddev(params=q) == INV, (k, v)
    q = lib.cloud_params(view_frame[0])                          # the fields that are not read may hold anything
    for k in (0, 1, 2, 3, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 24, 27):
        q.f[k] = nan
    assert vhost(params=q, v=view()) == OK and dhost(params=q) == OK
    for k in range(9):
        for bad in (nan, inf, -inf):
            b = RR.column_major(BASIS).copy()
            b[k] = bad
            assert vhost(v=view(basis=b)) == INV and vdev(v=view(basis=b)) == INV, (k, bad)
    for fov in (0.0, 180.0, -1.0, 200.0, nan, inf):
        assert vhost(v=view(fov=fov)) == INV and vdev(v=view(fov=fov)) == INV, fov
    bare = pkg.Context(0)
    try:
        b = bare._h
        assert vhost(ctx=b, v=view()) == STATE and vdev(ctx=b, v=view()) == STATE and dhost(ctx=b) == STATE and ddev(ctx=b) == STATE
        assert b"csky_set_noise" in L.csky_last_error(b)
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.render_cloud_depth_view(view_frame[0], BASIS, 70.0, 16, 16)
        assert e.value.code == STATE
        bare.set_noise(*noise)                                    # the noise is all the call needs: no LUT
        assert vhost(ctx=b, v=view()) == OK and dhost(ctx=b) == OK and bare.sky_lut_launches() == 0
    finally:
        bare.close()

    # ---- the apply calls
    a = ctxs[0]._h
    cloud, depth, res = np.zeros((16, 16, 4), np.uint16), np.zeros((16, 16, 4), np.uint16), np.zeros((16, 16, 4), np.uint16)
    cp, zp, rp = (x.ctypes.data_as(C.c_void_p) for x in (cloud, depth, res))
    dc, dz, dr = (torch.zeros((16, 16, 4), dtype=torch.int16, device="cuda") for _ in range(3))
    dcp, dzp, drp = (C.c_void_p(t.data_ptr()) for t in (dc, dz, dr))

    def ap(width=16, height=16, steps=4, sun=(0.6, 0.8, 0.0)):
        return lib.CloudAerialParams(width, height, steps, (C.c_float * 3)(*sun))

    def avhost(ctx=a, s=None, v=None, c=cp, z=zp, o=rp):
        return L.csky_apply_cloud_aerial_view(ctx, ref(s), ref(v), c, z, o)

    def avdev(ctx=a, s=None, v=None, c=dcp, z=dzp, o=drp):
        return L.csky_apply_cloud_aerial_view_device(ctx, ref(s), ref(v), c, z, o, None)

    def adhost(ctx=a, s=None, di=hd, c=cp, z=zp, o=rp):
        return L.csky_apply_cloud_aerial_dirs(ctx, ref(s), di, c, z, o)

    def addev(ctx=a, s=None, di=ddp, c=dcp, z=dzp, o=drp):
        return L.csky_apply_cloud_aerial_dirs_device(ctx, ref(s), di, c, z, o, None)

    forms = (lambda **kw: avhost(v=view(), **kw), lambda **kw: avdev(v=view(), **kw), adhost, addev)
    for f in forms:
        assert f(s=ap()) == OK and f(s=ap(steps=0)) == OK and f(s=ap(steps=1)) == OK and f(s=ap(steps=64)) == OK
    ctxs[0].sync()
    for f in forms:
        assert f(ctx=None, s=ap()) == INV and f(s=None) == INV and f(s=ap(), c=None) == INV and f(s=ap(), z=None) == INV and f(s=ap(), o=None) == INV
        for bad in (ap(width=0), ap(width=8193), ap(height=0), ap(height=8193), ap(height=-1), ap(steps=-1), ap(steps=65), ap(sun=(nan, 0.8, 0.0)),
                    ap(sun=(0.6, inf, 0.0)), ap(sun=(0.6, 0.8, -inf))):
            assert f(s=bad) == INV, (bad.width, bad.height, bad.steps, list(bad.sun_direction))
    assert avhost(s=ap(), v=None) == INV and avdev(s=ap(), v=None) == INV and adhost(s=ap(), di=None) == INV and addev(s=ap(), di=None) == INV
    for k in range(9):
        b = RR.column_major(BASIS).copy()
        b[k] = nan if k % 2 else inf
        assert avhost(s=ap(), v=view(basis=b)) == INV and avdev(s=ap(), v=view(basis=b)) == INV, k
    for fov in (0.0, 180.0, -1.0, 200.0, nan, inf):
        assert avhost(s=ap(), v=view(fov=fov)) == INV and avdev(s=ap(), v=view(fov=fov)) == INV, fov
    bare = pkg.Context(0)
    try:
        bare.set_noise(*noise)                                    # the noise is not what the call needs
        b = bare._h
        for f in forms:
            assert f(ctx=b, s=ap()) == STATE
        bare.render_transmittance(256, 64)
        for f in forms:
            assert f(ctx=b, s=ap()) == OK
        bare.set_transmittance_mapping(1)                         # the table goes with the switch
        for f in forms:
            assert f(ctx=b, s=ap()) == STATE
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.apply_cloud_aerial_view((0.6, 0.8, 0.0), BASIS, 70.0, cloud.view(np.float16), depth.view(np.float16))
        assert e.value.code == STATE
        bare.render_transmittance(256, 64)
        for f in forms:
            assert f(ctx=b, s=ap()) == OK
        bare.sync()
    finally:
        bare.close()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- VG6
def test_python_mirror(pkg, noise):
    """CloudSky.cloud_view_depth, cloud_view(aerial=True) and sky_view(direct=True, aerial=True) are the C calls fed the same frames; aerial=False is
    what it was."""
    import torch

    def host(t):
        return t.cpu().numpy() if hasattr(t, "cpu") else t
    for device_buffers in (True, False):
        sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=device_buffers)
        try:
            sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
            sky.update_sky()
            pc, light = sky._fill_push_constant(), sky.frame_data.LIGHT_DIRECTION
            cv_c = sky.ctx.render_clouds_view(pc, BASIS, FOV, VW, VH)
            z_c = sky.ctx.render_cloud_depth_view(pc, BASIS, FOV, VW, VH)
            air_c = sky.ctx.apply_cloud_aerial_view(light, BASIS, FOV, cv_c, z_c, 16)
            z = sky.cloud_view_depth(BASIS, FOV, VW, VH)
            air = sky.cloud_view(BASIS, FOV, VW, VH, aerial=True)
            assert isinstance(z, torch.Tensor) == device_buffers and isinstance(air, torch.Tensor) == device_buffers
            if device_buffers:
                assert all(t.dtype == torch.float16 and t.is_cuda for t in (z, air))
            z, air = host(z), host(air)
            assert z.shape == (VH, VW, 4) and z.dtype == np.float16 and air.shape == (VH, VW, 4) and air.dtype == np.float16
            assert (bits(z) == bits(z_c)).all() and (bits(air) == bits(air_c)).all()
            assert (bits(air)[..., 3] == bits(cv_c)[..., 3]).all()
            d = ulp_diff(z[..., 3], cv_c[..., 3])
            print("device_buffers=%s: depth alpha vs the view frame's: %d of %d halves differ, worst %d ulp" % (device_buffers, int((d > 0).sum()), d.size, int(d.max())))
            assert d.max() <= 1 and (cv_c[..., 3] > 0).mean() >= 0.1
            assert (ulp_diff(air[..., :3], cv_c[..., :3])[cv_c[..., 3] > 0] > 8).mean() >= 0.5
            five = host(sky.cloud_view(BASIS, FOV, VW, VH, aerial=True, aerial_steps=5))
            assert (bits(five) == bits(sky.ctx.apply_cloud_aerial_view(light, BASIS, FOV, cv_c, z_c, 5))).all() and (bits(five) != bits(air)).any()
            # aerial=False: the existing bytes
            assert (bits(host(sky.cloud_view(BASIS, FOV, VW, VH))) == bits(cv_c)).all()
            assert (bits(host(sky.cloud_view(BASIS, FOV, VW, VH, aerial=False))) == bits(cv_c)).all()
            sf, st = (host(t) for t in sky.sky_lut.back_texture)
            plain = sky.ctx.composite_view_frames(cv_c, cv_c, sf, st, light, BASIS, FOV, sky.blend_amount, sky.sun_disk_scale)
            assert (bits(sky.sky_view(BASIS, FOV, VW, VH, direct=True)) == bits(plain)).all()
            assert (bits(sky.sky_view(BASIS, FOV, VW, VH, direct=True, aerial=False)) == bits(plain)).all()
            want = sky.ctx.composite_view_frames(air_c, air_c, sf, st, light, BASIS, FOV, sky.blend_amount, sky.sun_disk_scale)
            got = sky.sky_view(BASIS, FOV, VW, VH, direct=True, aerial=True)
            assert (bits(got) == bits(want)).all() and (bits(got) != bits(plain)).any()
            bf, bt = host(sky.textures[sky.texture_to_blend_from]), host(sky.textures[sky.texture_to_blend_to])
            today = sky.ctx.composite_view(bf, bt, sf, st, light, BASIS, FOV, sky.blend_amount, sky.sun_disk_scale, VW, VH)
            assert (bits(sky.sky_view(BASIS, FOV, VW, VH)) == bits(today)).all()
            with pytest.raises(ValueError):
                sky.sky_view(BASIS, FOV, VW, VH, direct=False, aerial=True)
            with pytest.raises(ValueError):
                sky.sky_view(BASIS, FOV, VW, VH, aerial=True)
        finally:
            sky.close()
