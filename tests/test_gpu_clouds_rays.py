"""The direct cloud march (csky_render_clouds_dirs / _view and their _device forms; csrc/rays_core.h, cloud_kernels.hip clouds_rays_kernel) and the
compositor over view frames (csky_composite_view_frames) on the GPU through the C ABI.  Fed the hemisphere grid's own directions the march must
return the bytes of csky_render_clouds (same Ray, same march_compact); a camera view is held to the host core's march of the same rays
(tests/rays_host) at the gate for frames rendered from the shipped assets (parity_metrics.cloud_tight).  Then what a launch may touch, what state it
needs and leaves, every error path, the switches, and the Python mirror."""
import ctypes as C

import numpy as np
import pytest

import clouds_rays_reference as RR
import shadow_reference as SR
from conftest import norm, ulp_diff
from parity_metrics import cloud_tight
from test_clouds_rays_host import chains, grid, host_composite, host_march, host_view_dirs, rays_host  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu
GUARD = 3                           # guard rows before and after an image
V = RR.VIEW
BASIS = RR.camera_basis(V["pitch"], V["yaw"])
MARCH = {"A": (128, 6), "B": (30, 4)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def with_lut(ctx, p):
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(np.asarray(p[16:19], np.float32), 200, 100)


@pytest.fixture(scope="module")
def whole_ctx(pkg, noise):
    """whole rays for every launch size (csky_set_segments(1)): the march the rays kernel runs"""
    if pkg.lib().csky_device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible (libcloudsky has no CPU fallback)")
    ctx = pkg.Context(0)
    ctx.set_noise(*noise)
    ctx.set_segments(1)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def exact_ctx(pkg, noise):
    """exact-cells mode: the march on TexSet32 (always whole rays)"""
    ctx = pkg.Context(0)
    ctx.set_exact_cells(1)
    ctx.set_noise(*noise)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def view_frame(whole_ctx, oracle):
    """scene A through the view tests' camera, host form: (params, float16 [H, W, 4])"""
    p = SR.scene(oracle, "A")
    whole_ctx.set_march(*MARCH["A"])
    with_lut(whole_ctx, p)
    return p, whole_ctx.render_clouds_view(p, BASIS, V["fov"], V["width"], V["height"]).copy()


# ---------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("exact", [False, True], ids=["fp16-cells", "exact-cells"])
def test_grid_directions_give_the_bytes_of_the_cloud_frame(whole_ctx, exact_ctx, rays_host, oracle, name, exact):  # noqa: F811
    import torch
    ctx = exact_ctx if exact else whole_ctx
    p = SR.scene(oracle, name)
    N, ls = MARCH[name]
    ctx.set_march(N, ls)
    try:
        with_lut(ctx, p)
        frame = ctx.render_clouds(p, 64, 32)
        d, _ = grid(rays_host, 64, 32, N)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dd = torch.from_numpy(d).cuda()
            out = torch.zeros((32, 64, 4), dtype=torch.float16, device="cuda")
            s.synchronize()
            got = ctx.render_clouds_dirs(p, dd, out=out, stream=s.cuda_stream)
            assert got is out
            got = out.cpu().numpy()
        differ = int((bits(got) != bits(frame)).sum())
        print("scene %s, %s: %d of %d halves differ from csky_render_clouds; alpha > 0 in %.1f %% of the pixels" % (name, "exact" if exact else "fp16", differ, got.size,
                                                                                                             100.0 * (frame[..., 3] > 0).mean()))
        assert (frame[..., 3] > 0).mean() >= 0.25
        assert differ == 0
        assert (bits(ctx.render_clouds_dirs(p, d)) == bits(frame)).all()      # the host form
    finally:
        ctx.set_march(128, 6)


# ---------------------------------------------------------------------------------------------------------------- G2
def test_view_matches_the_host_core_and_the_dirs_form(whole_ctx, view_frame, rays_host, chains):  # noqa: F811
    """The 64 x 36 view of the view tests (fov 70, pitched up 25 degrees, yawed 40), scene A.  On the CPU the host core gives alpha > 0 in 57.4 % of its
    pixels and 16.7 % of them lie under the horizon (the preconditions below: neither an empty nor a trivial frame passes)."""
    p, got = view_frame
    d = host_view_dirs(rays_host, BASIS, V["fov"], V["width"], V["height"])
    core, marched, _ = host_march(rays_host, chains, p, whole_ctx.read_sky_lut(), d)
    cloudy, under = float((core[..., 3] > 0).mean()), float((d[..., 1] <= 0).mean())
    ok, info = cloud_tight(got, core)
    print("view vs host core: alpha > 0 in %.1f %% of the pixels, %.1f %% under the horizon; %s" % (100 * cloudy, 100 * under, info))
    assert cloudy >= 0.25 and under >= 0.10
    assert ok, info
    assert not bits(got)[~marched].any()                        # under the horizon: zeros
    via_dirs = whole_ctx.render_clouds_dirs(p, d)
    assert (bits(via_dirs) == bits(got)).all()


# ---------------------------------------------------------------------------------------------------------------- G3
@pytest.mark.parametrize("size", [(37, 21, 0), (37, 21, 24), (1, 1, 0), (1, 1, 24)], ids=["37x21", "37x21-pitched", "1x1", "1x1-pitched"])
@pytest.mark.parametrize("form", ["view", "dirs"])
def test_write_coverage(whole_ctx, view_frame, rays_host, size, form):  # noqa: F811
    """The device forms into a tensor of 0xFFFF halfs (a NaN no frame contains) with guard rows and row padding."""
    import torch
    w, h, pad = size
    p, _ = view_frame
    d = host_view_dirs(rays_host, BASIS, V["fov"], w, h)
    host = whole_ctx.render_clouds_view(p, BASIS, V["fov"], w, h) if form == "view" else whole_ctx.render_clouds_dirs(p, d)
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
                out = whole_ctx.render_clouds_view(p, BASIS, V["fov"], w, h, out=share, stream=stream)
            else:
                out = whole_ctx.render_clouds_dirs(p, dd, out=share, stream=stream)
            assert out is share
            if stream is None:
                whole_ctx.sync()
            got = t.cpu().numpy().view(np.uint16)
        inside = np.zeros(got.shape, bool)
        inside[GUARD:GUARD + h, :4 * w] = True
        assert not (got[inside] == 0xFFFF).any()
        assert (got[~inside] == 0xFFFF).all(), np.argwhere(~inside & (got != 0xFFFF))[:4]
        assert (got[GUARD:GUARD + h, :4 * w].reshape(h, w, 4) == bits(host)).all()


# ---------------------------------------------------------------------------------------------------------------- G4
def test_cloud_frames_and_luts_are_what_they_were(pkg, noise, oracle):
    """Two frames in flight on two streams: three cloud frames with two rays calls before, between and after them are the frames without."""
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
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]

        def run(with_rays):
            frames = [torch.zeros((64, 128, 4), dtype=torch.float16, device="cuda") for _ in blocks]
            views = [torch.zeros((V["height"], V["width"], 4), dtype=torch.float16, device="cuda") for _ in range(2 if with_rays else 0)]
            torch.cuda.synchronize()
            for k, q in enumerate(blocks):
                s = streams[k % 2]
                if with_rays and k > 0:                          # on the stream of the frame still in flight, beside the one about to start
                    ctx.render_clouds_view(pb, BASIS, V["fov"], V["width"], V["height"], out=views[k - 1], stream=streams[(k + 1) % 2].cuda_stream)
                ctx.render_clouds_device(q, 128, (8, 0, 1, 8), frames[k].data_ptr(), 128 * 8, s.cuda_stream)
            torch.cuda.synchronize()
            return [f.cpu().numpy() for f in frames], [v.cpu().numpy() for v in views]
        plain, _ = run(False)
        mixed, views = run(True)
        again, _ = run(False)
        for a, b, c in zip(plain, mixed, again):
            assert bits(a).any() and (bits(a) == bits(b)).all() and (bits(a) == bits(c)).all()
        assert len(views) == 2 and (bits(views[0]) == bits(views[1])).all() and (views[0][..., 3] > 0).any()
        assert (bits(views[0]) == bits(ctx.render_clouds_view(pb, BASIS, V["fov"], V["width"], V["height"]))).all()
        assert (bits(ctx.read_sky_lut()) == bits(lut)).all() and (bits(ctx.read_transmittance()) == bits(tr)).all()
    finally:
        ctx.close()


def test_error_paths(pkg, whole_ctx, view_frame, noise):
    """Every CSKY_ERR_INVALID and CSKY_ERR_STATE case of the header."""
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

    def vhost(ctx=h, params=p, v=None, w=16, hh=16, o=optr):
        return L.csky_render_clouds_view(ctx, ref(params), ref(v), w, hh, o)

    def vdev(ctx=h, params=p, v=None, w=16, hh=16, o=dptr, pitch=128):
        return L.csky_render_clouds_view_device(ctx, ref(params), ref(v), w, hh, o, pitch, None)

    def dhost(ctx=h, params=p, w=16, hh=16, di=hd, o=optr):
        return L.csky_render_clouds_dirs(ctx, ref(params), w, hh, di, o)

    def ddev(ctx=h, params=p, w=16, hh=16, di=ddp, o=dptr, pitch=128):
        return L.csky_render_clouds_dirs_device(ctx, ref(params), w, hh, di, o, pitch, None)

    assert vhost(v=view()) == OK and vdev(v=view()) == OK and vdev(v=view(), pitch=136) == OK and dhost() == OK and ddev() == OK and ddev(pitch=256) == OK
    whole_ctx.sync()
    assert vhost(ctx=None, v=view()) == INV and vhost(params=None, v=view()) == INV and vhost(v=None) == INV and vhost(v=view(), o=None) == INV
    assert vdev(ctx=None, v=view()) == INV and vdev(params=None, v=view()) == INV and vdev(v=None) == INV and vdev(v=view(), o=None) == INV
    assert dhost(ctx=None) == INV and dhost(params=None) == INV and dhost(di=None) == INV and dhost(o=None) == INV
    assert ddev(ctx=None) == INV and ddev(params=None) == INV and ddev(di=None) == INV and ddev(o=None) == INV
    for w, hh in ((0, 16), (8193, 16), (16, 0), (16, 8193), (-1, 16), (16, -1)):
        assert vhost(v=view(), w=w, hh=hh) == INV and vdev(v=view(), w=w, hh=hh, pitch=8 * 8193) == INV and dhost(w=w, hh=hh) == INV and ddev(w=w, hh=hh, pitch=8 * 8193) == INV, (w, hh)
    for pitch in (120, 132, 0):
        assert vdev(v=view(), pitch=pitch) == INV and ddev(pitch=pitch) == INV, pitch
    assert b"pitch" in L.csky_last_error(h)
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
        bare.set_noise(*noise)
        assert vhost(ctx=b, v=view()) == STATE and vdev(ctx=b, v=view()) == STATE and dhost(ctx=b) == STATE and ddev(ctx=b) == STATE
        assert b"sky LUT" in L.csky_last_error(b)
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.render_clouds_view(view_frame[0], BASIS, 70.0, 16, 16)
        assert e.value.code == STATE
        with_lut(bare, view_frame[0])
        assert vhost(ctx=b, v=view()) == OK and dhost(ctx=b) == OK
    finally:
        bare.close()

    # ---- the compositor over view frames
    img = np.zeros((16, 16, 4), np.uint16)
    sky = np.zeros((10, 20, 4), np.uint16)
    ip, sp = img.ctypes.data_as(C.c_void_p), sky.ctypes.data_as(C.c_void_p)

    def cp(out_w=16, out_h=16, cw=16, ch=16):
        q = lib.CompositeParams(out_w, out_h, cw, ch, 20, 10, 0.25, 2.0)
        q.light_direction[0], q.light_direction[1], q.light_direction[2] = 0.6, 0.8, 0.0
        return q

    def comp(ctx=h, q=None, v=None, cf=ip, ct=ip, sf=sp, st=sp, o=optr):
        return L.csky_composite_view_frames(ctx, ref(q), C.c_void_p(C.addressof(v)) if v is not None else None, cf, ct, sf, st, o)

    assert comp(q=cp(), v=view()) == OK
    assert comp(ctx=None, q=cp(), v=view()) == INV and comp(q=None, v=view()) == INV and comp(q=cp(), v=None) == INV
    assert comp(q=cp(), v=view(), cf=None) == INV and comp(q=cp(), v=view(), ct=None) == INV and comp(q=cp(), v=view(), sf=None) == INV
    assert comp(q=cp(), v=view(), st=None) == INV and comp(q=cp(), v=view(), o=None) == INV
    assert comp(q=cp(cw=8), v=view()) == INV and comp(q=cp(ch=32), v=view()) == INV and comp(q=cp(out_w=0, cw=0), v=view()) == INV
    assert comp(q=cp(), v=view(fov=0.0)) == INV and comp(q=cp(), v=view(fov=180.0)) == INV
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- G5
def test_switches_and_unread_fields_leave_the_bytes_alone(whole_ctx, view_frame):
    p, ref = view_frame
    q = np.array(p, np.float32)
    q[0:4] = np.nan                                              # texture_size, update_position
    assert (bits(whole_ctx.render_clouds_view(q, BASIS, V["fov"], V["width"], V["height"])) == bits(ref)).all()
    q[0:4] = (4096.0, 2048.0, 512.0, 256.0)
    assert (bits(whole_ctx.render_clouds_view(q, BASIS, V["fov"], V["width"], V["height"])) == bits(ref)).all()
    try:
        whole_ctx.set_height_window(False)                       # the exact specialisations are switched together: height window and saturation skip off
        off = whole_ctx.render_clouds_view(p, BASIS, V["fov"], V["width"], V["height"])
    finally:
        whole_ctx.set_height_window(True)
    assert (bits(off) == bits(ref)).all()
    assert (bits(whole_ctx.render_clouds_view(p, BASIS, V["fov"], V["width"], V["height"])) == bits(ref)).all()
    # csky_set_march acts: other step counts give another frame
    try:
        whole_ctx.set_march(64, 4)
        coarse = whole_ctx.render_clouds_view(p, BASIS, V["fov"], V["width"], V["height"])
    finally:
        whole_ctx.set_march(*MARCH["A"])
    assert (bits(coarse) != bits(ref)).any()


# ---------------------------------------------------------------------------------------------------------------- G6
def test_composite_view_frames_is_the_host_core(whole_ctx, view_frame, rays_host):  # noqa: F811
    p, cv = view_frame
    sun = np.asarray(p[16:19], np.float32)
    sf = whole_ctx.read_sky_lut()
    st = whole_ctx.render_sky_lut(norm((0.2, 0.9, -0.3)), 200, 100).copy()
    try:
        tr = whole_ctx.read_transmittance()
        other = np.ascontiguousarray(cv[::-1]).copy()           # a second view frame: blend 0.3 between two different images
        got = whole_ctx.composite_view_frames(cv, other, sf, st, sun, BASIS, V["fov"], 0.3, 2.0)
        core = host_composite(rays_host, 1, BASIS, V["fov"], V["width"], V["height"], cv, other, sf, st, tr, 0.3, 2.0, sun).view(np.float16)
        d = ulp_diff(got, core)
        print("composite_view_frames vs host core: worst %d fp16 ulp, %.2f %% of the halves differ" % (int(d.max()), 100.0 * (d > 0).mean()))
        assert d.max() <= 2
        clear = np.zeros_like(cv)
        assert (bits(whole_ctx.composite_view_frames(clear, clear, sf, st, sun, BASIS, V["fov"], 0.3, 2.0)) != bits(got)).any()
    finally:
        whole_ctx.render_sky_lut(sun, 200, 100)                 # the fixture's LUT again


def test_python_mirror(pkg, noise):
    """CloudSky.cloud_view and sky_view(direct=True) are the C calls fed the same frame; direct=False is csky_composite_view as before."""
    import torch

    def host(t):
        return t.cpu().numpy() if hasattr(t, "cpu") else t
    w, h = V["width"], V["height"]
    for device_buffers in (True, False):
        sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=device_buffers)
        try:
            sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
            sky.update_sky()
            cv = sky.cloud_view(BASIS, V["fov"], w, h)
            assert isinstance(cv, torch.Tensor) == device_buffers
            cv = host(cv)
            assert cv.shape == (h, w, 4) and cv.dtype == np.float16 and (cv[..., 3] > 0).mean() >= 0.1
            direct_c = sky.ctx.render_clouds_view(sky._fill_push_constant(), BASIS, V["fov"], w, h)
            assert (bits(cv) == bits(direct_c)).all()
            sf, st = (host(t) for t in sky.sky_lut.back_texture)
            light = sky.frame_data.LIGHT_DIRECTION
            want = sky.ctx.composite_view_frames(direct_c, direct_c, sf, st, light, BASIS, V["fov"], sky.blend_amount, sky.sun_disk_scale)
            assert (bits(sky.sky_view(BASIS, V["fov"], w, h, direct=True)) == bits(want)).all()
            bf, bt = host(sky.textures[sky.texture_to_blend_from]), host(sky.textures[sky.texture_to_blend_to])
            today = sky.ctx.composite_view(bf, bt, sf, st, light, BASIS, V["fov"], sky.blend_amount, sky.sun_disk_scale, w, h)
            assert (bits(sky.sky_view(BASIS, V["fov"], w, h)) == bits(today)).all()
            assert (bits(sky.sky_view(BASIS, V["fov"], w, h, direct=False)) == bits(today)).all()
        finally:
            sky.close()
