"""The direct cloud march from an observer's position (csky_render_clouds_view_from / _dirs_from and their _device forms; csrc/observer_core.h,
cloud_kernels.hip clouds_observer_kernel) on the GPU through the C ABI.  At the reference's own place without a cap it must return the bytes of
csky_render_clouds_view / _dirs (anchor (a) of the definition); every other observer of tests/observers.py is held to the host core's march of the
same rays (tests/observer_host: march(), which has no early end and assumes nothing about where a ray runs) at the gate for frames rendered from
the shipped assets (parity_metrics.cloud_tight).  Then what a launch may touch, the height window and the saturation skip on rays that descend,
what state a call needs and leaves, every error path, and the Python mirror."""
import ctypes as C

import numpy as np
import pytest

import clouds_rays_reference as RR
import observers as OB
import shadow_reference as SR
from parity_metrics import cloud_tight
from test_clouds_rays_host import chains, host_view_dirs, rays_host  # noqa: F401  (module-scoped fixtures)
from test_observer_host import host_march_from, host_rays, obs_host  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD = 3                           # guard rows before and after an image
V = RR.VIEW
W, H = V["width"], V["height"]
BASIS = RR.camera_basis(V["pitch"], V["yaw"])
MARCH = {"A": (128, 6), "B": (30, 4)}
INF = float("inf")
ORIGIN = (0.0, 0.0, 0.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def with_lut(ctx, p):
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(np.asarray(p[16:19], np.float32), 200, 100)


@pytest.fixture(scope="module")
def whole_ctx(pkg, noise):
    if pkg.lib().csky_device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible (libcloudsky has no CPU fallback)")
    ctx = pkg.Context(0)
    ctx.set_noise(*noise)
    ctx.set_segments(1)
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
def scene_a(whole_ctx, oracle):
    """scene A bound to whole_ctx at 128 x 6 steps: its push-constant block"""
    p = SR.scene(oracle, "A")
    whole_ctx.set_march(*MARCH["A"])
    with_lut(whole_ctx, p)
    return p


def view_from(ctx, p, name, **kw):
    pos, cap, basis, fov, w, h = OB.observer(name)
    return ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap, **kw)


# ---------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("exact", [False, True], ids=["fp16-cells", "exact-cells"])
def test_the_ground_observer_gives_the_bytes_of_the_direct_march(whole_ctx, exact_ctx, rays_host, oracle, name, exact):  # noqa: F811
    import torch
    ctx = exact_ctx if exact else whole_ctx
    p = SR.scene(oracle, name)
    ctx.set_march(*MARCH[name])
    try:
        with_lut(ctx, p)
        view = ctx.render_clouds_view(p, BASIS, V["fov"], W, H)
        d = host_view_dirs(rays_host, BASIS, V["fov"], W, H)
        via_dirs = ctx.render_clouds_dirs(p, d)
        assert (view[..., 3] > 0).mean() >= 0.25 and (d[..., 1] <= 0).mean() >= 0.10
        got = {"view host": ctx.render_clouds_view_from(p, BASIS, V["fov"], W, H, ORIGIN), "dirs host": ctx.render_clouds_dirs_from(p, d, ORIGIN)}
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dd = torch.from_numpy(d).cuda()
            o1 = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
            o2 = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
            s.synchronize()
            assert ctx.render_clouds_view_from(p, BASIS, V["fov"], W, H, ORIGIN, out=o1, stream=s.cuda_stream) is o1
            assert ctx.render_clouds_dirs_from(p, dd, ORIGIN, INF, out=o2, stream=s.cuda_stream) is o2
            got["view device"], got["dirs device"] = o1.cpu().numpy(), o2.cpu().numpy()
        for form, img in got.items():
            want = view if form.startswith("view") else via_dirs
            differ = int((bits(img) != bits(want)).sum())
            print("scene %s, %s, %s: %d of %d halves differ from the direct march" % (name, "exact" if exact else "fp16", form, differ, img.size))
            assert differ == 0, form
    finally:
        ctx.set_march(128, 6)


# ---------------------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("name", OB.MOVED)
def test_a_moved_observer_matches_the_host_core_and_the_dirs_form(whole_ctx, scene_a, obs_host, rays_host, chains, name):  # noqa: F811
    p = scene_a
    pos, cap, basis, fov, w, h = OB.observer(name)
    got = view_from(whole_ctx, p, name)
    d = host_view_dirs(rays_host, basis, fov, w, h)
    core, marched, _ = host_march_from(obs_host, chains, p, whole_ctx.read_sky_lut(), pos, cap, d)
    _, seg, _ = host_rays(obs_host, pos, cap, d, MARCH["A"][0])
    OB.assert_conditions(name, d, core[..., 3].astype(np.float32), marched, seg)
    ok, info = cloud_tight(got, core)
    print("%s vs host core: %s" % (name, info))
    assert ok, info
    assert not bits(got)[~marched].any()                        # no segment: zeros
    assert (bits(whole_ctx.render_clouds_dirs_from(p, d, pos, cap)) == bits(got)).all()


# ---------------------------------------------------------------------------------------------------------------- G3
@pytest.mark.parametrize("size", [(37, 21, 0), (37, 21, 24), (1, 1, 0), (1, 1, 24)], ids=["37x21", "37x21-pitched", "1x1", "1x1-pitched"])
@pytest.mark.parametrize("form", ["view", "dirs"])
def test_write_coverage(whole_ctx, scene_a, rays_host, size, form):  # noqa: F811
    """The device forms into a tensor of 0xFFFF halfs (a NaN no frame contains) with guard rows and row padding, from above the layer."""
    import torch
    w, h, pad = size
    p = scene_a
    pos, cap, basis, fov, _, _ = OB.observer("above_down")
    d = host_view_dirs(rays_host, basis, fov, w, h)
    host = whole_ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap) if form == "view" else whole_ctx.render_clouds_dirs_from(p, d, pos, cap)
    assert not (bits(host) == 0xFFFF).any()
    if w > 1:
        assert len(np.unique(bits(host))) > 8
    else:
        assert d[0, 0, 1] < 0                                      # the single ray looks down
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
                out = whole_ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap, out=share, stream=stream)
            else:
                out = whole_ctx.render_clouds_dirs_from(p, dd, pos, cap, out=share, stream=stream)
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
@pytest.mark.parametrize("name", ["inside", "inside_up", "above_down"])
def test_the_height_window_and_the_saturation_skip_leave_the_bytes_alone(whole_ctx, scene_a, name):
    """csky_set_height_window(0) switches the exact specialisations off together: the per-sample window and the saturation skip.  Both are
    positional or bound-based, so rays that descend, or dip and rise, must give the same halves with them as without."""
    on = view_from(whole_ctx, scene_a, name)
    try:
        whole_ctx.set_height_window(False)
        off = view_from(whole_ctx, scene_a, name)
    finally:
        whole_ctx.set_height_window(True)
    differ = int((bits(on) != bits(off)).sum())
    print("%s: %d of %d halves differ with the window and the saturation skip off; alpha > 0 in %.1f %% of the pixels" % (name, differ, on.size, 100.0 * (on[..., 3] > 0).mean()))
    assert (on[..., 3] > 0).mean() >= 0.25
    assert differ == 0


# ---------------------------------------------------------------------------------------------------------------- G5
def test_cloud_frames_and_luts_are_what_they_were(pkg, noise, oracle):
    """Two frames in flight on two streams: three cloud frames with _from calls before, between and after them are the frames without."""
    import torch
    ctx = pkg.Context(0)
    try:
        ctx.set_noise(*noise)
        ctx.set_frames_in_flight(2)
        pa = SR.scene(oracle, "A")
        with_lut(ctx, pa)
        lut, tr = ctx.read_sky_lut().copy(), ctx.read_transmittance().copy()
        view0 = ctx.render_clouds_view(pa, BASIS, V["fov"], W, H).copy()
        blocks = []
        for k in range(3):
            q = oracle.default_params(128, 64, (1, 1, 0))
            q[4:6] = (0.5 * k, -0.25 * k)
            q[23] = 3.0 * k
            blocks.append(q)
        pb = SR.scene(oracle, "B")
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pos, cap, basis, fov, w, h = OB.observer("above_down")

        def run(with_from):
            frames = [torch.zeros((64, 128, 4), dtype=torch.float16, device="cuda") for _ in blocks]
            views = [torch.zeros((h, w, 4), dtype=torch.float16, device="cuda") for _ in range(4 if with_from else 0)]
            torch.cuda.synchronize()
            if with_from:
                ctx.render_clouds_view_from(pb, basis, fov, w, h, pos, cap, out=views[0], stream=streams[1].cuda_stream)
            for k, q in enumerate(blocks):
                s = streams[k % 2]
                if with_from and k > 0:                          # on the stream of the frame still in flight, beside the one about to start
                    ctx.render_clouds_view_from(pb, basis, fov, w, h, pos, cap, out=views[k], stream=streams[(k + 1) % 2].cuda_stream)
                ctx.render_clouds_device(q, 128, (8, 0, 1, 8), frames[k].data_ptr(), 128 * 8, s.cuda_stream)
            if with_from:
                ctx.render_clouds_view_from(pb, basis, fov, w, h, pos, cap, out=views[3], stream=streams[0].cuda_stream)
            torch.cuda.synchronize()
            return [f.cpu().numpy() for f in frames], [v.cpu().numpy() for v in views]
        plain, _ = run(False)
        mixed, views = run(True)
        again, _ = run(False)
        for a, b, c in zip(plain, mixed, again):
            assert bits(a).any() and (bits(a) == bits(b)).all() and (bits(a) == bits(c)).all()
        assert len(views) == 4 and (views[0][..., 3] > 0).any()
        for v in views[1:]:
            assert (bits(v) == bits(views[0])).all()
        assert (bits(views[0]) == bits(ctx.render_clouds_view_from(pb, basis, fov, w, h, pos, cap))).all()
        assert (bits(ctx.render_clouds_view(pa, BASIS, V["fov"], W, H)) == bits(view0)).all()
        assert (bits(ctx.read_sky_lut()) == bits(lut)).all() and (bits(ctx.read_transmittance()) == bits(tr)).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- G6
def test_error_paths(pkg, whole_ctx, scene_a, noise):
    """Every CSKY_ERR_INVALID and CSKY_ERR_STATE case of the header, view and dirs forms, host and device."""
    import torch
    L, lib = pkg.lib(), pkg._lib
    h = whole_ctx._h
    INV, STATE, OK = lib.ERR_INVALID, lib.ERR_STATE, lib.OK
    nan, inf = float("nan"), INF
    p = lib.cloud_params(scene_a)
    out = np.zeros((16, 16, 4), np.uint16)
    optr = out.ctypes.data_as(C.c_void_p)
    dirs = np.zeros((16, 16, 3), np.float32)
    dirs[..., 1] = -1.0
    hd = dirs.ctypes.data_as(C.c_void_p)
    d = torch.zeros((16, 32, 4), dtype=torch.int16, device="cuda")
    dptr = C.c_void_p(d.data_ptr())
    dd = torch.from_numpy(dirs).cuda()
    ddp = C.c_void_p(dd.data_ptr())

    def view(basis=RR.column_major(BASIS), fov=70.0):
        return lib.View((C.c_float * 9)(*[float(x) for x in basis]), fov)

    def obs(pos=(0.0, 8000.0, 0.0), cap=inf):
        return lib.Observer((C.c_float * 3)(*pos), cap)

    def ref(x):
        return C.byref(x) if x is not None else None
    good_v, good_o = view(), obs()

    def vhost(ctx=h, params=p, v=good_v, o=good_o, w=16, hh=16, out_=optr):
        return L.csky_render_clouds_view_from(ctx, ref(params), ref(v), ref(o), w, hh, out_)

    def vdev(ctx=h, params=p, v=good_v, o=good_o, w=16, hh=16, out_=dptr, pitch=128):
        return L.csky_render_clouds_view_from_device(ctx, ref(params), ref(v), ref(o), w, hh, out_, pitch, None)

    def dhost(ctx=h, params=p, o=good_o, w=16, hh=16, di=hd, out_=optr):
        return L.csky_render_clouds_dirs_from(ctx, ref(params), w, hh, di, ref(o), out_)

    def ddev(ctx=h, params=p, o=good_o, w=16, hh=16, di=ddp, out_=dptr, pitch=128):
        return L.csky_render_clouds_dirs_from_device(ctx, ref(params), w, hh, di, ref(o), out_, pitch, None)
    forms = (vhost, vdev, dhost, ddev)

    assert all(f() == OK for f in forms) and vdev(pitch=136) == OK and ddev(pitch=256) == OK
    whole_ctx.sync()
    assert (d.cpu().numpy().view(np.uint16)[:, :16] == out).all()  # the last device call (pitch 256) and the last host call: the same rays
    for f in forms:
        assert f(ctx=None) == INV and f(params=None) == INV and f(out_=None) == INV and f(o=None) == INV, f.__name__
    assert b"observer is NULL" in L.csky_last_error(h)
    assert vhost(v=None) == INV and vdev(v=None) == INV and dhost(di=None) == INV and ddev(di=None) == INV
    for w, hh in ((0, 16), (8193, 16), (16, 0), (16, 8193), (-1, 16), (16, -1)):
        assert vhost(w=w, hh=hh) == INV and vdev(w=w, hh=hh, pitch=8 * 8193) == INV and dhost(w=w, hh=hh) == INV and ddev(w=w, hh=hh, pitch=8 * 8193) == INV, (w, hh)
    for pitch in (120, 132, 0):
        assert vdev(pitch=pitch) == INV and ddev(pitch=pitch) == INV, pitch
    b = RR.column_major(BASIS).copy()
    b[4] = nan
    assert vhost(v=view(basis=b)) == INV and vdev(v=view(basis=b)) == INV
    for fov in (0.0, 180.0, nan):
        assert vhost(v=view(fov=fov)) == INV and vdev(v=view(fov=fov)) == INV, fov
    # the observer's own rules (observer_core.h observer_invalid; tests/test_observer_host.py holds the rule itself)
    bad = [obs(pos=(nan, 0.0, 0.0)), obs(pos=(0.0, inf, 0.0)), obs(pos=(0.0, 0.0, -inf)), obs(pos=(1.0001e6, 0.0, 0.0)), obs(pos=(0.0, 0.0, -1.0001e6)),
           obs(pos=(0.0, -1.0, 0.0)), obs(pos=(50000.0, -300.0, 0.0)), obs(pos=(0.0, 100001.0, 0.0)), obs(cap=0.0), obs(cap=-1.0), obs(cap=nan), obs(cap=-inf)]
    for k, o in enumerate(bad):
        for f in forms:
            assert f(o=o) == INV, (k, f.__name__)
    for o in (obs(pos=(0.0, 100000.0, 0.0)), obs(pos=(1e6, -80000.0, 0.0)), obs(cap=1e-3), obs(pos=(0.0, 0.0, 0.0))):
        assert all(f(o=o) == OK for f in forms)
    bare = pkg.Context(0)
    try:
        bh = bare._h
        assert all(f(ctx=bh) == STATE for f in forms)
        assert b"csky_set_noise" in L.csky_last_error(bh)
        assert all(f(ctx=bh, o=bad[0]) == INV for f in forms)     # a bad observer is refused before the context's state is looked at
        bare.set_noise(*noise)
        assert all(f(ctx=bh) == STATE for f in forms)
        assert b"sky LUT" in L.csky_last_error(bh)
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.render_clouds_view_from(scene_a, BASIS, 70.0, 16, 16, (0.0, 8000.0, 0.0))
        assert e.value.code == STATE
        with_lut(bare, scene_a)
        assert vhost(ctx=bh) == OK and dhost(ctx=bh) == OK
    finally:
        bare.close()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- G7
def test_python_mirror(pkg, noise):
    """CloudSky.cloud_view(position=...) is the C call fed the same frame; without a position it is csky_render_clouds_view as before."""
    import torch
    pos, cap, basis, fov, w, h = OB.observer("above_down")
    for device_buffers in (True, False):
        sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=device_buffers)
        try:
            sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
            sky.update_sky()
            cv = sky.cloud_view(basis, fov, w, h, position=pos, max_distance=cap)
            assert isinstance(cv, torch.Tensor) == device_buffers
            cv = cv.cpu().numpy() if device_buffers else cv
            assert cv.shape == (h, w, 4) and cv.dtype == np.float16 and (cv[..., 3] > 0).mean() >= 0.1
            pc = sky._fill_push_constant()
            assert (bits(cv) == bits(sky.ctx.render_clouds_view_from(pc, basis, fov, w, h, pos, cap))).all()
            capped = sky.cloud_view(basis, fov, w, h, position=pos, max_distance=5000.0)
            capped = capped.cpu().numpy() if device_buffers else capped
            assert (bits(capped) == bits(sky.ctx.render_clouds_view_from(pc, basis, fov, w, h, pos, 5000.0))).all() and (bits(capped) != bits(cv)).any()
            plain = sky.cloud_view(BASIS, V["fov"], W, H)
            plain = plain.cpu().numpy() if device_buffers else plain
            assert (bits(plain) == bits(sky.ctx.render_clouds_view(pc, BASIS, V["fov"], W, H))).all()
            with pytest.raises(ValueError):
                sky.cloud_view(basis, fov, w, h, aerial=True, position=pos)
        finally:
            sky.close()
