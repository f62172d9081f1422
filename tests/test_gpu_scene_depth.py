"""The observer's cloud march behind a per-pixel scene depth (csky_render_clouds_view_from_depth / _dirs_from_depth and their _device forms;
csrc/scene_depth_core.h, cloud_kernels.hip clouds_observer_depth_kernel) on the GPU through the C ABI.  Anchors: a buffer of +inf gives the bytes
of the _from forms, a constant c those of the _from forms with max_distance = min(max_distance, c), a piecewise-constant buffer those of the
uniform-cap _from frames pixel for pixel.  The buffers of tests/scene_depths.py are held to the host core's march of the same rays
(tests/scene_depth_host) at the gate for frames rendered from the shipped assets (parity_metrics.cloud_tight).  Then what a launch may touch, the
height window, what state a call needs and leaves, every error path, the texel rule and the Python mirror."""
import ctypes as C

import numpy as np
import pytest

import clouds_rays_reference as RR
import observer_reference as OR
import observers as OB
import scene_depth_reference as DR
import scene_depths as SD
import shadow_reference as SR
from parity_metrics import cloud_tight
from test_clouds_rays_host import chains  # noqa: F401  (module-scoped fixtures)
from test_observer_host import host_march_from, obs_host  # noqa: F401
from test_scene_depth_host import TEXELS, advance, cam_of, depth_host, host_march_depth  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD = 3                           # guard rows before and after an image or a depth buffer
GUARD_Z = 12345.0                   # what the guard texels of a depth buffer hold
V = RR.VIEW
MARCH = {"A": (128, 6), "B": (30, 4)}
INF = float("inf")
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def bind(ctx, oracle, scene="A"):
    """the scene's push-constant block, with its step counts and its sky LUT bound to ctx"""
    p = SR.scene(oracle, scene)
    ctx.set_march(*MARCH[scene])
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(np.asarray(p[16:19], np.float32), 200, 100)
    return p


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


def view_depth(ctx, p, name, z, kind="distance", **kw):
    pos, cap, basis, fov, w, h = OB.observer(name)
    return ctx.render_clouds_view_from_depth(p, basis, fov, w, h, pos, z, kind, cap, **kw)


def view_from(ctx, p, name, cap=None, **kw):
    pos, own, basis, fov, w, h = OB.observer(name)
    return ctx.render_clouds_view_from(p, basis, fov, w, h, pos, own if cap is None else min(own, cap), **kw)


# ---------------------------------------------------------------------------------------------------------------- G1
G1_CASES = [(n, "A", False) for n in OB.NAMES] + [(n, s, e) for n in ("inside", "above_down") for s, e in (("A", True), ("B", False), ("B", True))]


@pytest.mark.parametrize("name,scene,exact", G1_CASES, ids=["%s-%s-%s" % (n, s, "exact" if e else "fp16") for n, s, e in G1_CASES])
def test_nothing_in_the_way_and_one_constant_give_the_bytes_of_the_from_forms(whole_ctx, exact_ctx, oracle, name, scene, exact):
    """Anchors (a) and (b): view and dirs, host and device forms."""
    import torch
    ctx = exact_ctx if exact else whole_ctx
    try:
        p = bind(ctx, oracle, scene)
        pos, cap, basis, fov, w, h = OB.observer(name)
        d = OB.dirs(name)
        for c in (INF, 6000.0):
            z = np.full((h, w), c, F)
            want_view = view_from(ctx, p, name, c)
            want_dirs = ctx.render_clouds_dirs_from(p, d, pos, min(cap, c))
            if c == INF and scene == "A":
                assert (want_view[..., 3] > 0).mean() >= 0.25
            got = {"view host": view_depth(ctx, p, name, z), "dirs host": ctx.render_clouds_dirs_from_depth(p, d, pos, z, max_distance=cap)}
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                dd, zz = torch.from_numpy(d).cuda(), torch.from_numpy(z).cuda()
                o1 = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
                s.synchronize()
                assert view_depth(ctx, p, name, zz, out=o1, stream=s.cuda_stream) is o1
                o2 = ctx.render_clouds_dirs_from_depth(p, dd, pos, zz, max_distance=cap, stream=s.cuda_stream)
                got["view device"], got["dirs device"] = o1.cpu().numpy(), o2.cpu().numpy()
            for form, img in got.items():
                want = want_view if form.startswith("view") else want_dirs
                differ = int((bits(img) != bits(want)).sum())
                print("%s, scene %s, %s, constant %g, %s: %d of %d halves differ from the _from form" % (name, scene, "exact" if exact else "fp16", c, form, differ, img.size))
                assert differ == 0, (form, c)
    finally:
        ctx.set_march(128, 6)


# ---------------------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("name", ["inside", "above_down"])
def test_a_piecewise_constant_buffer_is_the_uniform_cap_frames_pixel_for_pixel(whole_ctx, oracle, name):
    """Anchor (c): a transposed, mis-pitched or tile-shifted depth read moves a quadrant's edge."""
    import torch
    p = bind(whole_ctx, oracle)
    _, _, _, _, w, h = OB.observer(name)
    z, idx = SD.quad(name), SD.quad_index(h, w)
    want = np.zeros((h, w, 4), np.float16)
    frames = []
    for q, c in enumerate(SD.QUAD_CAPS):                         # three capped _from calls and the observer's own
        frames.append(view_from(whole_ctx, p, name, c))
        want[idx == q] = frames[-1][idx == q]
    assert all((bits(frames[a]) != bits(frames[a + 1])).any() for a in range(2))   # the three caps do give three different frames
    zt = torch.from_numpy(z).cuda()
    dev = view_depth(whole_ctx, p, name, zt)                     # asynchronous on the context's own stream
    whole_ctx.sync()
    for form, got in (("host", view_depth(whole_ctx, p, name, z)), ("device", dev.cpu().numpy())):
        differ = int((bits(got) != bits(want)).sum())
        print("%s, quad, %s: %d of %d halves differ from the per-quadrant _from frames" % (name, form, differ, got.size))
        assert differ == 0, form


# ---------------------------------------------------------------------------------------------------------------- G3
@pytest.mark.parametrize("name", OB.MOVED)
def test_a_mixed_buffer_matches_the_host_core(whole_ctx, oracle, depth_host, obs_host, chains, name):  # noqa: F811
    p = bind(whole_ctx, oracle)
    pos, cap, _, _, _, _ = OB.observer(name)
    d, cam, z = OB.dirs(name), cam_of(name), SD.mixed(name)
    sky = whole_ctx.read_sky_lut()
    core, marched, _ = host_march_depth(depth_host, chains, p, sky, pos, cap, d, z)
    free, fm, _ = host_march_from(obs_host, chains, p, sky, pos, cap, d)
    SD.assert_conditions(name, z, core, free, fm)
    got = view_depth(whole_ctx, p, name, z)
    ok, info = cloud_tight(got, core)
    print("%s, mixed vs host core: %s" % (name, info))
    assert ok, info
    assert not bits(got)[~marched].any()                         # not marched: zeros
    via_dirs = whole_ctx.render_clouds_dirs_from_depth(p, d, pos, z, max_distance=cap)
    assert (bits(via_dirs) == bits(got)).all()
    # view-z: the same scene as a rasteriser's linear depth
    zv = DR.view_z(cam, d, z)
    got_vz = view_depth(whole_ctx, p, name, zv, "view_z")
    core_vz, marched_vz, _ = host_march_depth(depth_host, chains, p, sky, pos, cap, d, zv, DR.VIEW_Z, cam)
    ok, info = cloud_tight(got_vz, core_vz)
    print("%s, mixed as view-z vs host core: %s" % (name, info))
    assert ok, info
    assert not bits(got_vz)[~marched_vz].any()
    dist, valid = DR.cap(DR.VIEW_Z, cam, d, zv)
    assert valid.all()
    assert (bits(whole_ctx.render_clouds_dirs_from_depth(p, d, pos, dist, max_distance=cap)) == bits(got_vz)).all()


# ---------------------------------------------------------------------------------------------------------------- G4
def small_depth(w, h):
    """a depth buffer for an image no observer has: a ramp across the layer seen from above_down, with a texel of each special kind"""
    j, i = np.mgrid[0:h, 0:w]
    z = (4500.0 + 150.0 * i + 400.0 * j).astype(F)
    if w > 1:
        z[h // 2, w // 3], z[h // 3, w // 2], z[h - 1, w - 1], z[0, w - 1] = INF, 0.0, np.nan, -1.0
    else:
        z[:] = 12000.0                                           # behind the layer's top along the one ray
    return z


@pytest.mark.parametrize("size", [(37, 21), (1, 1)], ids=["37x21", "1x1"])
@pytest.mark.parametrize("form", ["view", "dirs"])
def test_write_coverage(whole_ctx, oracle, size, form):
    """The device forms into a tensor of 0xFFFF halfs with guard rows and row padding, from a depth tensor with guard rows and row padding of its
    own: the w x h texels are written and nothing else, the depth tensor is unchanged, and the host form gives the same bytes."""
    import torch
    w, h = size
    p = bind(whole_ctx, oracle)
    pos, cap, basis, fov, _, _ = OB.observer("above_down")
    d = RR.view_dirs(basis, fov, w, h)
    z = small_depth(w, h)

    def call(zz, dd, **kw):
        if form == "view":
            return whole_ctx.render_clouds_view_from_depth(p, basis, fov, w, h, pos, zz, "distance", cap, **kw)
        return whole_ctx.render_clouds_dirs_from_depth(p, dd, pos, zz, max_distance=cap, **kw)
    host = call(z, d)
    assert not (bits(host) == 0xFFFF).any()
    if w > 1:
        assert len(np.unique(bits(host))) > 8 and not bits(host)[h // 3, w // 2].any() and not bits(host)[h - 1, w - 1].any()
        zp = np.full((h, w + 5), GUARD_Z, F)                     # the host form with a pitch of its own
        zp[:, :w] = z
        assert (bits(call(zp[:, :w], d)) == bits(host)).all()
    else:
        assert d[0, 0, 1] < 0 and bits(host).any()               # the single ray looks down, into cloud
    s = torch.cuda.Stream()
    for pad, zpad in ((0, 0), (24, 0), (0, 12), (24, 12)):
        pitch_h, zpitch = (8 * w + pad) // 2, (4 * w + zpad) // 4
        for stream in (s.cuda_stream, None):
            with torch.cuda.stream(s):
                t = torch.empty((h + 2 * GUARD, pitch_h), dtype=torch.int16, device="cuda")
                t.fill_(-1)
                zt = torch.full((h + 2 * GUARD, zpitch), GUARD_Z, dtype=torch.float32, device="cuda")
                zt[GUARD:GUARD + h, :w] = torch.from_numpy(z).cuda()
                before = zt.cpu().numpy().copy()
                dd = torch.from_numpy(d).cuda()
                s.synchronize()                                  # the NULL form runs on the context's own stream
                share = t[GUARD:GUARD + h, :4 * w].unflatten(1, (w, 4))
                zshare = zt[GUARD:GUARD + h, :w]
                assert (share.stride(0) * 2 == 8 * w + pad and zshare.stride(0) * 4 == 4 * w + zpad) or h == 1
                assert call(zshare, dd, out=share, stream=stream) is share
                if stream is None:
                    whole_ctx.sync()
                got = t.cpu().numpy().view(np.uint16)
                after = zt.cpu().numpy()
            inside = np.zeros(got.shape, bool)
            inside[GUARD:GUARD + h, :4 * w] = True
            assert not (got[inside] == 0xFFFF).any()
            assert (got[~inside] == 0xFFFF).all(), np.argwhere(~inside & (got != 0xFFFF))[:4]
            assert (got[GUARD:GUARD + h, :4 * w].reshape(h, w, 4) == bits(host)).all(), (pad, zpad)
            assert (after.view(np.uint32) == before.view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------------------------- G5
@pytest.mark.parametrize("name", ["inside", "above_down"])
def test_the_height_window_and_the_saturation_skip_leave_the_bytes_alone(whole_ctx, oracle, name):
    p = bind(whole_ctx, oracle)
    z = SD.mixed(name)
    on = view_depth(whole_ctx, p, name, z)
    try:
        whole_ctx.set_height_window(False)
        off = view_depth(whole_ctx, p, name, z)
    finally:
        whole_ctx.set_height_window(True)
    differ = int((bits(on) != bits(off)).sum())
    print("%s, mixed: %d of %d halves differ with the window and the saturation skip off; alpha > 0 in %.1f %% of the pixels" % (name, differ, on.size, 100.0 * (on[..., 3] > 0).mean()))
    assert (on[..., 3] > 0).mean() >= 0.25
    assert differ == 0


# ---------------------------------------------------------------------------------------------------------------- G6
def test_cloud_frames_luts_and_from_frames_are_what_they_were(pkg, noise, oracle):
    """A 128 x 64 cloud frame, the sky LUT, the transmittance table and one _from frame before and after depth calls on a second stream."""
    import torch
    ctx = pkg.Context(0)
    try:
        ctx.set_noise(*noise)
        pa = bind(ctx, oracle)
        q = oracle.default_params(128, 64, (1, 1, 0))
        pos, cap, basis, fov, w, h = OB.observer("above_down")
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]

        def state():
            frame = torch.zeros((64, 128, 4), dtype=torch.float16, device="cuda")
            torch.cuda.synchronize()
            ctx.render_clouds_device(q, 128, (8, 0, 1, 8), frame.data_ptr(), 128 * 8, streams[0].cuda_stream)
            torch.cuda.synchronize()
            return [frame.cpu().numpy(), ctx.read_sky_lut().copy(), ctx.read_transmittance().copy(), view_from(ctx, pa, "above_down").copy()]
        before = state()
        assert bits(before[0]).any() and bits(before[3]).any()
        zt = torch.from_numpy(SD.mixed("above_down")).cuda()
        zq = torch.from_numpy(SD.quad("above_down")).cuda()
        dd = torch.from_numpy(OB.dirs("above_down")).cuda()
        torch.cuda.synchronize()
        outs = [view_depth(ctx, pa, "above_down", zt, stream=streams[1].cuda_stream), view_depth(ctx, pa, "above_down", zq, stream=streams[1].cuda_stream),
                ctx.render_clouds_dirs_from_depth(pa, dd, pos, zt, max_distance=cap, stream=streams[1].cuda_stream)]
        torch.cuda.synchronize()
        assert (bits(outs[0].cpu().numpy()) == bits(outs[2].cpu().numpy())).all() and bits(outs[1].cpu().numpy()).any()
        after = state()
        for k, (a, b) in enumerate(zip(before, after)):
            assert (bits(a) == bits(b)).all(), k
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- G7
def test_error_paths(pkg, whole_ctx, oracle, noise):
    """Every CSKY_ERR_INVALID and CSKY_ERR_STATE case of the header, view and dirs forms, host and device; INVALID comes before STATE."""
    import torch
    scene_a = bind(whole_ctx, oracle)
    L, lib = pkg.lib(), pkg._lib
    h = whole_ctx._h
    INV, STATE, OK = lib.ERR_INVALID, lib.ERR_STATE, lib.OK
    nan = float("nan")
    p = lib.cloud_params(scene_a)
    out = np.zeros((16, 16, 4), np.uint16)
    optr = out.ctypes.data_as(C.c_void_p)
    dirs = np.zeros((16, 16, 3), np.float32)
    dirs[..., 1] = -1.0
    hd = dirs.ctypes.data_as(C.c_void_p)
    zh = np.full((16, 32), 5000.0, np.float32)                    # rows of 32: pitches 64 (tight) and 128
    zh[:, 16:] = nan
    big = torch.zeros((64, 32, 4), dtype=torch.int16, device="cuda")    # 64 rows of 256 bytes: the image and, behind it, room for an overlapping depth
    dptr = big.data_ptr()
    dd = torch.from_numpy(dirs).cuda()
    ddp = C.c_void_p(dd.data_ptr())
    zd = torch.from_numpy(zh).cuda()

    def view(basis=RR.column_major(RR.camera_basis(-30.0, V["yaw"])), fov=70.0):
        return lib.View((C.c_float * 9)(*[float(x) for x in basis]), fov)

    def obs(pos=(0.0, 8000.0, 0.0), cap=INF):
        return lib.Observer((C.c_float * 3)(*pos), cap)

    def hdepth(texels=zh.ctypes.data, pitch=128, kind=0):
        return lib.SceneDepth(C.c_void_p(texels), pitch, kind)

    def ddepth(texels=zd.data_ptr(), pitch=128, kind=0):
        return lib.SceneDepth(C.c_void_p(texels), pitch, kind)

    def ref(x):
        return C.byref(x) if x is not None else None
    good_v, good_o, good_h, good_d = view(), obs(), hdepth(), ddepth()

    def vhost(ctx=h, params=p, v=good_v, o=good_o, w=16, hh=16, z=good_h, out_=optr):
        return L.csky_render_clouds_view_from_depth(ctx, ref(params), ref(v), ref(o), w, hh, ref(z), out_)

    def vdev(ctx=h, params=p, v=good_v, o=good_o, w=16, hh=16, z=good_d, out_=C.c_void_p(dptr), pitch=128):
        return L.csky_render_clouds_view_from_depth_device(ctx, ref(params), ref(v), ref(o), w, hh, ref(z), out_, pitch, None)

    def dhost(ctx=h, params=p, o=good_o, w=16, hh=16, di=hd, z=good_h, out_=optr):
        return L.csky_render_clouds_dirs_from_depth(ctx, ref(params), w, hh, di, ref(o), ref(z), out_)

    def ddev(ctx=h, params=p, o=good_o, w=16, hh=16, di=ddp, z=good_d, out_=C.c_void_p(dptr), pitch=128):
        return L.csky_render_clouds_dirs_from_depth_device(ctx, ref(params), w, hh, di, ref(o), ref(z), out_, pitch, None)
    forms, hosts, devs = (vhost, vdev, dhost, ddev), (vhost, dhost), (vdev, ddev)

    assert all(f() == OK for f in forms) and vdev(pitch=136) == OK and ddev(pitch=256) == OK
    whole_ctx.sync()
    assert (big.cpu().numpy().view(np.uint16)[:16, :16] == out).all()   # the last device call (pitch 256) and the last host call: the same rays
    zt = np.ascontiguousarray(zh[:, :16])
    assert vhost(z=hdepth(zt.ctypes.data, 0)) == OK and vhost(z=hdepth(zt.ctypes.data, 64)) == OK and vhost(z=hdepth(kind=1)) == OK and vdev(z=ddepth(kind=1)) == OK
    for f in forms:
        assert f(ctx=None) == INV and f(params=None) == INV and f(out_=None) == INV and f(o=None) == INV and f(z=None) == INV, f.__name__
    assert b"depth is NULL" in L.csky_last_error(h)
    assert vhost(v=None) == INV and vdev(v=None) == INV and dhost(di=None) == INV and ddev(di=None) == INV
    # the depth buffer's own rules (scene_depth_core.h scene_depth_invalid; tests/test_scene_depth_host.py holds the rule itself)
    for f, mk in ((vhost, hdepth), (dhost, hdepth), (vdev, ddepth), (ddev, ddepth)):
        assert f(z=mk(texels=0)) == INV, f.__name__
        for kind in (2, -1, 7):
            assert f(z=mk(kind=kind)) == INV, (f.__name__, kind)
        for pitch in (60, 66, 126, 4):
            assert f(z=mk(pitch=pitch)) == INV, (f.__name__, pitch)
    assert dhost(z=hdepth(kind=1)) == INV and ddev(z=ddepth(kind=1)) == INV
    assert b"CSKY_DEPTH_VIEW_Z" in L.csky_last_error(h)
    assert vdev(z=ddepth(pitch=0)) == INV and ddev(z=ddepth(pitch=0)) == INV       # 0 means tight in the host forms only
    for f in devs:                                                # the image: 16 rows of 128 bytes from dptr = [dptr, dptr + 2048)
        for at_ in (dptr, dptr + 2044, dptr - 15 * 128 - 60, dptr + 64):
            assert f(z=ddepth(texels=at_)) == INV, (f.__name__, at_ - dptr)
        assert b"overlap" in L.csky_last_error(h)
        assert f(z=ddepth(texels=dptr + 2048)) == OK, f.__name__  # the bytes right behind the image, whatever they hold: texel values are no error
    for w, hh in ((0, 16), (8193, 16), (16, 0), (16, 8193), (-1, 16), (16, -1)):
        assert vhost(w=w, hh=hh) == INV and vdev(w=w, hh=hh, pitch=8 * 8193) == INV and dhost(w=w, hh=hh) == INV and ddev(w=w, hh=hh, pitch=8 * 8193) == INV, (w, hh)
    for pitch in (120, 132, 0):
        assert vdev(pitch=pitch) == INV and ddev(pitch=pitch) == INV, pitch
    b = RR.column_major(RR.camera_basis(-30.0, V["yaw"])).copy()
    b[4] = nan
    assert vhost(v=view(basis=b)) == INV and vdev(v=view(basis=b)) == INV
    for fov in (0.0, 180.0, nan):
        assert vhost(v=view(fov=fov)) == INV and vdev(v=view(fov=fov)) == INV, fov
    bad_o = [obs(pos=(nan, 0.0, 0.0)), obs(pos=(1.0001e6, 0.0, 0.0)), obs(pos=(0.0, -1.0, 0.0)), obs(pos=(0.0, 100001.0, 0.0)), obs(cap=0.0), obs(cap=nan)]
    for k, o in enumerate(bad_o):
        for f in forms:
            assert f(o=o) == INV, (k, f.__name__)
    bare = pkg.Context(0)
    try:
        bh = bare._h
        assert all(f(ctx=bh) == STATE for f in forms)
        assert b"csky_set_noise" in L.csky_last_error(bh)
        for f, mk in ((vhost, hdepth), (dhost, hdepth), (vdev, ddepth), (ddev, ddepth)):     # INVALID comes before STATE
            assert f(ctx=bh, o=bad_o[0]) == INV and f(ctx=bh, z=None) == INV and f(ctx=bh, z=mk(kind=2)) == INV and f(ctx=bh, z=mk(pitch=60)) == INV, f.__name__
        assert vdev(ctx=bh, z=ddepth(texels=dptr)) == INV and dhost(ctx=bh, z=hdepth(kind=1)) == INV
        bare.set_noise(*noise)
        assert all(f(ctx=bh) == STATE for f in forms)
        assert b"sky LUT" in L.csky_last_error(bh)
        with pytest.raises(pkg.CloudSkyError) as e:
            bare.render_clouds_view_from_depth(scene_a, RR.camera_basis(-30.0, V["yaw"]), 70.0, 16, 16, (0.0, 8000.0, 0.0), zt)
        assert e.value.code == STATE
        bare.render_transmittance(256, 64)
        bare.render_sky_lut(np.asarray(scene_a[16:19], np.float32), 200, 100)
        assert vhost(ctx=bh) == OK and dhost(ctx=bh) == OK
    finally:
        bare.close()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- G8
def striped():
    """float32 [36, 64]: column i holds TEXELS[i % 9]"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(TEXELS, F)[np.arange(64) % len(TEXELS)], (36, 64)))


@pytest.mark.parametrize("name,buffer", [("inside", "striped"), ("above_down", "striped"), ("offset", "t0 + 2 ulp")])
def test_texel_values_are_the_per_pixel_rule(whole_ctx, oracle, depth_host, chains, name, buffer):  # noqa: F811
    """NaN, zeros, negatives, denormals, a millimetre and +inf side by side, and a buffer whose every texel sits two ulps behind its ray's t0
    (tests/test_scene_depth_host.py D4 holds that one on the CPU first): what the restatement does not march is a zero texel, every half is finite,
    the rest is the host core's."""
    p = bind(whole_ctx, oracle)
    pos, cap, _, _, _, _ = OB.observer(name)
    d = OB.dirs(name)
    if buffer == "striped":
        z = striped()
    else:
        t0, _, has = OR.segment(pos, cap, d)
        z = advance(np.where(has & (t0 > 0), t0, F(0.0)).astype(F), 2)
    want = DR.ray(pos, cap, d, z, MARCH["A"][0])
    marched = want[..., 10] > 0
    assert np.isfinite(want).all() and marched.any() and (~marched).any()
    got = view_depth(whole_ctx, p, name, z)
    assert np.isfinite(got.astype(F)).all()
    assert not bits(got)[~marched].any()
    core, cm, _ = host_march_depth(depth_host, chains, p, whole_ctx.read_sky_lut(), pos, cap, d, z)
    assert (cm == marched).all()
    ok, info = cloud_tight(got, core)
    print("%s, %s: %d of %d pixels marched; vs host core: %s" % (name, buffer, marched.sum(), marched.size, info))
    assert ok, info
    if buffer == "striped":
        free = view_from(whole_ctx, p, name)
        col = np.arange(64) % len(TEXELS) == TEXELS.index(INF)
        assert (bits(got)[:, col] == bits(free)[:, col]).all() and bits(got)[:, col].any()    # the +inf columns: the _from form's bytes
        assert (bits(whole_ctx.render_clouds_dirs_from_depth(p, d, pos, z, max_distance=cap)) == bits(got)).all()


# ---------------------------------------------------------------------------------------------------------------- G9
def test_python_mirror(pkg, noise):
    """CloudSky.cloud_view(scene_depth=...) is the C call fed the same frame; without a scene depth it is what it was."""
    import torch
    pos, cap, basis, fov, w, h = OB.observer("above_down")
    z = SD.mixed("above_down")
    zv = DR.view_z(cam_of("above_down"), OB.dirs("above_down"), z)
    for device_buffers in (True, False):
        sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=device_buffers)
        try:
            sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
            sky.update_sky()
            pc = sky._fill_push_constant()

            def mine(a):
                return torch.from_numpy(a).cuda() if device_buffers else a

            def host(t):
                assert isinstance(t, torch.Tensor) == device_buffers
                return t.cpu().numpy() if device_buffers else t
            cv = host(sky.cloud_view(basis, fov, w, h, position=pos, max_distance=cap, scene_depth=mine(z)))
            assert cv.shape == (h, w, 4) and cv.dtype == np.float16 and (cv[..., 3] > 0).mean() >= 0.1
            assert (bits(cv) == bits(sky.ctx.render_clouds_view_from_depth(pc, basis, fov, w, h, pos, z, "distance", cap))).all()
            plain = host(sky.cloud_view(basis, fov, w, h, position=pos, max_distance=cap))
            assert (bits(plain) == bits(sky.ctx.render_clouds_view_from(pc, basis, fov, w, h, pos, cap))).all() and (bits(plain) != bits(cv)).any()
            vz = host(sky.cloud_view(basis, fov, w, h, position=pos, scene_depth=mine(zv), depth_kind="view_z"))
            assert (bits(vz) == bits(sky.ctx.render_clouds_view_from_depth(pc, basis, fov, w, h, pos, zv, "view_z"))).all()
            ground = host(sky.cloud_view(basis, fov, w, h, scene_depth=mine(np.full((h, w), INF, F))))      # no position beside a depth: (0, 0, 0)
            assert (bits(ground) == bits(sky.ctx.render_clouds_view_from(pc, basis, fov, w, h, (0.0, 0.0, 0.0)))).all()
            same = host(sky.cloud_view(RR.camera_basis(V["pitch"], V["yaw"]), V["fov"], V["width"], V["height"]))
            assert (bits(same) == bits(sky.ctx.render_clouds_view(pc, RR.camera_basis(V["pitch"], V["yaw"]), V["fov"], V["width"], V["height"]))).all()
            with pytest.raises(ValueError):
                sky.cloud_view(basis, fov, w, h, aerial=True, scene_depth=mine(z))
        finally:
            sky.close()
