"""The temporal split of a view frame (csky_render_clouds_view_update and its _device form; csrc/view_update_core.h, cloud_kernels.hip
clouds_view_fresh_kernel / clouds_view_reproject_kernel) on the GPU through the C ABI.  Marched pixels are held to csky_render_clouds_view_device byte
for byte (the same Ray, the same march_compact), tapped pixels to the host core's taps (tests/view_update_host), and which pixel is which to the numpy
restatement of the definition (tests/view_update_reference.py).  Then what a launch may touch, what it leaves of the context's state, every error
path, and the Python mirror.

The cameras: clouds_rays_reference.VIEW (64 x 36, fov 70, pitch 25, yaw 40) and the moved one (pitch +4, yaw +8).  Every test on the moved camera
asserts from the reference alone that holes are 5..40 % and tapped pixels >= 30 % of the image."""
import ctypes as C

import numpy as np
import pytest

import clouds_rays_reference as RR
import shadow_reference as SR
import view_update_reference as VU
from test_view_update_host import assert_moved_shares, core_tap, vu_host  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu
GUARD = 3                           # guard rows before and after an image
V = RR.VIEW
W, H, FOV = V["width"], V["height"], V["fov"]
BASIS = RR.camera_basis(V["pitch"], V["yaw"])
MOVED = RR.camera_basis(VU.MOVED["pitch"], VU.MOVED["yaw"])
MARCH = {"A": (128, 6), "B": (30, 4)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def with_lut(ctx, p):
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(np.asarray(p[16:19], np.float32), 200, 100)


def full_view(ctx, p, basis, w=W, h=H, fov=FOV):
    """csky_render_clouds_view_device's frame, on the host"""
    import torch
    out = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    ctx.render_clouds_view(p, basis, fov, w, h, out=out)
    ctx.sync()
    return out.cpu().numpy()


def update(ctx, form, p, basis, block, phase, prev=None, prev_basis=None, w=W, h=H, fov=FOV, prev_fov=FOV):
    """one update through the device or the host form; prev and the result are numpy float16 [h, w, 4]"""
    if form == "host":
        return ctx.render_clouds_view_update(p, basis, fov, w, h, block, phase, prev=prev, prev_basis=prev_basis, prev_fov=prev_fov)
    import torch
    out = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
    dp = None if prev is None else torch.from_numpy(np.ascontiguousarray(prev)).cuda()
    torch.cuda.synchronize()
    got = ctx.render_clouds_view_update(p, basis, fov, w, h, block, phase, prev=dp, prev_basis=prev_basis, prev_fov=prev_fov, out=out)
    assert got is out
    ctx.sync()
    if dp is not None:
        assert (bits(dp.cpu().numpy()) == bits(prev)).all()       # the previous frame is left as it was
    return out.cpu().numpy()


def marked_frame(h=H, w=W):
    """recognisable non-zero bytes: every half is 0x2000 + its own index (no zero, no NaN, no two alike)"""
    return (0x2000 + np.arange(h * w * 4, dtype=np.uint16)).reshape(h, w, 4).view(np.float16)


@pytest.fixture(scope="module")
def ctx(pkg, noise):
    if pkg.lib().csky_device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible (libcloudsky has no CPU fallback)")
    c = pkg.Context(0)
    c.set_noise(*noise)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exact_ctx(pkg, noise):
    """exact-cells mode: the march on TexSet32"""
    c = pkg.Context(0)
    c.set_exact_cells(1)
    c.set_noise(*noise)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene_a(ctx, oracle):
    """scene A at 128 x 6 with its LUT: (params, the full view frames of the still and the moved camera)"""
    p = SR.scene(oracle, "A")
    ctx.set_march(*MARCH["A"])
    with_lut(ctx, p)
    return p, {"still": full_view(ctx, p, BASIS), "moved": full_view(ctx, p, MOVED)}


# ---------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("exact", [False, True], ids=["fp16-cells", "exact-cells"])
def test_no_history_and_block_one_give_the_bytes_of_the_full_view(ctx, exact_ctx, oracle, name, exact, form):
    c = exact_ctx if exact else ctx
    p = SR.scene(oracle, name)
    c.set_march(*MARCH[name])
    try:
        with_lut(c, p)
        want = full_view(c, p, BASIS)
        assert (want[..., 3] > 0).mean() >= 0.25 and not bits(want)[RR.view_dirs(BASIS, FOV, W, H)[..., 1] <= 0].any()
        got = update(c, form, p, BASIS, 4, 7)                                  # prev = NULL
        differ = int((bits(got) != bits(want)).sum())
        poison = np.full((H, W, 4), 0xFFFF, np.uint16).view(np.float16)
        one = update(c, form, p, BASIS, 1, 0, prev=poison, prev_basis=MOVED)   # B = 1: every pixel is fresh
        differ1 = int((bits(one) != bits(want)).sum())
        print("scene %s, %s, %s form: %d (no history) and %d (B = 1) of %d halves differ from csky_render_clouds_view_device" % (
            name, "exact" if exact else "fp16", form, differ, differ1, want.size))
        assert differ == 0 and differ1 == 0
    finally:
        c.set_march(*MARCH["A"])
        if c is ctx:
            with_lut(c, SR.scene(oracle, "A"))                                  # scene_a's LUT again


# ---------------------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("form", ["device", "host"])
def test_still_camera_copies_and_converges(ctx, scene_a, form):
    p, full = scene_a
    want, prev = full["still"], marked_frame()
    for phase in (0, 5, 15):
        kind = VU.classify(BASIS, FOV, BASIS, FOV, W, H, 4, phase)["kind"]
        got = update(ctx, form, p, BASIS, 4, phase, prev=prev, prev_basis=BASIS)
        fresh, zero, copy = kind == VU.FRESH, kind == VU.ZERO, kind == VU.COPY
        assert fresh.sum() > 0 and zero.sum() > 0 and copy.sum() > 0.5 * W * H and (fresh | zero | copy).all()
        assert (bits(got)[fresh] == bits(want)[fresh]).all()
        assert not bits(got)[zero].any()
        assert (bits(got)[copy] == bits(prev)[copy]).all()
    frame = np.zeros((H, W, 4), np.float16)
    order = VU.bayer_phases(4)
    assert sorted(order) == list(range(16))
    for phase in order:
        frame = update(ctx, form, p, BASIS, 4, phase, prev=frame, prev_basis=BASIS)
    differ = int((bits(frame) != bits(want)).sum())
    print("%s form, sixteen calls from zeros: %d of %d halves differ from the full view" % (form, differ, want.size))
    assert differ == 0


# ---------------------------------------------------------------------------------------------------------------- G3
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("block,phase", [(4, 0), (4, 5), (4, 15), (2, 1)])
def test_moved_camera_marches_taps_and_finds_the_reference_holes(ctx, scene_a, vu_host, form, block, phase):  # noqa: F811
    p, full = scene_a
    prev, want = full["still"], full["moved"]
    ref = VU.classify(MOVED, FOV, BASIS, FOV, W, H, block, phase)
    kind = ref["kind"]
    assert_moved_shares(kind)
    got = update(ctx, form, p, MOVED, block, phase, prev=prev, prev_basis=BASIS)
    marched, tapped = (kind == VU.FRESH) | (kind == VU.HOLE), kind == VU.TAP
    d_march = int((bits(got)[marched] != bits(want)[marched]).sum())
    taps = core_tap(vu_host, prev, ref["ux"][tapped], ref["uy"][tapped])
    d_tap = int((bits(got)[tapped] != bits(taps)).sum())
    print("B = %d phase %d, %s form: %d of %d marched halves differ from the full view, %d of %d tapped halves from the host core's taps" % (
        block, phase, form, d_march, 4 * marched.sum(), d_tap, 4 * tapped.sum()))
    assert d_march == 0 and d_tap == 0
    assert not bits(got)[kind == VU.ZERO].any()
    assert (taps[..., 3] > 0).mean() > 0.25                           # the taps read a frame with clouds in it
    # which pixels are holes: a previous frame of (2, 2, 2, 2) shows in every pixel taken from it (a tap of equal texels is that texel, and no march
    # gives alpha 2)
    twos = np.full((H, W, 4), 0x4000, np.uint16).view(np.float16)
    seen = update(ctx, form, p, MOVED, block, phase, prev=twos, prev_basis=BASIS)
    from_prev = (bits(seen) == 0x4000).all(-1)
    assert (from_prev == tapped).all(), np.argwhere(from_prev != tapped)[:4]
    holes = ~from_prev & (kind != VU.ZERO) & (kind != VU.FRESH)
    assert (holes == (kind == VU.HOLE)).all()
    assert (bits(seen)[~from_prev] == np.where((kind != VU.ZERO)[..., None], bits(want), 0)[~from_prev]).all()


# ---------------------------------------------------------------------------------------------------------------- G4
@pytest.mark.parametrize("w,h,block,phases", [(37, 21, 4, (0, 7)), (1, 1, 4, (0, 9)), (5, 3, 8, (0, 4, 5, 24, 63))], ids=["37x21", "1x1", "5x3-B8"])
@pytest.mark.parametrize("pads", [(0, 0), (24, 0), (0, 24), (24, 24)], ids=["tight", "prev-pitched", "out-pitched", "both-pitched"])
def test_write_coverage(ctx, scene_a, w, h, block, phases, pads):
    """The device form into a tensor of 0xFFFF halfs (a NaN no frame contains) with guard rows and row padding, from a previous frame likewise."""
    import torch
    p, _ = scene_a
    prev = full_view(ctx, p, BASIS, w, h)
    s = torch.cuda.Stream()
    for phase in phases:
        host = update(ctx, "host", p, MOVED, block, phase, prev=prev, prev_basis=BASIS, w=w, h=h)
        assert not (bits(host) == 0xFFFF).any()
        kind = VU.classify(MOVED, FOV, BASIS, FOV, w, h, block, phase)["kind"]
        if w > 1:
            assert len(np.unique(bits(host))) > 8
        else:
            assert kind[0, 0] == (VU.FRESH if phase == 0 else VU.HOLE) and bits(host).any()   # the single ray looks up and is marched either way
        for stream in (s.cuda_stream, None):
            with torch.cuda.stream(s):
                bufs = []
                for pad in pads:
                    t = torch.empty((h + 2 * GUARD, (8 * w + pad) // 2), dtype=torch.int16, device="cuda")
                    t.fill_(-1)
                    bufs.append(t)
                tp, to = bufs
                sp, so = (t[GUARD:GUARD + h, :4 * w].unflatten(1, (w, 4)) for t in bufs)
                sp.copy_(torch.from_numpy(bits(prev).view(np.int16)).cuda())
                before = tp.cpu().numpy().copy()
                s.synchronize()                                      # the NULL form runs on the context's own stream
                out = ctx.render_clouds_view_update(p, MOVED, FOV, w, h, block, phase, prev=sp, prev_basis=BASIS, prev_fov=FOV, out=so, stream=stream)
                assert out is so
                if stream is None:
                    ctx.sync()
                got = to.cpu().numpy().view(np.uint16)
                assert (tp.cpu().numpy() == before).all()             # prev unchanged, padding and guard rows included
            inside = np.zeros(got.shape, bool)
            inside[GUARD:GUARD + h, :4 * w] = True
            assert not (got[inside] == 0xFFFF).any()
            assert (got[~inside] == 0xFFFF).all(), np.argwhere(~inside & (got != 0xFFFF))[:4]
            assert (got[GUARD:GUARD + h, :4 * w].reshape(h, w, 4) == bits(host)).all()


# ---------------------------------------------------------------------------------------------------------------- G5
def test_cloud_frames_luts_and_the_full_view_are_what_they_were(pkg, noise, oracle):
    """Two frames in flight on two streams: three cloud frames with update calls before, between and after them are the frames without."""
    import torch
    c = pkg.Context(0)
    try:
        c.set_noise(*noise)
        c.set_frames_in_flight(2)
        pa = SR.scene(oracle, "A")
        with_lut(c, pa)
        lut, tr = c.read_sky_lut().copy(), c.read_transmittance().copy()
        view_before = c.render_clouds_view(pa, BASIS, FOV, W, H).copy()
        blocks = []
        for k in range(3):
            q = oracle.default_params(128, 64, (1, 1, 0))
            q[4:6] = (0.5 * k, -0.25 * k)
            q[23] = 3.0 * k
            blocks.append(q)
        pb = SR.scene(oracle, "B")
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        prev = torch.from_numpy(view_before).cuda()

        def run(with_updates):
            frames = [torch.zeros((64, 128, 4), dtype=torch.float16, device="cuda") for _ in blocks]
            views = [torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(4 if with_updates else 0)]
            torch.cuda.synchronize()

            def upd(k, s):
                c.render_clouds_view_update(pb, MOVED, FOV, W, H, 4, 5, prev=prev, prev_basis=BASIS, prev_fov=FOV, out=views[k], stream=s.cuda_stream)
            if with_updates:
                upd(0, streams[1])
            for k, q in enumerate(blocks):
                s = streams[k % 2]
                if with_updates and k > 0:                         # on the stream of the frame still in flight, beside the one about to start
                    upd(k, streams[(k + 1) % 2])
                c.render_clouds_device(q, 128, (8, 0, 1, 8), frames[k].data_ptr(), 128 * 8, s.cuda_stream)
            if with_updates:
                upd(3, streams[0])
            torch.cuda.synchronize()
            return [f.cpu().numpy() for f in frames], [v.cpu().numpy() for v in views]
        plain, _ = run(False)
        mixed, views = run(True)
        again, _ = run(False)
        for a, b, d in zip(plain, mixed, again):
            assert bits(a).any() and (bits(a) == bits(b)).all() and (bits(a) == bits(d)).all()
        assert len(views) == 4 and all((bits(v) == bits(views[0])).all() for v in views) and (views[0][..., 3] > 0).any()
        assert (bits(views[0]) == bits(c.render_clouds_view_update(pb, MOVED, FOV, W, H, 4, 5, prev=view_before, prev_basis=BASIS, prev_fov=FOV))).all()
        assert (bits(c.read_sky_lut()) == bits(lut)).all() and (bits(c.read_transmittance()) == bits(tr)).all()
        assert (bits(c.render_clouds_view(pa, BASIS, FOV, W, H)) == bits(view_before)).all()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- G6
def test_error_paths(pkg, ctx, scene_a, noise):
    """Every CSKY_ERR_INVALID and CSKY_ERR_STATE case of the header, by return code."""
    import torch
    L, lib = pkg.lib(), pkg._lib
    h = ctx._h
    INV, STATE, OK = lib.ERR_INVALID, lib.ERR_STATE, lib.OK
    nan, inf = float("nan"), float("inf")
    p = lib.cloud_params(scene_a[0])
    out, prev = np.zeros((16, 16, 4), np.uint16), np.zeros((16, 16, 4), np.uint16)
    optr, pptr = out.ctypes.data_as(C.c_void_p), prev.ctypes.data_as(C.c_void_p)
    d = torch.zeros((2, 16, 32, 4), dtype=torch.int16, device="cuda")          # two images of pitch 256
    dout, dprev = d[0].data_ptr(), d[1].data_ptr()

    def view(basis=RR.column_major(BASIS), fov=70.0):
        return lib.View((C.c_float * 9)(*[float(x) for x in basis]), fov)

    def ref(x):
        return C.byref(x) if x is not None else None

    def host(c=h, params=p, v=view(), pv=view(), w=16, hh=16, block=4, phase=5, pr=pptr, o=optr):
        return L.csky_render_clouds_view_update(c, ref(params), ref(v), ref(pv), w, hh, block, phase, pr, o)

    def dev(c=h, params=p, v=view(), pv=view(), w=16, hh=16, block=4, phase=5, pr=dprev, ppitch=256, o=dout, pitch=256):
        return L.csky_render_clouds_view_update_device(c, ref(params), ref(v), ref(pv), w, hh, block, phase, C.c_void_p(pr) if pr else None, ppitch,
                                                       C.c_void_p(o) if o else None, pitch, None)

    assert L.csky_render_clouds_view_update(None, None, None, None, 0, 0, 0, 0, None, None) != OK     # all-zero arguments
    assert L.csky_render_clouds_view_update_device(None, None, None, None, 0, 0, 0, 0, None, 0, None, 0, None) != OK
    assert host() == OK and dev() == OK and dev(ppitch=128, pitch=136) == OK
    assert host(pr=None, pv=None) == OK and dev(pr=None, pv=None, ppitch=0) == OK and dev(pr=None, pv=view(fov=nan), ppitch=7) == OK   # no history: neither is read
    for block in (1, 8):
        assert host(block=block, phase=block * block - 1) == OK and dev(block=block, phase=block * block - 1) == OK
    ctx.sync()
    assert host(c=None) == INV and host(params=None) == INV and host(v=None) == INV and host(o=None) == INV
    assert dev(c=None) == INV and dev(params=None) == INV and dev(v=None) == INV and dev(o=None) == INV
    for block, phase in ((0, 0), (9, 0), (-1, 0), (4, 16), (4, -1), (1, 1), (8, 64), (2, 4)):
        assert host(block=block, phase=phase) == INV and dev(block=block, phase=phase) == INV, (block, phase)
    assert b"block" in L.csky_last_error(h)
    assert host(pv=None) == INV and dev(pv=None) == INV                                               # a previous frame without its view
    for w, hh in ((0, 16), (8193, 16), (16, 0), (16, 8193), (-1, 16), (16, -1)):
        assert host(w=w, hh=hh) == INV and dev(w=w, hh=hh, pitch=8 * 8193, ppitch=8 * 8193) == INV, (w, hh)
    for pitch in (120, 132, 0):
        assert dev(pitch=pitch) == INV and dev(ppitch=pitch) == INV, pitch
    assert b"pitch" in L.csky_last_error(h)
    for k in range(9):
        for bad in (nan, inf, -inf):
            b = RR.column_major(BASIS).copy()
            b[k] = bad
            assert host(v=view(basis=b)) == INV and dev(v=view(basis=b)) == INV and host(pv=view(basis=b)) == INV and dev(pv=view(basis=b)) == INV, (k, bad)
    for fov in (0.0, 180.0, -1.0, 200.0, nan, inf):
        assert host(v=view(fov=fov)) == INV and dev(v=view(fov=fov)) == INV and host(pv=view(fov=fov)) == INV and dev(pv=view(fov=fov)) == INV, fov
    # overlap: the same image, one row on (pitch 256: the last row of out is the first of prev + 15 rows), one texel inside, and the interleaved halves of one allocation
    assert host(pr=optr) == INV and dev(pr=dout) == INV
    assert dev(pr=dout + 15 * 256 + 120) == INV and dev(pr=dout - 15 * 256 - 120) == INV
    assert dev(pr=dout + 128, w=16, ppitch=256, pitch=256) == INV                                      # disjoint texels, overlapping byte ranges
    assert b"overlap" in L.csky_last_error(h)
    assert dev(pr=dout + 15 * 256 + 128, hh=16) == OK                                                  # ends where the other begins
    ctx.sync()
    bare = pkg.Context(0)
    try:
        b = bare._h
        assert host(c=b) == STATE and dev(c=b) == STATE
        assert b"csky_set_noise" in L.csky_last_error(b)
        assert host(c=b, block=0) == INV and dev(c=b, pr=dout) == INV                                  # a bad argument is INVALID whatever the context holds
        bare.set_noise(*noise)
        assert host(c=b) == STATE and dev(c=b) == STATE
        assert b"sky LUT" in L.csky_last_error(b)
        with_lut(bare, scene_a[0])
        assert host(c=b) == OK
    finally:
        bare.close()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- G7
@pytest.mark.parametrize("device_buffers", [True, False], ids=["device", "host"])
def test_python_mirror(pkg, noise, device_buffers):
    """CloudSky.cloud_view_temporal is the C calls in the Bayer order; B * B calls on a still camera are cloud_view; a size change drops the history."""
    import torch

    def host(t):
        return (t.cpu().numpy() if hasattr(t, "cpu") else t).copy()
    sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=device_buffers)
    try:
        sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
        sky.update_sky()
        pc = sky._fill_push_constant()
        assert pkg.CloudSky.temporal_phases(4) == VU.bayer_phases(4) and pkg.CloudSky.temporal_phases(2) == [0, 3, 1, 2] and pkg.CloudSky.temporal_phases(1) == [0]
        for b in (2, 8):
            assert sorted(pkg.CloudSky.temporal_phases(b)) == list(range(b * b)) and pkg.CloudSky.temporal_phases(b) == VU.bayer_phases(b)
        full = {name: host(sky.cloud_view(b, FOV, W, H)) for name, b in (("still", BASIS), ("moved", MOVED))}
        assert (full["still"][..., 3] > 0).mean() >= 0.1
        # the first call has no history: the full view; the second, with a moved camera, is the C call fed the first
        first = sky.cloud_view_temporal(BASIS, FOV, W, H, block=2)
        assert isinstance(first, torch.Tensor) == device_buffers
        first = host(first)
        assert (bits(first) == bits(full["still"])).all()
        second = host(sky.cloud_view_temporal(MOVED, FOV, W, H, block=2))
        want = sky.ctx.render_clouds_view_update(pc, MOVED, FOV, W, H, 2, VU.bayer_phases(2)[1], prev=first, prev_basis=BASIS, prev_fov=FOV)
        assert (bits(second) == bits(want)).all() and (bits(second) != bits(full["moved"])).any()
        # a size change drops the history: the next frame is the full view of its size
        small = host(sky.cloud_view_temporal(MOVED, FOV, 37, 21, block=2))
        assert (bits(small) == bits(host(sky.cloud_view(MOVED, FOV, 37, 21)))).all()
        # so does a change of block; then B * B calls on a still camera, the first of them fed a frame of another camera, are cloud_view
        assert (bits(host(sky.cloud_view_temporal(MOVED, FOV, 37, 21, block=4))) == bits(small)).all()
        sky.cloud_view_temporal(MOVED, FOV, W, H, block=4)
        for _ in range(16):
            last = sky.cloud_view_temporal(BASIS, FOV, W, H, block=4)
        assert (bits(host(last)) == bits(full["still"])).all()
        sky.cleanup()                                                 # drops it as well
        assert (bits(host(sky.cloud_view_temporal(MOVED, FOV, W, H, block=4))) == bits(full["moved"])).all()
        with pytest.raises(ValueError):
            sky.cloud_view_temporal(BASIS, FOV, W, H, block=3)
    finally:
        sky.close()
