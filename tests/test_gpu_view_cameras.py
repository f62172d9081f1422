"""The view forms (csky_render_clouds_view, csky_render_cloud_depth_view, csky_apply_cloud_aerial_view) and the temporal split
(csky_render_clouds_view_update and its _device form) on the GPU at the cameras of tests/view_cameras.py: rolled, zoomed between two frames,
portrait, at the horizon and the zenith, a previous camera that looks elsewhere, very narrow, very wide, a fresh sub-grid three workgroups wide.
Scene A at 128 x 6.  Every gate is "0 halves differ": marched pixels against csky_render_clouds_view_device of the same camera, tapped pixels
against numpy's view_update_reference.tap, which pixel is which against view_update_reference.classify, the view forms against the dirs forms fed
clouds_rays_reference.view_dirs.  What each case is there for is asserted from the reference alone before anything is compared."""
import numpy as np
import pytest

import clouds_rays_reference as RR
import shadow_reference as SR
import view_cameras as VC
import view_update_reference as VU
from test_gpu_cloud_aerial import ctxs  # noqa: F401  (module-scoped fixture)
from test_gpu_view_update import GUARD, MARCH, bits, ctx, full_view, scene_a, update, with_lut  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu
FORMS = ["device", "host"]


@pytest.fixture(scope="module")
def frames(ctx, scene_a):  # noqa: F811
    """scene A's full view frame (csky_render_clouds_view_device) of a camera, marched once per module: get(basis, fov, w, h)"""
    p, _ = scene_a
    cache = {}

    def get(basis, fov, w, h):
        k = (basis.tobytes(), float(fov), w, h)
        if k not in cache:
            cache[k] = full_view(ctx, p, basis, w, h, fov)
        return cache[k].copy()                                       # the cached frame stays as it was marched
    return get


# ---------------------------------------------------------------------------------------------------------------- C1
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("block,phase", VC.PAIRS)
@pytest.mark.parametrize("name", VC.NAMES)
def test_update_is_the_composition_of_the_full_views_at_every_camera(ctx, scene_a, frames, name, block, phase, form):  # noqa: F811
    p, _ = scene_a
    b, fov, pb, pfov, w, h = VC.views(name)
    VC.assert_shares(name)
    ref = VU.classify(b, fov, pb, pfov, w, h, block, phase)
    kind = ref["kind"]
    tapped = kind == VU.TAP
    print("%s B = %d phase %d, %s form: %s" % (name, block, phase, form, VC.counts(kind)))
    prev, want_full = frames(pb, pfov, w, h), frames(b, fov, w, h)
    if name == "horizon":                                            # taps over a previous frame with zero texels in it, and across their rim
        zero = ~bits(prev).any(-1)
        mixed = VC.mixed_zero_taps(prev, ref["ux"][tapped], ref["uy"][tapped])
        print("horizon: %.1f %% of the previous frame's texels are zero; %.1f %% of the taps read a zero and a non-zero texel" % (100 * zero.mean(), 100 * mixed.mean()))
        assert zero.mean() >= 0.30 and mixed.mean() >= 0.05
    want = VU.compose(ref, want_full, prev)
    got = update(ctx, form, p, b, block, phase, prev=prev, prev_basis=pb, w=w, h=h, fov=fov, prev_fov=pfov)
    marched = (kind == VU.FRESH) | (kind == VU.HOLE)
    d_march, d_tap = int((bits(got)[marched] != bits(want)[marched]).sum()), int((bits(got)[tapped] != bits(want)[tapped]).sum())
    print("%d of %d marched halves differ from the full view, %d of %d tapped halves from numpy's taps" % (d_march, 4 * marched.sum(), d_tap, 4 * tapped.sum()))
    assert d_march == 0 and d_tap == 0
    assert (bits(got) == bits(want)).all()                           # and the zeros
    assert (want_full[..., 3] > 0).mean() >= 0.25                    # frames with clouds in them
    # which pixels come from the previous frame: (2, 2, 2, 2) shows in every pixel taken from it (a tap of equal texels is that texel, and no march
    # gives alpha 2).  Where the previous camera has pixels behind it (view_cameras.MIRRORED) this holds the `front` test.
    twos = np.full((h, w, 4), 0x4000, np.uint16).view(np.float16)
    seen = update(ctx, form, p, b, block, phase, prev=twos, prev_basis=pb, w=w, h=h, fov=fov, prev_fov=pfov)
    from_prev = (bits(seen) == 0x4000).all(-1)
    assert (from_prev == tapped).all(), np.argwhere(from_prev != tapped)[:4]
    assert (bits(seen)[~from_prev] == bits(want)[~from_prev]).all()


# ---------------------------------------------------------------------------------------------------------------- C2
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["roll-both", "zoom-out"])
def test_taps_of_halves_no_cloud_frame_holds(ctx, scene_a, name, form):  # noqa: F811
    """The device's h2f / lerp / f2h chain over finite halves of both signs, subnormals and +-65504 (view_cameras.edge_frame), against numpy's.
    This is the test that found the device's lerp fused into an fma: 1 to 5 of some 4 800 tapped halves differed in the last bit."""
    p, _ = scene_a
    b, fov, pb, pfov, w, h = VC.views(name)
    prev = VC.edge_frame(h, w, 0)
    assert np.isfinite(prev.astype(np.float32)).all()
    for block, phase in VC.PAIRS:
        ref = VU.classify(b, fov, pb, pfov, w, h, block, phase)
        tapped = ref["kind"] == VU.TAP
        want = VU.tap(prev, ref["ux"][tapped], ref["uy"][tapped])
        sub, neg, big = VC.tap_edge_shares(want)
        assert tapped.mean() >= 0.20 and sub >= 0.01 and neg >= 0.20 and big >= 1
        got = update(ctx, form, p, b, block, phase, prev=prev, prev_basis=pb, w=w, h=h, fov=fov, prev_fov=pfov)
        differ = int((bits(got)[tapped] != bits(want)).sum())
        print("%s B = %d phase %d, %s form: %d of %d tapped halves differ from numpy's taps (expected: %.1f %% subnormal, %.1f %% negative, %d at 0x7BFF or above)" % (
            name, block, phase, form, differ, want.size, 100 * sub, 100 * neg, big))
        assert differ == 0


# ---------------------------------------------------------------------------------------------------------------- C3
def run_chain(march, step):
    """The forty cameras of view_cameras.chain_cameras: step(n, basis, fov, phase) is call n of the chain under test (fed its own frame before),
    march(basis, fov) the full view.  Every frame must be the numpy composition of the full view and the COMPOSITION's own frame before."""
    W, H = RR.VIEW["width"], RR.VIEW["height"]
    cams = VC.chain_cameras()
    order = VU.bayer_phases(4)
    frame, last, holes, out = None, None, 0, []
    for n, (b, fov) in enumerate(cams):
        phase = order[n % 16]
        ref = VU.classify(b, fov, None if last is None else last[0], None if last is None else last[1], W, H, 4, phase)
        kind = ref["kind"]
        full = march(b, fov)
        if n == 0:
            assert not ((kind == VU.TAP) | (kind == VU.COPY)).any()
        elif n < VC.CHAIN_MOVING:
            assert (kind == VU.TAP).mean() >= 0.40 and not (kind == VU.COPY).any()
            holes += int((kind == VU.HOLE).sum())
        else:
            assert (kind == VU.COPY).mean() >= 0.80 and not ((kind == VU.TAP) | (kind == VU.HOLE)).any()
        frame = VU.compose(ref, full, frame)
        got = step(n, b, fov, phase)
        differ = int((bits(got) != bits(frame)).sum())
        print("call %2d phase %2d: %s; %d of %d halves differ from the composition" % (n, phase, VC.counts(kind), differ, got.size))
        assert differ == 0
        out.append(got)
        last = (b, fov)
    assert holes > 0 and (full[..., 3] > 0).mean() >= 0.10
    assert (bits(out[-1]) == bits(full)).all()                       # sixteen calls on the last camera: its full view
    assert (bits(out[VC.CHAIN_MOVING - 1]) != bits(full)).any()      # which the last moving frame is not
    return out


def c_chain(c, p):
    """the chain through csky_render_clouds_view_update_device on two alternating tensors"""
    import torch
    W, H = RR.VIEW["width"], RR.VIEW["height"]
    bufs = [torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(2)]
    cams = VC.chain_cameras()
    torch.cuda.synchronize()

    def step(n, b, fov, phase):
        prev, pv = (None, (None, fov)) if n == 0 else (bufs[1 - n % 2], cams[n - 1])
        got = c.render_clouds_view_update(p, b, fov, W, H, 4, phase, prev=prev, prev_basis=pv[0], prev_fov=pv[1], out=bufs[n % 2])
        assert got is bufs[n % 2]
        c.sync()
        return got.cpu().numpy()
    return step


def test_chain_of_forty_calls_through_the_c_calls(ctx, scene_a, frames):  # noqa: F811
    p, _ = scene_a
    run_chain(lambda b, fov: frames(b, fov, RR.VIEW["width"], RR.VIEW["height"]), c_chain(ctx, p))


def test_chain_of_forty_calls_through_the_python_mirror(pkg, noise):
    """CloudSky.cloud_view_temporal gives the composition of its own cloud_view frames, and the frames of the C calls on its context."""
    W, H = RR.VIEW["width"], RR.VIEW["height"]
    sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=True)
    try:
        sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
        sky.update_sky()
        mirror = run_chain(lambda b, fov: sky.cloud_view(b, fov, W, H).cpu().numpy(), lambda n, b, fov, phase: sky.cloud_view_temporal(b, fov, W, H, block=4).cpu().numpy())
        c_step = c_chain(sky.ctx, sky._fill_push_constant())
        order = VU.bayer_phases(4)
        for n, (b, fov) in enumerate(VC.chain_cameras()):
            assert (bits(c_step(n, b, fov, order[n % 16])) == bits(mirror[n])).all(), n
    finally:
        sky.close()


# ---------------------------------------------------------------------------------------------------------------- C4
@pytest.mark.parametrize("block,phase,sub_w", [(2, 0, 80), (2, 3, 80), (1, 0, 160)])
@pytest.mark.parametrize("pads", [(0, 0), (24, 24)], ids=["tight", "both-pitched"])
def test_fresh_sub_grid_wider_than_one_workgroup(ctx, scene_a, frames, block, phase, sub_w, pads):  # noqa: F811
    """160 x 24: the fresh launch is three (B = 2: the last one ragged) or five (B = 1) workgroups wide.  The device form into a tensor of 0xFFFF
    halves with guard rows and row padding, from a previous frame likewise: inside, the host form's bytes; outside, nothing."""
    import torch
    p, _ = scene_a
    b, fov, pb, pfov, w, h = VC.views("wide-sub")
    assert len(range(phase % block, w, block)) == sub_w and (sub_w + 31) // 32 >= 3
    prev = frames(pb, pfov, w, h)
    ref = VU.classify(b, fov, pb, pfov, w, h, block, phase)
    host = update(ctx, "host", p, b, block, phase, prev=prev, prev_basis=pb, w=w, h=h, fov=fov, prev_fov=pfov).copy()
    assert (bits(host) == bits(VU.compose(ref, frames(b, fov, w, h), prev))).all()
    fresh = ref["kind"] == VU.FRESH
    assert bits(host)[fresh & (np.arange(w) >= 2 * 32 * block)[None, :]].reshape(-1, 4).any(-1).mean() >= 0.25   # the third workgroup's fresh pixels hold clouds
    s = torch.cuda.Stream()
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
        s.synchronize()
        out = ctx.render_clouds_view_update(p, b, fov, w, h, block, phase, prev=sp, prev_basis=pb, prev_fov=pfov, out=so, stream=s.cuda_stream)
        assert out is so
        got = to.cpu().numpy().view(np.uint16)
        assert (tp.cpu().numpy() == before).all()                    # prev unchanged, padding and guard rows included
    inside = np.zeros(got.shape, bool)
    inside[GUARD:GUARD + h, :4 * w] = True
    unwritten = (got[GUARD:GUARD + h, :4 * w].reshape(h, w, 4) == 0xFFFF).any(-1)
    assert not unwritten.any(), np.argwhere(unwritten)[:4]
    assert (got[~inside] == 0xFFFF).all(), np.argwhere(~inside & (got != 0xFFFF))[:4]
    assert (got[GUARD:GUARD + h, :4 * w].reshape(h, w, 4) == bits(host)).all()


# ---------------------------------------------------------------------------------------------------------------- C5
@pytest.mark.parametrize("name", VC.NAMES)
def test_view_forms_are_the_dirs_forms_fed_the_restatement_directions(ctx, ctxs, scene_a, frames, name):  # noqa: F811
    p, _ = scene_a
    b, fov, _, _, w, h = VC.views(name)
    d = RR.view_dirs(b, fov, w, h)
    ok = RR.accept(d)
    sun = np.asarray(p[16:19], np.float32)
    cv = ctx.render_clouds_view(p, b, fov, w, h).copy()
    cloudy = float((cv[..., 3] > 0)[ok].mean())
    differ = int((bits(cv) != bits(ctx.render_clouds_dirs(p, d))).sum())
    assert (bits(cv) == bits(frames(b, fov, w, h))).all() and not bits(cv)[~ok].any()
    z = ctx.render_cloud_depth_view(p, b, fov, w, h, MARCH["A"][0]).copy()
    differ_z = int((bits(z) != bits(ctx.render_cloud_depth_dirs(p, d, MARCH["A"][0]))).sum())
    print("%s: %.1f %% accepted, alpha > 0 in %.1f %% of them; %d of %d halves of the view frame and %d of the depth frame differ from the dirs forms" % (
        name, 100 * ok.mean(), 100 * cloudy, differ, cv.size, differ_z))
    assert cloudy >= 0.10 and (z[..., 3] > 0)[ok].mean() >= 0.10
    assert differ == 0 and differ_z == 0
    for mapping in (0, 1):
        air = ctxs[mapping].apply_cloud_aerial_view(sun, b, fov, cv, z, 16).copy()
        changed = float((bits(air) != bits(cv)).any(-1)[ok].mean())
        differ_a = int((bits(air) != bits(ctxs[mapping].apply_cloud_aerial_dirs(sun, d, cv, z, 16))).sum())
        print("%s, mapping %d: the aerial step changes %.1f %% of the accepted pixels; %d of %d halves differ from the dirs form" % (name, mapping, 100 * changed, differ_a, air.size))
        assert changed >= 0.20 and (bits(air)[~ok] == bits(cv)[~ok]).all()
        assert differ_a == 0


# ---------------------------------------------------------------------------------------------------------------- C6
def test_frame_constants_are_handed_from_one_rays_call_to_the_next(pkg, noise, oracle):
    """Every rays call writes its frame constants into the context's one block, and the next call's set-up waits for the march before it
    (api_rays.cpp rays_setup).  Four calls with two scenes' params are enqueued on two streams without a synchronization in between: a large view
    of scene A, a small one of B, an update of B, a small view of A; each must be what it is alone.
    What this test is: it passes on correct code whatever the timing, and it can catch a missing wait only when the second call's set-up lands
    inside the first call's march.  1280 x 720 is chosen for that: by ray count against the 1.19 ms the project measured for 1920 x 1080 the march
    takes about half a millisecond, against a few tens of microseconds to enqueue the next call.  That figure is scaled, not measured, and the
    test does not prove the wait is there.  Tried once on an MI355X against a scratch build without the wait, it passed: in a kernel trace of that
    run the march took 0.7 ms, but the second call's set-up started 0.6 ms after the march had ended, and the only set-up that ran inside a march
    (the update's, inside view(B)'s) wrote the same scene's bytes (profiles/r27/c6_without_the_wait_timeline.txt).  What the test does hold is
    that four calls with different params on two streams, enqueued back to back, each give their own bytes."""
    import torch
    W, H, FOV = RR.VIEW["width"], RR.VIEW["height"], RR.VIEW["fov"]
    BW, BH = 1280, 720
    cam, moved = VC.basis(RR.VIEW["pitch"], RR.VIEW["yaw"]), VC.basis(VU.MOVED["pitch"], VU.MOVED["yaw"])
    c = pkg.Context(0)
    try:
        c.set_noise(*noise)
        c.set_march(*MARCH["A"])
        pa, pb = SR.scene(oracle, "A"), SR.scene(oracle, "B")
        with_lut(c, pa)
        big, small_b, upd, small_a = (torch.zeros(shape, dtype=torch.float16, device="cuda") for shape in ((BH, BW, 4), (H, W, 4), (H, W, 4), (H, W, 4)))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()

        def calls(serial):
            def done():
                if serial:
                    torch.cuda.synchronize()
            c.render_clouds_view(pa, cam, FOV, BW, BH, out=big, stream=s1.cuda_stream); done()
            c.render_clouds_view(pb, cam, FOV, W, H, out=small_b, stream=s2.cuda_stream); done()
            c.render_clouds_view_update(pb, moved, FOV, W, H, 4, 5, prev=prev, prev_basis=cam, prev_fov=FOV, out=upd, stream=s1.cuda_stream); done()
            c.render_clouds_view(pa, cam, FOV, W, H, out=small_a, stream=s2.cuda_stream); done()
            torch.cuda.synchronize()
            return [t.cpu().numpy() for t in (big, small_b, upd, small_a)]
        prev = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
        c.render_clouds_view(pb, cam, FOV, W, H, out=prev, stream=s2.cuda_stream)   # the serial frame of B the update reads
        torch.cuda.synchronize()
        want = calls(True)
        assert (bits(want[1]) == bits(prev.cpu().numpy())).all()
        differ = float((bits(want[1]) != bits(want[3])).mean())
        print("scenes A and B through the same camera differ in %.1f %% of their halves" % (100 * differ))
        assert differ >= 0.20 and (want[0][..., 3] > 0).mean() >= 0.25 and (bits(want[2]) != bits(want[1])).any()
        for k in range(8):
            for t in (big, small_b, upd, small_a):
                t.zero_()
            torch.cuda.synchronize()
            got = calls(False)
            for what, g, x in zip(("view(A, 1280 x 720)", "view(B)", "update(B)", "view(A)"), got, want):
                n = int((bits(g) != bits(x)).sum())
                assert n == 0, "round %d, %s: %d of %d halves differ from the call alone" % (k, what, n, g.size)
    finally:
        c.close()
