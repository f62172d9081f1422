"""The direct cloud march from an observer's position (cloud_kernels.hip clouds_observer_kernel: observer_core.h observer_ray in front of
march_compact<..., RISING = false>) on the GPU, at the observers tests/test_gpu_observer.py never reaches (tests/observers.py EDGE): rays that enter
and leave through the top shell or dip and rise inside the layer, a cap that lies in front of the layer for some pixels and inside it for their
neighbours, 100 km up, 1000 km out, |o| exactly on a shell, and the rays observer_ray's last clause refuses (a max_distance within the fp32 quantum
of t0: before the clause a ray reported as marched with NaN fields).  Every frame is 64 x 36; the reference is the host core's march of the same
rays (tests/observer_host: the lock-step march(), no early end, nothing assumed about where a ray runs) at the gate for frames rendered from the
shipped assets (parity_metrics.cloud_tight).

Mutation check (done once on scratch builds of the library, not part of the suite; figures: pixels beyond the gate's 2 fp16 ulp, of 2 304):
  * clouds_observer_kernel instantiated with RISING = true (march_store<true>): G1 fails at above_graze (1 300 pixels in scene A, 281 in B, fp16 and
    exact cells alike), high_graze (1 260), high_down, far_above and on_top, 14 of its 21 cases, and G2's gate fails at above_graze and high_graze:
    a wavefront whose lanes all start above the window ends at once.  inside_dip passes, and must: its rays start inside the window, and a ray
    that dips and rises from there leaves through the top for good, so "every lane is above the window" is a correct end for it.  The rays that
    RISING = false exists for are the ones that start above the window: from above the layer.
  * observer_segment with a chord's end moved to its midpoint (`above`: t1 = (ht.near + ht.far) / 2 where hb.D < 0; `inside`: t1 = ht.far / 2 where
    b < 0 and hb.D < 0; finite, so no NaN ray): G1 fails at above_graze, inside_dip, high_graze, far_above (0.5 % chords) and on_top (2.9 %), 14 of
    its 21 cases; G2's gate fails at all three chord observers.  high_down, far_ground, on_bottom and capped_ring, which have no chord, pass.
  * the same function with the issue's `t1 = hb.near` in the chord case: on the HOST build only.  hb.near is NaN there, fminf makes the end +inf and
    the ray one of the NaN rays this file exists to keep off a GPU.  On the host core it fails the bit-for-bit test against the restatement at the
    five observers above (both N) and the float64 test of the segment's ends at those and at inside_up and above_down: 21 tests.
  * observer_ray without its last clause: never run on a GPU.  The host corner tests fail (tests/test_observer_edges_host.py): the three
    reproductions, the cap sweep, caps 1e-30, 1e-10, 1e-3 and 0.1 m, and the program under the sanitizers (79 704 expectations); caps 0.3 and
    1 m pass."""
import numpy as np
import pytest

import observers as OB
import observer_reference as OR
import shadow_reference as SR
from parity_metrics import cloud_tight
from test_clouds_rays_host import chains, host_view_dirs, rays_host  # noqa: F401  (module-scoped fixtures)
from test_gpu_observer import GUARD, bits, exact_ctx, whole_ctx, with_lut  # noqa: F401
from test_observer_edges_host import CORNER_POS, SCENE_B, beside_refused, random_directions
from test_observer_host import host_march_from, host_rays, obs_host  # noqa: F401

pytestmark = pytest.mark.gpu
MARCH = {"A": (128, 6), "B": (30, 4)}
INF = float("inf")
F = np.float32


def frames(ctx, p, name, d):
    """the four forms of one observer's frame: {form: float16 [H, W, 4]}"""
    import torch
    pos, cap, basis, fov, w, h = OB.observer(name)
    got = {"view host": ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap), "dirs host": ctx.render_clouds_dirs_from(p, d, pos, cap)}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dd = torch.from_numpy(d).cuda()
        o1 = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
        o2 = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
        s.synchronize()
        assert ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap, out=o1, stream=s.cuda_stream) is o1
        assert ctx.render_clouds_dirs_from(p, dd, pos, cap, out=o2, stream=s.cuda_stream) is o2
        got["view device"], got["dirs device"] = o1.cpu().numpy(), o2.cpu().numpy()
    return got


def host_frame(obs_host, chains, ctx, p, name, d, scene="A", **kw):  # noqa: F811
    pos, cap, _, _, _, _ = OB.observer(name)
    return host_march_from(obs_host, chains, p, ctx.read_sky_lut(), pos, cap, d, *MARCH[scene], **kw)


# ---------------------------------------------------------------------------------------------------------------- G1
CASES = [(n, "A", False) for n in OB.EDGE_NAMES] + [(n, s, e) for n in SCENE_B for s, e in (("A", True), ("B", False), ("B", True))]


@pytest.mark.parametrize("name,scene,exact", CASES, ids=["%s-%s-%s" % (n, s, "exact" if e else "fp16") for n, s, e in CASES])
def test_an_edge_observer_matches_the_host_core_in_every_form(whole_ctx, exact_ctx, obs_host, rays_host, chains, oracle, name, scene, exact):  # noqa: F811
    ctx = exact_ctx if exact else whole_ctx
    p = SR.scene(oracle, scene)
    pos, cap, basis, fov, w, h = OB.observer(name)
    ctx.set_march(*MARCH[scene])
    try:
        with_lut(ctx, p)
        d = host_view_dirs(rays_host, basis, fov, w, h)
        core, marched, _ = host_frame(obs_host, chains, ctx, p, name, d, scene)
        _, seg, _ = host_rays(obs_host, pos, cap, d, MARCH[scene][0])
        OB.assert_edge_conditions(name, d, core[..., 3].astype(F), marched, seg)
        got = frames(ctx, p, name, d)
        view = got["view host"]
        for form, img in got.items():
            assert (bits(img) == bits(view)).all(), form
        ok, info = cloud_tight(view, core)
        print("%s, scene %s, %s cells vs host core: %s" % (name, scene, "exact" if exact else "fp16", info))
        assert np.isfinite(view.astype(F)).all()
        assert ok, info
        assert not bits(view)[~marched].any()                  # not marched: zeros
    finally:
        ctx.set_march(128, 6)


# ---------------------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("name", OB.CHORD)
def test_the_height_window_and_the_saturation_skip_are_invisible_on_rays_that_leave_the_window_and_return(whole_ctx, obs_host, rays_host, chains, oracle, name):  # noqa: F811
    """csky_set_height_window(0) switches the exact specialisations off together (the per-sample window and the saturation skip; there is no switch
    for one of them alone): the frame without them meets the gate against the same host march as the frame with them, and has its bytes."""
    p = SR.scene(oracle, "A")
    pos, cap, basis, fov, w, h = OB.observer(name)
    whole_ctx.set_march(*MARCH["A"])
    try:
        with_lut(whole_ctx, p)
        d = host_view_dirs(rays_host, basis, fov, w, h)
        core, marched, _ = host_frame(obs_host, chains, whole_ctx, p, name, d)
        plain, _, _ = host_frame(obs_host, chains, whole_ctx, p, name, d, window=False)
        assert (bits(core) == bits(plain)).all()               # the host march itself: the window is exact
        on = whole_ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap)
        try:
            whole_ctx.set_height_window(False)
            off = whole_ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap)
        finally:
            whole_ctx.set_height_window(True)
        for label, img in (("on", on), ("off", off)):
            ok, info = cloud_tight(img, core)
            print("%s, window and saturation skip %s, vs host core: %s" % (name, label, info))
            assert ok, (label, info)
        differ = int((bits(on) != bits(off)).sum())
        print("%s: %d of %d halves differ with the window and the saturation skip off; alpha > 0 in %.1f %% of the pixels" % (name, differ, on.size, 100.0 * (on[..., 3] > 0).mean()))
        assert (on[..., 3] > 0).mean() >= 0.25
        assert differ == 0
    finally:
        whole_ctx.set_march(128, 6)


# ---------------------------------------------------------------------------------------------------------------- G3
@pytest.mark.parametrize("name", OB.EDGE_NAMES)
def test_a_depth_buffer_of_inf_gives_the_bytes_of_the_from_form(whole_ctx, oracle, name):
    p = SR.scene(oracle, "A")
    pos, cap, basis, fov, w, h = OB.observer(name)
    whole_ctx.set_march(*MARCH["A"])
    try:
        with_lut(whole_ctx, p)
        want = whole_ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap)
        got = whole_ctx.render_clouds_view_from_depth(p, basis, fov, w, h, pos, np.full((h, w), np.inf, F), "distance", cap)
        assert bits(want).any() and (bits(got) == bits(want)).all()
        if name == "capped_ring":                              # the cap as a constant depth
            got = whole_ctx.render_clouds_view_from_depth(p, basis, fov, w, h, pos, np.full((h, w), cap, F), "distance", INF)
            assert (bits(got) == bits(want)).all()
    finally:
        whole_ctx.set_march(128, 6)


# ---------------------------------------------------------------------------------------------------------------- G4
def _corner_frame(ctx, p, d, pos, cap):
    """the device dirs form into a tensor of 0xFFFF halves with guard rows: the image's halves, after asserting the guards untouched"""
    import torch
    h, w = d.shape[:2]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.empty((h + 2 * GUARD, 4 * w), dtype=torch.int16, device="cuda")
        t.fill_(-1)
        dd = torch.from_numpy(d).cuda()
        s.synchronize()
        share = t[GUARD:GUARD + h].unflatten(1, (w, 4))
        assert ctx.render_clouds_dirs_from(p, dd, pos, cap, out=share, stream=s.cuda_stream) is share
        got = t.cpu().numpy().view(np.uint16)
    assert (got[:GUARD] == 0xFFFF).all() and (got[GUARD + h:] == 0xFFFF).all()
    return got[GUARD:GUARD + h].reshape(h, w, 4)


CORNERS = [("up", float(np.nextafter(F(1500.0), F(2000.0)))), ("up", 1500.2), ("up", 1500.3), ("up", 1501.0), ("random", 0.1), ("random", 1e-30)]


@pytest.mark.parametrize("rays,cap", CORNERS, ids=["%s-%g" % c for c in CORNERS])
def test_a_cap_within_the_quantum_of_t0_gives_no_nan_and_the_host_cores_frame(whole_ctx, obs_host, chains, oracle, rays, cap):  # noqa: F811
    """On the library with observer_ray's last clause only: 64 x 36 copies of (0, 1, 0) from (0, 0, 0), t0 = 1500, and the first 2 304 seeded random
    directions from inside the layer."""
    p = SR.scene(oracle, "A")
    w, h = 64, 36
    if rays == "up":
        pos, d = (0.0, 0.0, 0.0), np.ascontiguousarray(np.broadcast_to(np.array([0.0, 1.0, 0.0], F), (h, w, 3)))
    else:
        pos, d = CORNER_POS, np.ascontiguousarray(random_directions()[:w * h].reshape(h, w, 3))
    whole_ctx.set_march(*MARCH["A"])
    try:
        with_lut(whole_ctx, p)
        want, marched, _ = host_march_from(obs_host, chains, p, whole_ctx.read_sky_lut(), pos, cap, d, *MARCH["A"])
        ref = OR.ray(pos, cap, d, MARCH["A"][0])
        assert np.isfinite(ref).all() and ((ref[..., 10] > 0) == marched).all()
        got = _corner_frame(whole_ctx, p, d, pos, cap)
        halves = got.view(np.float16).astype(F)
        differ = int((got != bits(want)).sum())
        print("%s, cap %g: %d of %d rays marched, %d non-finite halves, %d of %d halves differ from the host core's" %
              (rays, cap, marched.sum(), marched.size, (~np.isfinite(halves)).sum(), differ, got.size))
        assert np.isfinite(halves).all()
        assert not got[~marched].any()
        assert differ == 0
    finally:
        whole_ctx.set_march(128, 6)


# ---------------------------------------------------------------------------------------------------------------- G5
def test_the_cap_ring(whole_ctx, obs_host, rays_host, chains, oracle):  # noqa: F811
    """capped_ring: the cap ends some rays in front of the layer while their neighbours are marched."""
    p = SR.scene(oracle, "A")
    pos, cap, basis, fov, w, h = OB.observer("capped_ring")
    whole_ctx.set_march(*MARCH["A"])
    try:
        with_lut(whole_ctx, p)
        d = host_view_dirs(rays_host, basis, fov, w, h)
        t0, t1, has = OR.segment(pos, cap, d)
        _, _, free = OR.segment(pos, INF, d)
        marched = OR.ray(pos, cap, d, MARCH["A"][0])[..., 10] > 0
        refused = free & ~marched
        capped = marched & (t1 == F(cap))
        got = whole_ctx.render_clouds_view_from(p, basis, fov, w, h, pos, cap)
        whole = whole_ctx.render_clouds_view_from(p, basis, fov, w, h, pos, INF)
        beside = beside_refused(refused, marched)             # marched pixels in a wavefront's tile with a refused one
        changed = (bits(got) != bits(whole)).any(-1)
        print("capped_ring: %d refused, %d marched in a tile with one, %d capped, %d texels change without the cap" % (refused.sum(), beside.sum(), capped.sum(), changed.sum()))
        assert refused.sum() >= 0.10 * refused.size and beside.sum() >= 64
        assert not bits(got)[refused].any()
        assert (got[..., 3][beside] > 0).sum() >= 16
        assert changed.any() and not changed[~(capped | refused)].any()
    finally:
        whole_ctx.set_march(128, 6)
