"""The per-lane core of the temporal split of a view frame (csrc/view_update_core.h: what the lanes of clouds_view_fresh_kernel and
clouds_view_reproject_kernel run around the march), compiled for the host by tests/view_update_host and held to the numpy restatement of its
definition (tests/view_update_reference.py).  A unit test of device code, not a render path: libcloudsky itself has no CPU implementation.

The cameras: clouds_rays_reference.VIEW (64 x 36, fov 70, pitch 25, yaw 40) and the moved one (pitch +4, yaw +8).  Every test on the moved camera
asserts from the reference alone that holes are 5..40 % and tapped pixels >= 30 % of the image: no kind of pixel is absent from a passing run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clouds_rays_reference as RR
import shadow_reference as SR
import view_update_reference as VU
from conftest import ROOT
from test_clouds_rays_host import P, chains, host_march, host_view_dirs, rays_host  # noqa: F401  (module-scoped fixtures)

F = np.float32
V = RR.VIEW
W, H = V["width"], V["height"]
BASIS = RR.camera_basis(V["pitch"], V["yaw"])
MOVED = RR.camera_basis(VU.MOVED["pitch"], VU.MOVED["yaw"])


@pytest.fixture(scope="module")
def vu_host():
    d = os.path.join(ROOT, "tests", "view_update_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libview_update_host.so"))
    for f in ("view_update_host_geom", "view_update_host_classify", "view_update_host_tap", "view_update_host_update"):
        getattr(L, f).restype = None
    L.view_update_host_geom.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.view_update_host_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.view_update_host_tap.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.view_update_host_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def core_classify(L, view, prev_view, w, h, block, phase, force_formula=False):
    """(kind uint8 [h, w], ux, uy float32 [h, w], dirs float32 [h, w, 3]) of the host core; view / prev_view: ten floats (prev_view None: no history)"""
    kind, uv, d = np.zeros((h, w), np.uint8), np.zeros((h, w, 2), F), np.zeros((h, w, 3), F)
    L.view_update_host_classify(P(view), P(prev_view), w, h, block, phase, int(force_formula), P(kind), P(uv), P(d))
    return kind, uv[..., 0].copy(), uv[..., 1].copy(), d


def core_tap(L, prev, ux, uy):
    """the core's taps of float16 [h, w, 4] `prev` at the coordinates ux, uy -> float16 [n, 4]"""
    h, w = prev.shape[:2]
    uv = np.ascontiguousarray(np.stack([np.asarray(ux, F).reshape(-1), np.asarray(uy, F).reshape(-1)], -1))
    out = np.zeros((uv.shape[0], 4), np.uint16)
    img = np.ascontiguousarray(prev).view(np.uint16)
    L.view_update_host_tap(P(img), w, w, h, uv.shape[0], P(uv), P(out))
    return out.view(np.float16)


def core_update(L, chains, params, sky, view, prev_view, w, h, block, phase, prev, primary=128, light=6):  # noqa: F811
    """the host core's whole update: (float16 [h, w, 4], kind [h, w], texels of prev read)"""
    out, kind, taps = np.zeros((h, w, 4), np.uint16), np.zeros((h, w), np.uint8), np.zeros(1, np.uint64)
    s = np.ascontiguousarray(sky).view(np.uint16)
    pv = None if prev is None else np.ascontiguousarray(prev).view(np.uint16)
    L.view_update_host_update(P(chains[0]), P(chains[1]), P(chains[2]), P(np.ascontiguousarray(params, F)), primary, light, P(s), s.shape[1], s.shape[0], P(view),
                              P(prev_view), w, h, block, phase, P(pv), P(out), P(kind), P(taps))
    return out.view(np.float16), kind, int(taps[0])


def assert_moved_shares(kind):
    holes, tapped = VU.shares(kind)
    print("reference: holes %.1f %%, tapped %.1f %%, fresh %.1f %%, not accepted %.1f %%" % (100 * holes, 100 * tapped, 100 * (kind == VU.FRESH).mean(), 100 * (kind == VU.ZERO).mean()))
    assert 0.05 <= holes <= 0.40 and tapped >= 0.30


def random_frame(h, w, seed):
    """float16 [h, w, 4]: finite halves of every kind (both signs, subnormals, zeros, large and small magnitudes)"""
    r = np.random.default_rng(seed)
    a = r.integers(0, 0x7C00, (h, w, 4)).astype(np.uint16) | (r.integers(0, 2, (h, w, 4)).astype(np.uint16) << 15)
    a[r.random((h, w, 4)) < 0.1] = 0
    return a.view(np.float16)


# ---- U1
CASES = {"still": (BASIS, V["fov"], BASIS, V["fov"]), "moved": (MOVED, V["fov"], BASIS, V["fov"]), "other-fov": (MOVED, V["fov"], BASIS, 50.0)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("block,phase", [(4, 0), (4, 5), (4, 15), (2, 3), (8, 37), (1, 0)])
def test_classification_and_coordinates_are_the_restatement_bit_for_bit(vu_host, case, block, phase):
    b, fov, pb, pfov = CASES[case]
    view, prev_view = VU.view_floats(b, fov), VU.view_floats(pb, pfov)
    for force in ((False, True) if case == "still" else (False,)):   # the still camera by the rule (copies), and through the formula
        ref = VU.classify(b, fov, pb, pfov, W, H, block, phase, same=False if force else None)
        kind, ux, uy, d = core_classify(vu_host, view, prev_view, W, H, block, phase, force_formula=force)
        assert (d.view(np.uint32) == ref["e"].view(np.uint32)).all()
        assert (kind == ref["kind"]).all(), np.argwhere(kind != ref["kind"])[:4]
        ran = (kind == VU.TAP) | (kind == VU.HOLE)
        if case == "still" and not force:
            assert not ran.any() and ((kind == VU.COPY) | (kind == VU.FRESH) | (kind == VU.ZERO)).all() and (kind == VU.COPY).any() == (block > 1)
        elif block > 1:
            assert ran.any() and (ux.view(np.uint32)[ran] == ref["ux"].view(np.uint32)[ran]).all() and (uy.view(np.uint32)[ran] == ref["uy"].view(np.uint32)[ran]).all()
        if case == "moved" and block == 4:
            assert_moved_shares(ref["kind"])
    none = VU.classify(b, fov, None, None, W, H, block, phase)       # no previous frame
    kind, _, _, _ = core_classify(vu_host, view, None, W, H, block, phase)
    assert (kind == none["kind"]).all() and not ((kind == VU.TAP) | (kind == VU.COPY)).any()


@pytest.mark.parametrize("w,h,block,phase", [(5, 3, 8, 0), (5, 3, 8, 4), (5, 3, 8, 5), (5, 3, 8, 24), (5, 3, 8, 63), (37, 21, 4, 7), (1, 1, 4, 0), (1, 1, 4, 9), (33, 9, 2, 3)])
def test_sub_grid_is_the_set_of_fresh_pixels(vu_host, w, h, block, phase):
    g = np.zeros(7, np.int32)
    view = VU.view_floats(BASIS, V["fov"])
    vu_host.view_update_host_geom(P(view), P(view), w, h, block, phase, P(g))
    px, py = phase % block, phase // block
    xs, ys = np.arange(px, w, block), np.arange(py, h, block)
    assert tuple(g) == (block, px, py, len(xs), len(ys), 1, 1)
    vu_host.view_update_host_geom(P(view), None, w, h, block, phase, P(g))
    assert tuple(g[5:]) == (0, 0)
    minus = view.copy()
    minus[1] = -view[1] if view[1] != 0 else F(-0.0)              # one float differs
    vu_host.view_update_host_geom(P(view), P(minus), w, h, block, phase, P(g))
    assert tuple(g[5:]) == (0, 1)


# ---- U2
@pytest.mark.parametrize("w,h,pad", [(64, 36, 0), (37, 21, 3), (1, 1, 0), (2, 1, 1)])
def test_tap_is_the_restatement(vu_host, w, h, pad):
    prev = random_frame(h, w, 7 + w)
    r = np.random.default_rng(w * h)
    n = 4096
    ux, uy = (r.random(n) * (w - 1)).astype(F), (r.random(n) * (h - 1)).astype(F)
    ux[:64], uy[:64] = np.floor(ux[:64]), np.floor(uy[:64])         # texel centres
    ux[64:72], uy[64:72] = (0, w - 1, 0, w - 1, 0, w - 1, 0, w - 1), (0, 0, h - 1, h - 1, 0, 0, h - 1, h - 1)   # the corners: x1 / y1 clamp
    if w > 1:
        ux[72:80] = np.nextafter(F(w - 1), F(0))
    want = VU.tap(prev, ux, uy)
    rows = np.full((h, (w + pad) * 4), 0xFFFF, np.uint16)           # a pitched copy: padding no tap may read (a NaN would show)
    rows[:, :w * 4] = bits(prev).reshape(h, w * 4)
    got = core_tap(vu_host, prev, ux, uy)
    differ = int((bits(got) != bits(want)).sum())
    print("%d x %d: %d of %d halves differ" % (w, h, differ, got.size))
    assert differ == 0
    out = np.zeros((n, 4), np.uint16)
    uv = np.ascontiguousarray(np.stack([ux, uy], -1))
    vu_host.view_update_host_tap(P(rows), w + pad, w, h, n, P(uv), P(out))
    assert (out == bits(want)).all()
    assert len(np.unique(bits(want))) > (8 if w > 1 else 0)


# ---- U3
@pytest.mark.parametrize("phase", [0, 5, 15])
def test_same_rule_copies_and_the_formula_alone_would_not(vu_host, chains, oracle, o_skies, phase):  # noqa: F811
    view = VU.view_floats(BASIS, V["fov"])
    prev = random_frame(H, W, 3)
    p = SR.scene(oracle, "A")
    got, kind, read = core_update(vu_host, chains, p, o_skies["deg45"], view, view, W, H, 4, phase, prev, primary=16, light=2)
    ref = VU.classify(BASIS, V["fov"], BASIS, V["fov"], W, H, 4, phase)
    assert (kind == ref["kind"]).all()
    copy = kind == VU.COPY
    assert copy.sum() == ((kind != VU.ZERO) & (kind != VU.FRESH)).sum() > 0.5 * W * H and read == int(copy.sum())
    assert (bits(got)[copy] == bits(prev)[copy]).all()
    assert not bits(got)[kind == VU.ZERO].any()
    # without the rule: the formula puts the unmoved camera's own edge pixels outside [0, w - 1] x [0, h - 1], where they would be marched on every call
    formula = VU.classify(BASIS, V["fov"], BASIS, V["fov"], W, H, 4, phase, same=False)
    out = formula["kind"] == VU.HOLE
    j, i = np.nonzero(out)
    t = formula["kind"] == VU.TAP
    print("phase %d, the formula on the still camera: %d pixels (%.1f %%) fall outside, max |ux - i| = %.3g" % (
        phase, out.sum(), 100.0 * out.mean(), np.abs(formula["ux"][t] - np.arange(W, dtype=F)[None, :].repeat(H, 0)[t]).max()))
    assert out.sum() > 0
    assert ((i == 0) | (i == W - 1) | (j == 0) | (j == H - 1)).all()   # the image's own border, nothing else


# ---- U4
def test_directions_under_the_horizon_are_zero_texels_without_a_tap(vu_host, chains, oracle, o_skies):  # noqa: F811
    down = RR.camera_basis(-10.0, V["yaw"])                         # pitched down: the lower rows look under the horizon
    prev_b = RR.camera_basis(-6.0, V["yaw"] - 8.0)
    view, prev_view = VU.view_floats(down, V["fov"]), VU.view_floats(prev_b, V["fov"])
    ref = VU.classify(down, V["fov"], prev_b, V["fov"], W, H, 4, 5)
    under = ~RR.accept(ref["e"])
    assert under[H - 8:].all() and (ref["kind"] == VU.TAP).any() and 0.3 < under.mean() < 0.9
    prev = np.full((H, W, 4), 0x3C00, np.uint16).view(np.float16)    # ones everywhere: a tap or a copy would show
    p = SR.scene(oracle, "A")
    got, kind, read = core_update(vu_host, chains, p, o_skies["deg45"], view, prev_view, W, H, 4, 5, prev, primary=16, light=2)
    assert (kind == ref["kind"]).all() and (kind[under] == VU.ZERO).all()
    assert not bits(got)[under].any()
    assert read == 4 * int((kind == VU.TAP).sum())                    # no texel read for the pixels under the horizon
    assert (bits(got)[kind == VU.TAP] == 0x3C00).all()


@pytest.mark.parametrize("slot", range(10))
def test_nan_in_the_previous_view_gives_holes_and_no_address(vu_host, chains, oracle, o_skies, slot):  # noqa: F811
    view = VU.view_floats(MOVED, V["fov"])
    prev_view = VU.view_floats(BASIS, V["fov"])
    prev_view[slot] = np.nan
    kind, ux, uy, d = core_classify(vu_host, view, prev_view, W, H, 4, 5)
    ok, fresh = RR.accept(d), VU.classify(MOVED, V["fov"], None, None, W, H, 4, 5)["kind"] == VU.FRESH
    assert (kind[~ok] == VU.ZERO).all() and (kind[ok & fresh] == VU.FRESH).all() and (kind[ok & ~fresh] == VU.HOLE).all() and (ok & ~fresh).sum() > 0.5 * W * H
    if slot == 0:                                                     # the whole update: no texel of prev is read (prev is NOT W x H texels: one texel)
        p = SR.scene(oracle, "A")
        one = np.zeros((1, 1, 4), np.float16)
        got, k2, read = core_update(vu_host, chains, p, o_skies["deg45"], view, prev_view, 9, 5, 4, 5, one, primary=8, light=2)
        assert read == 0 and not ((k2 == VU.TAP) | (k2 == VU.COPY)).any() and (k2 == VU.HOLE).any()


# ---- U5
@pytest.fixture(scope="module")
def full_views(rays_host, chains, oracle, o_skies):  # noqa: F811
    """host_march's full view frames of scene A for the two cameras, marched once"""
    p = SR.scene(oracle, "A")
    out = {}
    for name, b in (("still", BASIS), ("moved", MOVED)):
        img, _, _ = host_march(rays_host, chains, p, o_skies["deg45"], host_view_dirs(rays_host, b, V["fov"], W, H))
        out[name] = img
    return p, out


@pytest.mark.parametrize("case,block,phase", [("moved", 4, 0), ("moved", 4, 5), ("moved", 4, 15), ("moved", 2, 1), ("still", 4, 5), ("none", 4, 7), ("moved", 1, 0)])
def test_whole_update_is_the_composition_of_the_full_view_and_the_reference_taps(vu_host, chains, o_skies, full_views, case, block, phase):  # noqa: F811
    p, full = full_views
    cur = MOVED if case == "moved" else BASIS
    want_full = full["moved" if case == "moved" else "still"]
    prev = None if case == "none" else full["still"]
    ref = VU.classify(cur, V["fov"], None if prev is None else BASIS, V["fov"], W, H, block, phase)
    if case == "moved" and block > 1:
        assert_moved_shares(ref["kind"])
    want = VU.compose(ref, want_full, prev)
    got, kind, _ = core_update(vu_host, chains, p, o_skies["deg45"], VU.view_floats(cur, V["fov"]), None if prev is None else VU.view_floats(BASIS, V["fov"]), W, H, block,
                               phase, prev)
    assert (kind == ref["kind"]).all()
    differ = int((bits(got) != bits(want)).sum())
    print("%s B = %d phase %d: %d of %d halves differ; alpha > 0 in %.1f %% of the pixels" % (case, block, phase, differ, got.size, 100.0 * (want[..., 3] > 0).mean()))
    assert (want[..., 3] > 0).mean() >= 0.25
    assert differ == 0
    if case == "none" or block == 1:
        assert (bits(got) == bits(want_full)).all()                  # no history, or B = 1: the full view frame
