"""The shadowed aerial-perspective volume's per-lane code (csrc/shafts_core.h on aerial_core.h and lut_core.h: the definition shafts.hip's wavefronts
must equal), compiled for the host by tests/shafts_host, against the unshadowed core (tests/aerial_host) and the numpy restatement of the contract
(tests/shafts_reference.py).  A unit test of device code, not a render path: libcloudsky itself has no CPU implementation.

The gate is the volume's own (aerial_reference.gate): every half within 1 fp16 ulp.  C6 is the chain the product runs at sunrise: the helper's
rectangle, a cloud shadow map with chord texels from the host build of the shadow core (tests/shadow_host), the volume."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aerial_reference as AR
import shadow_reference as SHR
import shafts_reference as SR
from conftest import ROOT
from test_aerial_host import CASES, SUNS, P, aerial_host, case_view, host_luts, host_volume  # noqa: F401  (aerial_host, host_luts: module-scoped fixtures)
from test_shadow_host import chains, host_map, shadow_host  # noqa: F401  (shadow_host, chains: module-scoped fixtures)
from test_tlut_mapping import tlut_host  # noqa: F401  (host_luts needs it)

M, M_CENTER, M_EXTENT = SR.synthetic_map()
# the height rule's case (C4): panorama 8 x 4, D = 40, S = 1, 8 km, a zenith sun, one black texel over 100 km
C4 = dict(W=8, H=4, D=40, S=1, far=8.0, sun=np.array([0.0, 1.0, 0.0], np.float32), shadow=np.zeros((1, 1), np.float16), center=(0.0, 0.0), extent=(100000.0, 100000.0))


# the chain the product runs at sunrise: the helper's rectangle -> a 64 x 16 cloud shadow map -> a 13 x 7 x 8 volume, S = 2, 32 km.  The map's push
# constants are the sweep scene's of that sun (tests/shadow_reference.py); the views: the panorama and the camera of case "up".
LOW_SUNS = {"deg1.1": "deg1.1", "deg0.66": "deg0.66-z"}
LOW_MAP = dict(width=64, height=16, steps=32)
LOW_VOLUME = dict(W=13, H=7, D=8, S=2, far=32.0)
LOW_VIEWS = ("panorama", "up")


def low_sun_map_args(oracle, sun):
    """(push-constant block, its unit sun, the helper's (center, extent) by the contract's text, the kind of every texel of the 64 x 16 map)"""
    p, _ = SHR.sweep_scene(oracle, LOW_SUNS[sun])
    l = np.asarray(p[16:19], np.float32)
    center, extent = SHR.helper_rect(l, LOW_VOLUME["far"])
    return p, l, center, extent, SHR.texel_kinds(p, LOW_MAP["width"], LOW_MAP["height"], center, extent)


def low_sun_reference(trans, mapping, l, shadow, center, extent, kind, view):
    """The restatement's volume over `shadow`, behind its precondition: at least one tapped step projects into a chord texel of the map."""
    v = LOW_VOLUME
    vw, aspect = case_view(view)
    ref = SR.volume(v["W"], v["H"], v["D"], v["S"], v["far"], l, trans, shadow, center, extent, mapping, vw, 0.0 if vw is None else aspect)
    assert not ref["near"].any() and np.isfinite(ref["out"].astype(np.float32)).all()
    tapped = ref["take"] & ref["tapped"]
    i = np.floor(((ref["gx"][tapped] - np.float32(center[0])) / np.float32(extent[0]) + 0.5) * LOW_MAP["width"]).astype(int)
    j = np.floor(((ref["gz"][tapped] - np.float32(center[1])) / np.float32(extent[1]) + 0.5) * LOW_MAP["height"]).astype(int)
    ok = (i >= 0) & (i < LOW_MAP["width"]) & (j >= 0) & (j < LOW_MAP["height"])
    in_chord = kind[j[ok], i[ok]] == SHR.CHORD
    assert in_chord.any(), "no tapped step projects into a chord texel"
    return ref, int(in_chord.sum()), int(tapped.sum())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.fixture(scope="module")
def shafts_host():
    d = os.path.join(ROOT, "tests", "shafts_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libshafts_host.so"))
    L.shafts_host_volume.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                     C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.shafts_host_steps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p]
    L.shafts_host_rect.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    return L


def _view_args(view):
    cam = np.ascontiguousarray(np.asarray(view[0], np.float32).T.reshape(-1)) if view is not None else np.zeros(9, np.float32)   # column-major
    return int(view is not None), cam, (float(view[1]) if view is not None else 0.0)


def _map_args(shadow, center, extent, pitch_h=None):
    """(the map's halfs, width, height, pitch in halfs, geometry); pitch_h > width: the rows are spread and the padding is NaN halfs"""
    m = bits(np.asarray(shadow, np.float16))
    mh, mw = m.shape
    if pitch_h is not None:
        padded = np.full((mh, pitch_h), 0x7E00, np.uint16)
        padded[:, :mw] = m
        m = padded
    return np.ascontiguousarray(m), mw, mh, m.shape[1], np.array([center[0], center[1], extent[0], extent[1]], np.float32)


def shafts_volume(L, mapping, trans, W, H, D, S, far_km, sun, shadow, center, extent, view=None, aspect=0.0, state=False, pitch_h=None):
    """The host core's shadowed volume float16 [D, H, W, 4] (and the spectral (L, Tr) float32 [D, H, W, 8] with state=True)."""
    tr = bits(trans)
    out = np.zeros((D, H, W, 4), np.uint16)
    st = np.zeros((D, H, W, 8), np.float32) if state else None
    vm, cam, fov = _view_args(view)
    m, mw, mh, pitch, geom = _map_args(shadow, center, extent, pitch_h)
    s = np.ascontiguousarray(sun, np.float32)
    rc = L.shafts_host_volume(mapping, P(tr), tr.shape[1], tr.shape[0], W, H, D, S, float(far_km), P(s), vm, P(cam), fov, float(aspect), P(m), mw, mh, pitch, P(geom),
                              P(out), P(st))
    assert rc == 0
    return (out.view(np.float16), st) if state else out.view(np.float16)


def shafts_steps(L, W, H, D, S, far_km, sun, shadow, center, extent, view=None, aspect=0.0):
    """What the core makes of the map at every step: float32 [H, W, D * S, 6] = taken, h, gx, gz, m (NaN: no texel read), s."""
    out = np.zeros((H, W, D * S, 6), np.float32)
    vm, cam, fov = _view_args(view)
    m, mw, mh, pitch, geom = _map_args(shadow, center, extent)
    s = np.ascontiguousarray(sun, np.float32)
    assert L.shafts_host_steps(W, H, D, S, float(far_km), P(s), vm, P(cam), fov, float(aspect), P(m), mw, mh, pitch, P(geom), P(out)) == 0
    return out


@pytest.fixture(scope="module")
def restated_shafts(host_luts):  # noqa: F811
    """The restatement's shadowed volumes with the map M, computed once per (case, sun, mapping)."""
    cache = {}

    def get(case, sun, mapping):
        k = (case, sun, mapping)
        if k not in cache:
            W, H, D, S, far = CASES[case][:5]
            view, aspect = case_view(case)
            cache[k] = SR.volume(W, H, D, S, far, SUNS[sun], host_luts[mapping], M, M_CENTER, M_EXTENT, mapping, view, aspect)
        return cache[k]
    return get


# ---------------------------------------------------------------------------------------------------------------- C1. an all-ones map is the plain volume
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("case", list(CASES))
def test_all_ones_map_is_the_plain_volume(shafts_host, aerial_host, host_luts, case, sun, mapping):  # noqa: F811
    W, H, D, S, far = CASES[case][:5]
    view, aspect = case_view(case)
    plain = host_volume(aerial_host, mapping, host_luts[mapping], W, H, D, S, far, SUNS[sun], view, aspect)
    got = shafts_volume(shafts_host, mapping, host_luts[mapping], W, H, D, S, far, SUNS[sun], np.ones_like(M), M_CENTER, M_EXTENT, view, aspect)
    assert (bits(got) == bits(plain)).all()                        # pins sky_step_shadowed to sky_step
    if sun != "degm2":                                             # the map was really read: the same call with M differs
        assert (bits(shafts_volume(shafts_host, mapping, host_luts[mapping], W, H, D, S, far, SUNS[sun], M, M_CENTER, M_EXTENT, view, aspect)) != bits(plain)).any()


# ---------------------------------------------------------------------------------------------------------------- C2. core against restatement
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("case", list(CASES))
def test_core_matches_the_restatement(shafts_host, host_luts, restated_shafts, case, sun, mapping):  # noqa: F811
    W, H, D, S, far = CASES[case][:5]
    view, aspect = case_view(case)
    ref = restated_shafts(case, sun, mapping)
    assert not ref["near"].any()
    assert np.isfinite(ref["out"].astype(np.float32)).all()
    # preconditions on the RESTATEMENT: the map shadows a real share of the steps, and that moves a real share of the volume
    take = ref["take"]
    shadowed = (ref["s"][take] < 1).mean()
    plain = AR.volume(W, H, D, S, far, SUNS[sun], host_luts[mapping], mapping, view, aspect)
    moved = (AR.ulp_dist(ref["out"][..., :3], plain["out"][..., :3]) > 8).mean()
    print("%s %s mapping %d: %.1f %% of the taken steps have s < 1, %.1f %% of the rgb halves lie more than 8 fp16 ulp from the unshadowed volume"
          % (case, sun, mapping, 100 * shadowed, 100 * moved))
    if sun == "degm2":
        assert shadowed == 0 and moved == 0 and (bits(ref["out"]) == bits(plain["out"])).all()
    else:
        assert shadowed >= (0.15 if sun == "deg45" else 0.04) and moved >= 0.15
        assert ref["s"][take].min() == np.float32(0.25)
    assert (bits(ref["out"][..., 3]) == bits(plain["out"][..., 3])).all()           # alpha does not see the map
    got, st = shafts_volume(shafts_host, mapping, host_luts[mapping], W, H, D, S, far, SUNS[sun], M, M_CENTER, M_EXTENT, view, aspect, state=True)
    differ, cancel = AR.gate(got, ref["out"], st[..., :4], ref["L"], what="%s %s mapping %d" % (case, sun, mapping))
    print("%s %s mapping %d: %d of %d halves differ from the restatement, %d let through as cancellation in M * L" % (case, sun, mapping, differ, got.size, cancel))
    # the core's per-step decisions are the restatement's
    steps = shafts_steps(shafts_host, W, H, D, S, far, SUNS[sun], M, M_CENTER, M_EXTENT, view, aspect)
    assert (np.moveaxis(steps[..., 0], -1, 0) == take).all()
    assert (np.moveaxis(steps[..., 5], -1, 0)[take] == ref["s"][take]).all()


# ---------------------------------------------------------------------------------------------------------------- C3. structure
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("sun", ["deg45", "demo"])
@pytest.mark.parametrize("case", list(CASES))
def test_alpha_and_spectral_bound(shafts_host, aerial_host, host_luts, case, sun, mapping):  # noqa: F811
    W, H, D, S, far = CASES[case][:5]
    view, aspect = case_view(case)
    plain, pst = host_volume(aerial_host, mapping, host_luts[mapping], W, H, D, S, far, SUNS[sun], view, aspect, state=True)
    got, st = shafts_volume(shafts_host, mapping, host_luts[mapping], W, H, D, S, far, SUNS[sun], M, M_CENTER, M_EXTENT, view, aspect, state=True)
    assert (bits(got[..., 3]) == bits(plain[..., 3])).all()        # alpha bytes
    assert (st[..., 4:] == pst[..., 4:]).all()                     # Tr itself
    # a shadow only removes light, per spectral component (not per rgb channel: the matrix M has negative entries)
    assert (st[..., :4] <= pst[..., :4] * (1 + 1e-6)).all()
    assert (st[..., :4] < pst[..., :4]).any()


def test_equal_map_filters_exactly(shafts_host):
    """A map of 0.5 everywhere under a zenith sun, wide enough to hold every projection away from its edge: every tapped step filters exactly 0.5."""
    zenith = np.array([0.0, 1.0, 0.0], np.float32)
    for case in CASES:
        W, H, D, S, far = CASES[case][:5]
        view, aspect = case_view(case)
        ext = 4000.0 * far                                          # |g| <= far km: fx, fy stay in the middle half of the map
        steps = shafts_steps(shafts_host, W, H, D, S, far, zenith, np.full((4, 4), 0.5, np.float16), (0.0, 0.0), (ext, ext), view, aspect)
        taken, h, m, s = steps[..., 0] == 1, steps[..., 1], steps[..., 4], steps[..., 5]
        tapped = taken & (h < 4000)
        assert tapped.sum() >= 0.2 * taken.sum() and not np.isnan(m[tapped]).any()
        assert (m[tapped] == np.float32(0.5)).all()
        assert np.isnan(m[taken & ~tapped]).all() and (s[taken & ~tapped] == 1).all()
        assert (s[tapped & (h <= 1500)] == np.float32(0.5)).all() and (s[tapped] >= np.float32(0.5)).all()


@pytest.mark.parametrize("mapping", [0, 1])
def test_no_sun_no_shafts_and_padding_is_not_read(shafts_host, aerial_host, host_luts, mapping):  # noqa: F811
    W, H, D, S, far = CASES["down"][:5]
    view, aspect = case_view("down")
    t = host_luts[mapping]
    for sun in (SUNS["degm2"], np.array([1.0, 0.0, 0.0], np.float32), np.array([0.3, -0.0, 0.2], np.float32), np.zeros(3, np.float32)):   # l.y < 0, == 0, == -0, NaN
        plain = host_volume(aerial_host, mapping, t, W, H, D, S, far, sun, view, aspect)
        got = shafts_volume(shafts_host, mapping, t, W, H, D, S, far, sun, M, M_CENTER, M_EXTENT, view, aspect)
        assert (bits(got) == bits(plain)).all(), sun
    tight = shafts_volume(shafts_host, mapping, t, W, H, D, S, far, SUNS["deg45"], M, M_CENTER, M_EXTENT, view, aspect)
    pitched = shafts_volume(shafts_host, mapping, t, W, H, D, S, far, SUNS["deg45"], M, M_CENTER, M_EXTENT, view, aspect, pitch_h=M.shape[1] + 8)
    assert (bits(pitched) == bits(tight)).all() and np.isfinite(tight.astype(np.float32)).all()


# ---------------------------------------------------------------------------------------------------------------- C4. the height rule
@pytest.fixture(scope="module")
def restated_c4(host_luts):  # noqa: F811
    c = C4
    return {m: SR.volume(c["W"], c["H"], c["D"], c["S"], c["far"], c["sun"], host_luts[m], c["shadow"], c["center"], c["extent"], m) for m in (0, 1)}


@pytest.mark.parametrize("mapping", [0, 1])
def test_height_rule(shafts_host, host_luts, restated_c4, mapping):  # noqa: F811
    c, ref = C4, restated_c4[mapping]
    assert not ref["near"].any()
    h = ref["h"][ref["take"]]
    shares = [(h <= 1500).mean(), ((h > 1500) & (h < 4000)).mean(), (h >= 4000).mean()]
    print("height rule: %.0f / %.0f / %.0f %% of the taken steps under, inside and above the layer" % tuple(100 * x for x in shares))
    assert min(shares) >= 0.20
    s = ref["s"][ref["take"]]
    assert (s[h >= 4000] == 1).all() and (s[h <= 1500] < 1).all()
    got, st = shafts_volume(shafts_host, mapping, host_luts[mapping], c["W"], c["H"], c["D"], c["S"], c["far"], c["sun"], c["shadow"], c["center"], c["extent"], state=True)
    differ, cancel = AR.gate(got, ref["out"], st[..., :4], ref["L"], what="height rule, mapping %d" % mapping)
    print("height rule mapping %d: %d of %d halves differ from the restatement, %d let through as cancellation" % (mapping, differ, got.size, cancel))
    steps = shafts_steps(shafts_host, c["W"], c["H"], c["D"], c["S"], c["far"], c["sun"], c["shadow"], c["center"], c["extent"])
    assert (np.moveaxis(steps[..., 5], -1, 0)[ref["take"]] == ref["s"][ref["take"]]).all()


# ---------------------------------------------------------------------------------------------------------------- C5. the rectangle
@pytest.mark.parametrize("sun", ["deg45", "demo"])
@pytest.mark.parametrize("case", list(CASES))
def test_shadow_rect_holds_every_projection(pkg, shafts_host, restated_shafts, case, sun):
    far = CASES[case][4]
    center, extent = pkg.aerial_shadow_rect(SUNS[sun], far)
    want = SR.shadow_rect(SUNS[sun], far)
    assert np.allclose(center, want[0], rtol=1e-6, atol=0) and np.allclose(extent, want[1], rtol=1e-6, atol=0)
    ce, ex = (C.c_float * 2)(), (C.c_float * 2)()
    assert shafts_host.shafts_host_rect(P(np.ascontiguousarray(SUNS[sun], np.float32)), far, ce, ex) == 0 and (tuple(ce), tuple(ex)) == (center, extent)
    ref = restated_shafts(case, sun, 0)                              # the projections do not depend on the map or the mapping
    low = ref["take"] & (ref["h"] < 4000)
    assert low.sum() >= 100
    for axis, g in enumerate((ref["gx"], ref["gz"])):
        assert (np.abs(g[low].astype(np.float64) - center[axis]) <= 0.5 * extent[axis]).all(), axis


def test_shadow_rect_errors_and_default(pkg):
    lib = pkg._lib
    for sun in (SUNS["degm2"], (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (np.cos(np.radians(0.1)), np.sin(np.radians(0.1)), 0.0), (0.6, float("nan"), 0.0)):
        with pytest.raises(pkg.CloudSkyError) as e:
            pkg.aerial_shadow_rect(sun, 32.0)
        assert e.value.code == lib.ERR_INVALID, sun
    for far in (-1.0, 2000.5, float("nan"), float("inf")):
        with pytest.raises(pkg.CloudSkyError) as e:
            pkg.aerial_shadow_rect(SUNS["deg45"], far)
        assert e.value.code == lib.ERR_INVALID, far
    assert pkg.aerial_shadow_rect(SUNS["deg45"], 0.0) == pkg.aerial_shadow_rect(SUNS["deg45"], 32.0)          # far_km 0 = 32
    center, extent = pkg.aerial_shadow_rect((0.0, 1.0, 0.0), 10.0)
    assert center == (0.0, 0.0) and extent == (20000.0, 20000.0)
    L = pkg.lib()
    p = lib.AerialParams(0, 0, 0, 0, 32.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0))
    two = (C.c_float * 2)()
    assert L.csky_aerial_shadow_rect(None, two, two) == lib.ERR_INVALID and L.csky_aerial_shadow_rect(C.byref(p), None, two) == lib.ERR_INVALID
    assert L.csky_aerial_shadow_rect(C.byref(p), two, None) == lib.ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- C6. rectangle -> map -> volume at sunrise
@pytest.mark.parametrize("view", LOW_VIEWS)
@pytest.mark.parametrize("sun", list(LOW_SUNS))
def test_low_sun_chain(shafts_host, aerial_host, host_luts, shadow_host, chains, oracle, sun, view):  # noqa: F811
    """A map with chord texels (cloudsky.h: the sun's line passes over the cloud base) from the host build of the shadow core, inside the volume:
    finite, at the volume's gate against the restatement fed the same map, and alpha is the plain volume's."""
    p, l, center, extent, kind = low_sun_map_args(oracle, sun)
    assert (kind == SHR.CHORD).any()
    shadow, _ = host_map(shadow_host, chains, p, center=center, extent=extent, **LOW_MAP)
    assert np.isfinite(shadow.astype(np.float32)).all() and len(np.unique(bits(shadow)[kind == SHR.CHORD])) > 2
    ref, n_chord, n_tapped = low_sun_reference(host_luts[0], 0, l, shadow, center, extent, kind, view)
    print("%s %s: %d of %d tapped steps project into a chord texel" % (sun, view, n_chord, n_tapped))
    v = LOW_VOLUME
    vw, aspect = case_view(view)
    aspect = 0.0 if vw is None else aspect
    got, st = shafts_volume(shafts_host, 0, host_luts[0], v["W"], v["H"], v["D"], v["S"], v["far"], l, shadow, center, extent, vw, aspect, state=True)
    assert np.isfinite(got.astype(np.float32)).all() and np.isfinite(st).all()
    differ, cancel = AR.gate(got, ref["out"], st[..., :4], ref["L"], what="low sun %s %s" % (sun, view))
    print("low sun %s %s: %d of %d halves differ from the restatement, %d let through as cancellation" % (sun, view, differ, got.size, cancel))
    plain = host_volume(aerial_host, 0, host_luts[0], v["W"], v["H"], v["D"], v["S"], v["far"], l, vw, aspect)
    assert (bits(got[..., 3]) == bits(plain[..., 3])).all() and (bits(got[..., :3]) != bits(plain[..., :3])).any()


# ---------------------------------------------------------------------------------------------------------------- the C ABI, without a GPU
def test_entry_points_reject_a_null_context(pkg):
    L, lib = pkg.lib(), pkg._lib
    p = lib.AerialParams(4, 4, 4, 2, 32.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0))
    sp = lib.ShadowParams(24, 16, (C.c_float * 2)(*M_CENTER), (C.c_float * 2)(*M_EXTENT), 0)
    out = np.zeros((4, 4, 4, 4), np.uint16)
    assert L.csky_render_aerial_perspective_shadowed(None, C.byref(p), None, C.byref(sp), P(bits(M)), P(out)) == lib.ERR_INVALID
    assert L.csky_render_aerial_perspective_shadowed_device(None, C.byref(p), None, C.byref(sp), P(bits(M)), 48, P(out), None) == lib.ERR_INVALID
    assert b"ctx is NULL" in L.csky_last_error(None)
    assert L.csky_abi_version() == 9
