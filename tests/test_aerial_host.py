"""The aerial-perspective volume's per-lane code (csrc/aerial_core.h on lut_core.h and composite_core.h: the definition aerial.hip's wavefronts
must equal), compiled for the host by tests/aerial_host, against the reference's sky LUT (the anchor) and the numpy restatement of the contract
(tests/aerial_reference.py).  A unit test of device code, not a render path: libcloudsky itself has no CPU implementation.

The gate is the project's sky-LUT gate, every half within 1 fp16 ulp: it is the same per-step code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aerial_reference as AR
import tlut_reference as TR
from conftest import ROOT, ulp_diff
from test_tlut_mapping import host_trans, tlut_host  # noqa: F401  (tlut_host: the module-scoped fixture)

SUNS = {"deg45": TR.norm(TR.SUNS["deg45"]), "demo": TR.norm(TR.SUNS["demo"]), "degm2": TR.norm(TR.SUNS["degm2"])}   # degm2: 2 degrees under the horizon
# (name, W, H, D, S, far_km, view (yaw, pitch, fov) or None, aspect)
CASES = {
    "up": (13, 7, 5, 3, 40.0, (30.0, 10.0, 70.0), 16.0 / 9.0),
    "down": (13, 7, 5, 3, 64.0, (30.0, -30.0, 70.0), 16.0 / 9.0),
    "panorama": (16, 8, 6, 3, 40.0, None, 0.0),
}


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def aerial_host():
    d = os.path.join(ROOT, "tests", "aerial_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libaerial_host.so"))
    L.aerial_host_volume.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.aerial_host_columns.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.aerial_host_sky_texels.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    return L


def case_view(case):
    """(view as the restatement and the Python mirror take it, or None; aspect)"""
    v = CASES[case][5]
    return (None if v is None else (AR.camera_basis(v[0], v[1]), v[2])), CASES[case][6]


def host_volume(L, mapping, trans, W, H, D, S, far_km, sun, view=None, aspect=0.0, state=False):
    """The host core's volume float16 [D, H, W, 4] (and the spectral (L, Tr) float32 [D, H, W, 8] with state=True)."""
    tr = np.ascontiguousarray(trans).view(np.uint16)
    out = np.zeros((D, H, W, 4), np.uint16)
    st = np.zeros((D, H, W, 8), np.float32) if state else None
    cam = np.ascontiguousarray(np.asarray(view[0], np.float32).T.reshape(-1)) if view is not None else np.zeros(9, np.float32)   # column-major
    s = np.ascontiguousarray(sun, np.float32)
    rc = L.aerial_host_volume(mapping, P(tr), tr.shape[1], tr.shape[0], W, H, D, S, float(far_km), P(s), int(view is not None), P(cam),
                              float(view[1]) if view is not None else 0.0, float(aspect), P(out), P(st))
    assert rc == 0
    return (out.view(np.float16), st) if state else out.view(np.float16)


def host_columns(L, mapping, trans, e, far_km, sun, D, S):
    """Columns given by their EYEDIRs [n, 3] and reaches [n]: float16 [n, D, 4]."""
    tr = np.ascontiguousarray(trans).view(np.uint16)
    e, far = np.ascontiguousarray(e, np.float32), np.ascontiguousarray(far_km, np.float32)
    out = np.zeros((e.shape[0], D, 4), np.uint16)
    s = np.ascontiguousarray(sun, np.float32)
    assert L.aerial_host_columns(mapping, P(tr), tr.shape[1], tr.shape[0], e.shape[0], P(e), P(far), P(s), D, S, P(out), None) == 0
    return out.view(np.float16)


@pytest.fixture(scope="module")
def host_luts(tlut_host):  # noqa: F811
    return {m: host_trans(tlut_host, m) for m in (0, 1)}


def anchor_texels():
    """About 200 texels of the 200 x 100 sky LUT: the horizon rows 48-52 and rows from the nadir to the zenith; the rows up to 45 look at the ground (the horizon dips 0.72 degrees)."""
    px, py = [], []
    for row in (48, 49, 50, 51, 52):
        for col in range(3, 200, 10):
            px.append(col); py.append(row)
    for row in (0, 5, 20, 35, 45, 47, 53, 60, 75, 99):
        for col in range(7, 200, 20):
            px.append(col); py.append(row)
    return np.array(px, np.int32), np.array(py, np.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. the anchor
@pytest.mark.parametrize("sun", ["deg45", "demo"])
def test_anchor_last_slice_is_the_sky_lut_texel(aerial_host, o_trans, o_skies, sun):
    s = SUNS[sun]
    px, py = anchor_texels()
    n = px.size
    assert 190 <= n <= 210
    tr = np.ascontiguousarray(o_trans).view(np.uint16)
    texel, rd, t_d = np.zeros((n, 4), np.uint16), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    aerial_host.aerial_host_sky_texels(0, P(tr), 256, 64, 200, 100, P(s), n, P(px), P(py), P(texel), P(rd), P(t_d))
    # the core: ray_dir = (-e.x, -e.z, e.y) is exact in fp32, so e = (-rd.x, rd.z, -rd.y) hands the column the texel's own direction floats
    e = np.stack([-rd[:, 0], rd[:, 2], -rd[:, 1]], -1)
    col = host_columns(aerial_host, 0, o_trans, e, t_d, s, 30, 1)
    assert (col[:, 29, :3].view(np.uint16) == texel[:, :3]).all()                 # bit for bit
    lut = o_skies[sun][py, px]
    assert ulp_diff(col[:, 29, :3], lut[:, :3]).max() <= 1
    assert ulp_diff(texel.view(np.float16)[:, :3], lut[:, :3]).max() <= 1
    # the restatement, from the WORLD direction of the same texels: pins the e -> LUT-frame mapping to the compositor's convention
    ew = AR.sky_texel_eyedir(px, py)
    far, hits = AR.ray_length(ew)
    assert hits.sum() >= 40 and (~hits).sum() >= 100                               # rays that hit the ground, and rays that do not
    assert np.abs(far - t_d).max() <= 1e-3 * t_d.max()
    r = AR.columns(ew, s, far, 30, 1, o_trans)
    assert (r["taken"] == 30).all()
    d = ulp_diff(r["out"][29][:, :3], lut[:, :3])
    print("anchor %s: restatement vs oracle sky LUT max %d fp16 ulp, %.2f %% of halves differ" % (sun, d.max(), 100.0 * (d > 0).mean()))
    assert d.max() <= 1
    # an unflipped axis is far outside the gate: the mapping is really pinned (both suns lie in the x-y plane: it is x that tells)
    wrong = AR.columns(np.stack([-ew[:, 0], ew[:, 1], ew[:, 2]], -1), s, far, 30, 1, o_trans)
    assert ulp_diff(wrong["out"][29][:, :3], lut[:, :3]).max() > 8


# ---------------------------------------------------------------------------------------------------------------- 2. core against restatement
@pytest.fixture(scope="module")
def restated(host_luts):
    """The restatement's volumes of every (case, sun, mapping), computed once (the GPU tests share them)."""
    cache = {}

    def get(case, sun, mapping):
        k = (case, sun, mapping)
        if k not in cache:
            W, H, D, S, far = CASES[case][:5]
            view, aspect = case_view(case)
            cache[k] = AR.volume(W, H, D, S, far, SUNS[sun], host_luts[mapping], mapping, view, aspect)
        return cache[k]
    return get


@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("case", list(CASES))
def test_core_matches_the_restatement(aerial_host, host_luts, restated, case, sun, mapping):
    W, H, D, S, far = CASES[case][:5]
    view, aspect = case_view(case)
    ref = restated(case, sun, mapping)
    assert not ref["near"].any()                                                   # the cameras are chosen so that no column has to be left out
    a = ref["out"][D - 1][..., 3].astype(np.float32)
    assert a.max() - a.min() >= 0.2                                                # preconditions on the REFERENCE: a blank volume cannot pass
    if case == "down":
        assert (ref["t_stop"] < np.float32(far)).mean() >= 0.25
    assert np.isfinite(ref["out"].astype(np.float32)).all()
    got, st = host_volume(aerial_host, mapping, host_luts[mapping], W, H, D, S, far, SUNS[sun], view, aspect, state=True)
    differ, cancel = AR.gate(got, ref["out"], st[..., :4], ref["L"], what="%s %s mapping %d" % (case, sun, mapping))
    print("%s %s mapping %d: %d of %d halves differ from the restatement, %d let through as cancellation in M * L" % (case, sun, mapping, differ, got.size, cancel))
    assert cancel == 0                                                             # (DESIGN.md §14 records this count)


# ---------------------------------------------------------------------------------------------------------------- 3. exact structure
def test_exact_structure(aerial_host, host_luts):
    view, aspect = case_view("down")
    s, t = SUNS["deg45"], host_luts[0]
    fine = host_volume(aerial_host, 0, t, 13, 7, 16, 2, 64.0, s, view, aspect).view(np.uint16)
    coarse = host_volume(aerial_host, 0, t, 13, 7, 8, 4, 64.0, s, view, aspect).view(np.uint16)
    assert (coarse == fine[1::2]).all()                                            # (D = 8, S = 4) is every second slice of (D = 16, S = 2)
    # slices past a column's stop are the slice of its last taken step (the restatement says which that is)
    ref = AR.volume(13, 7, 16, 2, 64.0, s, t, 0, view, aspect)
    assert not ref["near"].any()
    last = np.maximum((ref["taken"] + 1) // 2 - 1, 0)                              # the slice that holds the last taken step
    stopped = ref["taken"] < 32
    assert stopped.mean() >= 0.25
    for j, i in zip(*np.nonzero(stopped)):
        assert (fine[last[j, i]:, j, i] == fine[last[j, i], j, i]).all(), (i, j)
    a = fine.view(np.float16)[..., 3].astype(np.float32)
    assert (np.diff(a, axis=0) <= 0).all()                                         # alpha never increases with k
    assert a[-1].max() - a[-1].min() >= 0.2
    tiny = host_volume(aerial_host, 0, t, 13, 7, 4, 2, 1e-3, s, view, aspect)
    assert (tiny.view(np.uint16)[..., 3] == 0x3C00).all() and np.abs(tiny[..., :3].astype(np.float32)).max() < 1e-3


def test_towards_the_sun_is_brighter(aerial_host, host_luts):
    """deg45, the panorama's row nearest the sun's elevation: the column nearest e = (+x, y, 0) against the one nearest (-x, y, 0)."""
    s, t = SUNS["deg45"], host_luts[0]
    ref = AR.volume(16, 8, 6, 3, 40.0, s, t)["out"][5].astype(np.float32)
    e = AR.eyedir_panorama(16, 8)
    assert e[2, 8, 0] > 0.8 and e[2, 0, 0] < -0.8 and abs(e[2, 8, 1] - e[2, 0, 1]) < 1e-6 and e[2, 8, 1] > 0.3
    ratio = ref[2, 8, :3].sum() / ref[2, 0, :3].sum()
    assert ratio >= 1.5                                                            # precondition, from the restatement
    got = host_volume(aerial_host, 0, t, 16, 8, 6, 3, 40.0, s)[5].astype(np.float32)
    assert abs(got[2, 8, :3].sum() / got[2, 0, :3].sum() - ratio) <= 0.01 * ratio


# ---------------------------------------------------------------------------------------------------------------- the C ABI, without a GPU
def test_entry_points_reject_a_null_context(pkg):
    L, lib = pkg.lib(), pkg._lib
    p = lib.AerialParams(4, 4, 4, 2, 32.0, 0.0, (C.c_float * 3)(0.6, 0.8, 0.0))
    out = np.zeros((4, 4, 4, 4), np.uint16)
    assert L.csky_render_aerial_perspective(None, C.byref(p), None, P(out)) == lib.ERR_INVALID
    assert L.csky_render_aerial_perspective_device(None, C.byref(p), None, P(out), None) == lib.ERR_INVALID
    assert b"ctx is NULL" in L.csky_last_error(None)
    assert C.sizeof(lib.AerialParams) == 36 and C.sizeof(lib.View) == 40
