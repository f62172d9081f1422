"""The per-lane code of the depth frame and of the aerial step for view frames and ray frames (csrc/view_depth_core.h: what the lanes of
depth_rays_kernel and cloud_aerial_rays_kernel run), compiled for the host by tests/view_depth_host.  Fed the hemisphere grid's own directions it must
give the bytes of the hemisphere forms' host cores (tests/cloud_aerial_host); a camera view is held to the numpy restatement of the definition
(tests/view_depth_reference.py) with the gates of tests/test_cloud_aerial_host.py; a direction the march does not accept gives a zero depth texel,
an untouched cloud texel and no sample.  A unit test of device code, not a render path: libcloudsky itself has no CPU implementation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloud_depth_reference as CR
import clouds_rays_reference as RR
import shadow_reference as SR
import view_depth_reference as VR
from conftest import ROOT
from test_aerial_host import SUNS, aerial_host, host_luts  # noqa: F401  (the module-scoped fixtures)
from test_cloud_aerial_host import H, W, bits, ca_host, chains, golden_cloud, host_apply, host_depth  # noqa: F401
from test_clouds_rays_host import _rejected_directions, grid, host_view_dirs, rays_host  # noqa: F401
from test_tlut_mapping import tlut_host  # noqa: F401

F = np.float32
V = RR.VIEW                                                          # 64 x 36, fov 70, pitch 25, yaw 40
BASIS = RR.camera_basis(V["pitch"], V["yaw"])


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def vd_host():
    d = os.path.join(ROOT, "tests", "view_depth_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libview_depth_host.so"))
    L.view_depth_host_view_dirs.restype = None
    L.view_depth_host_view_dirs.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p]
    L.view_depth_host_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.view_depth_host_apply.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    return L


def _view(view):
    """(basis pointer's array, fov) of view = (basis, fov) or None"""
    if view is None:
        return None, 0.0
    return RR.column_major(view[0]), float(view[1])


def vd_view_dirs(L, basis, fov, w, h):
    d = np.zeros((h, w, 3), F)
    L.view_depth_host_view_dirs(P(RR.column_major(basis)), float(fov), w, h, P(d))
    return d


def vd_depth(L, chains, params, width, height, steps, dirs=None, view=None, window=True):  # noqa: F811
    """The host core's depth frame of a ray frame (dirs float32 [h, w, 3]) or of a view (basis, fov): host_depth's dict."""
    assert (dirs is None) != (view is None)
    out = np.zeros((height, width, 4), np.uint16)
    t0, ss = np.zeros((height, width), F), np.zeros((height, width), F)
    inc = np.zeros((height, width), np.uint32)
    n = C.c_uint64()
    p = np.ascontiguousarray(params, F)
    d = None if dirs is None else np.ascontiguousarray(dirs, F)
    assert d is None or d.shape == (height, width, 3)
    b, fov = _view(view)
    rc = L.view_depth_host_frame(P(chains[0]), P(chains[1]), P(chains[2]), P(p), width, height, steps, int(window), P(d), P(b), fov, P(out), P(t0), P(ss),
                                 P(inc), C.byref(n))
    assert rc == 0
    return dict(out=out.view(np.float16), t0=t0, ss=ss, incloud=inc.astype(np.int64), taken=n.value)


def vd_apply(L, mapping, trans, cloud, depth, sun, steps, dirs=None, view=None, state=False, in_place=False):
    """The host core's corrected ray frame float16 [h, w, 4] and the number of pixels that did not pass (and (L, Tr) float32 [h, w, 8] with state)."""
    assert (dirs is None) != (view is None)
    tr = np.ascontiguousarray(trans).view(np.uint16)
    c, z = np.ascontiguousarray(cloud, np.float16).copy(), np.ascontiguousarray(depth, np.float16)
    h, w = c.shape[:2]
    out = c if in_place else np.zeros((h, w, 4), np.float16)
    st = np.zeros((h, w, 8), F) if state else None
    s = np.ascontiguousarray(sun, F)
    d = None if dirs is None else np.ascontiguousarray(dirs, F)
    assert d is None or d.shape == (h, w, 3)
    b, fov = _view(view)
    n = C.c_uint64()
    assert L.view_depth_host_apply(mapping, P(tr), tr.shape[1], tr.shape[0], w, h, steps, P(s), P(d), P(b), fov, P(c), P(z), P(out), P(st), C.byref(n)) == 0
    return (out, n.value, st) if state else (out, n.value)


# ---------------------------------------------------------------------------------------------------------------- VH1
@pytest.mark.parametrize("name", ["A", "B"])
def test_grid_directions_give_the_bytes_of_the_hemisphere_depth_core(vd_host, ca_host, rays_host, chains, oracle, name):  # noqa: F811
    p = SR.scene(oracle, name)
    N = CR.STEPS[name]
    d, _ = grid(rays_host, W, H, N)
    ref = host_depth(ca_host, chains, p, W, H, N)
    got = vd_depth(vd_host, chains, p, W, H, N, dirs=d)
    hit = bits(ref["out"]).any(-1)
    print("scene %s: %.1f %% of the pixels in cloud" % (name, 100.0 * hit.mean()))
    assert hit.mean() >= 0.40 and (~hit).mean() >= 0.20
    assert (bits(got["out"]) == bits(ref["out"])).all()
    assert (got["t0"].view(np.uint32) == ref["t0"].view(np.uint32)).all() and (got["ss"].view(np.uint32) == ref["ss"].view(np.uint32)).all()
    assert (got["incloud"] == ref["incloud"]).all() and got["taken"] == ref["taken"]


# ---------------------------------------------------------------------------------------------------------------- VH2
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("steps", [16, 5])
def test_grid_directions_give_the_bytes_of_the_hemisphere_apply_core(vd_host, ca_host, rays_host, chains, oracle, golden_cloud, host_luts, steps, mapping):  # noqa: F811
    d, _ = grid(rays_host, W, H, 128)
    z = host_depth(ca_host, chains, SR.scene(oracle, "A"), W, H, 128)["out"]
    ref = host_apply(ca_host, mapping, host_luts[mapping], golden_cloud, z, SUNS["deg45"], steps)
    got, worked, st = vd_apply(vd_host, mapping, host_luts[mapping], golden_cloud, z, SUNS["deg45"], steps, dirs=d, state=True)
    assert worked == int((~CR.passes(golden_cloud, z)).sum()) and worked >= 0.40 * W * H
    assert (bits(ref) != bits(golden_cloud)).any(-1).sum() >= 0.9 * worked
    assert (bits(got) == bits(ref)).all()
    _, st_ref = host_apply(ca_host, mapping, host_luts[mapping], golden_cloud, z, SUNS["deg45"], steps, state=True)
    assert (st.view(np.uint32) == st_ref.view(np.uint32)).all()
    same, _ = vd_apply(vd_host, mapping, host_luts[mapping], golden_cloud, z, SUNS["deg45"], steps, dirs=d, in_place=True)
    assert (bits(same) == bits(ref)).all()                        # out may be the cloud frame


# ---------------------------------------------------------------------------------------------------------------- VH3
def test_view_form_matches_the_restatement(vd_host, rays_host, chains, oracle, otex):  # noqa: F811
    w, h, N = V["width"], V["height"], 128
    d = vd_view_dirs(vd_host, BASIS, V["fov"], w, h)
    assert (d.view(np.uint32) == host_view_dirs(rays_host, BASIS, V["fov"], w, h).view(np.uint32)).all()
    p = SR.scene(oracle, "A")
    ref = VR.depth_frame_dirs(oracle, otex, p, d, N)
    hit = ref["hit"]
    thin = hit & (ref["alpha"] > 0) & (ref["alpha"] < CR.THIN)
    print("view restated: %.1f %% of the pixels in cloud, %.1f %% empty, %.1f %% of the in-cloud pixels thinner than 2^-6"
          % (100.0 * hit.mean(), 100.0 * (~hit).mean(), 100.0 * thin.sum() / hit.sum()))
    assert hit.mean() >= 0.40 and (~hit).mean() >= 0.20          # preconditions on the RESTATEMENT: an empty or a full frame cannot pass
    assert thin.sum() <= 0.05 * hit.sum()
    got = vd_depth(vd_host, chains, p, w, h, N, view=(BASIS, V["fov"]))
    via_dirs = vd_depth(vd_host, chains, p, w, h, N, dirs=d)
    assert (bits(via_dirs["out"]) == bits(got["out"])).all() and via_dirs["taken"] == got["taken"]
    up = ref["above"]
    assert (up == (d[..., 1] > 0)).all() and (~up).mean() >= 0.10
    assert (got["t0"][up].view(np.uint32) == ref["t0"][up].view(np.uint32)).all() and (got["ss"][up].view(np.uint32) == ref["ss"][up].view(np.uint32)).all()
    assert not got["t0"][~up].any() and not got["ss"][~up].any()
    same = got["incloud"] == ref["incloud"]
    differ = int((~same & (hit | (got["incloud"] > 0))).sum())
    print("view: %d pixels whose in-cloud sample count differs from the restatement's (of %d in cloud); samples %d vs %d"
          % (differ, int(hit.sum()), int(got["incloud"].sum()), int(ref["incloud"].sum())))
    assert differ <= 0.005 * hit.sum()
    sel = same & hit
    o, r = bits(got["out"]), bits(ref["out"])
    assert (o[sel][:, 1:3] == r[sel][:, 1:3]).all()               # front, back: bit-equal
    assert (o[same & ~hit] == 0).all()
    thick = sel & (ref["alpha"] >= CR.THIN)
    assert thick.sum() >= 0.9 * hit.sum()
    SR.assert_gate(got["out"][..., 0][thick], ref["out"][..., 0][thick], "view depth core, mean distance")
    SR.assert_gate(got["out"][..., 3][sel], ref["out"][..., 3][sel], "view depth core, alpha")
    g = got["out"].astype(F)
    nz = o.any(-1)
    assert (g[nz][:, 1] <= g[nz][:, 0]).all() and (g[nz][:, 0] <= g[nz][:, 2]).all()
    # the height window and its wave-uniform exit are exact: the same bytes without them, from every sample
    nowin = vd_depth(vd_host, chains, p, w, h, N, view=(BASIS, V["fov"]), window=False)
    assert (bits(nowin["out"]) == o).all() and (nowin["incloud"] == got["incloud"]).all()
    assert nowin["taken"] == int(up.sum()) * N and got["taken"] <= nowin["taken"]


# ---------------------------------------------------------------------------------------------------------------- VH4
def test_directions_that_are_not_accepted(vd_host, chains, oracle, host_luts):  # noqa: F811
    bad = _rejected_directions()                                  # e.y = 0, -0, < 0; |e|^2 = 0.98, 1.02; 0; NaN and +-inf in every component
    n = len(bad)
    assert not RR.accept(bad).any()
    d = bad.reshape(1, n, 3)
    p = SR.scene(oracle, "A")
    got = vd_depth(vd_host, chains, p, n, 1, 128, dirs=d)
    assert not bits(got["out"]).any() and got["taken"] == 0 and not got["incloud"].any()
    assert not got["t0"].any() and not got["ss"].any()
    cloud = np.zeros((1, n, 4), np.float16)
    cloud[..., :3] = (0.5, 0.25, 0.125)
    cloud[..., 3] = 0.75
    z = np.zeros((1, n, 4), np.float16)
    z[..., :3] = (12.0, 8.0, 20.0)
    z[..., 3] = 0.75
    up = np.tile(np.array([0.6, 0.8, 0.0], F), (1, n, 1))
    for mapping in (0, 1):
        out, worked = vd_apply(vd_host, mapping, host_luts[mapping], cloud, z, SUNS["deg45"], 16, dirs=d)
        assert worked == 0 and (bits(out) == bits(cloud)).all()
        moved, worked = vd_apply(vd_host, mapping, host_luts[mapping], cloud, z, SUNS["deg45"], 16, dirs=up)   # the same texels along an accepted direction do not pass
        assert worked == n and (bits(moved)[..., :3] != bits(cloud)[..., :3]).all() and (bits(moved)[..., 3] == bits(cloud)[..., 3]).all()
