"""The front end of the direct cloud march (csrc/rays_core.h: what the lanes of clouds_rays_kernel run in front of the march), compiled for the host
by tests/rays_host, and cloud_core.h's ray_setup behind it, held to the host frame of tests/hostsim and to the numpy restatement of their definition
(tests/clouds_rays_reference.py, tests/ray_reference.py).  A unit test of device code, not a render path: libcloudsky itself has no CPU implementation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clouds_rays_reference as RR
import ray_reference as XR
from conftest import ROOT, SUNS, norm
from test_hostsim_core import hs_clouds

F = np.float32


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def rays_host():
    d = os.path.join(ROOT, "tests", "rays_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "librays_host.so"))
    for f in ("rays_host_grid", "rays_host_view_dirs", "rays_host_accept", "rays_host_march", "rays_host_walk", "rays_host_composite"):
        getattr(L, f).restype = None
    L.rays_host_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.rays_host_view_dirs.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p]
    L.rays_host_accept.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.rays_host_march.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.rays_host_walk.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.rays_host_composite.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def chains(pkg, noise):
    large, small, weather = noise
    return pkg.assets.build_mips(large, 8), pkg.assets.build_mips(small, 6), np.ascontiguousarray(weather, np.uint8)


def grid(L, w, h, steps):
    """(dirs [h, w, 3], ray_setup's fields [h, w, 11]) of a w x h hemisphere frame"""
    d, a = np.zeros((h, w, 3), F), np.zeros((h, w, 11), F)
    L.rays_host_grid(w, h, steps, P(d), P(a))
    return d, a


def host_view_dirs(L, basis, fov, w, h):
    d = np.zeros((h, w, 3), F)
    L.rays_host_view_dirs(P(RR.column_major(basis)), float(fov), w, h, P(d))
    return d


def host_march(L, chains, params, sky, dirs, primary=128, light=6, eps=0.0, window=True):
    """The host core's texels of the directions float32 [..., 3]: (float16 [..., 4], marched bool [...], in-cloud samples int64 [...])"""
    d = np.ascontiguousarray(dirs, F)
    n = d.size // 3
    out, marched, inc = np.zeros((n, 4), np.uint16), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    p = np.ascontiguousarray(params, F)
    s = np.ascontiguousarray(sky).view(np.uint16)
    L.rays_host_march(P(chains[0]), P(chains[1]), P(chains[2]), P(p), primary, light, eps, P(s), s.shape[1], s.shape[0], int(window), n, P(d), P(out), P(marched), P(inc))
    shp = d.shape[:-1]
    return out.view(np.float16).reshape(shp + (4,)), marched.astype(bool).reshape(shp), inc.astype(np.int64).reshape(shp)


def host_composite(L, mode, basis, fov, out_w, out_h, cf, ct, sf, st, trans, blend, sds, sun):
    a = [np.ascontiguousarray(x).view(np.uint16) for x in (cf, ct, sf, st, trans)]
    out = np.zeros((out_h, out_w, 4), np.uint16)
    s = np.ascontiguousarray(sun, F)
    L.rays_host_composite(mode, out_w, out_h, P(RR.column_major(basis)), float(fov), P(a[0]), P(a[1]), a[0].shape[1], a[0].shape[0], P(a[2]), P(a[3]), a[2].shape[1],
                          a[2].shape[0], P(a[4]), a[4].shape[1], a[4].shape[0], float(blend), float(sds), P(s), P(out))
    return out


# ---- H1
@pytest.mark.parametrize("w,h", [(64, 32), (37, 21)])
@pytest.mark.parametrize("steps", [128, 30])
def test_ray_setup_is_the_numpy_restatement_of_the_ray_bit_for_bit(rays_host, w, h, steps):
    """All eleven fields of ray_setup(i, j), which is ray_from_dir(pixel_dir(i, j)), against the restatement of the definition: `above` and the zero
    fields under the horizon included."""
    e = XR.pixel_dirs(w, h)
    up = e[..., 1] > 0
    assert up.sum() > 0.9 * w * h                            # the RESTATEMENT's rays are above the horizon but for the grid's rim
    r = XR.ray(e, steps)
    want = np.concatenate([r["p"], r["inc"], r["dir"], r["ss"][..., None], np.ones((h, w, 1), F)], -1)
    want = np.where(up[..., None], want, F(0.0))
    assert want.dtype == F and want.shape == (h, w, 11)
    d, got = grid(rays_host, w, h, steps)
    assert (d.view(np.uint32) == e.view(np.uint32)).all()
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


# ---- H2
@pytest.mark.parametrize("sun", ["deg45", "zenith"])
def test_host_march_over_the_grid_directions_gives_the_bytes_of_the_host_frame(rays_host, hostsim, pkg, oracle, noise, chains, o_skies, sun):
    p = oracle.default_params(64, 32, SUNS[sun])
    ref, ic_ref = hs_clouds(hostsim, pkg, noise, p, o_skies[sun], 64, (8, 0, 1, 4))
    d, _ = grid(rays_host, 64, 32, 128)
    q = p.copy()
    q[0:4] = np.nan                                          # texture_size and update_position are not read
    img, marched, inc = host_march(rays_host, chains, q, o_skies[sun], d)
    assert (img.view(np.uint16) == ref.view(np.uint16)).all()
    assert int(inc.sum()) == ic_ref and ic_ref > 0


# ---- H3
def _rejected_directions():
    base = np.array([0.6, 0.8, 0.0], F)
    out = []
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            e = base.copy(); e[k] = bad
            out.append(e)
    out.append(np.zeros(3, F))
    out.append(base * F(0.99))                               # |e|^2 = 0.9801
    out.append(base * F(1.01))                               # |e|^2 = 1.0201
    for y in (0.0, -0.0, -1e-3):
        e = np.array([np.sqrt(1.0 - y * y), y, 0.0], F)
        out.append(e)
    return np.stack(out).astype(F)


def test_accept_rule(rays_host, chains, oracle, o_skies):
    p = oracle.default_params(64, 32, SUNS["deg45"])
    bad = _rejected_directions()
    ok = np.zeros(len(bad), np.uint8)
    rays_host.rays_host_accept(len(bad), P(bad), P(ok))
    assert not ok.any() and not RR.accept(bad).any()
    img, marched, inc = host_march(rays_host, chains, p, o_skies["deg45"], bad)
    assert (img.view(np.uint16) == 0).all()
    assert int(marched.sum()) == 0 and int(inc.sum()) == 0   # no ray marches: no sample is taken
    base = np.array([0.6, 0.8, 0.0], np.float64)
    good = np.stack([base * np.sqrt(0.995), base * np.sqrt(1.005)]).astype(F)
    ok = np.zeros(2, np.uint8)
    rays_host.rays_host_accept(2, P(good), P(ok))
    assert ok.all() and RR.accept(good).all()
    img, marched, _ = host_march(rays_host, chains, p, o_skies["deg45"], good)
    assert marched.all() and np.isfinite(img.astype(F)).all()
    # the band's own ends, and the rule on random directions against the restatement
    rng = np.random.default_rng(7)
    e = rng.normal(size=(4096, 3)).astype(F)
    e /= np.linalg.norm(e, axis=1, keepdims=True).astype(F)
    e *= rng.uniform(0.98, 1.02, size=(4096, 1)).astype(F)
    ok = np.zeros(len(e), np.uint8)
    rays_host.rays_host_accept(len(e), P(np.ascontiguousarray(e)), P(ok))
    assert (ok.astype(bool) == RR.accept(e)).all()
    assert 0 < ok.sum() < len(e)


# ---- H4
@pytest.mark.parametrize("steps", [128, 1024])
def test_grazing_rays_meet_the_preconditions_of_sqrt_shell_and_of_the_early_march_end(rays_host, steps):
    """Unit directions the grid never has, down to 1e-7 above the horizon: the radius never decreases along the primary samples, and every |p|^2 of
    a primary or light sample lies inside the range sqrt_shell is proven on.  Light samples under four suns, one of them under the horizon."""
    dirs = []
    for y in (1e-7, 1e-5, 1e-3, 0.05):
        for k in range(8):
            az = 2.0 * np.pi * (k + 0.3) / 8.0
            c = np.sqrt(1.0 - y * y)
            dirs.append([c * np.cos(az), y, c * np.sin(az)])
    dirs = np.ascontiguousarray(dirs, F)
    assert RR.accept(dirs).all()
    for sun in (SUNS["zenith"], SUNS["deg45"], SUNS["demo"], (0.3, -0.9, 0.1)):
        out = np.zeros(6, np.float64)
        s = norm(sun)
        rays_host.rays_host_walk(len(dirs), P(dirs), steps, P(s), P(out))
        assert out[0] == len(dirs)
        assert out[1] == 0, (sun, out)                       # the radius never decreases
        assert out[2] == 0, (sun, out)                       # every |p|^2 inside [SHELL_SQRT_LO, SHELL_SQRT_HI]
        assert out[3] > 0.0


# ---- H5
def test_numpy_view_directions_equal_the_core_bit_for_bit(rays_host):
    v = RR.VIEW
    basis = RR.camera_basis(v["pitch"], v["yaw"])
    got = host_view_dirs(rays_host, basis, v["fov"], v["width"], v["height"])
    ref = RR.view_dirs(basis, v["fov"], v["width"], v["height"])
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()
    assert RR.accept(got[0]).all() and not RR.accept(got[-1]).any()   # the top row looks up, the bottom row under the horizon


# ---- H6
def test_cloud_mode_1_with_constant_frames_gives_the_bytes_of_mode_0(rays_host, o_trans, o_skies):
    v = RR.VIEW
    W, H = v["width"], v["height"]
    basis = RR.camera_basis(v["pitch"], v["yaw"])
    sun = norm(SUNS["deg45"])
    sf, st = o_skies["deg45"], o_skies["zenith"]

    def both(texel_from, texel_to, blend):
        hemi = [np.broadcast_to(np.asarray(t, np.float16), (8, 16, 4)).copy() for t in (texel_from, texel_to)]
        view = [np.broadcast_to(np.asarray(t, np.float16), (H, W, 4)).copy() for t in (texel_from, texel_to)]
        a = host_composite(rays_host, 0, basis, v["fov"], W, H, hemi[0], hemi[1], sf, st, o_trans, blend, 2.0, sun)
        b = host_composite(rays_host, 1, basis, v["fov"], W, H, view[0], view[1], sf, st, o_trans, blend, 2.0, sun)
        return a, b
    a, b = both((0, 0, 0, 0), (0, 0, 0, 0), 0.3)
    assert (a == b).all()
    a, b = both((0.25, 0.5, 0.125, 0.75), (1.5, 0.0625, 0.3, 0.2), 0.3)
    assert (a == b).all()
    z, _ = both((0, 0, 0, 0), (0, 0, 0, 0), 0.3)
    assert (a != z).any()                                    # the cloud texels reach the output


def test_cloud_mode_1_reads_the_texel_of_the_output_pixel(rays_host, o_trans, o_skies):
    """A view frame that is opaque black in one pixel only changes that output pixel only."""
    v = RR.VIEW
    W, H = v["width"], v["height"]
    basis = RR.camera_basis(v["pitch"], v["yaw"])
    sun = norm(SUNS["deg45"])
    sf = o_skies["deg45"]
    clear = np.zeros((H, W, 4), np.float16)
    one = clear.copy()
    one[5, 9] = (0, 0, 0, 1)
    a = host_composite(rays_host, 1, basis, v["fov"], W, H, clear, clear, sf, sf, o_trans, 0.0, 2.0, sun)
    b = host_composite(rays_host, 1, basis, v["fov"], W, H, one, one, sf, sf, o_trans, 0.0, 2.0, sun)
    diff = (a != b).any(axis=-1)
    assert diff[5, 9] and diff.sum() == 1
