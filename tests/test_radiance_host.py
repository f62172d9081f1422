"""Radiance cubemap on the CPU: csrc/radiance_core.h compiled for the host (tests/radiance_host) against the independent numpy restatement of
the contract (tests/radiance_reference.py), plus the Python binding's argument checks that need no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import radiance_reference as R
from conftest import ulp_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rh():
    d = os.path.join(ROOT, "tests", "radiance_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libradiance_host.so"))
    L.rad_host_cones.restype = C.c_int
    return L


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def core_dirs(rh, n):
    out = np.zeros((6, n, n, 3), np.float32)
    rh.rad_host_dirs(n, P(out))
    return out


@pytest.mark.parametrize("n", [1, 2, 8, 16, 64])
def test_core_directions_invert_to_their_own_texel(rh, n):
    d = core_dirs(rh, n)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max() < 1e-6
    face, i, j = R.dir_to_texel(d, n)
    F, J, I = np.meshgrid(np.arange(6), np.arange(n), np.arange(n), indexing="ij")
    assert (face == F).all() and (i == I).all() and (j == J).all()
    assert np.abs(d - R.face_dirs(n)).max() < 1e-6


@pytest.mark.parametrize("n", [1, 8, 16, 64, 512])
def test_solid_angles_sum_to_4pi(rh, n):
    om = np.zeros((n, n), np.float64)
    rh.rad_host_solid_angles(n, P(om))
    assert abs(6.0 * om.sum() - 4.0 * np.pi) < 1e-5
    assert np.abs(om - R.solid_angles(n)).max() < 1e-12
    assert (om > 0).all()


@pytest.mark.parametrize("n", [8, 16, 64])
def test_block_cones_bound_their_texels(rh, n):
    nb = 6 * (n // min(n, 8)) ** 2
    cones = np.zeros((nb, 4), np.float32)
    assert rh.rad_host_cones(n, P(cones)) == nb
    d = R.face_dirs(n)
    bs = min(n, 8)
    k = 0
    for f in range(6):
        for by in range(n // bs):
            for bx in range(n // bs):
                blk = d[f, by * bs:(by + 1) * bs, bx * bs:(bx + 1) * bs].reshape(-1, 3)
                ang = np.arccos(np.clip(blk @ cones[k, :3].astype(np.float64), -1, 1))
                assert ang.max() < cones[k, 3], (f, by, bx)
                k += 1


def host_prefilter(rh, cube, L, Ss):
    S = cube.shape[1]
    out = np.zeros((L - 1, 6, S, S, 4), np.float32)
    rh.rad_host_prefilter(P(cube.view(np.uint16)), S, L, Ss, P(out))
    return out


# every layer count 2..10 (filter kernel NL = 1..9), source blocks smaller than 8 x 8 (Ss < 8) with a non-constant cube
@pytest.mark.parametrize("S,Ss,L", [(8, 8, 8), (16, 16, 8), (16, 8, 5), (16, 4, 10), (8, 8, 2), (16, 2, 3), (8, 1, 4), (16, 16, 6), (32, 4, 7),
                                    (16, 8, 9)])
def test_host_filter_matches_numpy(rh, S, Ss, L):
    cube = R.smooth_cube(S, S + Ss)
    out = host_prefilter(rh, cube, L, Ss)
    ref = R.prefilter(cube.astype(np.float64), L, Ss).reshape(L - 1, 6, S, S, 3)
    rel = np.abs(out[..., :3] - ref) / np.abs(ref)
    assert rel.max() < 1e-5, rel.max()


# (S, Ss, relative bound).  At 512/2 one receiver sees the disc's source texel at c = N.L ~ 2e-3, where the filter's fp32 c = 1 - e2/2
# (about 1e-7 absolute) is 1e-5 relative: that is the filter's own arithmetic, not the block mean, hence 2e-5 there
@pytest.mark.parametrize("S,Ss,rtol", [(512, 1, 1e-5), (512, 2, 2e-5), (512, 4, 1e-5), (256, 1, 1e-5)])
def test_host_filter_bright_disc_large_reduction(rh, S, Ss, rtol):
    """A 30000 disc in a smooth cube, source texels that average up to 512 x 512 layer-0 texels: the block mean must stay accurate (the GPU
    gate of tests/test_radiance_gpu.py check_filtered, and a relative gate)."""
    L = 3
    cube = R.hdr_cube(S, 30000.0)
    out = host_prefilter(rh, cube, L, Ss)
    ref = R.prefilter(cube.astype(np.float64), L, Ss, chunk=65536).reshape(L - 1, 6, S, S, 3)
    assert np.isfinite(out).all()
    d = ulp_diff(out[..., :3].astype(np.float16), ref.astype(np.float16))
    assert d.max() <= 2 and (d <= 1).mean() >= 0.99, (d.max(), (d <= 1).mean())
    rel = np.abs(out[..., :3] - ref) / np.abs(ref)
    assert rel.max() < rtol, rel.max()


def test_numpy_reference_known_answers():
    S = 16
    d = R.face_dirs(S)
    const = np.ones((6, S, S, 4)) * np.array([0.75, 1.5, 3.0, 1.0])
    p = R.prefilter(const, 8, S)
    assert np.abs(p - np.array([0.75, 1.5, 3.0])).max() < 1e-12
    lin = np.ones((6, S, S, 4))
    lin[..., :3] = 1.0 + 0.5 * d[..., 1:2]
    top = R.prefilter(lin, 8, S)[-1].reshape(6, S, S, 3)
    assert np.abs(top[..., 0] / (1.0 + d[..., 1] / 3.0) - 1.0).max() < 5e-3


def test_binding_rejects_bad_cubes(pkg):
    """prefilter_cube checks the shape before it touches the library (no GPU needed)."""
    ctx = object.__new__(pkg._lib.Context)           # an unopened context: the shape check comes first
    with pytest.raises(ValueError):
        pkg._lib.Context.prefilter_cube(ctx, np.zeros((5, 8, 8, 4), np.float16))
    with pytest.raises(ValueError):
        pkg._lib.Context.prefilter_cube(ctx, np.zeros((6, 8, 4, 4), np.float16))
