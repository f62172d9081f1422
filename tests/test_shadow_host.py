"""The cloud shadow map's per-lane code (csrc/shadow_core.h on the cloud cores: what shadow.hip's lanes run), compiled for the host by
tests/shadow_host, against the numpy restatement of the definition (tests/shadow_reference.py, which calls the oracle per sample).
A unit test of device code, not a render path: libcloudsky itself has no CPU implementation.

The gate is the project's own for values rendered from the shipped assets (tests/parity_metrics.py) on the one channel: every texel within 2 fp16 ulp,
99.9 % within 1, largest difference 2e-3.  It rests on the sample positions being bit-identical (the first test checks exactly that)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shadow_reference as SR
from conftest import ROOT


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def shadow_host():
    d = os.path.join(ROOT, "tests", "shadow_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libshadow_host.so"))
    L.shadow_host_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.POINTER(C.c_uint64)]
    return L


@pytest.fixture(scope="module")
def chains(pkg, noise):
    large, small, weather = noise
    return pkg.assets.build_mips(large, 8), pkg.assets.build_mips(small, 6), np.ascontiguousarray(weather, np.uint8)


def host_map(L, chains, params, width, height, center=(0.0, 0.0), extent=(16384.0, 16384.0), steps=64, exact_end=True, window=True):
    """(map float16 [height, width], lane-samples taken)"""
    out = np.zeros((height, width), np.uint16)
    n = C.c_uint64()
    p, c, e = np.ascontiguousarray(params, np.float32), np.asarray(center, np.float32), np.asarray(extent, np.float32)
    rc = L.shadow_host_map(P(chains[0]), P(chains[1]), P(chains[2]), P(p), width, height, P(c), P(e), steps, int(exact_end), int(window), P(out), C.byref(n))
    assert rc == 0
    return out.view(np.float16), n.value


@pytest.mark.parametrize("name", ["A", "B"])
def test_host_core_matches_reference(shadow_host, chains, oracle, otex, name):
    """Test 1: scenes A and B at the gate, and the same bytes with the exact end on and off."""
    p = SR.scene(oracle, name)
    ref, _ = SR.shadow_map(oracle, otex, p, **SR.SCENE_SIZE)
    r = ref.astype(np.float32)
    if name == "A":                                              # preconditions on the REFERENCE: a blank map cannot pass
        assert (ref.view(np.uint16) == 0x3C00).mean() >= 0.30 and (r < 0.9).mean() >= 0.40
    else:
        assert (ref.view(np.uint16) == 0).mean() >= 0.25 and (ref.view(np.uint16) == 0x3C00).mean() >= 0.02
    on, n_on = host_map(shadow_host, chains, p, exact_end=True, **SR.SCENE_SIZE)
    off, n_off = host_map(shadow_host, chains, p, exact_end=False, **SR.SCENE_SIZE)
    SR.assert_gate(on, ref, "host core, scene " + name)
    assert (on.view(np.uint16) == off.view(np.uint16)).all()
    nowin, n_all = host_map(shadow_host, chains, p, exact_end=False, window=False, **SR.SCENE_SIZE)
    assert (on.view(np.uint16) == nowin.view(np.uint16)).all()   # the height window and its early exit are exact too
    assert n_all == 64 * 64 * 32 and n_on <= n_off <= n_all
    print("scene %s: lane-samples %d of %d with the height-window exit, %d with the exact end as well (%.1f %% removed by the exact end)"
          % (name, n_off, n_all, n_on, 100.0 * (n_off - n_on) / n_off))
    if name == "B":
        assert n_on < n_off                                      # the exact end fires


def test_known_answers(shadow_host, chains, oracle, otex):
    """Test 2: no coverage -> every half is 1.0 (the reference agrees, with no in-cloud sample); a sun below the horizon -> every half is 0."""
    p = oracle.default_params(64, 32, (1, 1, 0), coverage=0.0)
    ref, incloud = SR.shadow_map(oracle, otex, p, 16, 16, steps=32)
    assert incloud == 0 and (ref.view(np.uint16) == 0x3C00).all()
    m, _ = host_map(shadow_host, chains, p, 16, 16, steps=32)
    assert (m.view(np.uint16) == 0x3C00).all()
    p = SR.scene(oracle, "A")
    p[16:19] = (0.3, -0.2, 0.9)
    m, n = host_map(shadow_host, chains, p, 16, 16, steps=32)
    assert (m.view(np.uint16) == 0).all() and n == 0
    ref, _ = SR.shadow_map(oracle, otex, p, 16, 16, steps=32)
    assert (ref.view(np.uint16) == 0).all()


def test_addressing(shadow_host, chains, oracle, otex):
    """Test 3: a map moved by one texel along x (z) is the same map one column (row) on, bit for bit; x and z are not swapped."""
    p = SR.scene(oracle, "A")
    size = dict(width=32, height=32, extent=(16384.0, 16384.0), steps=32)
    for fn in (lambda **kw: SR.shadow_map(oracle, otex, p, **kw)[0], lambda **kw: host_map(shadow_host, chains, p, **kw)[0]):
        base = fn(center=(0.0, 0.0), **size).view(np.uint16)
        mx = fn(center=(512.0, 0.0), **size).view(np.uint16)
        mz = fn(center=(0.0, 512.0), **size).view(np.uint16)
        assert (mx[:, 0:31] == base[:, 1:32]).all()
        assert (mz[0:31, :] == base[1:32, :]).all()
        assert (base != base.T).any()
    ref = SR.shadow_map(oracle, otex, p, center=(0.0, 0.0), **size)[0]
    assert (ref.view(np.uint16) != ref.view(np.uint16).T).mean() > 0.1
    SR.assert_gate(host_map(shadow_host, chains, p, center=(0.0, 0.0), **size)[0], ref, "host core, 32 x 32")


def test_ragged(shadow_host, chains, oracle, otex):
    """Test 4: a map that is no multiple of the tile, an odd step count, an off-centre rectangle."""
    p = SR.scene(oracle, "A")
    size = dict(width=37, height=21, center=(1000.0, -3000.0), extent=(9000.0, 9000.0), steps=17)
    ref, _ = SR.shadow_map(oracle, otex, p, **size)
    assert (ref.view(np.uint16) == 0x3C00).mean() >= 0.30 and (ref.astype(np.float32) < 0.9).mean() >= 0.40
    m, _ = host_map(shadow_host, chains, p, **size)
    SR.assert_gate(m, ref, "host core, ragged 37 x 21")
