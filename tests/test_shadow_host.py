"""The cloud shadow map's per-lane code (csrc/shadow_core.h on the cloud cores: what shadow.hip's lanes run), compiled for the host by
tests/shadow_host, against the numpy restatement of the definition (tests/shadow_reference.py, which calls the oracle per sample).
A unit test of device code, not a render path: libcloudsky itself has no CPU implementation.

The gate is the project's own for values rendered from the shipped assets (tests/parity_metrics.py) on the one channel: every texel within 2 fp16 ulp,
99.9 % within 1, largest difference 2e-3.  It rests on the sample positions being bit-identical (test 5 checks exactly that, on every scene of the sweep).

Tests 1-4: scenes A and B, known answers, addressing, a ragged map, all within 8 km of the observer.  Tests 5-6 (and the table's own check): the
scene sweep of shadow_reference.SCENES, 12 scenes from a zenith sun down to a third of a degree over the rectangles csky_aerial_shadow_rect hands
out, where a texel is ORDINARY, CHORD or MISS (include/cloudsky.h); 30 tests in all.

Mutations of csrc/shadow_core.h, run on this host build:
 (a) the three kinds reverted to the one formula (the reference kept): test 6 fails on exactly the eight scenes that have chord texels (deg1.1,
     deg1.1-n1, deg0.66-z, deg0.66-str, deg0.34, deg1.1-white, one-texel, miss: their chord and miss texels come out as NaN halfs) and passes on
     zenith, deg45, deg6 and deg2.7; test 5 cannot run without the kinds.
 (b) chord lanes allowed to vote on the height rule (`more = live && !(hf >= fc.hf_hi)`): test 6's "height window on and off: same bytes" fails on
     deg1.1 (37 texels), deg0.66-z (1), deg0.34 (118) and one-texel (1).
Against the parent commit: the 4 334 ordinary texels of the sweep have the same bytes, the 2 053 chord and miss texels were NaN; scenes A and B,
the 32 x 32 and the ragged map are byte-identical."""
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
    L.shadow_host_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def chains(pkg, noise):
    large, small, weather = noise
    return pkg.assets.build_mips(large, 8), pkg.assets.build_mips(small, 6), np.ascontiguousarray(weather, np.uint8)


@pytest.fixture(scope="module")
def sweep_tex(pkg, noise, oracle, otex, chains):
    """weather name of the sweep -> (the host build's chains, the oracle's textures), built on first use and shared"""
    large, small, weather = noise
    cache = {"shipped": (chains, otex)}

    def get(which):
        if which not in cache:
            w = SR.weather_map(weather, which)
            cache[which] = ((chains[0], chains[1], np.ascontiguousarray(w, np.uint8)), oracle.OracleTextures(large, small, w))
        return cache[which]
    return get


def host_rays(L, params, width, height, center, extent, steps):
    """(first sample position [height, width, 3], step [height, width, 3], step length [height, width], kind [height, width]) of shadow_ray_setup"""
    rays, kind = np.zeros((height, width, 7), np.float32), np.zeros((height, width), np.int32)
    p, c, e = np.ascontiguousarray(params, np.float32), np.asarray(center, np.float32), np.asarray(extent, np.float32)
    assert L.shadow_host_rays(P(p), width, height, P(c), P(e), steps, P(rays), P(kind)) == 0
    return rays[..., 0:3], rays[..., 3:6], rays[..., 6], kind


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


def sweep_preconditions(name, ref, kind):
    """On the REFERENCE alone, so that a blank map cannot pass: the census the table states, no NaN, texels strictly between the halfs 0 and 1.0
    (the scene made for the third kind: 1.0 texels and others), and where there is a chord texel, one that is neither 0 nor 1.0."""
    sc, b = SR.SCENES[name], ref.view(np.uint16)
    census, mixed = SR.tile_census(kind)
    assert census == sc["kinds"] and mixed == sc["mixed"], (name, census, mixed)
    assert np.isfinite(ref.astype(np.float32)).all(), name
    mid = (b != 0) & (b != 0x3C00)
    if name == "miss":
        assert census[2] > 0 and (b[kind == SR.MISS] == 0x3C00).all() and (b != 0x3C00).any()
    else:
        assert mid.mean() >= 0.10, (name, mid.mean())
    if census[1]:
        assert (mid & (kind == SR.CHORD)).any(), name


def test_sweep_table_covers_the_classes():
    """The table as a whole: scenes of the first kind only, scenes with ordinary and chord texels in one 8 x 8 tile, one scene with the third kind;
    the step counts 1, 3, 5, 17 and 0; every weather map; scene B's push constants on two low suns; 1 x 1 and 37 x 5."""
    S = SR.SCENES
    assert sum(s["kinds"][1:] == (0, 0) for s in S.values()) >= 4 and sum(s["mixed"] > 0 for s in S.values()) >= 4 and S["miss"]["kinds"][2] > 0
    assert {s["steps"] for s in S.values()} >= {0, 1, 3, 5, 17} and {s["weather"] for s in S.values()} == {"shipped", "stratus", "white"}
    assert sum(s["wind"] and s["kinds"][1] > 0 for s in S.values()) >= 2
    assert any(s["coverage"] == 0.1 and s["density"] == 0.01 for s in S.values())
    assert {(1, 1), (37, 5)} <= {(s["width"], s["height"]) for s in S.values()}
    low = [s for s in S.values() if s["sun"][1] / np.linalg.norm(s["sun"]) < np.sin(np.radians(0.5))]
    assert low and all(s["rect"] == "helper" for s in low)                                      # within half a degree of the horizon, the helper's own rectangle


@pytest.mark.parametrize("name", list(SR.SCENES))
def test_sweep_sample_positions(shadow_host, oracle, name):
    """Test 5: the kind of every texel and every sample position, bit for bit, between shadow_ray_setup and the restatement."""
    p, size = SR.sweep_scene(oracle, name)
    n = size["steps"] or 64
    geo = (size["width"], size["height"], size["center"], size["extent"], n)
    _, pos, ss, kind = SR.sample_positions(p, *geo)
    p0, step, hss, hkind = host_rays(shadow_host, p, *geo)
    assert (hkind == kind).all()
    assert (ss.view(np.uint32) == hss.view(np.uint32)).all()
    q = np.moveaxis(p0, -1, 0).copy()
    st = np.moveaxis(step, -1, 0)
    for k in range(n):                                               # the march's own advance: p = p + step in fp32
        assert (q.view(np.uint32) == pos[k].view(np.uint32)).all(), (name, k)
        q = (q + st).astype(np.float32)
    live = kind != SR.MISS
    assert np.isfinite(pos[:, :, live]).all() and (ss[live] > 0).all()


@pytest.mark.parametrize("name", list(SR.SCENES))
def test_sweep_matches_reference(shadow_host, sweep_tex, oracle, name):
    """Test 6: every scene of the sweep at the gate over all its texels; exact end on and off, height window on and off: the same bytes; with
    both off every texel but those of the third kind takes its N samples."""
    chains_w, otex_w = sweep_tex(SR.SCENES[name]["weather"])
    p, size = SR.sweep_scene(oracle, name)
    size = dict(size, steps=size["steps"] or 64)
    kind = SR.texel_kinds(p, size["width"], size["height"], size["center"], size["extent"])
    ref, _ = SR.shadow_map(oracle, otex_w, p, **size)
    sweep_preconditions(name, ref, kind)
    on, n_on = host_map(shadow_host, chains_w, p, exact_end=True, **size)
    SR.assert_gate(on, ref, "host core, sweep " + name)
    off, n_off = host_map(shadow_host, chains_w, p, exact_end=False, **size)
    assert (on.view(np.uint16) == off.view(np.uint16)).all(), name
    nowin, n_nowin = host_map(shadow_host, chains_w, p, exact_end=True, window=False, **size)
    assert (on.view(np.uint16) == nowin.view(np.uint16)).all(), name
    plain, n_all = host_map(shadow_host, chains_w, p, exact_end=False, window=False, **size)
    assert (on.view(np.uint16) == plain.view(np.uint16)).all(), name
    assert n_all == (size["width"] * size["height"] - SR.SCENES[name]["kinds"][2]) * size["steps"] and n_on <= n_off <= n_all
    assert (on.view(np.uint16)[kind == SR.MISS] == 0x3C00).all()
