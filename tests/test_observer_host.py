"""The front end of the direct cloud march from an observer's position (csrc/observer_core.h: what the lanes of clouds_observer_kernel run in front of
the march), compiled for the host by tests/observer_host, held to its two anchors, to the numpy restatement of its definition
(tests/observer_reference.py) and to answers known from geometry.  A unit test of device code, not a render path: libcloudsky has no CPU implementation.

Anchor (a): at position (0, 0, 0) without a cap, all eleven fields of the ray are rays_core.h rays_ray's bit for bit, for every direction.
Anchor (b): every primary and light sample's fp32 |p|^2 stays inside [SHELL_SQRT_LO, SHELL_SQRT_HI], the range sqrt_shell is proven on.

Figures this file reports (asserted with the margins stated at the tests):
    O3  largest deviation of a known segment end or length: 0.248 m (slack 2 m)
    O4  the farthest a primary sample's radius strays outside [SKY_B_RADIUS, SKY_T_RADIUS]: 31.98 m at N = 128, 255.27 m at N = 1024, and as much
        for the reference's own observer (31.61 m, 255.26 m) as for any other: p.y is near 6e6, where fp32 has a quantum of 0.5 m, so every
        `p += dir * ss` of clouds.glsl:173 rounds p.y by up to 0.25 m, and a ray whose increment has the same fraction at every step rounds the
        same way N times: N / 4 metres.  Asserted at twice the measured figures."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clouds_rays_reference as RR
import observer_reference as OR
import observers as OB
import shadow_reference as SR
import view_cameras as VC
from conftest import ROOT, SUNS, norm
from test_clouds_rays_host import _rejected_directions, chains, grid, host_march, rays_host  # noqa: F401  (module-scoped fixtures)

F = np.float32
INF = float("inf")
STRAY_M = {128: 31.98, 1024: 255.27}                          # O4's measured figures (see the docstring); the test asserts twice that


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def obs_host():
    d = os.path.join(ROOT, "tests", "observer_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libobserver_host.so"))
    for f in ("observer_host_accept", "observer_host_rays", "observer_host_march", "observer_host_walk"):
        getattr(L, f).restype = None
    L.observer_host_invalid.restype = C.c_int
    L.observer_host_invalid.argtypes = [C.c_void_p, C.c_float]
    L.observer_host_accept.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.observer_host_rays.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.observer_host_march.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.observer_host_walk.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return L


def host_rays(L, position, cap, dirs, steps):
    """(observer_ray's fields [..., 11], the capped segments [..., 2], rays_ray's fields [..., 11]) of the directions float32 [..., 3]"""
    d = np.ascontiguousarray(dirs, F)
    n = d.size // 3
    rays, seg, ref = np.zeros((n, 11), F), np.zeros((n, 2), F), np.zeros((n, 11), F)
    L.observer_host_rays(P(np.ascontiguousarray(position, F)), float(cap), steps, n, P(d), P(rays), P(seg), P(ref))
    shp = d.shape[:-1]
    return rays.reshape(shp + (11,)), seg.reshape(shp + (2,)), ref.reshape(shp + (11,))


def host_march_from(L, chains, params, sky, position, cap, dirs, primary=128, light=6, eps=0.0, window=True):  # noqa: F811
    """test_clouds_rays_host.host_march from an observer's position"""
    d = np.ascontiguousarray(dirs, F)
    n = d.size // 3
    out, marched, inc = np.zeros((n, 4), np.uint16), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    p = np.ascontiguousarray(params, F)
    s = np.ascontiguousarray(sky).view(np.uint16)
    L.observer_host_march(P(chains[0]), P(chains[1]), P(chains[2]), P(p), primary, light, eps, P(s), s.shape[1], s.shape[0], int(window),
                          P(np.ascontiguousarray(position, F)), float(cap), n, P(d), P(out), P(marched), P(inc))
    shp = d.shape[:-1]
    return out.view(np.float16).reshape(shp + (4,)), marched.astype(bool).reshape(shp), inc.astype(np.int64).reshape(shp)


def extra_directions():
    """unit directions no camera has: e.y in {+-1e-7, +-1e-3, +-0.05, +-0.5} at eight azimuths, float32 [64, 3]"""
    out = []
    for y in (1e-7, 1e-3, 0.05, 0.5):
        for sgn in (1.0, -1.0):
            for k in range(8):
                az = 2.0 * np.pi * (k + 0.3) / 8.0
                c = np.sqrt(1.0 - y * y)
                out.append([c * np.cos(az), sgn * y, c * np.sin(az)])
    return np.ascontiguousarray(out, F)


def camera_directions():
    """the directions of the twelve cameras of view_cameras.py, float32 [n, 3]"""
    out = []
    for name in VC.NAMES:
        b, fov, _, _, w, h = VC.views(name)
        out.append(RR.view_dirs(b, fov, w, h).reshape(-1, 3))
    return np.ascontiguousarray(np.concatenate(out), F)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F else np.uint16)


# ---- O1
@pytest.mark.parametrize("steps", [128, 30])
def test_the_ground_observer_without_a_cap_is_rays_ray_bit_for_bit(obs_host, rays_host, steps):  # noqa: F811
    """Anchor (a), the rays: the 64 x 32 grid's directions, those of the twelve cameras (above and under the horizon), the directions no camera has
    and the refused ones."""
    g, _ = grid(rays_host, 64, 32, steps)
    d = np.concatenate([g.reshape(-1, 3), camera_directions(), extra_directions(), _rejected_directions()])
    got, seg, ref = host_rays(obs_host, (0, 0, 0), INF, d, steps)
    up, ok = d[:, 1] > 0, RR.accept(d)
    print("N = %d: %d directions, %d accepted by rays_accept, %d at or under the horizon" % (steps, len(d), ok.sum(), (~up).sum()))
    assert ok.sum() > 0.4 * len(d) and (~up).sum() > 0.1 * len(d)
    assert (ref[:, 10] == ok).all()
    assert (bits(got) == bits(ref)).all(), np.argwhere(bits(got) != bits(ref))[:4]


@pytest.mark.parametrize("scene,steps,light", [("A", 128, 6), ("B", 30, 4)])
def test_the_ground_observer_marches_the_bytes_of_the_direct_march(obs_host, rays_host, chains, oracle, o_skies, scene, steps, light):  # noqa: F811
    """Anchor (a), the march: the host march of the grid's directions and of three cameras' from (0, 0, 0) against rays_host_march's."""
    p = SR.scene(oracle, scene)
    sky = o_skies["deg45"]                                   # any sky LUT: both marches read the same
    g, _ = grid(rays_host, 64, 32, steps)
    cams = ["roll"] if scene == "B" else ["roll", "horizon", "wide"]
    for name, d in [("grid", g)] + [(c, RR.view_dirs(*[VC.views(c)[k] for k in (0, 1, 4, 5)])) for c in cams]:
        want, m0, i0 = host_march(rays_host, chains, p, sky, d, steps, light)
        got, m1, i1 = host_march_from(obs_host, chains, p, sky, (0, 0, 0), INF, d, steps, light)
        assert (want[..., 3] > 0).mean() >= 0.1, name
        assert (bits(got) == bits(want)).all() and (m0 == m1).all() and (i0 == i1).all(), name


# ---- O2
@pytest.mark.parametrize("steps", [128, 30])
@pytest.mark.parametrize("name", OB.NAMES)
def test_the_core_is_the_numpy_restatement_bit_for_bit(obs_host, name, steps):
    pos, cap, _, _, _, _ = OB.observer(name)
    d = np.concatenate([OB.dirs(name).reshape(-1, 3), extra_directions(), _rejected_directions()])
    got, seg, _ = host_rays(obs_host, pos, cap, d, steps)
    want = OR.ray(pos, cap, d, steps)
    marched = want[:, 10] > 0
    assert 0.5 * len(d) < marched.sum() < len(d)
    assert (bits(got) == bits(want)).all(), np.argwhere(bits(got) != bits(want))[:4]
    t0, t1, has = OR.segment(pos, cap, d)
    assert (bits(seg[marched, 0]) == bits(t0[marched])).all() and (bits(seg[marched, 1]) == bits(t1[marched])).all()
    ok = np.zeros(len(d), np.uint8)
    obs_host.observer_host_accept(len(d), P(d), P(ok))
    assert (ok.astype(bool) == OR.accept(d)).all() and not ok[-len(_rejected_directions()):-3].any()   # (the last three are unit vectors at or under the horizon)
    assert ok[-3:].all()


# ---- O3
def test_known_answers_from_geometry(obs_host):
    """Each case is marched, or refused, as geometry says; a segment's ends within 2 m of it (the 0.5 m fp32 quantum at 6e6 on each end, plus the
    cancellation in -b +- d)."""
    up, down, level = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0)
    worst = 0.0

    def one(alt, e, cap=INF):
        r, s, _ = host_rays(obs_host, (0.0, alt, 0.0), cap, np.array([e], F), 128)
        return r[0], float(s[0, 0]), float(s[0, 1])

    def near(x, want):
        nonlocal worst
        worst = max(worst, abs(x - want))
        return abs(x - want) <= 2.0
    r, t0, t1 = one(8000.0, down)                            # from above: 4000 m of air, then the whole layer
    assert r[10] == 1 and near(t0, 4000.0) and near(t1 - t0, 2500.0) and near(r[1], 6004000.0) and r[7] == -1.0
    assert near(128.0 * r[9], 2500.0)
    r, t0, t1 = one(2750.0, up)                              # from the middle of the layer: half of it either way
    assert r[10] == 1 and t0 == 0.0 and near(t1, 1250.0) and r[1] == F(6002750.0)
    r, t0, t1 = one(2750.0, down)
    assert r[10] == 1 and t0 == 0.0 and near(t1, 1250.0) and r[7] == -1.0
    assert one(8000.0, up)[0][10] == 0                       # above the layer looking up
    assert one(1000.0, down)[0][10] == 0 and one(0.0, down)[0][10] == 0   # under it looking down: the ground
    r, _, _ = one(8000.0, down, cap=3000.0)                  # a cap in front of the layer
    assert r[10] == 0 and not r.any()
    r, t0, t1 = one(8000.0, down, cap=5000.0)                # a cap inside the segment
    assert r[10] == 1 and near(t0, 4000.0) and t1 == 5000.0 and near(128.0 * r[9], 1000.0)
    r, t0, t1 = one(2750.0, level)                           # level, inside: out through the top
    end = r[0:3].astype(np.float64) + 128.0 * r[3:6].astype(np.float64)
    assert r[10] == 1 and t0 == 0.0 and near(float(np.linalg.norm(end)), 6004000.0)
    want = np.sqrt(6004000.0 ** 2 - 6002750.0 ** 2)          # 122.5 km; the end's RADIUS has the 2 m, its distance 2 m / (t / r)
    assert abs(t1 - want) <= 2.0 * 6004000.0 / want
    r, t0, t1 = one(1000.0, up)                              # under the layer looking up: 500 m of air, the layer
    assert r[10] == 1 and near(t0, 500.0) and near(t1 - t0, 2500.0)
    print("known answers: largest deviation %.3f m" % worst)


# ---- the test cameras see what they are there for
@pytest.fixture(scope="module")
def host_views(obs_host, chains, oracle, o_skies):  # noqa: F811
    """{name: (dirs, float16 image, marched, segments)} of every observer: the host core's march of scene A"""
    p = SR.scene(oracle, "A")
    out = {}
    for name in OB.NAMES:
        pos, cap, _, _, _, _ = OB.observer(name)
        d = OB.dirs(name)
        img, marched, _ = host_march_from(obs_host, chains, p, o_skies["deg45"], pos, cap, d)
        _, seg, _ = host_rays(obs_host, pos, cap, d, 128)
        out[name] = (d, img, marched, seg)
    return out


@pytest.mark.parametrize("name", OB.NAMES)
def test_every_observer_sees_what_it_is_in_the_table_for(host_views, name):
    d, img, marched, seg = host_views[name]
    OB.assert_conditions(name, d, img[..., 3].astype(F), marched, seg)
    assert not bits(img)[~marched].any()                     # not marched: a zero texel


# ---- O4
@pytest.mark.parametrize("steps", [128, 1024])
def test_every_sample_stays_inside_the_range_sqrt_shell_is_proven_on(obs_host, steps):
    """Anchor (b): the walk over all observers, their cameras' directions and the directions no camera has, light samples under four suns, one of
    them under the horizon.  And how far a primary sample's radius strays outside the layer: the ends are on the shells to within the fp32 quantum
    of the intersection, and N fp32 additions follow."""
    worst = 0.0
    for name in OB.NAMES:
        pos, cap, _, _, _, _ = OB.observer(name)
        d = np.ascontiguousarray(np.concatenate([OB.dirs(name).reshape(-1, 3), extra_directions()]), F)
        for sun in (SUNS["zenith"], SUNS["deg45"], SUNS["demo"], (0.3, -0.9, 0.1)):
            out = np.zeros(6, np.float64)
            obs_host.observer_host_walk(P(pos), float(cap), len(d), P(d), steps, P(norm(sun)), P(out))
            assert out[0] > 0.5 * len(d), (name, out)
            assert out[1] == 0, (name, sun, out)             # every |p|^2 inside [SHELL_SQRT_LO, SHELL_SQRT_HI]
            if name in ("inside", "above_down"):
                assert out[5] > 0                            # these rays do descend: the early end of the rising rays would be wrong for them
            worst = max(worst, out[4])
        print("%s, N = %d: primary samples stray at most %.3f m outside the layer; |p|^2 in [%.6e, %.6e]" % (name, steps, out[4], out[2], out[3]))
    print("N = %d: smallest s = %.3f m" % (steps, worst))
    assert worst <= 2.0 * STRAY_M[steps]


# ---- O5
def test_which_observers_are_refused(obs_host):
    def rule(pos, cap=INF):
        return obs_host.observer_host_invalid(P(np.asarray(pos, F)), float(cap))
    nan = float("nan")
    assert rule((0, 0, 0)) == 0 and rule((0, 0, 0), 1e-3) == 0 and rule((0, 100000.0, 0)) == 0
    assert rule((1e6, -80000.0, 0)) == 0 and rule((0, -80000.0, -1e6)) == 0     # 1000 km out the sphere is 83.9 km lower
    for name in OB.NAMES:
        pos, cap, _, _, _, _ = OB.observer(name)
        assert rule(pos, cap) == 0
    for k in range(3):
        for bad in (nan, INF, -INF):
            p = [0.0, 10.0, 0.0]
            p[k] = bad
            assert rule(p) == 1, (k, bad)
    assert rule((1.0001e6, 90000.0, 0)) == 2 and rule((0, 90000.0, -1.0001e6)) == 2
    assert rule((0, -1.0, 0)) == 3 and rule((50000.0, 0.0, 0.0)) == 0 and rule((50000.0, -300.0, 0.0)) == 3   # 50 km out the sphere is 208 m lower
    assert rule((0, 100001.0, 0)) == 4 and rule((1e6, 100000.0, 0)) == 4
    for cap in (0.0, -0.0, -1.0, nan, -INF):
        assert rule((0, 0, 0), cap) == 5, cap
