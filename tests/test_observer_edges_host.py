"""The front end of the direct cloud march from an observer's position (csrc/observer_core.h) on the host, at the ends of what observer_invalid
accepts and on the rays the six observers of tests/observers.py never reach (observers.EDGE): chord rays (in through the top shell, past the inner
shell, out through the top; or, from inside, dipping and rising), a cap that lies in front of the layer for some rays and inside it for others, 100 km
of altitude, 1000 km of horizontal offset, |o| exactly on a shell, and the corner observer_ray's last clause closes: a max_distance within the fp32
quantum of a ray's t0, which used to round the end onto the start and give a ray reported as marched with NaN fields.  A unit test of device code
compiled for the host (tests/observer_host), not a render path.

Figures this file reports (asserted with the margins stated at the tests):
    E2  what each edge observer sees: the table at observers.assert_edge_conditions
    E3  the farthest a primary sample's radius strays outside [SKY_B_RADIUS, SKY_T_RADIUS] from an edge observer: EDGE_STRAY_M (segments reach
        342 km from 100 km up, steps 2.7 km)
    E4  the radius (float64) of a marched segment's ends against the shell the definition puts them on: SEGMENT_M, the numpy restatement's own
        worst; and in how many rays float64 geometry takes another branch than fp32 did: at most BRANCH_SHARE per observer
    E5  the corner: no ray is marched with a field that is not finite"""
import os
import subprocess

import numpy as np
import pytest

import observer_reference as OR
import observers as OB
import shadow_reference as SR
from conftest import ROOT, SUNS, norm
from test_clouds_rays_host import _rejected_directions, chains, rays_host  # noqa: F401  (module-scoped fixtures)
from test_observer_host import P, bits, extra_directions, host_march_from, host_rays, obs_host  # noqa: F401

F = np.float32
INF = float("inf")
MARCH = {"A": (128, 6), "B": (30, 4)}
SCENE_B = ["above_graze", "inside_dip", "high_down", "far_above"]          # the observers the GPU tests also run with scene B
# E3's measured figures: the walk's largest stray over the edge observers (beside test_observer_host.STRAY_M, which is the six observers'); the test
# asserts twice that
EDGE_STRAY_M = {128: 33.36, 1024: 256.75}
# E4's measured figure: the worst deviation in metres of the numpy restatement's own segment ends from their shells, over all fifteen observers; the
# test asserts the core at twice that
SEGMENT_M = 0.5975                                            # (far_above; the six observers of OBSERVERS: 0.4810, inside_up)
BRANCH_SHARE = 0.01                                            # a cap, not a measurement
CORNER_POS = (30000.0, 2750.0, -20000.0)
CORNER_CAPS = (1e-30, 1e-10, 1e-3, 0.1, 0.3, 1.0)


def random_directions(n=50000, seed=20240917):
    """seeded unit directions, float32 [n, 3], uniform on the sphere"""
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return np.ascontiguousarray(g / np.linalg.norm(g, axis=1, keepdims=True), F)


# ---- E1: O2 at the edge observers
@pytest.mark.parametrize("steps", [128, 30])
@pytest.mark.parametrize("name", OB.EDGE_NAMES)
def test_the_core_is_the_numpy_restatement_bit_for_bit_at_the_edges(obs_host, name, steps):
    pos, cap, _, _, _, _ = OB.observer(name)
    assert obs_host.observer_host_invalid(P(pos), float(cap)) == 0
    d = np.concatenate([OB.dirs(name).reshape(-1, 3), extra_directions(), _rejected_directions()])
    got, seg, _ = host_rays(obs_host, pos, cap, d, steps)
    want = OR.ray(pos, cap, d, steps)
    marched = want[:, 10] > 0
    assert 0.4 * len(d) < marched.sum() < len(d)
    assert np.isfinite(got).all()
    assert (bits(got) == bits(want)).all(), np.argwhere(bits(got) != bits(want))[:4]
    t0, t1, has = OR.segment(pos, cap, d)
    assert (bits(seg[marched, 0]) == bits(t0[marched])).all() and (bits(seg[marched, 1]) == bits(t1[marched])).all()
    ok = np.zeros(len(d), np.uint8)
    obs_host.observer_host_accept(len(d), P(d), P(ok))
    assert (ok.astype(bool) == OR.accept(d)).all()


# ---- E2: the edge observers see what they are there for
@pytest.fixture(scope="module")
def host_edge_views(obs_host, chains, oracle, o_skies):  # noqa: F811
    """{(name, scene): (dirs, float16 image, marched, segments)}: the host core's march of scene A from every edge observer, of scene B from four"""
    out = {}
    for scene in ("A", "B"):
        p = SR.scene(oracle, scene)
        for name in (OB.EDGE_NAMES if scene == "A" else SCENE_B):
            pos, cap, _, _, _, _ = OB.observer(name)
            d = OB.dirs(name)
            img, marched, _ = host_march_from(obs_host, chains, p, o_skies["deg45"], pos, cap, d, *MARCH[scene])
            _, seg, _ = host_rays(obs_host, pos, cap, d, MARCH[scene][0])
            out[name, scene] = (d, img, marched, seg)
    return out


@pytest.mark.parametrize("name,scene", [(n, "A") for n in OB.EDGE_NAMES] + [(n, "B") for n in SCENE_B])
def test_every_edge_observer_sees_what_it_is_in_the_table_for(host_edge_views, name, scene):
    d, img, marched, seg = host_edge_views[name, scene]
    print("scene %s:" % scene, end=" ")
    OB.assert_edge_conditions(name, d, img[..., 3].astype(F), marched, seg)
    assert np.isfinite(img.astype(F)).all()
    assert not bits(img)[~marched].any()                     # not marched: a zero texel


def beside_refused(refused, marched):
    """bool [H, W]: the marched pixels that share an 8 x 8 tile, one wavefront of clouds_observer_kernel, with a pixel whose ray the cap refuses.  (The
    marched pixels that TOUCH a refused one have segments a few metres long at the foot of the layer, where no scene has cloud.)"""
    h, w = refused.shape
    out = np.zeros_like(refused)
    for j in range(0, h, 8):
        for i in range(0, w, 8):
            if refused[j:j + 8, i:i + 8].any():
                out[j:j + 8, i:i + 8] = marched[j:j + 8, i:i + 8]
    return out


def test_the_cap_ring_runs_through_wavefronts_that_also_march(host_edge_views):
    """capped_ring on the host core: what the GPU test of the ring relies on."""
    d, img, marched, seg = host_edge_views["capped_ring", "A"]
    pos, cap, _, _, _, _ = OB.observer("capped_ring")
    _, _, free = OR.segment(pos, INF, d)
    refused = free & ~marched
    beside = beside_refused(refused, marched)
    print("capped_ring: %d refused, %d marched in a tile with one, %d of those with alpha > 0" % (refused.sum(), beside.sum(), (img[..., 3][beside] > 0).sum()))
    assert refused.sum() >= 0.10 * refused.size and beside.sum() >= 64
    assert not bits(img)[refused].any()
    assert (img[..., 3][beside] > 0).sum() >= 16


# ---- E3: O4 at the edge observers
@pytest.mark.parametrize("steps", [128, 1024])
def test_every_sample_of_an_edge_observer_stays_inside_the_range_sqrt_shell_is_proven_on(obs_host, steps):
    """test_observer_host's anchor (b) from the edge observers: their cameras' directions and the directions no camera has, light samples under
    four suns, one of them under the horizon."""
    worst = 0.0
    for name in OB.EDGE_NAMES:
        pos, cap, _, _, _, _ = OB.observer(name)
        d = np.ascontiguousarray(np.concatenate([OB.dirs(name).reshape(-1, 3), extra_directions()]), F)
        stray = 0.0
        for sun in (SUNS["zenith"], SUNS["deg45"], SUNS["demo"], (0.3, -0.9, 0.1)):
            out = np.zeros(6, np.float64)
            obs_host.observer_host_walk(P(pos), float(cap), len(d), P(d), steps, P(norm(sun)), P(out))
            assert out[0] > 0.4 * len(d), (name, out)
            assert out[1] == 0, (name, sun, out)             # every |p|^2 inside [SHELL_SQRT_LO, SHELL_SQRT_HI]
            if name in OB.CHORD:
                assert out[5] > 0                            # these rays do descend
            stray = max(stray, out[4])
        worst = max(worst, stray)
        print("%s, N = %d: primary samples stray at most %.3f m outside the layer; |p|^2 in [%.6e, %.6e]" % (name, steps, stray, out[2], out[3]))
    print("N = %d: the largest stray from an edge observer %.3f m" % (steps, worst))
    assert worst <= 2.0 * EDGE_STRAY_M[steps]


# ---- E4: the segment against float64
def _end_deviation(pos, d, t, shell):
    """metres by which the float64 radius of o + e t misses `shell`: a radius, or None for "within the layer" """
    o = OR.origin(pos).astype(np.float64)
    p = o + d.astype(np.float64) * t.astype(np.float64)[:, None]
    r = np.sqrt((p * p).sum(-1))
    if shell is None:
        return np.maximum(np.maximum(float(OR.RB) - r, r - float(OR.RT)), 0.0)
    return np.abs(r - shell)


def _segment_deviation(pos, cap, d, t0, t1, marched):
    """the largest deviation in metres of the ends of the marched rays' segments [t0, t1] (float32) from where the definition puts them, by the
    branch fp32 took"""
    where, _, _, top = OR.classify(pos, d)
    d, t0, t1, top = d[marched], t0[marched], t1[marched], top[marched]
    rb, rt = float(OR.RB), float(OR.RT)
    start = _end_deviation(pos, d, t0, {0: rb, 1: None, 2: rt}[where])
    free = t1 != F(cap)
    end = np.where(free, np.where(top, _end_deviation(pos, d, t1, rt), _end_deviation(pos, d, t1, rb)), _end_deviation(pos, d, t1, None))
    return float(max(start.max(), end.max()))


def _branches(pos, d, dtype):
    where, has, chord, top = OR.classify(pos, d, dtype)
    return where, has, has & chord, has & top


@pytest.mark.parametrize("name", OB.ALL_NAMES)
def test_the_segments_ends_lie_on_their_shells_in_float64(obs_host, name):
    """Radii are well conditioned at tangency, the distances t are not: what is compared is where the ends are, not the t.  The bound is the
    restatement's own worst deviation (SEGMENT_M), asserted on the core at twice that; and float64 geometry of the same fp32 inputs takes the
    branch fp32 took (under / inside / above, a segment or none, chord or not, which shell ends it) on all but BRANCH_SHARE of the camera's rays."""
    pos, cap, _, _, _, _ = OB.observer(name)
    d = np.ascontiguousarray(OB.dirs(name).reshape(-1, 3))
    t0, t1, has = OR.segment(pos, cap, d)
    ref_marched = OR.ray(pos, cap, d, 128)[:, 10] > 0
    ref = _segment_deviation(pos, cap, d, t0, t1, ref_marched)
    got, seg, _ = host_rays(obs_host, pos, cap, d, 128)
    marched = got[:, 10] > 0
    core = _segment_deviation(pos, cap, d, seg[:, 0], seg[:, 1], marched)
    w32, h32, c32, e32 = _branches(pos, d, F)
    w64, h64, c64, e64 = _branches(pos, d, np.float64)
    differ = float(((h32 != h64) | (c32 != c64) | (e32 != e64)).mean())
    print("%s: segment ends deviate from their shells by at most %.4f m (numpy restatement), %.4f m (core); float64 takes another branch on %.3f %% of %d rays" %
          (name, ref, core, 100.0 * differ, len(d)))
    assert marched.sum() > 0.4 * len(d)
    assert w32 == w64
    assert differ <= BRANCH_SHARE
    assert core <= 2.0 * SEGMENT_M                           # (`ref` is printed, not asserted: SEGMENT_M is its measured worst, as STRAY_M is the walk's)


# ---- E5: the corner
def _assert_marched_or_zero(rays, what):
    """every ray is not marched and all zero, or marched with finite fields, ss > 0 and |dir| within 2 ulp of 1"""
    marched = rays[:, 10] > 0
    assert np.isfinite(rays).all(), what
    assert not bits(rays[~marched]).any(), what
    m = rays[marched].astype(np.float64)
    worst = 0.0
    if len(m):
        assert (m[:, 9] > 0).all(), what
        worst = float(np.abs(np.sqrt((m[:, 6:9] ** 2).sum(-1)) - 1.0).max())
        assert worst <= 2.0 * 2.0 ** -23, (what, worst)
    return int(marched.sum()), worst


def test_the_three_reproductions_of_the_corner_are_not_marched(obs_host):
    """What the unguarded tail made of these: above = true, ss = 0, NaN dir and inc."""
    up = np.array([[0.0, 1.0, 0.0]], F)
    for cap in (float(np.nextafter(F(1500.0), F(2000.0))), 1500.1, 1500.2, 1500.25):
        got, _, _ = host_rays(obs_host, (0, 0, 0), cap, up, 128)
        assert not bits(got).any(), cap
        assert (bits(got) == bits(OR.ray((0, 0, 0), cap, up, 128))).all()
    d = random_directions()
    got, _, _ = host_rays(obs_host, CORNER_POS, 0.1, d, 128)
    want = OR.ray(CORNER_POS, 0.1, d, 128)
    _, _, has = OR.segment(CORNER_POS, 0.1, d)
    closed = has & ~(want[:, 10] > 0)
    print("cap 0.1 m from %s: the last clause refuses %d of %d directions" % (CORNER_POS, closed.sum(), len(d)))
    assert closed.sum() >= 1
    assert np.isfinite(got).all() and not bits(got[closed]).any()
    assert (bits(got) == bits(want)).all()
    mid = np.concatenate([extra_directions(), d])             # every direction does
    for cap in (1e-30, 1e-22):                               # 1e-30: shelldist = 0; 1e-22 (the header's example): shelldist > 0, a raystep whose squares underflow
        got, _, _ = host_rays(obs_host, (0, 2750.0, 0), cap, mid, 128)
        assert not bits(got).any(), cap
        assert (bits(got) == bits(OR.ray((0, 2750.0, 0), cap, mid, 128))).all()


def test_the_cap_sweep_above_a_rays_start(obs_host):
    """Position (0, 0, 0), direction (0, 1, 0), t0 = 1500: max_distance the 4096 floats above 1500 (to 1500.5: across the quantum of 0.5 m at 6e6)."""
    up = np.array([[0.0, 1.0, 0.0]], F)
    cap, rows, refs = F(1500.0), [], []
    for _ in range(4096):
        cap = np.nextafter(cap, F(2000.0))
        rows.append(host_rays(obs_host, (0, 0, 0), float(cap), up, 128)[0][0])
        refs.append(OR.ray((0, 0, 0), float(cap), up, 128)[0])
    rows, refs = np.stack(rows), np.stack(refs)
    n, worst = _assert_marched_or_zero(rows, "sweep")
    print("caps 1500 + 1 ... 4096 ulp: %d marched, ||dir| - 1| at most %.3g" % (n, worst))
    assert 0 < n < 4096                                      # both sides of the clause
    assert (bits(rows) == bits(refs)).all()


@pytest.mark.parametrize("cap", CORNER_CAPS)
def test_small_caps_from_inside_the_layer(obs_host, cap):
    d = random_directions()
    for steps in (128, 30):
        got, _, _ = host_rays(obs_host, CORNER_POS, cap, d, steps)
        n, worst = _assert_marched_or_zero(got, (cap, steps))
        print("cap %g m, N = %d: %d of %d marched, ||dir| - 1| at most %.3g" % (cap, steps, n, len(d), worst))
        assert (bits(got) == bits(OR.ray(CORNER_POS, cap, d, steps))).all()
    if cap <= 1e-10:
        assert n == 0
    if cap >= 1.0:
        assert n > 0.9 * len(d)


# ---- E6: under the sanitizers
def test_the_front_end_and_the_march_run_clean_under_the_sanitizers():
    """tests/observer_asan: a program of its own (its own main, -fsanitize=address,undefined), run here on the CPU as a child process.  Nothing of it
    is loaded into Python and nothing of it runs on a GPU."""
    d = os.path.join(ROOT, "tests", "observer_asan")
    subprocess.check_call(["make", "-C", d, "-s"])
    r = subprocess.run([os.path.join(d, "observer_asan")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    assert words[:3] == ["observer", "asan", "ok"] and int(words[3]) > 9000 and int(words[4]) > 1000
