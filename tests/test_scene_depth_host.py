"""The front end of the observer's cloud march behind a per-pixel scene depth (csrc/scene_depth_core.h: what the lanes of
clouds_observer_depth_kernel run in front of the march), compiled for the host by tests/scene_depth_host, held to its anchors, to the numpy
restatement of its definition (tests/scene_depth_reference.py) and to the texel rule.  A unit test of device code, not a render path: libcloudsky
has no CPU implementation.

Anchor (a): a buffer of +inf gives observer_core.h observer_ray's eleven fields bit for bit; no ray of the six observers has shelldist == 0.
Anchor (b): a constant c gives observer_ray's with max_distance = min(cap, c).
Anchor (c): the host march over a piecewise-constant buffer is, pixel for pixel, the host march at the pixel's cap.

D4 found that the clause `shelldist > 0` alone lets a NaN ray through: from `inside` (o.x = o.z = 0, t0 = 0) a depth of 1e-22 m gives
shelldist > 0, a raystep whose squares underflow, ss = 0 and eleven non-finite fields on all 2 304 rays.  The definition's clause is therefore
that both square roots of the ray take an argument >= 2^-102 (scene_depth_core.h), and D4 sweeps the depths between 1e-45 and 1e-3 by decades.
D4 reports how many rays the segment's length alone rejects when every depth texel sits on, or a few ulps behind, its ray's t0 (measured at
N = 128, of the rays that pass every other clause): at 0 ulps none (t1 > t0 fails first); at 1 ulp ground 23 of 1 920, hill 25 of 1 984,
above_down 26 of 2 010, offset 1 836 of 1 984 (x and z near 5e4 round as well); at 2 / 8 / 64 / 4 096 ulps none but offset's 1 761 / 1 431 /
390 / 0.  Inside the layer (t0 = 0) every depth up to 1e-15 m is rejected on all 2 304 rays and every depth from 1e-12 m on is marched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clouds_rays_reference as RR
import observer_reference as OR
import observers as OB
import scene_depth_reference as DR
import scene_depths as SD
import shadow_reference as SR
from conftest import ROOT
from test_clouds_rays_host import chains  # noqa: F401  (module-scoped fixture)
from test_observer_host import host_march_from, obs_host  # noqa: F401

F = np.float32
INF = float("inf")
NAN = float("nan")
TEXELS = (NAN, 0.0, -0.0, -1.0, -INF, 1e-45, 1e-38, 1e-3, INF)          # D3's values
ULPS = (0, 1, 2, 8, 64, 4096)                                             # D4's offsets behind t0
TINY = (1e-45, 1e-38, 1e-30, 1e-25, 1e-22, 1e-20, 1e-18, 1e-15, 1e-12, 1e-9, 1e-6, 1e-3)   # D4's depths for the observers inside the layer


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F else np.uint16)


@pytest.fixture(scope="module")
def depth_host():
    d = os.path.join(ROOT, "tests", "scene_depth_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libscene_depth_host.so"))
    for f in ("scene_depth_host_rays", "scene_depth_host_shelldist", "scene_depth_host_march", "scene_depth_host_walk"):
        getattr(L, f).restype = None
    L.scene_depth_host_invalid.restype = C.c_int
    L.scene_depth_host_invalid.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64]
    L.scene_depth_host_rays.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
    L.scene_depth_host_shelldist.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    L.scene_depth_host_march.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                         C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scene_depth_host_walk.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def cam_of(name):
    """csky_view.basis of the observer's camera: nine floats, column-major"""
    return RR.column_major(OB.observer(name)[2])


def host_depth_rays(L, position, cap, dirs, z, steps=128, kind=DR.DISTANCE, cam=None, ref_caps=None):
    """(d [...], valid bool [...], scene_depth_ray's fields [..., 11], observer_ray's fields at ref_caps [..., 11] or None)"""
    e = np.ascontiguousarray(dirs, F)
    zz = np.ascontiguousarray(np.broadcast_to(np.asarray(z, F), e.shape[:-1]), F)
    n = zz.size
    d, valid, rays = np.zeros(n, F), np.zeros(n, np.uint8), np.zeros((n, 11), F)
    rc = None if ref_caps is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ref_caps, F), e.shape[:-1]), F)
    ref = None if ref_caps is None else np.zeros((n, 11), F)
    L.scene_depth_host_rays(P(np.ascontiguousarray(position, F)), float(cap), kind, P(None if cam is None else np.ascontiguousarray(cam, F)), steps, n, P(e), P(zz), P(d),
                            P(valid), P(rays), P(rc), P(ref))
    shp = e.shape[:-1]
    return d.reshape(shp), valid.astype(bool).reshape(shp), rays.reshape(shp + (11,)), None if ref is None else ref.reshape(shp + (11,))


def host_march_depth(L, chains, params, sky, position, cap, dirs, z, kind=DR.DISTANCE, cam=None, primary=128, light=6, eps=0.0, window=True):  # noqa: F811
    """test_observer_host.host_march_from with a depth texel per ray: (float16 [..., 4], marched bool [...], in-cloud samples int64 [...])"""
    e = np.ascontiguousarray(dirs, F)
    zz = np.ascontiguousarray(np.broadcast_to(np.asarray(z, F), e.shape[:-1]), F)
    n = zz.size
    out, marched, inc = np.zeros((n, 4), np.uint16), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    p = np.ascontiguousarray(params, F)
    s = np.ascontiguousarray(sky).view(np.uint16)
    L.scene_depth_host_march(P(chains[0]), P(chains[1]), P(chains[2]), P(p), primary, light, eps, P(s), s.shape[1], s.shape[0], int(window),
                             P(np.ascontiguousarray(position, F)), float(cap), kind, P(None if cam is None else np.ascontiguousarray(cam, F)), n, P(e), P(zz), P(out), P(marched),
                             P(inc))
    shp = e.shape[:-1]
    return out.view(np.float16).reshape(shp + (4,)), marched.astype(bool).reshape(shp), inc.astype(np.int64).reshape(shp)


def walk(L, position, cap, dirs, z, steps=128, kind=DR.DISTANCE, cam=None):
    """[marched rays, marched rays with a field that is not finite, smallest |dir|^2, largest |dir|^2, rays the shelldist clause alone rejects]"""
    e = np.ascontiguousarray(dirs, F)
    zz = np.ascontiguousarray(np.broadcast_to(np.asarray(z, F), e.shape[:-1]), F)
    out = np.zeros(5, np.float64)
    L.scene_depth_host_walk(P(np.ascontiguousarray(position, F)), float(cap), kind, P(None if cam is None else np.ascontiguousarray(cam, F)), steps, zz.size, P(e), P(zz), P(out))
    return out


def buffers(name):
    """{label: float32 [H, W] distances} of D2: shell, mixed and quad for the observer"""
    return {"shell": SD.shell(name, SD.ALTITUDE[name]), "mixed": SD.mixed(name), "quad": SD.quad(name)}


# ---- D1
@pytest.mark.parametrize("name", OB.NAMES)
def test_no_depth_in_the_way_is_the_observers_ray_bit_for_bit(depth_host, name):
    """Anchors (a) and (b) on the Ray, and that no ray of the uncapped observer has shelldist == 0: the one pixel a +inf buffer may differ on."""
    pos, cap, _, _, _, _ = OB.observer(name)
    d = OB.dirs(name)
    for c in (INF, 3000.0, 9000.0, 20000.0):
        _, valid, got, ref = host_depth_rays(depth_host, pos, cap, d, c, ref_caps=min(cap, c))
        assert valid.all()
        marched = ref[..., 10] > 0
        print("%s, constant %g: %d of %d rays marched" % (name, c, marched.sum(), marched.size))
        assert (bits(got) == bits(ref)).all(), (c, np.argwhere(bits(got) != bits(ref))[:4])
        if c == INF or c == 20000.0:
            assert marched.any()
    sd = np.zeros(d.shape[:-1], F)
    depth_host.scene_depth_host_shelldist(P(pos), float(cap), sd.size, P(np.ascontiguousarray(d, F)), P(sd))
    m = ~np.isnan(sd)
    assert m.sum() > 0.5 * m.size and (sd[m] > 0).all()
    print("%s: smallest shelldist of a marched ray without a depth buffer: %.3f m" % (name, sd[m].min()))


# ---- D2
@pytest.mark.parametrize("kind", [DR.DISTANCE, DR.VIEW_Z], ids=["distance", "view-z"])
@pytest.mark.parametrize("name", OB.NAMES)
def test_the_core_is_the_numpy_restatement_bit_for_bit(depth_host, name, kind):
    pos, cap, _, _, _, _ = OB.observer(name)
    e, cam = OB.dirs(name), cam_of(name)
    for label, dist in buffers(name).items():
        z = DR.view_z(cam, e, dist) if kind == DR.VIEW_Z else dist
        for steps in (128, 30):
            d, valid, got, _ = host_depth_rays(depth_host, pos, cap, e, z, steps, kind, cam)
            wd, wv = DR.cap(kind, cam, e, z)
            assert (valid == wv).all() and (bits(d) == bits(wd)).all(), label
            want = DR.ray(pos, cap, e, z, steps, kind, cam)
            assert (bits(got) == bits(want)).all(), (label, steps, np.argwhere(bits(got) != bits(want))[:4])
        t0, t1, has = DR.segment(pos, cap, e, z, kind, cam)
        marched = want[..., 10] > 0
        assert marched.any() and (marched <= (has & OR.accept(e))).all(), label
        # the ray's own fields say where its segment runs: p = o + e * t0, and N steps of ss span |end - start|
        o = OR.origin(pos)
        with np.errstate(all="ignore"):
            start = np.stack([o[k] + e[..., k] * t0 for k in range(3)], -1).astype(F)
        assert (bits(got[..., 0:3][marched]) == bits(start[marched])).all(), label


# ---- D3
@pytest.mark.parametrize("name", ["inside", "above_down"])
def test_the_texel_rule(depth_host, name):
    pos, cap, _, _, _, _ = OB.observer(name)
    e, cam = OB.dirs(name), cam_of(name)
    _, _, free, _ = host_depth_rays(depth_host, pos, cap, e, INF)
    for kind in (DR.DISTANCE, DR.VIEW_Z):
        for zv in TEXELS:
            z = np.full(e.shape[:-1], zv, F)
            d, valid, got, _ = host_depth_rays(depth_host, pos, cap, e, z, 128, kind, cam)
            want = DR.ray(pos, cap, e, z, 128, kind, cam)
            assert (bits(got) == bits(want)).all(), (kind, zv)
            marched = got[..., 10] > 0
            assert not bits(got)[~marched].any()                 # not marched: all-zero fields
            if not zv > 0:                                       # NaN, 0, -0, negatives, -inf: geometry at the lens
                assert not valid.any() and not marched.any(), (kind, zv)
            elif zv == INF:                                      # nothing in the way (the view's rays all look forward: f > 0)
                assert valid.all() and (bits(got) == bits(free)).all(), kind
            else:
                assert (valid == (d > 0)).all() and (marched <= valid).all(), (kind, zv)
            print("%s, kind %d, z = %r: %d valid, %d marched" % (name, kind, zv, valid.sum(), marched.sum()))
    for k in (6, 7, 8):                                          # view-z through a camera whose back axis is not finite: no texel is valid
        for bad in (NAN, INF, -INF):
            c = cam.copy()
            c[k] = bad
            _, valid, got, _ = host_depth_rays(depth_host, pos, cap, e, 5000.0, 128, DR.VIEW_Z, c)
            want = DR.ray(pos, cap, e, np.full(e.shape[:-1], 5000.0, F), 128, DR.VIEW_Z, c)
            assert (bits(got) == bits(want)).all(), (k, bad)
            assert not valid.any() and not bits(got).any(), (k, bad)   # f is NaN or +-inf: f > 0 fails, or d = z / inf = 0


# ---- D4
def advance(t, ulps):
    """float32 t moved up by `ulps` representable values (t >= 0)"""
    return (np.ascontiguousarray(t, F).view(np.uint32) + np.uint32(ulps)).view(F)


def silhouette_cases(name):
    """[(label, z float32 [H, W])]: every depth on its ray's t0 and a few ulps behind it; tiny depths for the observers inside the layer (t0 = 0)"""
    pos, cap, _, _, _, _ = OB.observer(name)
    t0, _, has = OR.segment(pos, cap, OB.dirs(name))
    t0 = np.where(has & (t0 > 0), t0, F(0.0)).astype(F)
    out = [("t0 + %d ulp" % u, advance(t0, u)) for u in ULPS]
    if name in ("inside", "inside_up"):
        out += [("%g m" % v, np.full(t0.shape, v, F)) for v in TINY]
    return out


@pytest.mark.parametrize("name", OB.NAMES)
def test_the_silhouette_corner(depth_host, name):
    """A depth within the fp32 quantum of t0 rounds the end onto the start.  Every ray that is marched has eleven finite fields and a unit dir."""
    pos, cap, _, _, _, _ = OB.observer(name)
    e = OB.dirs(name)
    for label, z in silhouette_cases(name):
        for steps in (128, 1024):
            out = walk(depth_host, pos, cap, e, z, steps)
            print("%s, z = %s, N = %d: %d marched, %d rejected by the segment's length alone; |dir|^2 in [%.7f, %.7f]" % (name, label, steps, out[0], out[4], out[2], out[3]))
            assert out[1] == 0, (label, out)
            if out[0]:
                assert abs(out[2] - 1.0) <= 1e-3 and abs(out[3] - 1.0) <= 1e-3, (label, out)
            want = DR.ray(pos, cap, e, z, steps)
            assert out[0] == (want[..., 10] > 0).sum()


# ---- D5
@pytest.fixture(scope="module")
def scene(oracle, o_skies):
    return SR.scene(oracle, "A"), o_skies["deg45"]


@pytest.mark.parametrize("name", OB.NAMES)
def test_the_host_march_composes_pixel_for_pixel(depth_host, obs_host, chains, scene, name):  # noqa: F811
    """Anchor (c) on the host: the host march behind `quad` is, in each quadrant, observer_host's march at that quadrant's cap, 0 halves differ;
    and `mixed` meets the conditions it is tested under."""
    p, sky = scene
    pos, cap, _, _, w, h = OB.observer(name)
    e = OB.dirs(name)
    got, marched, _ = host_march_depth(depth_host, chains, p, sky, pos, cap, e, SD.quad(name))
    idx = SD.quad_index(h, w)
    want, wm = np.zeros_like(got), np.zeros_like(marched)
    for q, c in enumerate(SD.QUAD_CAPS):
        img, m, _ = host_march_from(obs_host, chains, p, sky, pos, min(cap, c), e)
        want[idx == q], wm[idx == q] = img[idx == q], m[idx == q]
    differ = int((bits(got) != bits(want)).sum())
    print("%s, quad: %d of %d halves differ from the per-cap host marches; %d pixels marched" % (name, differ, got.size, marched.sum()))
    assert differ == 0 and (marched == wm).all() and marched.any()
    free, fm, _ = host_march_from(obs_host, chains, p, sky, pos, cap, e)
    z = SD.mixed(name)
    capped, cm, _ = host_march_depth(depth_host, chains, p, sky, pos, cap, e, z)
    SD.assert_conditions(name, z, capped, free, fm)
    assert not bits(capped)[~cm].any()
    untouched = fm & (z == F(INF))
    assert untouched.any() and (bits(capped)[untouched] == bits(free)[untouched]).all()


# ---- the rule for what the calls refuse
def test_which_depth_buffers_are_refused(depth_host):
    def rule(texels=0x10000, pitch=64, kind=0, view=1, host=0, w=16, h=16, out=0x90000, out_pitch=128):
        return depth_host.scene_depth_host_invalid(texels, pitch, kind, view, host, w, h, out, out_pitch)
    assert rule() == 0 and rule(kind=1) == 0 and rule(pitch=68) == 0 and rule(host=1, pitch=0) == 0
    assert rule(texels=0) == 1
    assert rule(kind=2) == 2 and rule(kind=-1) == 2
    assert rule(kind=1, view=0) == 3 and rule(kind=0, view=0) == 0
    assert rule(pitch=60) == 4 and rule(pitch=66) == 4 and rule(pitch=0) == 4 and rule(host=1, pitch=60) == 4
    # 16 rows of 64 bytes from 0x10000: [0x10000, 0x10400); out: 16 rows of 128 bytes: 0x800 bytes
    assert rule(out=0x10000) == 5 and rule(out=0x103FC) == 5 and rule(out=0x10400) == 0 and rule(out=0x10000 - 0x800) == 0 and rule(out=0x10000 - 0x7FF) == 5
    assert rule(w=0) == 0 and rule(w=8193, pitch=4) == 0      # the image's own check refuses these
