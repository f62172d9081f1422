"""The Bruneton parametrization of the transmittance LUT (cloudsky.h CSKY_TLUT_BRUNETON) without a GPU: the mapping through the C ABI's host
function, and the LUT cores (csrc/tlut_core.h, lut_core.h: the per-lane code the HIP kernels instantiate) compiled for the host by
tests/tlut_host, against the numpy restatement of tests/tlut_reference.py.  A unit test of device code, not a render path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tlut_reference as TR
from conftest import ROOT, ulp_diff

W, Hh = 256, 64


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def tlut_host():
    d = os.path.join(ROOT, "tests", "tlut_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libtlut_host.so"))
    L.tlut_host_transmittance.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.tlut_host_sky.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.tlut_host_lookup.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.tlut_host_texel_ray.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def host_trans(L, mapping, w=W, h=Hh):
    t = np.zeros((h, w, 4), np.uint16)
    L.tlut_host_transmittance(mapping, w, h, P(t))
    return t.view(np.float16)


def host_sky(L, mapping, sun, trans, w=200, h=100):
    s = np.zeros((h, w, 4), np.uint16)
    sn = np.ascontiguousarray(sun, np.float32)
    tr = np.ascontiguousarray(trans).view(np.uint16)
    L.tlut_host_sky(mapping, w, h, P(sn), P(tr), tr.shape[1], tr.shape[0], P(s))
    return s.view(np.float16)


def host_lookup(L, mapping, trans, r, mu):
    tr = np.ascontiguousarray(trans).view(np.uint16)
    r, mu = np.ascontiguousarray(r, np.float32).reshape(-1), np.ascontiguousarray(mu, np.float32).reshape(-1)
    out = np.zeros((r.size, 4), np.float32)
    L.tlut_host_lookup(mapping, P(tr), tr.shape[1], tr.shape[0], P(r), P(mu), r.size, P(out))
    return out


@pytest.fixture(scope="module")
def host_luts(tlut_host):
    return {m: host_trans(tlut_host, m) for m in (0, 1)}


@pytest.fixture(scope="module")
def np_trans1():
    return TR.transmittance_lut(W, Hh)


@pytest.fixture(scope="module")
def converged_table():
    return TR.transmittance_table64(1024, 256, 640)


def c_uv(pkg, mapping, w, h, r, mu):
    uv, hit = (C.c_float * 2)(), C.c_int(-1)
    rc = pkg.lib().csky_transmittance_uv(mapping, w, h, float(r), float(mu), uv, C.byref(hit))
    assert rc == 0, (rc, pkg.lib().csky_last_error(None))
    return float(uv[0]), float(uv[1]), hit.value


# ---------------------------------------------------------------------------------------------------------------- 1. the mapping
def test_known_answers_through_the_c_abi(pkg):
    u, v, hit = c_uv(pkg, 1, W, Hh, 6471.0, 1.0)
    assert (u, v, hit) == (float(np.float32(0.5 / 256)), float(np.float32(1 - 0.5 / 64)), 0)
    u, v, hit = c_uv(pkg, 1, W, Hh, 6371.0, 1.0)
    assert (u, v, hit) == (float(np.float32(0.5 / 256)), float(np.float32(0.5 / 64)), 0)
    u, v, hit = c_uv(pkg, 1, W, Hh, 6371.0, 0.0)
    assert (u, v, hit) == (float(np.float32(1 - 0.5 / 256)), float(np.float32(0.5 / 64)), 0)
    assert c_uv(pkg, 1, W, Hh, 6371.0, -1e-3)[2] == 1
    assert c_uv(pkg, 1, W, Hh, 6371.5, -0.02)[2] == 1
    assert c_uv(pkg, 1, W, Hh, 6371.5, -0.01)[2] == 0            # the horizon cosine at 6371.5 km is -0.01253
    assert abs(-np.sqrt(1 - (6371.0 / 6371.5) ** 2) + 0.01253) < 1e-5
    # mapping 0: the reference's (clamp(mu / 2 + 1 / 2), clamp((r - Rg) / 100)), and no ray is ever blocked
    f = np.float32
    for r, mu in ((6371.0, 1.0), (6421.0, -0.25), (6500.0, -3.0), (6300.0, 0.3), (6371.5, -0.02)):
        u, v, hit = c_uv(pkg, 0, W, Hh, r, mu)
        eu = min(max(f(mu) * f(0.5) + f(0.5), f(0)), f(1))
        ev = min(max((f(r) - f(6371.0)) / f(100.0), f(0)), f(1))
        assert (u, v, hit) == (float(eu), float(ev), 0), (r, mu)
    # the package's helper is the same function
    assert pkg.transmittance_uv(6371.5, -0.02) == c_uv(pkg, 1, W, Hh, 6371.5, -0.02)[:2] + (True,)
    assert pkg.transmittance_uv(6371.5, -0.02, mapping="reference", w=8, h=8)[2] is False


def test_mapping_matches_the_restatement_bit_for_bit(pkg):
    """fp32 in, double inside, fp32 out: the C function and the float64 restatement agree exactly, coordinates and hit decisions (no tolerance)."""
    rng = np.random.default_rng(7)
    r = np.concatenate([rng.uniform(6371.0, 6471.0, 3000), 6371.0 + rng.uniform(0, 1, 1000) ** 4 * 100.0, [6371.0, 6471.0, 6300.0, 6500.0]]).astype(np.float32)
    mu_h = -np.sqrt(np.maximum(1.0 - (6371.0 / np.maximum(r.astype(np.float64), 6371.0)) ** 2, 0.0))
    mu = np.concatenate([rng.uniform(-1, 1, 2000), (mu_h[2000:] + rng.normal(0, 1e-3, r.size - 2000))]).astype(np.float32)
    u, v, hit = TR.uv(r, mu, W, Hh)
    for k in range(r.size):
        got = c_uv(pkg, 1, W, Hh, r[k], mu[k])
        assert got == (float(u[k]), float(v[k]), int(hit[k])), (k, r[k], mu[k])
    assert 0.2 < hit.mean() < 0.8                                   # both outcomes are exercised


def test_round_trip_lands_on_texel_centres(pkg, tlut_host):
    r, mu, d = TR.texel_ray_exact(W, Hh)
    px, py = np.meshgrid(np.arange(W), np.arange(Hh))
    u, v = TR.uv_exact(r, mu, W, Hh)
    assert np.abs(u * W - 0.5 - px).max() <= 1e-6 and np.abs(v * Hh - 0.5 - py).max() <= 1e-6       # float64: every centre to 1e-6 of a texel
    # fp32 (r, mu) in, fp32 (u, v) out: how far the restatement lands from the centre, and the C function held to that + 1 fp32 ulp of u, v
    r32, mu32, _ = TR.texel_ray(W, Hh)
    u32, v32, hit = TR.uv(r32, mu32, W, Hh)
    du, dv = np.abs(u32.astype(np.float64) * W - 0.5 - px), np.abs(v32.astype(np.float64) * Hh - 0.5 - py)
    print("fp32 round trip, restatement: max distance to the centre %.3g / %.3g texels (u / v)" % (du.max(), dv.max()))
    worst = 0.0
    for y in range(Hh):
        for x in range(W):
            cu, cv, chit = c_uv(pkg, 1, W, Hh, r32[y, x], mu32[y, x])
            assert abs(cu * W - 0.5 - x) <= du[y, x] + float(np.spacing(np.float32(cu))) * W, (x, y)
            assert abs(cv * Hh - 0.5 - y) <= dv[y, x] + float(np.spacing(np.float32(cv))) * Hh, (x, y)
            worst = max(worst, abs(cu * W - 0.5 - x), abs(cv * Hh - 0.5 - y))
    print("fp32 round trip, C function: max distance to the centre %.3g texels" % worst)
    # the host core's texel rays are the restatement's
    out = np.zeros(3, np.float32)
    for x, y in ((0, 0), (255, 0), (0, 63), (255, 63), (17, 5), (200, 40), (255, 31), (1, 62)):
        tlut_host.tlut_host_texel_ray(x, y, W, Hh, P(out))
        assert (out[0], out[1]) == (r32[y, x], mu32[y, x]), (x, y)


# ---------------------------------------------------------------------------------------------------------------- 2, 3. host cores vs restatement
def test_transmittance_core_matches_the_restatement(host_luts, np_trans1):
    t = host_luts[1]
    d = ulp_diff(t, np_trans1)
    print("mapping-1 transmittance LUT, host core vs restatement: max %d fp16 ulp, %.4f %% of values differ" % (d.max(), 100.0 * (d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() < 0.01                  # the gate between the oracle and its restatement (tests/test_oracle_golden.py)
    assert (t[Hh - 1, 0].astype(np.float32) == 1.0).all()          # top of the atmosphere, d = 0: exactly 1
    assert np.isfinite(t.astype(np.float32)).all()


def test_mapping_0_core_is_the_reference(host_luts, hostsim):
    """The templated cores at mapping 0 are the code tests/hostsim has always run: same bytes."""
    t = np.zeros((Hh, W, 4), np.uint16)
    hostsim.hostsim_transmittance(W, Hh, P(t))
    assert (t == host_luts[0].view(np.uint16)).all()


@pytest.mark.parametrize("sun", list(TR.SUNS))
def test_sky_core_matches_the_restatement(tlut_host, host_luts, sun):
    s = TR.norm(TR.SUNS[sun])
    got = host_sky(tlut_host, 1, s, host_luts[1])
    ref = TR.sky_lut_bruneton(s, host_luts[1])
    d = ulp_diff(got, ref)
    print("mapping-1 sky LUT %s, host core vs restatement: max %d fp16 ulp, %.4f %% of values differ" % (sun, d.max(), 100.0 * (d > 0).mean()))
    assert np.isfinite(got.astype(np.float32)).all()
    assert d.max() <= 1 and (d > 0).mean() < 0.03


# ---------------------------------------------------------------------------------------------------------------- 4. the accuracy claim
def test_lookup_accuracy_against_converged_truth(tlut_host, host_luts):
    """Host-core LUTs of both mappings (256 x 64, 40 steps, fp16) looked up by the host-core readers on the query grid, against the converged
    float64 transmittance.  Queries are the fp32 pairs the readers receive; truth blocks a ray that meets the ground, decided on the same pair."""
    res = {}
    for near in (True, False):
        r, mu = TR.query_grid(near)
        truth = TR.transmittance_point(r, mu, 4000)
        quad = TR.transmittance_point(r, mu, 40)
        e = {m: np.abs(host_lookup(tlut_host, m, host_luts[m], r, mu).reshape(r.shape + (4,)) - truth).max(-1) for m in (0, 1)}
        eq = np.abs(quad - truth).max(-1)
        res[near] = (e[0].max(), e[0].mean(), e[1].max(), e[1].mean(), eq.max(), eq.mean())
        print("%s: reference mapping max %.4f mean %.4f | Bruneton max %.4f mean %.4f | 40-step quadrature at the queries max %.4f mean %.4f | blocked queries %d"
              % ("near horizon" if near else "up to zenith", *res[near], int(TR.hits_ground(r, mu).sum())))
    for near in (True, False):
        assert res[near][2] <= res[near][4] + 1e-3, (near, res[near])             # (a) on the quadrature floor + two fp16 steps
    assert res[True][0] >= 5.0 * res[True][2], res[True]                            # (b) near the horizon the reference mapping is >= 5 x worse


# ---------------------------------------------------------------------------------------------------------------- 5. sky-LUT level
def test_sky_lut_accuracy_against_converged_table(tlut_host, host_luts, converged_table):
    dist = {}
    for sun in ("zenith", "deg45", "demo", "deg0p5"):
        s = TR.norm(TR.SUNS[sun])
        hi = TR.sky_lut_bruneton(s, converged_table).astype(np.float64)[..., :3]
        peak = np.abs(hi).max()
        d = {m: np.abs(host_sky(tlut_host, m, s, host_luts[m]).astype(np.float64)[..., :3] - hi).max() / peak for m in (0, 1)}
        dist[sun] = d
        print("sky LUT %s vs converged: reference mapping %.2f %% of the peak, Bruneton %.2f %%" % (sun, 100 * d[0], 100 * d[1]))
    for sun in ("demo", "deg0p5"):
        assert dist[sun][1] <= 0.25 * dist[sun][0], (sun, dist[sun])
    for sun in ("zenith", "deg45"):
        assert dist[sun][1] <= dist[sun][0] + 0.005, (sun, dist[sun])


# ---------------------------------------------------------------------------------------------------------------- 6. state, without a GPU
def test_setters_reject_null_and_unknown_mappings(pkg):
    L, E = pkg.lib(), pkg._lib.ERR_INVALID
    assert L.csky_set_transmittance_mapping(None, 0) == E and L.csky_set_transmittance_mapping(None, 2) == E
    assert L.csky_multi_set_transmittance_mapping(None, 1) == E and L.csky_multi_set_transmittance_mapping(None, 2) == E
    assert L.csky_get_transmittance_mapping(None) < 0
    uv = (C.c_float * 2)()
    assert L.csky_transmittance_uv(2, W, Hh, 6400.0, 0.5, uv, None) == E
    assert L.csky_transmittance_uv(1, 1, Hh, 6400.0, 0.5, uv, None) == E and L.csky_transmittance_uv(1, W, 1, 6400.0, 0.5, uv, None) == E
    assert L.csky_transmittance_uv(1, W, Hh, 6400.0, 0.5, None, None) == E
    assert L.csky_transmittance_uv(1, 2, 2, 6400.0, 0.5, uv, None) == 0               # hits_ground may be NULL
    assert pkg._lib.TLUT_REFERENCE == 0 and pkg._lib.TLUT_BRUNETON == 1 and pkg._lib.ABI_VERSION == 9
    with pytest.raises(ValueError):
        pkg._lib.tlut_mapping("hosek")
