"""The per-lane code of the cloud depth frame (csrc/depth_core.h on the cloud cores: what depth.hip's lanes run) and of the aerial perspective on a
cloud frame (csrc/cloud_aerial_core.h on aerial_core.h: the definition cloud_aerial.hip must equal), compiled for the host by
tests/cloud_aerial_host, against the numpy restatement of their definitions (tests/cloud_depth_reference.py, which calls the oracle per sample and
tests/aerial_reference.columns per pixel).  A unit test of device code, not a render path: libcloudsky itself has no CPU implementation.

Gates: front and back are bit-equal wherever both sides see the same in-cloud samples; the mean distance is at the project's gate for values
rendered from the shipped assets (shadow_reference.GATE) on pixels with alpha >= 2^-6 and lies between front and back on the thinner ones; the apply
step is at the sky-LUT gate of the aerial-perspective volume (aerial_reference.gate): it is the same per-step code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aerial_reference as AR
import cloud_depth_reference as CR
import shadow_reference as SR
from conftest import ROOT, ulp_diff
from test_aerial_host import SUNS, aerial_host, host_luts  # noqa: F401  (the module-scoped fixtures)
from test_tlut_mapping import tlut_host  # noqa: F401

GOLDEN = os.path.join(ROOT, "tests", "golden")
W, H = CR.SIZE["width"], CR.SIZE["height"]


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.fixture(scope="module")
def ca_host():
    d = os.path.join(ROOT, "tests", "cloud_aerial_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libcloud_aerial_host.so"))
    L.cloud_depth_host_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_uint64)]
    L.cloud_aerial_host_dirs.restype = None
    L.cloud_aerial_host_dirs.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.cloud_aerial_host_apply.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def chains(pkg, noise):
    large, small, weather = noise
    return pkg.assets.build_mips(large, 8), pkg.assets.build_mips(small, 6), np.ascontiguousarray(weather, np.uint8)


@pytest.fixture(scope="module")
def golden_cloud():
    """scene A as the numpy restatement of the cloud march rendered it: float16 [32, 64, 4]"""
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "clouds_np.npz"))["deg45"]).view(np.float16).reshape(H, W, 4)


def host_depth(L, chains, params, width, height, steps, window=True):
    """The host core's depth frame: dict(out float16 [h, w, 4], t0, ss float32 [h, w], incloud [h, w], taken)"""
    out = np.zeros((height, width, 4), np.uint16)
    t0, ss = np.zeros((height, width), np.float32), np.zeros((height, width), np.float32)
    inc = np.zeros((height, width), np.uint32)
    n = C.c_uint64()
    p = np.ascontiguousarray(params, np.float32)
    rc = L.cloud_depth_host_frame(P(chains[0]), P(chains[1]), P(chains[2]), P(p), width, height, steps, int(window), P(out), P(t0), P(ss), P(inc), C.byref(n))
    assert rc == 0
    return dict(out=out.view(np.float16), t0=t0, ss=ss, incloud=inc.astype(np.int64), taken=n.value)


def host_apply(L, mapping, trans, cloud, depth, sun, steps, state=False, in_place=False):
    """The host core's corrected frame float16 [h, w, 4] (and the spectral (L, Tr) float32 [h, w, 8] with state=True)."""
    tr = np.ascontiguousarray(trans).view(np.uint16)
    c, z = np.ascontiguousarray(cloud, np.float16).copy(), np.ascontiguousarray(depth, np.float16)
    h, w = c.shape[:2]
    out = c if in_place else np.zeros((h, w, 4), np.float16)
    st = np.zeros((h, w, 8), np.float32) if state else None
    s = np.ascontiguousarray(sun, np.float32)
    assert L.cloud_aerial_host_apply(mapping, P(tr), tr.shape[1], tr.shape[0], w, h, steps, P(s), P(c), P(z), P(out), P(st)) == 0
    return (out, st) if state else out


def synthetic_depth(kind, cloud):
    """A depth frame for the apply tests: the distance in r, g and b, the cloud frame's alpha in a."""
    if kind == "ramp":
        d = np.linspace(0.5, 120.0, W * H, dtype=np.float32).reshape(H, W)
    else:
        d = np.full((H, W), float(kind), np.float32)
    z = np.zeros((H, W, 4), np.float16)
    z[..., 0] = z[..., 1] = z[..., 2] = d.astype(np.float16)
    z[..., 3] = cloud[..., 3]
    return z


DEPTHS = [1.5, 10.0, 65.0, "ramp"]


# ---------------------------------------------------------------------------------------------------------------- C1
@pytest.mark.parametrize("name", ["A", "B"])
def test_depth_core_matches_restatement(ca_host, chains, oracle, otex, name):
    p = SR.scene(oracle, name)
    N = CR.STEPS[name]
    ref = CR.depth_frame(oracle, otex, p, W, H, N)
    hit = ref["hit"]
    thin = hit & (ref["alpha"] > 0) & (ref["alpha"] < CR.THIN)
    print("scene %s restated: %.1f %% of the pixels in cloud, %.1f %% empty, %.1f %% of the in-cloud pixels thinner than 2^-6"
          % (name, 100.0 * hit.mean(), 100.0 * (~hit).mean(), 100.0 * thin.sum() / hit.sum()))
    assert hit.mean() >= 0.40 and (~hit).mean() >= 0.20          # preconditions on the RESTATEMENT: an empty or a full frame cannot pass
    assert thin.sum() <= 0.05 * hit.sum()
    got = host_depth(ca_host, chains, p, W, H, N)
    up = ref["above"]
    assert (got["t0"][up].view(np.uint32) == ref["t0"][up].view(np.uint32)).all() and (got["ss"][up].view(np.uint32) == ref["ss"][up].view(np.uint32)).all()
    same = got["incloud"] == ref["incloud"]
    differ = int((~same & (hit | (got["incloud"] > 0))).sum())
    print("scene %s: %d pixels whose in-cloud sample count differs from the restatement's (of %d in cloud); samples %d vs %d"
          % (name, differ, int(hit.sum()), int(got["incloud"].sum()), int(ref["incloud"].sum())))
    assert differ <= 0.005 * hit.sum()
    sel = same & hit
    o, r = bits(got["out"]), bits(ref["out"])
    assert (o[sel][:, 1:3] == r[sel][:, 1:3]).all()               # front, back: bit-equal
    assert (o[same & ~hit] == 0).all()
    thick = sel & (ref["alpha"] >= CR.THIN)
    assert thick.sum() >= 0.9 * hit.sum()
    SR.assert_gate(got["out"][..., 0][thick], ref["out"][..., 0][thick], "depth core, mean distance, scene " + name)
    SR.assert_gate(got["out"][..., 3][sel], ref["out"][..., 3][sel], "depth core, alpha, scene " + name)
    g = got["out"].astype(np.float32)
    nz = o.any(-1)
    assert (g[nz][:, 1] <= g[nz][:, 0]).all() and (g[nz][:, 0] <= g[nz][:, 2]).all()        # front <= mean <= back in halves, thin pixels included
    # the height window and its wave-uniform exit are exact: the same bytes without them, from every sample
    nowin = host_depth(ca_host, chains, p, W, H, N, window=False)
    assert (bits(nowin["out"]) == o).all() and (nowin["incloud"] == got["incloud"]).all()
    assert nowin["taken"] == int(up.sum()) * N and got["taken"] <= nowin["taken"]
    print("scene %s: lane-samples %d of %d with the height-window exit" % (name, got["taken"], nowin["taken"]))


# ---------------------------------------------------------------------------------------------------------------- C2
def test_depth_alpha_is_the_frames(ca_host, chains, oracle, golden_cloud):
    got = host_depth(ca_host, chains, SR.scene(oracle, "A"), W, H, 128)
    a, g = got["out"][..., 3], golden_cloud[..., 3]
    d = ulp_diff(a, g)
    print("depth frame alpha against the golden frame's: %d of %d halves differ, worst %d fp16 ulp" % (int((d > 0).sum()), d.size, int(d.max())))
    assert (g > 0).mean() >= 0.40 and d.max() <= 1


# ---------------------------------------------------------------------------------------------------------------- C3
def test_depth_known_answers(ca_host, chains, oracle):
    p0 = oracle.default_params(W, H, (1, 1, 0), coverage=0.0)
    assert not bits(host_depth(ca_host, chains, p0, W, H, 128)["out"]).any()
    p = SR.scene(oracle, "A")
    got = host_depth(ca_host, chains, p, W, H, 128)
    o = bits(got["out"])
    e = np.zeros((H, W, 3), np.float32)
    rd = np.zeros((H, W, 3), np.float32)
    ca_host.cloud_aerial_host_dirs(W, H, P(e), P(rd))
    assert (e.view(np.uint32) == CR.pixel_dirs(W, H).view(np.uint32)).all()                 # the direction the core derives is the definition's
    up = e[..., 1] > 0
    assert (~up).sum() == W + H - 1 and not o[~up].any()                                     # dir.y <= 0: the frame's first row and first column
    assert np.abs(rd[up] - e[up]).max() <= 4 * 2.0 ** -23                                    # ray_setup re-normalises a unit vector: a few fp32 ulp
    assert not rd[~up].any()
    nz = o.any(-1)
    assert nz.mean() >= 0.40
    t0, ss = got["t0"], got["ss"]
    lo = (t0 / np.float32(1000.0)).astype(np.float16)
    hi = ((t0 + np.float32(128.0) * ss) / np.float32(1000.0)).astype(np.float16)
    g = got["out"]
    assert (g[nz][:, 1] >= lo[nz]).all() and (g[nz][:, 2] <= hi[nz]).all()                   # front >= t0, back <= t0 + N ss: rounding is monotone
    assert (t0[up] >= 1500.0).all() and (ss[up] * 128 >= 2500.0 - 1.0).all()
    # the pixels of a 32 x 16 frame have the uv of every second pixel of the 64 x 32 one
    small = host_depth(ca_host, chains, p, W // 2, H // 2, 128)
    assert (bits(small["out"]) == o[::2, ::2]).all() and bits(small["out"]).any()


# ---------------------------------------------------------------------------------------------------------------- C4
@pytest.fixture(scope="module")
def applied(golden_cloud, host_luts):  # noqa: F811
    """The restated apply step of every (depth, mapping, sun) case at n = 16, computed once and shared."""
    memo = {}

    def get(depth, mapping, sun, steps=16):
        key = (depth, mapping, sun, steps)
        if key not in memo:
            memo[key] = CR.apply(golden_cloud, synthetic_depth(depth, golden_cloud), SUNS[sun], steps, host_luts[mapping], mapping)
        return memo[key]
    return get


@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("sun", ["deg45", "demo", "degm2"])
@pytest.mark.parametrize("depth", DEPTHS, ids=[str(d) for d in DEPTHS])
def test_apply_core_matches_restatement(ca_host, golden_cloud, host_luts, applied, depth, sun, mapping):  # noqa: F811
    z = synthetic_depth(depth, golden_cloud)
    ref = applied(depth, mapping, sun)
    worked = ref["worked"]
    assert worked.mean() >= 0.40 and (~worked).mean() >= 0.20
    moved = ulp_diff(ref["out"][..., :3], golden_cloud[..., :3])[worked] > 8
    print("apply %s km, %s, mapping %d: %.1f %% of the in-cloud rgb halves move by more than 8 fp16 ulp" % (depth, sun, mapping, 100.0 * moved.mean()))
    assert moved.mean() >= 0.50                                   # precondition on the RESTATEMENT: the air does something
    got, st = host_apply(ca_host, mapping, host_luts[mapping], golden_cloud, z, SUNS[sun], 16, state=True)
    assert (bits(got)[..., 3] == bits(golden_cloud)[..., 3]).all()
    assert (bits(got)[~worked] == bits(golden_cloud)[~worked]).all()
    assert np.isfinite(got.astype(np.float32)).all()
    differ, cancel = AR.gate(got[None], ref["out"][None], st[None, ..., :4], ref["L"][None], keep=worked, what="apply %s %s %d" % (depth, sun, mapping))
    print("apply %s km, %s, mapping %d: %d halves differ from the restatement, %d let through as cancellation" % (depth, sun, mapping, differ, cancel))
    same = host_apply(ca_host, mapping, host_luts[mapping], golden_cloud, z, SUNS[sun], 16, in_place=True)
    assert (bits(same) == bits(got)).all()                        # out may be the cloud frame


@pytest.mark.parametrize("steps", [1, 5, 64])
def test_apply_core_other_step_counts(ca_host, golden_cloud, host_luts, applied, steps):  # noqa: F811
    z = synthetic_depth("ramp", golden_cloud)
    ref = applied("ramp", 0, "deg45", steps)
    got, st = host_apply(ca_host, 0, host_luts[0], golden_cloud, z, SUNS["deg45"], steps, state=True)
    AR.gate(got[None], ref["out"][None], st[None, ..., :4], ref["L"][None], keep=ref["worked"], what="apply ramp, n = %d" % steps)


def test_apply_passes_through(ca_host, golden_cloud, host_luts):  # noqa: F811
    zero = np.zeros((H, W, 4), np.float16)
    assert (bits(host_apply(ca_host, 0, host_luts[0], golden_cloud, zero, SUNS["deg45"], 16)) == bits(golden_cloud)).all()
    odd = zero.copy()
    odd[..., 0] = np.where(np.arange(W)[None, :] % 2 == 0, np.float16(-3.0), np.float16(np.nan))      # negative and NaN distances are no distance
    assert (bits(host_apply(ca_host, 0, host_luts[0], golden_cloud, odd, SUNS["deg45"], 16)) == bits(golden_cloud)).all()
    clear = golden_cloud.copy()
    clear[..., 3] = 0
    clear[::2, :, 3] = np.float16(-0.0)
    z = synthetic_depth(10.0, golden_cloud)
    assert (bits(host_apply(ca_host, 1, host_luts[1], clear, z, SUNS["demo"], 16)) == bits(clear)).all()


# ---------------------------------------------------------------------------------------------------------------- C5
@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("sun", ["deg45", "demo", "degm2"])
def test_apply_is_the_volumes_column(ca_host, aerial_host, golden_cloud, host_luts, sun, mapping):  # noqa: F811
    """Each pixel equals the last (only) slice of a D = 1, S = 16 column of the aerial-perspective volume with far_km = the pixel's distance,
    composited in fp32 as the header says: bit for bit."""
    e = np.zeros((H, W, 3), np.float32)
    ca_host.cloud_aerial_host_dirs(W, H, P(e), None)
    tr = np.ascontiguousarray(host_luts[mapping]).view(np.uint16)
    s = np.ascontiguousarray(SUNS[sun], np.float32)
    f32 = np.float32
    for depth in DEPTHS:
        z = synthetic_depth(depth, golden_cloud)
        worked = ~CR.passes(golden_cloud, z)
        got = host_apply(ca_host, mapping, host_luts[mapping], golden_cloud, z, SUNS[sun], 16)
        far = np.ascontiguousarray(z[..., 0].astype(f32)[worked])
        ew = np.ascontiguousarray(e[worked])
        n = far.size
        assert n >= 0.40 * W * H
        out, st = np.zeros((n, 1, 4), np.uint16), np.zeros((n, 1, 8), f32)
        assert aerial_host.aerial_host_columns(mapping, P(tr), tr.shape[1], tr.shape[0], n, P(ew), P(far), P(s), 1, 16, P(out), P(st)) == 0
        L, Tr = st[:, 0, :4], st[:, 0, 4:]
        M = AR.NR.M
        rgb = M[0] * L[:, 0:1] + M[1] * L[:, 1:2] + M[2] * L[:, 2:3] + M[3] * L[:, 3:4]
        assert (rgb.astype(np.float16).view(np.uint16) == out[:, 0, :3]).all()              # the numpy matrix product is the slice's own
        t = (((Tr[:, 0] + Tr[:, 1]) + Tr[:, 2]) + Tr[:, 3]) * f32(0.25)
        assert (t.astype(np.float16).view(np.uint16) == out[:, 0, 3]).all()
        c = golden_cloud[worked].astype(f32)
        want = (c[:, :3] * t[:, None] + c[:, 3:4] * (rgb / f32(50.0)))
        assert want.dtype == f32
        assert (want.astype(np.float16).view(np.uint16) == bits(got)[worked][:, :3]).all(), (depth, sun, mapping)
