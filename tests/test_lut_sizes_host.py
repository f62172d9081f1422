"""The atmosphere LUT path and the compositor off their default sizes, without a GPU: the host-compiled cores (tests/tlut_host, tests/hostsim,
tests/rays_host: the per-lane code the HIP kernels instantiate) against the references that take a size -- the oracle (mapping 0), the numpy
restatement of tests/tlut_reference.py (mapping 1), oracle.composite / composite_view -- at the sizes tests/test_gpu_lut_sizes.py then runs on the
GPU.  A disagreement that is the reference's own shows here first, on the CPU.  The size lists, the suns and the compositor's case list live
here; the GPU file imports them.

Gates: the ones the default sizes are held to.  Mapping 0, host core vs oracle: the same bytes (tests/test_hostsim_core.py
test_lut_cores_bit_exact).  Mapping 1, host core vs restatement: <= 1 fp16 ulp, and < 1 % (table) / < 3 % (sky LUT) of the halves differing
(tests/test_tlut_mapping.py).  A share of differing halves is taken over the pooled size list: one half of a 1 x 1 LUT is 25 % of it.
Compositor, host core vs oracle: <= 1 ulp and < 1 % differing, pooled likewise (tests/test_compositor.py)."""
import ctypes as C

import numpy as np
import pytest

import shadow_reference as SR
import tlut_reference as TR
from conftest import ulp_diff
from test_clouds_rays_host import host_composite, rays_host  # noqa: F401  (rays_host: the module-scoped fixture)
from test_tlut_gpu import BELOW
from test_tlut_mapping import host_sky, host_trans, tlut_host  # noqa: F401  (tlut_host: the module-scoped fixture)

# transmittance_kernel handles 4 texels per block: its `live` tail runs when w * h is no multiple of 4
TRANS_SIZES = {
    0: [(1, 1),      # a one-texel table; w * h mod 4 = 1
        (1, 7),      # one column; mod 4 = 3
        (7, 1),      # one row; mod 4 = 3
        (3, 5),      # mod 4 = 3
        (5, 5),      # mod 4 = 1
        (13, 9),     # mod 4 = 1, more than one block per row
        (31, 9)],    # mod 4 = 3; SMALL_TABLE[0]
    1: [(2, 2),      # the smallest table the Bruneton mapping accepts; mod 4 = 0
        (3, 2),      # mod 4 = 2
        (5, 3),      # mod 4 = 3
        (7, 9),      # mod 4 = 3
        (33, 9)],    # mod 4 = 1; SMALL_TABLE[1]
}
# sky_lut_kernel and sky_lut_rows_kernel handle 8 texels per block
SKY_SIZES = [(1, 1),      # one texel: every tap of every consumer clamps to it; w * h mod 8 = 1
             (3, 3),      # mod 8 = 1
             (7, 5),      # mod 8 = 3
             (13, 7),     # mod 8 = 3
             (25, 13),    # mod 8 = 5
             (64, 33),    # mod 8 = 0 with an odd height
             (201, 3)]    # mod 8 = 3, wider than the default and three rows high
SMALL_TABLE = {0: (31, 9), 1: (33, 9)}      # a non-default transmittance table per mapping
DEFAULT_TABLE = (256, 64)

ZENITH = np.array([0.0, 1.0, 0.0], np.float32)
SUNS = {"deg45": TR.norm(TR.SUNS["deg45"]), "demo": TR.norm(TR.SUNS["demo"]), "below": BELOW, "zenith": ZENITH}
LUT_SUNS = ("deg45", "demo", "below")

# The compositor off the default shapes: a cross-section in which every value of every axis occurs at least once.
#   clouds 8 x 8, 9 x 5, 33 x 17 | skies (1, 1), (7, 5), (64, 33) | tables 256 x 64, 31 x 9 | blend 0, 1, 0.35 | disk scale 0, 1, 2 | four suns
#   panorama outputs (1, 1), (31, 7), (33, 9), (64, 1), (1, 64), (333, 111): narrower than one 32 x 8 block, one pixel high, one pixel wide, ragged
PANORAMA_CASES = [
    dict(cloud=(8, 8), sky=(1, 1), table=(256, 64), out=(1, 1), blend=0.0, disk=0.0, sun="deg45"),
    dict(cloud=(9, 5), sky=(7, 5), table=(31, 9), out=(31, 7), blend=1.0, disk=1.0, sun="demo"),
    dict(cloud=(33, 17), sky=(64, 33), table=(256, 64), out=(33, 9), blend=0.35, disk=2.0, sun="below"),
    dict(cloud=(9, 5), sky=(7, 5), table=(31, 9), out=(1, 64), blend=0.35, disk=2.0, sun="zenith"),
    dict(cloud=(8, 8), sky=(64, 33), table=(31, 9), out=(64, 1), blend=0.0, disk=1.0, sun="demo"),
    dict(cloud=(33, 17), sky=(7, 5), table=(256, 64), out=(333, 111), blend=0.35, disk=2.0, sun="deg45"),
]
# the view form: 33 x 33 and 31 x 7 (odd, so the centre pixel looks along the camera's axis); pitched +90 (the centre pixel is the zenith:
# atan2f(0, 0)), -90 and on the horizon; fov 1 and 179
VIEW_CASES = [
    dict(cloud=(33, 17), sky=(7, 5), table=(256, 64), out=(33, 33), blend=0.35, disk=2.0, sun="zenith", yaw=0, pitch=90, fov=179.0),
    dict(cloud=(9, 5), sky=(64, 33), table=(31, 9), out=(31, 7), blend=0.0, disk=1.0, sun="deg45", yaw=0, pitch=-90, fov=1.0),
    dict(cloud=(8, 8), sky=(7, 5), table=(31, 9), out=(33, 33), blend=1.0, disk=0.0, sun="demo", yaw=90, pitch=0, fov=1.0),
    dict(cloud=(9, 5), sky=(1, 1), table=(256, 64), out=(31, 7), blend=0.35, disk=2.0, sun="below", yaw=90, pitch=0, fov=179.0),
    dict(cloud=(33, 17), sky=(64, 33), table=(256, 64), out=(33, 33), blend=0.35, disk=2.0, sun="zenith", yaw=0, pitch=90, fov=1.0),
]
COVERAGE_FROM, COVERAGE_TO = 0.2, 0.3        # the two cloud images differ in their cover,
SUN_TO_SHIFT = (0.03, 0.02, 0.0)              # the two skies in their sun: the "to" sky's is this far from it (before normalising; the zenith's too)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def right_angle_basis(yaw, pitch):
    """test_compositor.camera_basis for multiples of 90 degrees, with exact 0 and +-1 entries: a camera pitched +-90 looks along (0, +-1, 0) exactly."""
    def cs(deg):
        return [(1, 0), (0, 1), (-1, 0), (0, -1)][(int(deg) // 90) % 4]
    assert yaw % 90 == 0 and pitch % 90 == 0
    (cy, sy), (cp, sp) = cs(yaw), cs(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float32)
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], np.float32)
    return (ry @ rx).astype(np.float32)


def sun_to(sun):
    return TR.norm(np.asarray(sun, np.float64) + np.array(SUN_TO_SHIFT))


def composite_inputs(case, table_fn, sky_fn, clouds_fn, memo):
    """The five images of a case from the given providers -- table_fn(w, h), sky_fn(sun, table, w, h), clouds_fn(params, sky) -- memoised in
    `memo`, so that what two cases share is rendered once.  Returns (cloud_from, cloud_to, sky_from, sky_to, table, sun)."""
    from oracle import oracle as O

    def once(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]
    sun = SUNS[case["sun"]]
    tw, th = case["table"]
    table = once(("table", tw, th), lambda: table_fn(tw, th))
    sw, sh = case["sky"]
    skies = [once(("sky", tw, th, sw, sh, s.tobytes()), lambda s=s: sky_fn(s, table, sw, sh)) for s in (sun, sun_to(sun))]
    cw, ch = case["cloud"]
    clouds = [once(("cloud", tw, th, sw, sh, cw, ch, sun.tobytes(), cov), lambda cov=cov: clouds_fn(O.default_params(cw, ch, sun, coverage=cov), skies[0]))
              for cov in (COVERAGE_FROM, COVERAGE_TO)]
    return clouds[0], clouds[1], skies[0], skies[1], table, sun


def oracle_composite(oracle, case, inputs):
    cf, ct, sf, st, table, sun = inputs
    w, h = case["out"]
    if "fov" in case:
        return oracle.composite_view(cf, ct, sf, st, table, sun, right_angle_basis(case["yaw"], case["pitch"]), case["fov"], case["blend"], case["disk"], w, h)
    return oracle.composite(cf, ct, sf, st, table, sun, case["blend"], case["disk"], w, h)


@pytest.fixture(scope="module")
def oracle_inputs(oracle, otex):
    """composite_inputs from the oracle alone"""
    memo = {}

    def get(case):
        return composite_inputs(case, oracle.transmittance_lut, oracle.sky_lut, lambda p, sky: oracle.clouds(otex, p, sky), memo)
    return get


def reference_trans(oracle, mapping, w, h):
    return oracle.transmittance_lut(w, h) if mapping == 0 else TR.transmittance_lut(w, h)


def reference_sky(oracle, mapping, sun, table, w, h):
    return oracle.sky_lut(sun, table, w, h) if mapping == 0 else TR.sky_lut_bruneton(sun, table, w, h)


class Pool:
    """ulp distances of several comparisons, pooled: the worst one and the share of halves that differ"""

    def __init__(self):
        self.worst, self.differ, self.n = 0, 0, 0

    def add(self, got, ref):
        d = ulp_diff(got, ref)
        self.worst, self.differ, self.n = max(self.worst, int(d.max())), self.differ + int((d > 0).sum()), self.n + d.size
        return d

    @property
    def share(self):
        return self.differ / max(1, self.n)

    def __str__(self):
        return "max %d fp16 ulp, %d of %d halves differ (%.4f %%)" % (self.worst, self.differ, self.n, 100.0 * self.share)


# ---------------------------------------------------------------------------------------------------------------- 1. transmittance
@pytest.mark.parametrize("mapping", [0, 1])
def test_transmittance_core_matches_the_reference_at_every_size(tlut_host, oracle, mapping):  # noqa: F811
    """Measured: mapping 0 the oracle's bytes at all seven sizes (1 804 halves); mapping 1 max 1 ulp, 1 of 1 540 halves differs (0.065 %)."""
    pool = Pool()
    for w, h in TRANS_SIZES[mapping]:
        got, ref = host_trans(tlut_host, mapping, w, h), reference_trans(oracle, mapping, w, h)
        assert got.shape == ref.shape == (h, w, 4) and np.isfinite(got.astype(np.float32)).all(), (w, h)
        d = pool.add(got, ref)
        assert d.max() <= 1, (mapping, w, h, int(d.max()))
        if mapping == 0:
            assert not d.any(), (w, h)
        else:
            assert (got[h - 1, 0].astype(np.float32) == 1.0).all(), (w, h)         # top of the atmosphere, d = 0: exactly 1
    print("mapping-%d transmittance LUT over %s, host core vs reference: %s" % (mapping, TRANS_SIZES[mapping], pool))
    assert pool.share < 0.01


# ---------------------------------------------------------------------------------------------------------------- 2. sky LUT
@pytest.mark.parametrize("table", ["default-table", "small-table"])
@pytest.mark.parametrize("mapping", [0, 1])
def test_sky_core_matches_the_reference_at_every_size(tlut_host, oracle, mapping, table):  # noqa: F811
    """Measured over the 7 sizes x 3 suns (38 112 halves): mapping 0 the oracle's bytes over both tables; mapping 1 max 1 ulp, 2.07 % of the halves
    differ over the 256 x 64 table and 1.21 % over the 33 x 9 one."""
    tw, th = DEFAULT_TABLE if table == "default-table" else SMALL_TABLE[mapping]
    trans = host_trans(tlut_host, mapping, tw, th)
    pool = Pool()
    for w, h in SKY_SIZES:
        for name in LUT_SUNS:
            got, ref = host_sky(tlut_host, mapping, SUNS[name], trans, w, h), reference_sky(oracle, mapping, SUNS[name], trans, w, h)
            assert got.shape == ref.shape == (h, w, 4) and np.isfinite(got.astype(np.float32)).all(), (w, h, name)
            d = pool.add(got, ref)
            assert d.max() <= 1, (mapping, w, h, name, int(d.max()))
            if mapping == 0:
                assert not d.any(), (w, h, name)
    print("mapping-%d sky LUT over the %d x %d table, %s x %s, host core vs reference: %s" % (mapping, tw, th, SKY_SIZES, LUT_SUNS, pool))
    assert pool.share < 0.03


# ---------------------------------------------------------------------------------------------------------------- 3. compositor
def test_compositor_core_matches_the_oracle_off_the_default_shapes(hostsim, rays_host, oracle, oracle_inputs):  # noqa: F811
    """Measured: the oracle's bytes in all six panorama cases (150 424 halves) and all five view cases (14 804 halves)."""
    pools = {"panorama": Pool(), "view": Pool()}
    for case in PANORAMA_CASES + VIEW_CASES:
        inputs = oracle_inputs(case)
        cf, ct, sf, st, table, sun = inputs
        assert not np.array_equal(bits(cf), bits(ct)) and not np.array_equal(bits(sf), bits(st)), case      # two different "from" and "to" images
        ref = oracle_composite(oracle, case, inputs)
        w, h = case["out"]
        if "fov" in case:
            out = host_composite(rays_host, 0, right_angle_basis(case["yaw"], case["pitch"]), case["fov"], w, h, cf, ct, sf, st, table, case["blend"], case["disk"], sun)
        else:
            out = np.zeros((h, w, 4), np.uint16)
            hostsim.hostsim_composite(w, h, P(bits(cf)), P(bits(ct)), cf.shape[1], cf.shape[0], P(bits(sf)), P(bits(st)), sf.shape[1], sf.shape[0],
                                      P(bits(table)), table.shape[1], table.shape[0], C.c_float(case["blend"]), C.c_float(case["disk"]), P(sun), P(out))
        assert np.isfinite(ref.astype(np.float32)).all() and (ref[..., 3].astype(np.float32) == 1).all(), case
        d = pools["view" if "fov" in case else "panorama"].add(out.view(np.float16), ref)
        assert d.max() <= 1, (case, int(d.max()))
    for k, pool in pools.items():
        print("compositor, %s cases, host core vs oracle: %s" % (k, pool))
        assert pool.share < 0.01, k


# ---------------------------------------------------------------------------------------------------------------- 4. the cases are not trivial
def test_the_sky_size_reaches_the_frame_and_the_composite(oracle, otex, oracle_inputs):
    """A frame marched over a 7 x 5 sky LUT is another frame than the one over 200 x 100 (the set-up's three taps land in other cells), and a
    panorama composited over 7 x 5 skies another panorama: a kernel that ignored sw, sh could not pass both sizes.  Scene A at 64 x 32 has
    alpha > 0 in 64.1 % of its pixels, and 47.3 % of the halves of the two frames differ; 74.1 % of those of the two panoramas (measured on the oracle)."""
    p = SR.scene(oracle, "A")
    sun = np.asarray(p[16:19], np.float32)
    table = oracle.transmittance_lut(*DEFAULT_TABLE)
    frames = [oracle.clouds(otex, p, oracle.sky_lut(sun, table, w, h)) for w, h in ((7, 5), (200, 100))]
    cloudy = float((frames[0][..., 3] > 0).mean())
    differ = float((bits(frames[0]) != bits(frames[1])).mean())
    print("scene A over a (7, 5) and a (200, 100) sky: alpha > 0 in %.1f %% of the pixels, %.1f %% of the halves differ" % (100 * cloudy, 100 * differ))
    assert cloudy >= 0.25 and differ > 0.10
    case = PANORAMA_CASES[-1]
    assert case["sky"] == (7, 5)
    small = oracle_composite(oracle, case, oracle_inputs(case))
    big = oracle_composite(oracle, case, oracle_inputs(dict(case, sky=(200, 100))))
    differ = float((bits(small) != bits(big)).mean())
    print("panorama %s over (7, 5) and (200, 100) skies: %.1f %% of the halves differ" % (case["out"], 100 * differ))
    assert differ > 0.10


def test_every_value_of_every_axis_occurs():
    want = dict(cloud={(8, 8), (9, 5), (33, 17)}, sky={(1, 1), (7, 5), (64, 33)}, table={(256, 64), (31, 9)}, blend={0.0, 1.0, 0.35}, disk={0.0, 1.0, 2.0},
                sun={"deg45", "demo", "below", "zenith"})
    for k, v in want.items():
        assert {c[k] for c in PANORAMA_CASES} == v, k
    assert {c["out"] for c in PANORAMA_CASES} == {(1, 1), (31, 7), (33, 9), (64, 1), (1, 64), (333, 111)}
    assert {c["out"] for c in VIEW_CASES} == {(33, 33), (31, 7)} and {c["pitch"] for c in VIEW_CASES} == {90, -90, 0} and {c["fov"] for c in VIEW_CASES} == {1.0, 179.0}
    assert [w * h % 4 for w, h in TRANS_SIZES[0]] == [1, 3, 3, 3, 1, 1, 3] and [w * h % 4 for w, h in TRANS_SIZES[1]] == [0, 2, 3, 3, 1]
    assert [w * h % 8 for w, h in SKY_SIZES] == [1, 1, 3, 3, 5, 0, 3]
    assert BELOW[1] < 0 and abs(np.degrees(np.arcsin(float(BELOW[1]))) + 1.0) < 1e-3
