"""The compact march per 8x8 tile on the CPU (tests/tilewalk: lock-step primary steps, the 64-sample flush, the in-order replay, the saturation test after
the replay, the carry), in both forms of the kernel's TALLY parameter (march_compact.h march_compact): the launch that delivers the in-cloud count, where a
latched ray keeps taking primary samples, and the launch that does not, where a latched ray is dead.  Required on the frames tests/test_saturation_skip.py
walks: no ray stores a different half than the plain walk in either form, the counting form delivers the plain walk's in-cloud count, and the dead-lane form
removes primary lane-steps.  The floors are a third of the cut the emulation measured when the change was proposed (-7.9 % of the in-window lane-steps
on the headline view at 1024 x 512, -23.5 % at coverage 0.35), so that the test cannot pass by never latching.  Every share is printed (pytest -s)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, norm
from saturation_scenes import TABLE, check_fired, mip_chains, params

BLOCK = ("light_marched", "incloud", "wave_steps", "lanes_weather", "lanes_shape", "lanes_detail", "differ", "latched")


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def tilewalk():
    d = os.path.join(ROOT, "tests", "tilewalk")
    subprocess.check_call(["make", "-C", d, "-s"])
    return C.CDLL(os.path.join(d, "libtilewalk.so"))


@pytest.fixture(scope="module")
def chains(pkg, noise):
    return mip_chains(pkg, noise)


def cut(a, b):
    return 100.0 * (a - b) / max(1, a)


def walk(tilewalk, chains, oracle, o_trans, w, h, sun, coverage=0.2, primary=128, light=6, alpha_min=-1.0, b_scale=1.0, params=None):
    from bench import usable_cores
    lc, sc, weather = chains
    sky = np.ascontiguousarray(oracle.sky_lut(norm(sun), o_trans, 200, 100)).view(np.uint16)
    p = np.ascontiguousarray(oracle.default_params(w, h, sun, coverage=coverage) if params is None else params, np.float32)
    out, misc = np.zeros(24, np.float64), np.zeros(2, np.float64)
    tilewalk.tile_walk(P(lc), P(sc), P(weather), P(p), primary, light, P(sky), 200, 100, w, h, C.c_float(alpha_min), C.c_float(b_scale),
                       max(1, min(16, usable_cores())), P(out), P(misc))
    r = {name: {k: int(v) for k, v in zip(BLOCK, out[8 * i:8 * i + 8])} for i, name in enumerate(("plain", "tally", "dead"))}
    r["rays"], r["on"] = int(misc[0]), int(misc[1])
    pl, ta, de = r["plain"], r["tally"], r["dead"]
    print("tile walk %dx%d sun=%s cov=%g %dx%d alpha_min=%g b_scale=%g: %d rays, %d in-cloud samples" % (w, h, tuple(sun), coverage, primary, light, alpha_min, b_scale, r["rays"], pl["incloud"]))
    print("  light-marched          plain %d   tally %d (%.2f %%)   dead %d (%.2f %%)" % (pl["light_marched"], ta["light_marched"], -cut(pl["light_marched"], ta["light_marched"]),
                                                                                        de["light_marched"], -cut(pl["light_marched"], de["light_marched"])))
    print("  primary wave-steps     tally %d   dead %d (%.2f %%)" % (ta["wave_steps"], de["wave_steps"], -cut(ta["wave_steps"], de["wave_steps"])))
    for k, what in (("lanes_weather", "in-window (weather tap)"), ("lanes_shape", "shape tap"), ("lanes_detail", "detail tap")):
        print("  lane-steps %-24s plain %d   tally %d   dead %d (%.2f %% of tally)" % (what, pl[k], ta[k], de[k], -cut(ta[k], de[k])))
    print("  rays latched           tally %d   dead %d;   rays with a differing stored half: tally %d   dead %d" % (ta["latched"], de["latched"], ta["differ"], de["differ"]))
    return r


def exact(r):
    assert r["on"] == 1
    assert r["tally"]["differ"] == 0 and r["dead"]["differ"] == 0, r
    assert r["tally"]["incloud"] == r["plain"]["incloud"], r                  # the counting form delivers the full march's count
    # both forms queue the same samples in the same order: same flushes, same latches
    assert r["dead"]["light_marched"] == r["tally"]["light_marched"] and r["dead"]["latched"] == r["tally"]["latched"], r
    assert r["dead"]["wave_steps"] <= r["tally"]["wave_steps"] and r["dead"]["lanes_weather"] <= r["tally"]["lanes_weather"], r


def test_headline_view_removes_lane_steps(tilewalk, chains, oracle, o_trans):
    """The C3 view at 1024 x 512 (bench.py: sun (1, 1, 0), coverage 0.2, 128 x 6 steps): at least 2.6 % of the in-window lane-steps go."""
    r = walk(tilewalk, chains, oracle, o_trans, 1024, 512, (1, 1, 0))
    exact(r)
    assert r["tally"]["light_marched"] < r["plain"]["light_marched"], r
    assert cut(r["tally"]["lanes_weather"], r["dead"]["lanes_weather"]) >= 2.6, r


def test_coverage_035_removes_lane_steps(tilewalk, chains, oracle, o_trans):
    """Coverage 0.35 at 1024 x 512: at least 7.8 % of the in-window lane-steps go."""
    r = walk(tilewalk, chains, oracle, o_trans, 1024, 512, (1, 1, 0), coverage=0.35)
    exact(r)
    assert cut(r["tally"]["lanes_weather"], r["dead"]["lanes_weather"]) >= 7.8, r


@pytest.mark.parametrize("coverage", [0.1, 0.35, 0.5, 0.8])
def test_coverages(tilewalk, chains, oracle, o_trans, coverage):
    exact(walk(tilewalk, chains, oracle, o_trans, 512, 256, (1, 1, 0), coverage=coverage))


@pytest.mark.parametrize("deg", [2.0, 178.0])
def test_grazing_suns_of_the_sweep(tilewalk, chains, oracle, o_trans, deg):
    """The first and last frame of bench.py's C5 sweep: sun = (cos th, sin th, 0), th = 2 / 178 degrees."""
    t = np.radians(deg)
    exact(walk(tilewalk, chains, oracle, o_trans, 512, 256, (float(np.cos(t)), float(np.sin(t)), 0.0)))


@pytest.mark.parametrize("primary,light", [(64, 4), (1024, 6)])
def test_other_march_lengths(tilewalk, chains, oracle, o_trans, primary, light):
    exact(walk(tilewalk, chains, oracle, o_trans, 192, 96, (1, 1, 0), coverage=0.35, primary=primary, light=light))


@pytest.mark.parametrize("sc", TABLE, ids=lambda s: s.name)
def test_scene_table(tilewalk, chains, oracle, o_trans, sc):
    """tests/saturation_scenes.py in both TALLY forms.  A scene that fires must latch at least the floor of the table (the test after the last flush
    latches a few rays more than the per-sample walk of tests/satwalk sees fire).  A control must leave no sample behind a latch: both forms light-march
    every in-cloud sample and the dead-lane form removes no lane-step; and no ray latches at all, except in the two shortest marches, whose steps are so
    long that alpha reaches 1 at the LAST flush, where nothing is left to skip (4 512 rays of the 2 x 0 scene latch there)."""
    r = walk(tilewalk, chains, oracle, o_trans, sc.size[0], sc.size[1], sc.sun, coverage=sc.coverage, primary=sc.primary, light=sc.light, params=params(oracle, sc))
    exact(r)
    if sc.fired:
        check_fired(sc, r["tally"]["latched"])
        assert r["tally"]["light_marched"] < r["plain"]["light_marched"], r
    else:
        if sc.name not in ("2x0", "1x6"):       # hi < 65504 / L >= 2^-14 / alpha >= 1 - 2^-12 can never hold in the other controls: no latch at all
            assert r["tally"]["latched"] == 0 and r["dead"]["latched"] == 0, r
        assert r["tally"]["light_marched"] == r["plain"]["light_marched"] == r["plain"]["incloud"], r
        assert all(r["dead"][k] == r["tally"][k] for k in ("wave_steps", "lanes_weather", "lanes_shape", "lanes_detail")), r


def test_mutation_control(tilewalk, chains, oracle, o_trans):
    """The alpha threshold weakened to 1 - 2^-9 MUST store different halfs on the coverage-0.35 frame, in both forms, or the comparisons above prove
    nothing.  At 1024 x 512: the once-per-flush test latches later than the per-sample test of tests/satwalk, so fewer rays are caught between the two
    thresholds (10 here; none of the 512 x 256 frame's).  The product's threshold through the same mutated path must store no differing half."""
    a = walk(tilewalk, chains, oracle, o_trans, 1024, 512, (1, 1, 0), coverage=0.35, alpha_min=1.0 - 2.0 ** -9)
    assert a["tally"]["differ"] > 0 and a["dead"]["differ"] > 0, a
    c = walk(tilewalk, chains, oracle, o_trans, 512, 256, (1, 1, 0), coverage=0.35, alpha_min=1.0 - 2.0 ** -12)
    assert c["tally"]["differ"] == 0 and c["dead"]["differ"] == 0, c
