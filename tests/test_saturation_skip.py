"""The saturation skip (csrc/cloud_core.h ray_saturated, exact reject (4)) on the CPU: tests/satwalk walks every ray of a frame with the kernel
cores, the full march against the march that freezes (L, alpha) the first time the predicate holds, evaluated before every in-cloud sample --
the earliest any flush of march_compact can latch the ray.  Required everywhere: no ray stores a different half, and the in-cloud tally is the
full march's.  Fired shares are printed for every case (pytest -s); only the headline view must fire."""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT, norm
from saturation_scenes import TABLE, check_fired, load_satwalk, mip_chains, params


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def satwalk():
    return load_satwalk(ROOT)


@pytest.fixture(scope="module")
def chains(pkg, noise):
    return mip_chains(pkg, noise)


def walk(satwalk, chains, oracle, o_trans, w, h, sun, coverage=0.2, density=0.05, primary=128, light=6, alpha_min=-1.0, b_scale=1.0, params=None):
    from bench import usable_cores
    lc, sc, weather = chains
    s = norm(sun)
    sky = np.ascontiguousarray(oracle.sky_lut(s, o_trans, 200, 100)).view(np.uint16)
    p = np.ascontiguousarray(oracle.default_params(w, h, sun, coverage=coverage, density=density) if params is None else params, np.float32)
    out = np.zeros(8, np.float64)
    satwalk.sat_walk(P(lc), P(sc), P(weather), P(p), primary, light, P(sky), 200, 100, w, h, C.c_float(alpha_min), C.c_float(b_scale),
                     max(1, min(16, usable_cores())), P(out), None)
    r = dict(rays=int(out[0]), incloud_full=int(out[1]), incloud_frozen=int(out[2]), fired=int(out[3]), after=int(out[4]), differ=int(out[5]), on=int(out[6]))
    print("saturation walk %dx%d sun=%s cov=%g dens=%g %dx%d alpha_min=%g b_scale=%g: %d of %d rays fired (%.1f %%), %.2f %% of %d in-cloud samples behind "
          "the firing, %d rays differ" % (w, h, tuple(sun), coverage, density, primary, light, alpha_min, b_scale, r["fired"], r["rays"], 100.0 * r["fired"] / max(1, r["rays"]),
                                          100.0 * r["after"] / max(1, r["incloud_full"]), r["incloud_full"], r["differ"]))
    return r


def exact(r):
    assert r["on"] == 1
    assert r["differ"] == 0, r
    assert r["incloud_frozen"] == r["incloud_full"], r


@pytest.mark.parametrize("size", [(1024, 512), (2048, 1024)])
def test_headline_view_is_exact_and_fires(satwalk, chains, oracle, o_trans, size):
    """The C3 view (bench.py: sun (1, 1, 0), coverage 0.2, 128 x 6 steps).  The prototype walk that motivated the change saw 16 % of the rays fire and 9.4 % of the
    in-cloud samples behind the firing; the floors below are a third of that, so the test cannot pass by (almost) never firing."""
    r = walk(satwalk, chains, oracle, o_trans, size[0], size[1], (1, 1, 0))
    exact(r)
    assert r["fired"] >= 0.05 * r["rays"] and r["after"] >= 0.03 * r["incloud_full"], r


@pytest.mark.parametrize("coverage,fired_floor", [(0.1, None), (0.35, 0.14), (0.5, 0.21), (0.8, None)])
def test_coverages(satwalk, chains, oracle, o_trans, coverage, fired_floor):
    """Headline view at other coverages (prototype: 42 % / 63 % of the rays fire at 0.35 / 0.5; floors at a third of that)."""
    r = walk(satwalk, chains, oracle, o_trans, 512, 256, (1, 1, 0), coverage=coverage)
    exact(r)
    if fired_floor is not None:
        assert r["fired"] >= fired_floor * r["rays"], r


@pytest.mark.parametrize("density", [0.01, 0.1])
def test_densities(satwalk, chains, oracle, o_trans, density):
    exact(walk(satwalk, chains, oracle, o_trans, 512, 256, (1, 1, 0), density=density))


@pytest.mark.parametrize("deg", [2.0, 178.0])
def test_grazing_suns_of_the_sweep(satwalk, chains, oracle, o_trans, deg):
    """The first and last frame of bench.py's C5 sweep: sun = (cos th, sin th, 0), th = 2 / 178 degrees."""
    t = np.radians(deg)
    exact(walk(satwalk, chains, oracle, o_trans, 512, 256, (float(np.cos(t)), float(np.sin(t)), 0.0)))


def test_sun_below_the_horizon(satwalk, chains, oracle, o_trans):
    exact(walk(satwalk, chains, oracle, o_trans, 512, 256, (1.0, -0.2, 0.3), coverage=0.35))


@pytest.mark.parametrize("primary,light", [(64, 4), (1024, 6)])
def test_other_march_lengths(satwalk, chains, oracle, o_trans, primary, light):
    """64 x 4 steps, and 1024 primary steps (the accumulation slop is sized from the step count)."""
    exact(walk(satwalk, chains, oracle, o_trans, 192, 96, (1, 1, 0), coverage=0.35, primary=primary, light=light))


@pytest.mark.parametrize("sc", TABLE, ids=lambda s: s.name)
def test_scene_table(satwalk, chains, oracle, o_trans, sc):
    """tests/saturation_scenes.py: where the bound is tight and where the guards L >= 2^-14 and hi < 65504 bind.  The firing counts of the table are this
    walk's; a scene that fires must keep firing (a third of its count), a control must not fire."""
    r = walk(satwalk, chains, oracle, o_trans, sc.size[0], sc.size[1], sc.sun, coverage=sc.coverage, density=sc.density, primary=sc.primary, light=sc.light,
             params=params(oracle, sc))
    exact(r)
    check_fired(sc, r["fired"])


def test_negative_colour_switches_the_skip_off(satwalk, chains, oracle, o_trans):
    """A push-constant block that breaks an assumption of the proof marks the frame (frame_setup_f): the skip stays off and nothing fires."""
    sky = np.ascontiguousarray(oracle.sky_lut(norm((1, 1, 0)), o_trans, 200, 100)).view(np.uint16)
    good = np.ascontiguousarray(oracle.default_params(256, 128, (1, 1, 0), coverage=0.5), np.float32)
    assert satwalk.sat_walk_guard(P(good), 128, P(sky), 200, 100) == 1
    for idx, val in ((12, -0.2), (13, -1e-3), (14, -5.0), (20, -1.0), (21, -0.01), (19, -1.0), (25, -0.05)):   # ground_color, LIGHT_COLOR, LIGHT_ENERGY, density
        bad = good.copy(); bad[idx] = val
        assert satwalk.sat_walk_guard(P(bad), 128, P(sky), 200, 100) == 0, (idx, val)
    bad = good.copy(); bad[13] = -5.0
    r = walk(satwalk, chains, oracle, o_trans, 256, 128, (1, 1, 0), coverage=0.5, params=bad)
    assert r["on"] == 0 and r["fired"] == 0 and r["incloud_frozen"] == r["incloud_full"], r
    assert satwalk.sat_walk_guard(P(good), 65537, P(sky), 200, 100) == 0      # the slop terms are first order in steps * 2^-24


def test_mutation_control(satwalk, chains, oracle, o_trans):
    """A deliberately weakened predicate MUST store different halfs on the coverage-0.35 frame, or the comparison above proves nothing: the alpha
    threshold alone at 1 - 2^-9 (the prototype walk: 7 rays at 512 x 256), and the colour bound alone at B / 8 (nearly always the binding one)."""
    a = walk(satwalk, chains, oracle, o_trans, 512, 256, (1, 1, 0), coverage=0.35, alpha_min=1.0 - 2.0 ** -9)
    assert a["differ"] > 0, a
    b = walk(satwalk, chains, oracle, o_trans, 512, 256, (1, 1, 0), coverage=0.35, alpha_min=1.0 - 2.0 ** -12, b_scale=0.125)
    assert b["differ"] > 0, b
    c = walk(satwalk, chains, oracle, o_trans, 512, 256, (1, 1, 0), coverage=0.35, alpha_min=1.0 - 2.0 ** -12, b_scale=1.0)   # the unmutated constants through the same path
    assert c["differ"] == 0, c
