"""The saturation skip on the device over the range its proof assumes (cloud_core.h ray_saturated, the comment above it; march_compact.h march_compact).
The headline path -- csky_render_clouds_device without a stats buffer, whole rays, TALLY = false, a latched ray is DEAD -- rests on that proof and on the
device's v_exp_f32 / v_rcp_f32 / v_cvt_f16_f32 behaving as it assumes.  Every scene of tests/saturation_scenes.py (light energies 0 .. 1e30, a dark colour
channel, a bright ground, density 0 and 5, suns below the horizon, 1 .. 1024 primary steps, a stratus-only weather map, the early-out, blocks the guard of
frame_setup_f must refuse) is rendered with csky_set_height_window(1) and (0) -- the second is the full march in the same kernel, fc.sat_skip == 0 -- in the host
form (stats buffer: TALLY = true) and the device form (none: DEAD), plain and persistent launches, one frame and two frames in flight.  Every frame must equal
the scene's full-march host frame half for half -- there is no tolerance --, and the stats launches must count the same samples with the skip on and off.
So that no scene passes by never firing, tests/satwalk walks the scene's own parameter block first: a scene of the `fires` kind must fire on at least a third
of the rays counted when the table was written, a control on none.

The second half runs conftest.fuzz_case(0..11) against the oracle on whole-ray launches (csky_set_segments(1)), plain and persistent, host and device form:
tests/test_gpu_parity.py::test_fuzz_parameters_vs_oracle renders the same tiles as 4 interleaved segments, which have no skip and no persistent form.

Mutation check (scratch builds of the library, MI355X; profiles/r20/saturation_range_mutations.txt): with SAT_ALPHA_MIN = 1 - 2^-9
8 scenes fail (energy 3e-3, 30, 1e3, 1e5, 1e6, the bright ground, the low sun at 1e-2 and 1e-3) with 1 to 3 differing halfs of 131 072, so 256 x 128 is large
enough for that threshold (the tile walk needed 1024 x 512); with the bound scaled by 1/8 in ray_saturation_bound 24 scenes fail, every scene that fires but
the early-out one, with 67 (ragged density 5) to 12 258 (energy 0) differing halfs.  In every failing scene all ten skip-on forms differ, by the same count,
and no skip-off form does.  The early-out scene at 1e-3 passes under both: the early-out takes a lane before it could latch, so the skip is inert there; at 1e-5 the
frames legitimately differ with the skip (test_early_out_below_the_latch_threshold says why and what is required instead)."""
import numpy as np
import pytest

from conftest import ROOT, cloud_tight, norm, ulp_diff
from saturation_scenes import EARLY_OUT, EARLY_OUT_DEEP, EDGES, RAGGED, REFUSED, STRATUS, TABLE, check_fired, load_satwalk, mip_chains, params, stratus
from test_gpu_small_detail_lds import _context, _device_frames, _host_frame
from test_saturation_skip import walk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain(pkg, noise):
    ctx = _context(pkg, 0, noise)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def persistent(pkg, noise):
    ctx = _context(pkg, 2, noise)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def satwalk():
    return load_satwalk(ROOT)


@pytest.fixture(scope="module")
def chains(pkg, noise):
    return mip_chains(pkg, noise)


def _all_forms(plain, persistent, p, sun, W, H):
    """-> [(form, frame, stats or None)] of one setting of the switch"""
    out = []
    for name, ctx in (("plain", plain), ("persistent", persistent)):
        img, st = _host_frame(ctx, p)
        out.append(("%s, stats" % name, img, st))
        for k, f in enumerate(_device_frames(ctx, p, W, H, 1, sun=sun)):
            out.append(("%s, no stats, pass %d" % (name, k), f, None))
    for k, f in enumerate(_device_frames(persistent, p, W, H, 2, sun=sun)):
        out.append(("persistent, no stats, two in flight, frame %d" % k, f, None))
    return out


def _render(plain, persistent, oracle, sc):
    """-> {switch: [(form, frame, stats or None)]}: the scene in every form with the skip off (0) and on (1)"""
    W, H = sc.size
    p, sun = params(oracle, sc), norm(sc.sun)
    forms = {}
    try:
        for ctx in (plain, persistent):
            ctx.set_march(sc.primary, sc.light); ctx.set_early_out(sc.early_out)
            ctx.render_sky_lut(sun, 200, 100)
        for switch in (0, 1):
            for ctx in (plain, persistent):
                ctx.set_height_window(switch)
            forms[switch] = _all_forms(plain, persistent, p, sun, W, H)
    finally:
        for ctx in (plain, persistent):
            ctx.set_height_window(1); ctx.set_march(128, 6); ctx.set_early_out(0.0)
    return forms


def _compare(plain, persistent, oracle, sc):
    """Renders the scene in every form with the skip on and off; -> the full-march host frame of the plain context (uint16 [H, W, 4])."""
    W, H = sc.size
    forms = _render(plain, persistent, oracle, sc)
    ref = forms[0][0][1]
    assert ref.shape == (H, W, 4)
    differing = ["skip %s, %s: %d" % (("off", "on")[switch], form, int((f != ref).sum())) for switch in (0, 1) for form, f, _ in forms[switch] if (f != ref).any()]
    assert not differing, "scene %s: halfs of %d that differ from the full-march host frame -- %s" % (sc.name, ref.size, "; ".join(differing))
    for (form, _, off), (_, _, on) in zip(forms[0], forms[1]):
        if off is not None:
            assert on["incloud_samples"] == off["incloud_samples"] and on["primary_samples"] == off["primary_samples"], (sc.name, form, on, off)
    covered = float((ref.view(np.float16)[..., 3] > 0).mean())
    print("scene %s: alpha > 0 in %.1f %% of the pixels, %d in-cloud samples" % (sc.name, 100.0 * covered, forms[0][0][2]["incloud_samples"]))
    if not sc.empty:
        assert covered >= 0.25, (sc.name, covered)
    return ref


def _walk(satwalk, chains, oracle, o_trans, sc, weather=None):
    """the CPU walk of the scene's own parameter block: it fires where the table says, and the earliest freeze stores the full march's halfs"""
    lc, sc_chain, w = chains
    r = walk(satwalk, (lc, sc_chain, w if weather is None else weather), oracle, o_trans, sc.size[0], sc.size[1], sc.sun, coverage=sc.coverage, density=sc.density,
             primary=sc.primary, light=sc.light, params=params(oracle, sc))
    assert r["differ"] == 0 and r["incloud_frozen"] == r["incloud_full"], (sc.name, r)
    check_fired(sc, r["fired"])
    return r


@pytest.mark.parametrize("sc", TABLE + EDGES + RAGGED, ids=lambda s: s.name)
def test_scene_equals_its_full_march(plain, persistent, satwalk, chains, oracle, o_trans, sc):
    r = _walk(satwalk, chains, oracle, o_trans, sc)
    assert r["on"] == 1, sc.name
    ref = _compare(plain, persistent, oracle, sc)
    if sc.name == "energy-1e7":
        # the upper guard hi < 65504 binds inside this frame: it holds finite values next to the largest half and halfs that overflowed
        v = ref[..., :3]
        finite = v[(v & 0x7C00) != 0x7C00].view(np.float16)
        assert (finite > 6.0e4).any() and (v == 0x7C00).any(), (float(finite.max()), int((v == 0x7C00).sum()))


def test_early_out_shares_the_live_flag(plain, persistent, satwalk, chains, oracle, o_trans):
    """csky_set_early_out(1e-3) on the default-lit scene: `live` goes false for a dead lane and for a lane whose transmittance is under the threshold alike.
    A ray that could latch (alpha >= 1 - 2^-12, transmittance about 2.4e-4) is taken by the early-out at the same flush with the skip on or off, so the frames
    stay equal -- and the skip is inert: the scene passes under both mutations of the docstring above."""
    _walk(satwalk, chains, oracle, o_trans, EARLY_OUT)
    _compare(plain, persistent, oracle, EARLY_OUT)


def test_early_out_below_the_latch_threshold(plain, persistent, satwalk, chains, oracle, o_trans):
    """csky_set_early_out(1e-5): rays latch (transmittance about 2.4e-4) before the early-out could take them, so dead lanes and early-out lanes do coexist.
    The frames with the skip on and off are NOT equal here, and neither side is wrong (MI355X: 353 of 131 072 halfs in 349 pixels differ, in every form alike).  The early-out
    is tested once per flush (march_compact, after the replay), so a ray whose transmittance falls under the threshold still composites what it had queued up
    to that flush; how much that is depends on how fast its wavefront's queue fills, and a latched neighbour queues nothing.  In the form without a stats
    buffer a wavefront of dead and early-out lanes also ends with its carried samples uncomposited, where the counting form, whose latched lanes stay live,
    composites them at its last flush.  The early-out is a bounded-error switch that is off by default; what holds exactly, and is required here:
      - a ray that neither latched nor fell under the threshold composites all its samples in order whatever its neighbours do, and every other ray has
        alpha >= 1 - 2^-12 (1 - alpha is the transmittance up to rounding, and 1e-5 < 2^-12), stored as the half 1.0: the alpha planes are equal, and a colour
        half differs only in a pixel whose stored alpha is 1.0;
      - with the skip off nothing latches, so the two TALLY forms queue and composite the same samples: all ten frames are equal;
      - with the skip on, the plain and the persistent launch of the same form are equal, as are both passes and all frames in flight.
    These catch a lane that is killed while it should march; they do not catch a predicate that fires too early (both mutated builds pass them): a ray
    latched too early moves by a half ulp or so, as a legitimately early-outed one may."""
    sc = EARLY_OUT_DEEP
    _walk(satwalk, chains, oracle, o_trans, sc)
    forms = _render(plain, persistent, oracle, sc)
    off, on = forms[0][0][1], forms[1][0][1]
    for form, f, _ in forms[0]:
        assert np.array_equal(f, off), (sc.name, "skip off", form, int((f != off).sum()))
    for form, f, _ in forms[1]:
        want = on if form.endswith("stats") and "no stats" not in form else forms[1][1][1]      # the stats launches; the launches without stats
        assert np.array_equal(f, want), (sc.name, "skip on", form, int((f != want).sum()))
        assert np.array_equal(f[..., 3], off[..., 3]), (sc.name, form, "alpha planes differ", int((f[..., 3] != off[..., 3]).sum()))
        moved = (f[..., :3] != off[..., :3]).any(axis=2)
        print("scene %s, skip on, %s: %d pixels differ from the skip-off frame" % (sc.name, form, int(moved.sum())))
        assert (off[..., 3][moved] == 0x3C00).all(), (sc.name, form, "a pixel that is not opaque moved", int((off[..., 3][moved] != 0x3C00).sum()))
    assert (off.view(np.float16)[..., 3] > 0).mean() >= 0.25


def test_stratus_only_weather_map(pkg, noise, satwalk, chains, oracle, o_trans):
    """ct_mode 2 (cloud type below 0.5 everywhere), coverage 0.6, on contexts of its own"""
    large, small, weather = noise
    w2 = stratus(weather)
    _walk(satwalk, chains, oracle, o_trans, STRATUS, weather=w2)
    a = _context(pkg, 0, (large, small, w2))
    try:
        b = _context(pkg, 2, (large, small, w2))
        try:
            _compare(a, b, oracle, STRATUS)
        finally:
            b.close()
    finally:
        a.close()


@pytest.mark.parametrize("sc", REFUSED, ids=lambda s: s.name)
def test_guard_refuses_on_the_device(plain, persistent, satwalk, chains, oracle, o_trans, sc):
    """frame_setup_kernel evaluates the guard: for a block it must refuse, the switch changes no bit of the frame, NaN halfs included.  The frames are not
    blank: alpha does not depend on the colours or the energy, so it is positive where the default scene's is (the negative density alone stores alpha 0
    everywhere and is marked empty in the table)."""
    r = _walk(satwalk, chains, oracle, o_trans, sc)
    assert r["on"] == 0 and r["fired"] == 0, (sc.name, r)
    _compare(plain, persistent, oracle, sc)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_whole_rays_vs_oracle(plain, persistent, oracle, otex, o_trans, seed):
    """tests/test_gpu_parity.py::test_fuzz_parameters_vs_oracle on the kernel that is shipped: whole rays (the skip is compiled in), plain and persistent, host
    form and device form, through the same gate."""
    from conftest import fuzz_case
    p, sun, (tw, th), primary, light = fuzz_case(seed)
    sk = oracle.sky_lut(sun, o_trans)
    ref, st = oracle.clouds(otex, p, sk, rect=(0, 0, tw, th), primary_steps=primary, light_steps=light, return_stats=True)
    try:
        for name, ctx in (("plain", plain), ("persistent", persistent)):
            ctx.set_march(primary, light)
            ctx.render_sky_lut(sun, 200, 100)
            d = ulp_diff(ctx.read_sky_lut(), sk)
            assert d.max() <= 1, (seed, name, d.max())
            img, stats = _host_frame(ctx, p, tw, th)
            ok, info = cloud_tight(img.view(np.float16), ref)
            assert ok, (seed, name, "host form", info)
            got = int(stats["incloud_samples"])
            assert abs(got - st["incloud_samples"]) <= 1e-3 * st["incloud_samples"] + 2, (seed, name, got, st["incloud_samples"])
            for k, f in enumerate(_device_frames(ctx, p, tw, th, 1, sun=sun, bands=(th, 0, 1, 1))):
                ok, info = cloud_tight(f.view(np.float16), ref)
                assert ok, (seed, name, "device form, pass %d" % k, info)
                assert np.array_equal(f, img), (seed, name, "device form against host form", k, int((f != img).sum()))
    finally:
        for ctx in (plain, persistent):
            ctx.set_march(128, 6)
