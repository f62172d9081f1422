"""The specialised persistent forms without a tally (cloud_kernels.hip clouds_kernel_persistent<3, false, 1 | 2>) run eight workgroups per CU on a queue
without two of its arrays (march_compact<.., SLIM = true>): a replayed step's first slot is counted up from the masks of the steps before it instead of
read from st_base, and a sample queued at slot >= 64 has its height fraction recomputed from its position when it is carried to the front instead of
read from ev_hf.  Same samples, same order, same flushes, same bits: a persistent frame must be the plain launch's frame byte for byte -- for an all-high, an
all-low and a mixed weather map (the forms CT = 1, 2 and the generic one), the height window on and off, both tally forms, 0, 1, 3 and 6 light steps, one and
two frames in flight, and after a rebind between the maps.

Queue stress: two scenes that drive the changed code to its ends, found with the tile walk of tests/tilewalk instrumented to print the largest `count` and
`cs` of any flush (a scratch copy; 128 x 64, on the shipped, the all-low and the mixed map):
  * coverage 0.8, density 5, 16 primary steps: a step queues close to 64 samples on top of a carry; count reaches 123 (all-low and mixed: 127) of
    CQ_CAP = 128, so the carried tail is up to 63 samples long and every one of them gets a recomputed height fraction;
  * the table's 1024 x 3 scene: long runs of steps with one sample each; cs reaches 64 of CQ_STEPS = 66 and count 127 on the shipped and the mixed map,
    so the derived base is a sum over 63 masks.  On the all-low map it stops at cs = 58; there the same march at coverage 0.6 reaches cs = 64 and
    count 126, so that scene runs too.

Mutation check (scratch builds of the kernel, MI355X; profiles/r30/occupancy8_ab.txt): with the derived base one step behind, and with the carried
sample's height fraction computed from its neighbour's position, this file fails."""
import numpy as np
import pytest

import saturation_scenes as S
from test_gpu_march_specialised import MAPS, SIZES, weather_map
from test_gpu_small_detail_lds import SUN, _context, _device_frames, _host_frame

pytestmark = pytest.mark.gpu

LIGHT_STEPS = [0, 1, 3, 6]
STRESS = [S.scene("dense-16x6", 0, size=(128, 64), coverage=0.8, density=5.0, primary=16, light=6),
          next(sc for sc in S.TABLE if sc.name == "1024x3"),
          S.scene("1024x3-cov-0.6", 0, size=(128, 64), coverage=0.6, primary=1024, light=3)]


@pytest.fixture(scope="module", params=MAPS)
def forms(request, pkg, noise):
    """(map kind, a context that never launches persistently, one that always does)"""
    mine = (noise[0], noise[1], weather_map(noise, request.param))
    plain, persistent = _context(pkg, 0, mine), _context(pkg, 2, mine)
    yield request.param, plain, persistent
    plain.close(); persistent.close()


def _agree(plain, persistent, p, W, H, what):
    """persistent against plain: the host form (tally) with its stats, the device form (no tally) with one and two frames in flight"""
    ref, st = _host_frame(plain, p)
    frames = [("plain, no tally", _device_frames(plain, p, W, H, 1)[-1], None)]
    got, st_p = _host_frame(persistent, p)
    frames.append(("persistent, tally", got, st_p))
    for fif in (1, 2):
        frames += [("persistent, no tally, %d in flight, frame %d" % (fif, k), f, None) for k, f in enumerate(_device_frames(persistent, p, W, H, fif))]
    for name, f, s in frames:
        assert np.array_equal(f, ref), (what, name, int((f != ref).sum()))
        assert s is None or s == st, (what, name, st, s)
    return ref, st


@pytest.mark.parametrize("window", [1, 0])
@pytest.mark.parametrize("light_steps", LIGHT_STEPS)
@pytest.mark.parametrize("size", SIZES)
def test_persistent_equals_plain(forms, oracle, size, light_steps, window):
    kind, plain, persistent = forms
    W, H = size
    p = oracle.default_params(W, H, SUN, coverage=0.6)
    try:
        for ctx in (plain, persistent):
            ctx.set_march(128, light_steps); ctx.set_height_window(window)
        ref, st = _agree(plain, persistent, p, W, H, (kind, size, light_steps, window))
        assert ref.any() and st["incloud_samples"] > 0
    finally:
        for ctx in (plain, persistent):
            ctx.set_height_window(1); ctx.set_march(128, 6)


@pytest.mark.parametrize("sc", STRESS, ids=lambda s: s.name)
def test_queue_stress(forms, oracle, sc):
    kind, plain, persistent = forms
    W, H = sc.size
    p = S.params(oracle, sc)
    try:
        for ctx in (plain, persistent):
            ctx.set_march(sc.primary, sc.light)
        ref, st = _agree(plain, persistent, p, W, H, (kind, sc.name))
        assert ref.any() and st["incloud_samples"] > 0
    finally:
        for ctx in (plain, persistent):
            ctx.set_march(128, 6)


def test_rebind_between_maps(pkg, oracle, noise):
    """one persistent context taken through high -> low -> mixed -> high: every frame is the one a plain context of that map renders"""
    W, H = SIZES[2]
    p = oracle.default_params(W, H, SUN, coverage=0.6)
    sets = {kind: (noise[0], noise[1], weather_map(noise, kind)) for kind in MAPS}
    want = {}
    for kind in MAPS:
        plain = _context(pkg, 0, sets[kind])
        try:
            want[kind] = _host_frame(plain, p)
        finally:
            plain.close()
    assert (want["high"][0] != want["low"][0]).any() and (want["high"][0] != want["mixed"][0]).any()
    ctx = _context(pkg, 2, sets["high"])
    try:
        for kind in ("high", "low", "mixed", "high"):
            ctx.set_noise(*sets[kind])
            for f in _device_frames(ctx, p, W, H, 2):
                assert np.array_equal(f, want[kind][0]), (kind, int((f != want[kind][0]).sum()))
            host, st = _host_frame(ctx, p)
            assert np.array_equal(host, want[kind][0]) and st == want[kind][1], (kind, st, want[kind][1])
    finally:
        ctx.close()
