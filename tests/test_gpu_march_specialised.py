"""Persistent launches run a march compiled for the bound weather map's cloud-type mode (cloud_kernels.hip clouds_kernel_persistent<3, TALLY, CT>:
CT = 1 every cloud-type texel >= 128, 2 every texel <= 127, 0 the generic form that reads FrameConsts::ct_mode) and, in the two specialised forms, a
light march with one copy of its body per sample index (light_samples_from).  Same expressions in the same order: for an all-high, an all-low and a mixed
weather map a persistent frame must be the plain launch's frame byte for byte with equal stats -- host form (tally) and device form (no tally), one and two
frames in flight, 0..6 light steps (every exit of the straight-line march) -- and so must the frame with csky_set_height_window(0), which every form marches
generically.  A rebind from the all-high to the all-low map must give a fresh context's frame: the instantiation follows the bound map.

Mutation check (scratch builds of the kernel, MI355X; profiles/r22/march_specialised_ab.txt): with the all-high launch wired to the mode-2 kernel, and
with light sample j = 4 given j = 3's levels, test_forms_agree fails."""
import numpy as np
import pytest

from test_gpu_small_detail_lds import SUN, _context, _device_frames, _host_frame

pytestmark = pytest.mark.gpu

SIZES = [(128, 64), (256, 128), (200, 104)]                   # 32 and 128 footprints of 4 tiles; ragged in both directions (200 = 6 * 32 + 8, 104 = 13 * 8)
LIGHT_STEPS = [0, 1, 3, 4, 6]                                 # no cone sample; the first exit; the last global tap; the first table tap; all six
MAPS = ["high", "low", "mixed"]


def weather_map(noise, kind):
    """the shipped map (R in 151..231: mode 1), the `stratus` map of tests/test_gpu_noise_rebind.py (R halved: mode 2), and one whose R spans 127 / 128 (mode 0)"""
    w = noise[2].copy()
    if kind == "low":
        w[..., 0] //= 2; w[..., 2] = np.minimum(w[..., 2], 200)
        assert w[..., 0].max() <= 127
    elif kind == "mixed":
        w[..., 0] -= 64
        assert w[..., 0].min() <= 127 and w[..., 0].max() >= 128 and noise[2][..., 0].min() >= 64
    else:
        assert w[..., 0].min() >= 128
    return w


@pytest.fixture(scope="module", params=MAPS)
def forms(request, pkg, noise):
    """(map kind, its noise set, a context that never launches persistently, one that always does)"""
    mine = (noise[0], noise[1], weather_map(noise, request.param))
    plain, persistent = _context(pkg, 0, mine), _context(pkg, 2, mine)
    yield request.param, mine, plain, persistent
    plain.close(); persistent.close()


@pytest.mark.parametrize("coverage", [0.2, 0.6])
@pytest.mark.parametrize("light_steps", LIGHT_STEPS)
@pytest.mark.parametrize("size", SIZES)
def test_forms_agree(forms, oracle, size, light_steps, coverage):
    kind, _, plain, persistent = forms
    W, H = size
    what = (kind, size, light_steps, coverage)
    p = oracle.default_params(W, H, SUN, coverage=coverage)
    try:
        for ctx in (plain, persistent):
            ctx.set_march(128, light_steps)
        ref, st = _host_frame(plain, p)
        assert ref.any() and st["incloud_samples"] > 0, what
        frames = [("plain, no tally", _device_frames(plain, p, W, H, 1)[-1], None)]
        got, st_p = _host_frame(persistent, p)
        frames.append(("persistent, tally", got, st_p))
        for fif in (1, 2):
            frames += [("persistent, no tally, %d in flight, frame %d" % (fif, k), f, None) for k, f in enumerate(_device_frames(persistent, p, W, H, fif))]
        for ctx, name in ((plain, "plain"), (persistent, "persistent")):
            ctx.set_height_window(0)                              # nothing rejected, nothing specialised: the generic march
            got, st_g = _host_frame(ctx, p)
            frames.append((name + ", window off, tally", got, st_g))
            frames.append((name + ", window off, no tally", _device_frames(ctx, p, W, H, 1)[-1], None))
            ctx.set_height_window(1)
        for name, f, s in frames:
            assert np.array_equal(f, ref), (what, name, int((f != ref).sum()))
            assert s is None or s == st, (what, name, st, s)
    finally:
        for ctx in (plain, persistent):
            ctx.set_height_window(1); ctx.set_march(128, 6)


def test_instantiation_follows_the_bound_map(pkg, oracle, noise):
    """all-high -> all-low on one persistent context: the second frame is a fresh all-low context's, and back again"""
    W, H = SIZES[2]
    p = oracle.default_params(W, H, SUN, coverage=0.6)
    high, low = (noise[0], noise[1], weather_map(noise, "high")), (noise[0], noise[1], weather_map(noise, "low"))
    want = {}
    for kind, mine in (("high", high), ("low", low)):
        fresh = _context(pkg, 2, mine)
        try:
            want[kind] = (_device_frames(fresh, p, W, H, 1)[-1], _host_frame(fresh, p))
        finally:
            fresh.close()
    assert (want["high"][0] != want["low"][0]).any()
    ctx = _context(pkg, 2, high)
    try:
        for kind, mine in (("high", high), ("low", low), ("high", high)):
            ctx.set_noise(*mine)
            dev = _device_frames(ctx, p, W, H, 2)
            host, st = _host_frame(ctx, p)
            for f in dev + [host]:
                assert np.array_equal(f, want[kind][0]), (kind, int((f != want[kind][0]).sum()))
            assert np.array_equal(host, want[kind][1][0]) and st == want[kind][1][1], (kind, st, want[kind][1][1])
    finally:
        ctx.close()
