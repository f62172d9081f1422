"""Persistent launches read detail LODs 3 and 4 from LDS (cloud_kernels.hip::clouds_kernel_persistent stages the 72 cells once per launch,
cloud_core.h::sample_density_eager<true> taps them for light samples j = 3 and 4).  Same cell, same arithmetic: a persistent frame must be the plain
launch's frame byte for byte -- both TALLY forms, one frame at a time and two on two streams, with light-step counts at which the table is read twice,
once and never --, also on a detail volume whose small levels differ from cell to cell (the shipped one's are nearly flat), and after a rebind.
CSKY_PERSISTENT is read when a context is made: 2 = every whole-ray launch is persistent (as tests/test_gpu_round2.py forces it), 0 = never.

Mutation check (scratch builds of the kernel, MI355X): with y and z swapped in the LDS index and with the LOD-4 cells read one cell early,
test_wrong_cell_shows fails at its first persistent-against-plain comparison with 22 684 and 14 599 differing halfs of 131 072
(profiles/r19/small_detail_lds_ab.txt, section 8)."""
import os

import numpy as np
import pytest

from conftest import cloud_tight, norm
from test_hostsim_core import hs_clouds

pytestmark = pytest.mark.gpu

SUN = (1, 1, 0)
SIZES = [(256, 128), (200, 104)]                              # 128 footprints of 4 tiles; ragged in both directions (200 = 6 * 32 + 8, 104 = 13 * 8)
DETAIL_LOD3 = (2 ** 18 - 2 ** 9) // 7                         # cloud_core.h::detail_level_offset(3): first cell of LOD 3; LOD 4 starts 64 cells later


def _context(pkg, persistent, noise):
    old = os.environ.get("CSKY_PERSISTENT")
    os.environ["CSKY_PERSISTENT"] = str(persistent)
    try:
        ctx = pkg.Context(0)
    finally:
        if old is None:
            del os.environ["CSKY_PERSISTENT"]
        else:
            os.environ["CSKY_PERSISTENT"] = old
    ctx.set_noise(*noise)
    ctx.set_segments(1)                                       # whole rays: the only launches that have a persistent form
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(norm(SUN), 200, 100)
    return ctx


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


def _host_frame(ctx, p, tile_w=None, tile_h=None):
    """csky_render_clouds: a launch with a stats buffer (TALLY = true)"""
    img = ctx.render_clouds(p, tile_w, tile_h).view(np.uint16).copy()
    return img, ctx.cloud_stats()


def _device_frames(ctx, p, W, H, fif, sun=None, bands=None):
    """csky_render_clouds_device, no stats buffer (TALLY = false): every one of `fif` streams and output tensors twice, the second time over 0xFFFF halfs.
    `bands`: the rows to render (default: H rows as bands of 8); `sun`: the unit vector the context's sky LUT was rendered for (default: norm(SUN))."""
    import torch
    if bands is None:
        bands = (8, 0, 1, (H + 7) // 8)
    if sun is None:
        sun = norm(SUN)
    ctx.set_frames_in_flight(fif)
    streams = [torch.cuda.Stream() for _ in range(fif)]
    outs = [torch.zeros((bands[3] * bands[0], W, 4), dtype=torch.int16, device="cuda") for _ in range(fif)]
    torch.cuda.synchronize()
    frames = []
    try:
        for k in range(2 * fif):
            i = k % fif
            with torch.cuda.stream(streams[i]):
                if k >= fif:
                    frames.append(outs[i].cpu().numpy().copy())
                    outs[i].fill_(-1)
                ctx.render_sky_lut_device(sun, 200, 100, streams[i].cuda_stream)
                ctx.render_clouds_device(p, W, bands, outs[i].data_ptr(), W * 8, streams[i].cuda_stream)
        torch.cuda.synchronize()
    finally:
        ctx.set_frames_in_flight(1)
    return [f.view(np.uint16)[:H] for f in frames + [o.cpu().numpy() for o in outs]]


def _assert_persistent_equals_plain(plain, persistent, p, W, H, what):
    """-> the plain frame.  Host form (stats) and device form (no stats) of the persistent context, one frame and two frames in flight."""
    ref, st = _host_frame(plain, p)
    assert ref.any(), what
    dev_plain = _device_frames(plain, p, W, H, 1)[-1]
    assert np.array_equal(dev_plain, ref), (what, "plain launches disagree", int((dev_plain != ref).sum()))
    got, st_p = _host_frame(persistent, p)
    assert np.array_equal(got, ref), (what, "stats launch", int((got != ref).sum()))
    assert st_p == st, (what, st, st_p)
    for fif in (1, 2):
        for k, f in enumerate(_device_frames(persistent, p, W, H, fif)):
            assert np.array_equal(f, ref), (what, "no stats", fif, k, int((f != ref).sum()))
    return ref


@pytest.mark.parametrize("coverage", [0.2, 0.35])
@pytest.mark.parametrize("light_steps", [6, 5, 4, 3])        # j = 4 exists from five light steps, j = 3 from four: at 3 the table is staged and never read
@pytest.mark.parametrize("size", SIZES)
def test_persistent_equals_plain(plain, persistent, oracle, noise, size, light_steps, coverage):
    W, H = size
    p = oracle.default_params(W, H, SUN, coverage=coverage)
    for ctx in (plain, persistent):
        ctx.set_noise(*noise); ctx.set_march(128, light_steps)
    try:
        _assert_persistent_equals_plain(plain, persistent, p, W, H, (size, light_steps, coverage))
    finally:
        for ctx in (plain, persistent):
            ctx.set_march(128, 6)


def block_detail(seed):
    """A 32^3 RGB8 detail volume in which every 8^3-texel block holds one level from {0, 4, .., 28} in all channels: LOD 3 (one texel per block) and
    LOD 4 (means of eight of them) differ from texel to texel, and every cell coefficient stays an integer far below 2048 (exact in fp16)."""
    lv = (np.random.default_rng(seed).integers(0, 8, (4, 4, 4)) * 4).astype(np.uint8)
    vol = np.repeat(np.repeat(np.repeat(lv, 8, 0), 8, 1), 8, 2)
    return np.ascontiguousarray(np.repeat(vol[..., None], 3, 3))


def _small_cells(ctx):
    """the baked 16-byte cells of detail LOD 3 (64) and LOD 4 (8)"""
    cells = ctx.read_baked_texture(1).reshape(-1, 16)
    return cells[DETAIL_LOD3:DETAIL_LOD3 + 64], cells[DETAIL_LOD3 + 64:DETAIL_LOD3 + 72]


def test_wrong_cell_shows(plain, persistent, hostsim, pkg, oracle, noise):
    """The block volume: neighbouring LOD-3 and LOD-4 cells differ, so a swapped or shifted index in the LDS tap moves the frame.  Persistent against
    plain byte for byte, and against the host build of the cores (lock-step march, global path) within the gate of the GPU parity tests."""
    W, H = SIZES[0]
    large, _, weather = noise
    mine = (large, block_detail(19), weather)
    p = oracle.default_params(W, H, SUN, coverage=0.35)
    try:
        for ctx in (plain, persistent):
            ctx.set_noise(*mine); ctx.set_march(128, 6)
            assert ctx.noise_inexact_coeffs() == 0                # else the set marches on TexSet32, which has no persistent form
        l3, l4 = _small_cells(persistent)
        assert len(np.unique(l3, axis=0)) > 1 and len(np.unique(l4, axis=0)) > 1   # not all equal: a wrong cell is another value
        ref = _assert_persistent_equals_plain(plain, persistent, p, W, H, "block volume")
        shipped = plain
        shipped.set_noise(*noise)
        other, _ = _host_frame(shipped, p)
        print("values the block volume moves against the shipped one: %d of %d" % (int((other != ref).sum()), ref.size))
        assert (other != ref).any()                               # the volume is seen at all
        sky = plain.render_sky_lut(norm(SUN), 200, 100)          # the LUT the frames were marched with
        core, _ = hs_clouds(hostsim, pkg, mine, p, sky, W, (8, 0, 1, H // 8))
        ok, info = cloud_tight(ref.view(np.float16), core)
        print("persistent / plain frame against the host core:", info)
        assert ok, info
    finally:
        for ctx in (plain, persistent):
            ctx.set_noise(*noise)


def test_rebind_restages_the_table(pkg, persistent, oracle, noise):
    """The table is staged by every launch from the set that launch was given: after a rebind the next persistent frame is a fresh context's."""
    W, H = SIZES[1]
    large, _, weather = noise
    a, b = (large, block_detail(19), weather), (large, block_detail(23), weather)
    p = oracle.default_params(W, H, SUN, coverage=0.35)
    fresh = _context(pkg, 2, b)
    try:
        want = _device_frames(fresh, p, W, H, 1)[-1]
    finally:
        fresh.close()
    try:
        persistent.set_noise(*a)
        first = _device_frames(persistent, p, W, H, 1)[-1]
        persistent.set_noise(*b)
        assert persistent.noise_inexact_coeffs() == 0
        second = _device_frames(persistent, p, W, H, 1)[-1]
        assert (first != want).any()                               # the two volumes give different frames
        assert np.array_equal(second, want), int((second != want).sum())
        host, _ = _host_frame(persistent, p)
        assert np.array_equal(host, want), int((host != want).sum())
    finally:
        persistent.set_noise(*noise)
