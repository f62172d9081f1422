"""Launches that deliver no in-cloud count stop marching a ray whose stored pixel is final (march_compact.h march_compact, TALLY = false): the C3-size
frame through csky_render_clouds_device, which passes no stats buffer, against the same frame through a stats launch (TALLY = true, the march as it was).
Frames must be equal array for array, and the stats launch's in-cloud count the full march's: the figure the kernel delivered before the change
(measured with the parent commit's library on an MI355X: profiles/r12/counts_parent_and_change.txt; the CPU walk of tests/tilewalk counts 6 and 7 samples
fewer, 40 799 429 and 77 038 436: samples whose density the device's exp2 / log2 put on the other side of zero)."""
import numpy as np
import pytest

from conftest import norm

pytestmark = pytest.mark.gpu

W, H = 2048, 1024
SUN = (1, 1, 0)
INCLOUD = {0.2: 40799435, 0.35: 77038443}     # 2048 x 1024, 128 x 6 steps: in-cloud samples of the full march


def _stats_frame(ctx, p):
    """the host form: a launch with the stats buffer, one frame at a time (the plain kernel)"""
    ctx.set_frames_in_flight(1)
    img = ctx.render_clouds(p).view(np.int16).copy()
    return img, ctx.cloud_stats()


def _device_frames(ctx, p, fif):
    """csky_render_clouds_device, no stats buffer: fif = 1 launches the plain kernel, fif = 2 the persistent form (a whole frame is 32 Ki wavefronts)"""
    import torch
    bands = (8, 0, 1, H // 8)
    ctx.set_frames_in_flight(fif)
    streams = [torch.cuda.Stream() for _ in range(fif)]
    outs = [torch.zeros((H, W, 4), dtype=torch.int16, device="cuda") for _ in range(fif)]
    torch.cuda.synchronize()
    frames = []
    for k in range(2 * fif):                                                       # every stream and output tensor twice
        i = k % fif
        with torch.cuda.stream(streams[i]):
            if k >= fif:
                # the second pass must not be masked by the first, which left the right answer in the tensor: keep the first pass's frame, then every half
                # becomes 0xFFFF, a NaN no frame holds, on the launch's own stream
                frames.append(outs[i].cpu().numpy().copy())
                outs[i].fill_(-1)
            ctx.render_sky_lut_device(norm(SUN), 200, 100, streams[i].cuda_stream)
            ctx.render_clouds_device(p, W, bands, outs[i].data_ptr(), W * 8, streams[i].cuda_stream)
    torch.cuda.synchronize()
    return frames + [o.cpu().numpy().copy() for o in outs]


@pytest.mark.parametrize("coverage", [0.2, 0.35])
def test_frames_without_stats_equal_the_stats_launch(pkg, noise, oracle, coverage):
    p = oracle.default_params(W, H, SUN, coverage=coverage)
    ctx = pkg.Context(0)
    try:
        ctx.set_noise(*noise); ctx.set_march(128, 6)
        ctx.render_transmittance(256, 64)
        ctx.render_sky_lut(norm(SUN), 200, 100)
        ref, st = _stats_frame(ctx, p)
        assert ref.any()
        print("coverage %g: in-cloud samples of the stats launch %d" % (coverage, st["incloud_samples"]))
        assert st["incloud_samples"] == INCLOUD[coverage], (coverage, st)
        for fif in (1, 2):
            for k, f in enumerate(_device_frames(ctx, p, fif)):
                assert np.array_equal(f, ref), (coverage, fif, k, int((f != ref).sum()))
        # csky_time_clouds: its first launch counts, its timed launches do not; the counts stay the full march's in the persistent form too
        _, st2 = ctx.time_clouds(p, W, (8, 0, 1, H // 8), warmup=1, iters=2)
        assert st2["incloud_samples"] == INCLOUD[coverage] and st2["primary_samples"] == st["primary_samples"], (coverage, st, st2)
        ref2, st3 = _stats_frame(ctx, p)                                            # and the stats launch after them is what it was
        assert np.array_equal(ref2, ref) and st3 == st, (coverage, st, st3)
    finally:
        ctx.close()


def test_multi_frame_equals_the_stats_launch(pkg, noise, oracle, gpu_ctx):
    """One csky_multi frame (two contexts, each a half of the bands, in-place stores, no stats buffer) against the single context's stats launch."""
    import torch
    p = oracle.default_params(W, H, SUN)
    gpu_ctx.set_march(128, 6); gpu_ctx.set_segments(0); gpu_ctx.set_schedule(-1)
    gpu_ctx.render_sky_lut(norm(SUN), 200, 100)
    ref, st = _stats_frame(gpu_ctx, p)
    assert st["incloud_samples"] == INCLOUD[0.2], st
    m = pkg.MultiContext([0, 0])
    try:
        m.set_noise(*noise); m.set_march(128, 6)
        out = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        m.render_sky_lut(norm(SUN))
        m.render_clouds_device(p, W, H, out.data_ptr(), W * 8, s.cuda_stream)
        m.sync(); torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got, ref), int((got != ref).sum())
        host = m.render_clouds(p).view(np.int16)
        assert np.array_equal(host, ref), int((host != ref).sum())
    finally:
        m.close()
