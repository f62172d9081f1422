"""The saturation skip on the GPU (march_compact.h march_compact; cloud_core.h ray_saturated): csky_set_height_window(1) against (0), which switches
the exact specialisations -- this one included -- off.  Frames must be equal array for array and the sample tallies equal."""
import numpy as np
import pytest

from conftest import norm

pytestmark = pytest.mark.gpu

W, H = 2048, 1024
SUN = (1, 1, 0)


def _pair(ctx, render):
    ctx.set_height_window(1)
    a = render()
    ctx.set_height_window(0)
    try:
        b = render()
    finally:
        ctx.set_height_window(1)
    return a, b


@pytest.mark.parametrize("coverage", [0.2, 0.35, 0.8])
def test_whole_frames_equal_with_and_without_the_skip(gpu_ctx, oracle, coverage):
    gpu_ctx.set_march(128, 6); gpu_ctx.set_segments(0); gpu_ctx.set_schedule(-1); gpu_ctx.set_frames_in_flight(1)
    gpu_ctx.render_sky_lut(norm(SUN), 200, 100)
    p = oracle.default_params(W, H, SUN, coverage=coverage)

    def render():
        img = gpu_ctx.render_clouds(p).view(np.int16).copy()
        return img, gpu_ctx.cloud_stats()
    (a, sa), (b, sb) = _pair(gpu_ctx, render)
    assert a.any() and sa["incloud_samples"] > 0
    assert np.array_equal(a, b), (coverage, int((a != b).sum()))
    assert sa["incloud_samples"] == sb["incloud_samples"] and sa["primary_samples"] == sb["primary_samples"], (coverage, sa, sb)


@pytest.mark.parametrize("coverage", [0.2, 0.35, 0.8])
def test_persistent_form_two_frames_in_flight(pkg, noise, oracle, coverage):
    """A whole 2048 x 1024 frame is 32 Ki wavefronts: with two frames in flight the policy launches it in the persistent form (launch_policy.h)."""
    import torch
    p = oracle.default_params(W, H, SUN, coverage=coverage)
    bands = (8, 0, 1, H // 8)
    ctx = pkg.Context(0)
    try:
        ctx.set_noise(*noise); ctx.set_march(128, 6)
        ctx.render_transmittance(256, 64)
        ctx.render_sky_lut(norm(SUN), 200, 100)
        ctx.set_frames_in_flight(2)
        streams = [torch.cuda.Stream() for _ in range(2)]
        outs = [torch.zeros((H, W, 4), dtype=torch.int16, device="cuda") for _ in range(2)]

        def render():
            frames = []
            torch.cuda.synchronize()
            for k in range(4):                                                 # both ring slots, two frames in flight
                i = k & 1
                if k >= 2:
                    streams[i].synchronize()
                    frames.append(outs[i].cpu().numpy().copy())
                    outs[i].zero_()
                    torch.cuda.current_stream().synchronize()
                ctx.render_sky_lut_device(norm(SUN), 200, 100, streams[i].cuda_stream)
                ctx.render_clouds_device(p, W, bands, outs[i].data_ptr(), W * 8, streams[i].cuda_stream)
            torch.cuda.synchronize()
            frames += [outs[0].cpu().numpy().copy(), outs[1].cpu().numpy().copy()]
            _, st = ctx.time_clouds(p, W, bands, warmup=1, iters=2)
            return frames, st
        (fa, sa), (fb, sb) = _pair(ctx, render)
        assert fa[0].any()
        for k, (a, b) in enumerate(zip(fa, fb)):
            assert np.array_equal(a, b), (coverage, k, int((a != b).sum()))
            assert np.array_equal(a, fa[0]), (coverage, k)
        assert sa["incloud_samples"] == sb["incloud_samples"] and sa["primary_samples"] == sb["primary_samples"], (coverage, sa, sb)
    finally:
        ctx.close()


@pytest.mark.parametrize("coverage", [0.2, 0.35, 0.8])
def test_one_eighth_band_share_equals_its_own_unskipped_render(gpu_ctx, oracle, coverage):
    """One rank's 1/8 share of the frame (bands 3, 11, ...), whichever launch form the policy picks for it."""
    import torch
    gpu_ctx.set_march(128, 6); gpu_ctx.set_segments(0); gpu_ctx.set_schedule(-1); gpu_ctx.set_frames_in_flight(1)
    p = oracle.default_params(W, H, SUN, coverage=coverage)
    bands = (8, 3, 8, H // 8 // 8)
    rows = bands[3] * 8
    s0 = torch.cuda.Stream()

    def render():
        o = torch.zeros((rows, W, 4), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.render_sky_lut_device(norm(SUN), 200, 100, s0.cuda_stream)
        gpu_ctx.render_clouds_device(p, W, bands, o.data_ptr(), W * 8, s0.cuda_stream)
        s0.synchronize()
        _, st = gpu_ctx.time_clouds(p, W, bands, warmup=0, iters=1)
        return o.cpu().numpy().copy(), st
    (a, sa), (b, sb) = _pair(gpu_ctx, render)
    assert a.any()
    assert np.array_equal(a, b), (coverage, int((a != b).sum()))
    assert sa["incloud_samples"] == sb["incloud_samples"] and sa["primary_samples"] == sb["primary_samples"], (coverage, sa, sb)
