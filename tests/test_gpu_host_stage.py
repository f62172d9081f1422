"""The blocking host forms share one staging buffer (csrc/host_stage.h, csky_ctx::stage): every feature's form uploads into it, launches into it and
copies out of it, one call after the other.  Each form is held to its _device form bit for bit by its own feature's tests; what is checked here is
what the sharing adds: forms of DIFFERENT features called on one context in an interleaved order, so that the bytes a call needs fall, rise and fall
again from call to call, while the buffer grows (first pass, on a context that has never seen these sizes) and once it has grown (second pass, in
another order).  Every result of the second pass must be the first pass's result of the same call, bit for bit."""
import numpy as np
import pytest

import clouds_rays_reference as RR
import shadow_reference as SR

pytestmark = pytest.mark.gpu

W, H = 33, 9                        # the frames: ragged against every tile size
BASIS = RR.camera_basis(RR.VIEW["pitch"], RR.VIEW["yaw"])
FOV = RR.VIEW["fov"]
RECT = dict(center=(0.0, 0.0), extent=(16384.0, 16384.0))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def halves(rng, shape, lo, hi):
    return rng.uniform(lo, hi, shape).astype(np.float16)


def test_forms_of_different_features_share_the_stage(pkg, noise, oracle):
    if pkg.lib().csky_device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible (libcloudsky has no CPU fallback)")
    rng = np.random.default_rng(7)
    p = SR.scene(oracle, "A")
    sun = np.asarray(p[16:19], np.float32)
    x, z = np.meshgrid(np.linspace(-0.7, 0.7, W), np.linspace(-0.5, 0.5, H))
    dirs = np.stack([x, np.sqrt(1.0 - x * x - z * z), z], axis=-1).astype(np.float32)       # unit directions above the horizon
    shadow_map = halves(rng, (32, 48), 0.0, 1.0)
    cloud = [halves(rng, (8, 16, 4), 0.0, 1.0) for _ in range(2)]
    sky = [halves(rng, (4, 8, 4), 0.0, 2.0) for _ in range(2)]
    cube = halves(rng, (6, 8, 8, 4), 0.0, 4.0)
    frame_in = halves(rng, (H, W, 4), 0.0, 1.0)                                             # apply_cloud_aerial's inputs: a frame, and
    depth_in = halves(rng, (H, W, 4), 0.5, 20.0)                                            # distances in km

    ctx = pkg.Context(0)                # a context of its own: its stage is empty, so the first pass is the growth path
    try:
        ctx.set_noise(*noise)
        ctx.set_march(30, 4)
        ctx.render_transmittance(256, 64)
        ctx.render_sky_lut(sun, 200, 100)
        # name -> (bytes of the stage the call needs: its regions, each begun on a 256-byte boundary; the call)
        calls = {
            "shadow": (1920, lambda: ctx.render_cloud_shadow(p, 40, 24, steps=16, **RECT)),
            "depth": (2376, lambda: ctx.render_cloud_depth(p, W, H, steps=17)),
            "composite": (3584, lambda: ctx.composite_sky(cloud[0], cloud[1], sky[0], sky[1], sun, blend_amount=0.25, out_w=16, out_h=8)),
            "view": (2376, lambda: ctx.render_clouds_view(p, BASIS, FOV, W, H)),
            "apply": (4936, lambda: ctx.apply_cloud_aerial(sun, frame_in, depth_in, steps=5)),
            "aerial": (3640, lambda: ctx.render_aerial_perspective(sun, 13, 7, 5, steps_per_slice=3)),
            "radiance": (8704, lambda: ctx.render_radiance(cloud[0], cloud[1], sky[0], sky[1], sun, blend_amount=0.25, face_size=8, layers=2)),
            "shadowed": (6712, lambda: ctx.render_aerial_perspective_shadowed(sun, shadow_map, RECT["center"], RECT["extent"], 13, 7, 5, steps_per_slice=3)),
            "dirs": (5960, lambda: ctx.render_clouds_dirs(p, dirs)),
            "prefilter": (6144, lambda: ctx.prefilter_cube(cube, layers=2)),
        }
        first_order = ["shadow", "depth", "composite", "view", "apply", "aerial", "radiance", "shadowed", "dirs", "prefilter"]
        second_order = ["prefilter", "shadow", "radiance", "view", "shadowed", "depth", "dirs", "composite", "apply", "aerial"]
        assert sorted(first_order) == sorted(second_order) == sorted(calls)
        for order in (first_order, second_order):
            need = [calls[k][0] for k in order]
            steps = np.sign(np.diff(need))
            # the bytes needed fall, rise and fall again (at least) along the order, and the first pass has to grow the stage more than once
            assert (steps[:-1] != steps[1:]).sum() >= 3, need
        assert sum(calls[k][0] > max(calls[j][0] for j in first_order[:i]) for i, k in enumerate(first_order) if i) >= 3

        first = {k: np.array(calls[k][1](), copy=True) for k in first_order}
        for k, a in first.items():
            assert np.isfinite(a.astype(np.float32)).all(), k
            print("%s: %.1f %% of the halves are not zero" % (k, 100.0 * (bits(a) != 0).mean()))
            assert (bits(a) != 0).any(), "%s: the result is empty, equality would say nothing" % k
        second = {k: np.array(calls[k][1](), copy=True) for k in second_order}
        for k in first_order:
            differ = int((bits(first[k]) != bits(second[k])).sum())
            print("%s: %d of %d halves differ between the passes" % (k, differ, first[k].size))
            assert first[k].shape == second[k].shape and differ == 0, k
        assert (bits(first["prefilter"][0]) == bits(cube)).all()                             # layer 0 is the input
    finally:
        ctx.close()
