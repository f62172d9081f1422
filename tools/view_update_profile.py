"""The timing run of the temporal split of a view frame (raw output: profiles/r26/view_update.txt).

    python tools/view_update_profile.py
One process.  The C3 parameters (128 x 6 steps, sun (1, 1, 0), the default block).  csky_set_kernel_timing's events around every call (one pair
around both launches of an update), one call at a time on one stream.  The view: 1920 x 1080, fov 70, pitched up 20 degrees, B = 4, the phases in
the ordered-dither order.  Groups of 3 + 32 calls in the order full view march (csky_render_clouds_view, the kernel the parent commit has), still
camera, camera yawing 1 degree per call, yawing, still, full, so that a drifting clock shows.  Each update is fed the frame of the call before.  The
shares of holes, tapped and fresh pixels are the numpy restatement's (tests/view_update_reference.py) for the same cameras."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VW, VH, FOV, PITCH, BLOCK = 1920, 1080, 70.0, 20.0, 4
STEPS, LIGHT = 128, 6
GROUP_WARM, GROUP = 3, 32
YAW_STEP = 1.0


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import clouds_rays_reference as RR
    import gvcd_amd
    import view_update_reference as VU
    from view_march_profile import c3_params

    ctx = gvcd_amd.Context(0)
    ctx.set_noise(*gvcd_amd.assets.load_default_noise())
    ctx.set_march(STEPS, LIGHT)
    p = c3_params(2048, 1024)
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(p[16:19], 200, 100)
    print("library %s" % gvcd_amd.library_path(), flush=True)
    phases = VU.bayer_phases(BLOCK)
    for name, yaw in (("still", 0.0), ("yawing %g degree per call" % YAW_STEP, YAW_STEP)):
        k = VU.classify(RR.camera_basis(PITCH, yaw), FOV, RR.camera_basis(PITCH, 0.0), FOV, VW, VH, BLOCK, phases[1])["kind"]
        print("%s, reference: holes %.2f %%, tapped %.2f %%, copied %.2f %%, fresh %.2f %%, not accepted %.2f %% of %d pixels" % (
            name, *[100.0 * (k == v).mean() for v in (VU.HOLE, VU.TAP, VU.COPY, VU.FRESH, VU.ZERO)], VW * VH), flush=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        frames = [torch.zeros((VH, VW, 4), dtype=torch.float16, device="cuda") for _ in range(2)]
        s.synchronize()
        state = {"calls": 0, "yaw": 0.0, "prev": None}

        def full():
            ctx.render_clouds_view(p, RR.camera_basis(PITCH, state["yaw"]), FOV, VW, VH, out=frames[state["calls"] % 2], stream=s.cuda_stream)

        def update(step):
            def call():
                n = state["calls"]
                basis = RR.camera_basis(PITCH, state["yaw"] + step)
                prev = state["prev"]
                ctx.render_clouds_view_update(p, basis, FOV, VW, VH, BLOCK, phases[n % len(phases)], prev=None if prev is None else frames[(n + 1) % 2],
                                              prev_basis=None if prev is None else prev, prev_fov=FOV, out=frames[n % 2], stream=s.cuda_stream)
                state["calls"], state["yaw"], state["prev"] = n + 1, state["yaw"] + step, basis
            return call

        def timed(label, n_warm, n, call):
            for _ in range(n_warm):
                call()
                s.synchronize()                              # one call at a time
            ctx.set_kernel_timing(True)
            ctx.kernel_ms()
            each = []
            for _ in range(n):
                call()
                s.synchronize()
                ms, launches = ctx.kernel_ms()
                assert launches == 1
                each.append(ms)
            ctx.set_kernel_timing(False)
            each.sort()
            print("%s: kernels %.4f ms mean of %d (min %.4f, median %.4f, max %.4f)" % (label, sum(each) / n, n, each[0], each[n // 2], each[-1]), flush=True)

        update(0.0)()                                          # the first call has no history: a full frame
        s.synchronize()
        for label, call in (("full view march", full), ("update, still camera", update(0.0)), ("update, yawing", update(YAW_STEP)), ("update, yawing", update(YAW_STEP)),
                            ("update, still camera", update(0.0)), ("full view march", full)):
            timed("%d x %d, fov %g, pitched up %g, B = %d: %s" % (VW, VH, FOV, PITCH, BLOCK, label), GROUP_WARM, GROUP, call)
        want = torch.empty((VH, VW, 4), dtype=torch.float16, device="cuda")
        ctx.render_clouds_view(p, RR.camera_basis(PITCH, state["yaw"]), FOV, VW, VH, out=want, stream=s.cuda_stream)
        s.synchronize()
        v = want.cpu().numpy()
        print("view frame: alpha > 0 on %.1f %% of the pixels, %.1f %% of them zero texels" % (100.0 * (v[..., 3] > 0).mean(), 100.0 * (~v.view(np.uint16).any(-1)).mean()))
    ctx.close()


if __name__ == "__main__":
    main()
