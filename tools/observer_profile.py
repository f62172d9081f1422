"""The timing run of the direct cloud march from an observer's position (raw output: profiles/r28/observer.txt).

    python tools/observer_profile.py
One process, in the manner of tools/view_march_profile.py, whose parameters and view it takes: the C3 block (128 x 6 steps, sun (1, 1, 0)), the
1920 x 1080 view of fov 70 pitched up 20 degrees.  csky_set_kernel_timing's events around every launch, one call at a time on one stream: 20
warm-up hemisphere frames, then groups of 3 + 20 launches in the order

    view (clouds_rays_kernel), view from `ground` (clouds_observer_kernel), view from `ground`, view

so that a drifting clock shows: the same rays through both kernels, and the difference is what the observer kernel pays for ending a wavefront on
"no lane is live" instead of "every lane is above the window".  Then `above_down` (8 000 m up, pitched down 30 degrees) and `inside` (2 750 m up,
level, capped at 20 000 m) at the same size and field of view."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from view_march_profile import FOV, GROUP, GROUP_WARM, LIGHT, PITCH, STEPS, VH, VW, H, W, basis, c3_params  # noqa: E402

INF = float("inf")


def main():
    sys.path.insert(0, ROOT)
    import torch

    import gvcd_amd
    ctx = gvcd_amd.Context(0)
    ctx.set_noise(*gvcd_amd.assets.load_default_noise())
    ctx.set_march(STEPS, LIGHT)
    p = c3_params(W, H)
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(p[16:19], 200, 100)
    print("library %s" % gvcd_amd.library_path(), flush=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        frame = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
        view = torch.empty((VH, VW, 4), dtype=torch.float16, device="cuda")
        other = torch.empty((VH, VW, 4), dtype=torch.float16, device="cuda")
        s.synchronize()

        def hemisphere():
            ctx.render_clouds_device(p, W, (8, 0, 1, H // 8), frame.data_ptr(), W * 8, s.cuda_stream)

        def direct():
            ctx.render_clouds_view(p, basis(PITCH), FOV, VW, VH, out=view, stream=s.cuda_stream)

        def observer(pitch, position, cap):
            return lambda: ctx.render_clouds_view_from(p, basis(pitch), FOV, VW, VH, position, cap, out=other, stream=s.cuda_stream)

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
            mean = sum(each) / len(each)
            print("%s: kernel %.4f ms mean of %d (min %.4f, max %.4f)" % (label, mean, n, min(each), max(each)), flush=True)
            return mean

        def shares(label, t):
            v = t.cpu().numpy()
            print("%s: alpha > 0 on %.1f %% of the pixels, %.1f %% of them zero texels" % (label, 100.0 * (v[..., 3] > 0).mean(), 100.0 * (~v.view(np.uint16).any(-1)).mean()), flush=True)

        timed("hemisphere 2048 x 1024, warm-up", 0, 20, hemisphere)
        ground = observer(PITCH, (0.0, 0.0, 0.0), INF)
        ms = {"rays": [], "ground": []}
        for kind, call in (("rays", direct), ("ground", ground), ("ground", ground), ("rays", direct)):
            ms[kind].append(timed("view 1920 x 1080, fov 70, pitched up 20, %s" % ("clouds_rays_kernel" if kind == "rays" else "clouds_observer_kernel at `ground`"),
                                  GROUP_WARM, GROUP, call))
        a, b = sum(ms["rays"]) / 2, sum(ms["ground"]) / 2
        print("the same rays: clouds_rays_kernel %.4f ms, clouds_observer_kernel %.4f ms, %+.2f %%" % (a, b, 100.0 * (b / a - 1.0)), flush=True)
        assert (view.cpu().numpy().view(np.uint16) == other.cpu().numpy().view(np.uint16)).all()
        shares("that view", view)
        for label, pitch, pos, cap in (("above_down: 8000 m up, pitched down 30", -30.0, (0.0, 8000.0, 0.0), INF), ("inside: 2750 m up, level, capped at 20000 m", 0.0, (0.0, 2750.0, 0.0), 20000.0)):
            timed("view 1920 x 1080, fov 70, %s" % label, GROUP_WARM, GROUP, observer(pitch, pos, cap))
            shares(label, other)
    ctx.close()


if __name__ == "__main__":
    main()
