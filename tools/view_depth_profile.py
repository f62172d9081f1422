"""The timing run of the depth frame and the aerial step for view frames (raw output: profiles/r24/view_depth.txt).

    python tools/view_depth_profile.py
One process.  The C3 parameters (128 x 6 steps, sun (1, 1, 0), the default block), tools/view_march_profile.py's view: 1920 x 1080, fov 70, pitched up
20 degrees.  HIP events through torch around every launch of a device form, one launch at a time on one stream: 20 warm-up hemisphere depth frames
(2048 x 1024), then groups of 3 + 20 launches in the order hemisphere depth, view march, view depth, view aerial, view depth, view aerial, view march,
hemisphere depth, hemisphere aerial, so that a drifting clock shows.  The view march (csky_render_clouds_view_device) and the hemisphere depth frame
(csky_render_cloud_depth_device) are what the two new launches are read against."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from view_march_profile import FOV, GROUP, GROUP_WARM, H, LIGHT, PITCH, STEPS, VH, VW, W, basis, c3_params  # noqa: E402

AERIAL_STEPS = 16


def main():
    sys.path.insert(0, ROOT)
    import torch

    import gvcd_amd
    ctx = gvcd_amd.Context(0)
    ctx.set_noise(*gvcd_amd.assets.load_default_noise())
    ctx.set_march(STEPS, LIGHT)
    p = c3_params(W, H)
    sun = p[16:19]
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(sun, 200, 100)
    print("library %s" % gvcd_amd.library_path(), flush=True)
    b = basis(PITCH)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        hemi = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
        hemi_z = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
        hemi_air = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
        view = torch.empty((VH, VW, 4), dtype=torch.float16, device="cuda")
        view_z = torch.empty((VH, VW, 4), dtype=torch.float16, device="cuda")
        view_air = torch.empty((VH, VW, 4), dtype=torch.float16, device="cuda")
        s.synchronize()
        st = s.cuda_stream
        ctx.render_clouds_device(p, W, (8, 0, 1, H // 8), hemi.data_ptr(), W * 8, st)   # the frames the aerial launches read
        ctx.render_clouds_view(p, b, FOV, VW, VH, out=view, stream=st)
        ctx.render_cloud_depth(p, W, H, out=hemi_z, stream=st)
        ctx.render_cloud_depth_view(p, b, FOV, VW, VH, out=view_z, stream=st)
        s.synchronize()

        calls = {
            "hemisphere depth 2048 x 1024": (W * H, lambda: ctx.render_cloud_depth(p, W, H, out=hemi_z, stream=st)),
            "hemisphere aerial 2048 x 1024, n = 16": (W * H, lambda: ctx.apply_cloud_aerial(sun, hemi, hemi_z, AERIAL_STEPS, out=hemi_air, stream=st)),
            "view march 1920 x 1080": (VW * VH, lambda: ctx.render_clouds_view(p, b, FOV, VW, VH, out=view, stream=st)),
            "view depth 1920 x 1080": (VW * VH, lambda: ctx.render_cloud_depth_view(p, b, FOV, VW, VH, out=view_z, stream=st)),
            "view aerial 1920 x 1080, n = 16": (VW * VH, lambda: ctx.apply_cloud_aerial_view(sun, b, FOV, view, view_z, AERIAL_STEPS, out=view_air, stream=st)),
        }

        def timed(label, n_warm, n):
            rays, call = calls[label]
            for _ in range(n_warm):
                call()
                s.synchronize()                              # one launch at a time
            each = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                call()
                e1.record(s)
                s.synchronize()
                each.append(e0.elapsed_time(e1))
            mean = sum(each) / len(each)
            print("%s: %.4f ms mean of %d between HIP events (min %.4f, max %.4f), %.1f Mrays/s over the image's %d rays"
                  % (label, mean, n, min(each), max(each), rays / mean / 1e3, rays), flush=True)

        timed("hemisphere depth 2048 x 1024", 20, 1)
        for label in ("hemisphere depth 2048 x 1024", "view march 1920 x 1080", "view depth 1920 x 1080", "view aerial 1920 x 1080, n = 16", "view depth 1920 x 1080",
                      "view aerial 1920 x 1080, n = 16", "view march 1920 x 1080", "hemisphere depth 2048 x 1024", "hemisphere aerial 2048 x 1024, n = 16"):
            timed(label, GROUP_WARM, GROUP)
        v, z, a = view.cpu().numpy(), view_z.cpu().numpy(), view_air.cpu().numpy()
        hz = hemi_z.cpu().numpy()
        print("view frame: alpha > 0 on %.1f %% of the pixels; view depth frame: not zero on %.1f %%; aerial step moved %.1f %% of the texels"
              % (100.0 * (v[..., 3] > 0).mean(), 100.0 * z.view(np.uint16).any(-1).mean(), 100.0 * (a.view(np.uint16) != v.view(np.uint16)).any(-1).mean()))
        print("hemisphere depth frame: not zero on %.1f %% of the pixels" % (100.0 * hz.view(np.uint16).any(-1).mean()))
    ctx.close()


if __name__ == "__main__":
    main()
