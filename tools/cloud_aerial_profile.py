"""The timing run of the cloud depth frame and of the aerial perspective on a cloud frame (raw output: profiles/r17/).  One process,
meant to run under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cloud_aerial -- python tools/cloud_aerial_profile.py
20 warm-up C3 cloud frames (2048 x 1024, 128 x 6 steps), then 3 + 10 of them for scale; then, on that frame, 3 + 30 depth frames (2048 x 1024,
N = 128, the frame's own block) and 3 + 30 apply steps for each of n = 16 and n = 64, in both orders so that a drifting clock shows.  Prints
device-event times per group as well (profiler overhead included when run under one).
    python tools/cloud_aerial_profile.py --summarise DIR/cloud_aerial_kernel_trace.csv
prints the mean kernel time of each kernel from the trace (no GPU needed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUP_WARM, GROUP = 3, 30
GROUPS = (("depth", 0), ("apply", 16), ("apply", 64), ("apply", 64), ("apply", 16), ("depth", 0))

if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
    import csv
    rows = list(csv.DictReader(open(sys.argv[2])))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
    by = lambda key: [us(r) for r in sorted((r for r in rows if key in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))]   # noqa: E731
    dk, ak, ck = by("depth_kernel"), by("cloud_aerial_kernel"), by("clouds_kernel")
    per = GROUP_WARM + GROUP
    dk = dk[1:]                                              # the launch that fills the depth frame before the groups
    assert len(dk) == 2 * per and len(ak) == 4 * per, (len(dk), len(ak))
    for g in range(2):
        x = dk[g * per + GROUP_WARM:(g + 1) * per]
        print("depth_kernel 2048 x 1024 x 128, group %d: %d launches, mean %.2f us, min %.2f, max %.2f" % (g, len(x), sum(x) / len(x), min(x), max(x)))
    for g, n in enumerate((16, 64, 64, 16)):
        x = ak[g * per + GROUP_WARM:(g + 1) * per]
        print("cloud_aerial_kernel 2048 x 1024, n = %d: %d launches, mean %.2f us, min %.2f, max %.2f" % (n, len(x), sum(x) / len(x), min(x), max(x)))
    x = ck[-10:]
    print("clouds_kernel 2048 x 1024 (C3): %d launches, mean %.2f us" % (len(x), sum(x) / len(x)))
    sys.exit(0)

import torch  # noqa: E402

import gvcd_amd  # noqa: E402
from oracle import oracle as O  # noqa: E402

ctx = gvcd_amd.Context(0)
ctx.set_noise(*gvcd_amd.assets.load_default_noise())
W, H = 2048, 1024
sun = np.array([1.0, 1.0, 0.0], np.float32) / np.sqrt(np.float32(2.0))
ctx.render_transmittance(256, 64)
ctx.render_sky_lut(sun, 200, 100)
pc = O.default_params(W, H, (1, 1, 0))
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    frame = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
    depth = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
    out = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")

    def timed(label, n_warm, n, call):
        for _ in range(n_warm):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(n):
            call()
        e1.record(s)
        s.synchronize()
        print("%s: %.4f ms per launch (events around %d launches)" % (label, e0.elapsed_time(e1) / n, n), flush=True)

    timed("C3 cloud frame 2048x1024, warm-up", 0, 20, lambda: ctx.render_clouds_device(pc, W, (8, 0, 1, 128), frame.data_ptr(), W * 8, s.cuda_stream))
    timed("C3 cloud frame 2048x1024", 3, 10, lambda: ctx.render_clouds_device(pc, W, (8, 0, 1, 128), frame.data_ptr(), W * 8, s.cuda_stream))
    ctx.render_cloud_depth(pc, W, H, 128, out=depth, stream=s.cuda_stream)
    for kind, n in GROUPS:
        if kind == "depth":
            timed("depth frame 2048x1024x128", GROUP_WARM, GROUP, lambda: ctx.render_cloud_depth(pc, W, H, 128, out=depth, stream=s.cuda_stream))
        else:
            timed("apply step 2048x1024, n = %d" % n, GROUP_WARM, GROUP, lambda: ctx.apply_cloud_aerial(sun, frame, depth, n, out=out, stream=s.cuda_stream))
    f, z, o = frame.cpu().numpy(), depth.cpu().numpy(), out.cpu().numpy()
    cloudy = f[..., 3] > 0
    print("frame: %.3f of the pixels in cloud; depth frame non-zero %.3f; mean distance of the in-cloud pixels %.2f km (min %.2f, max %.2f); halves the apply step moved: %.3f"
          % (float(cloudy.mean()), float(z.view(np.uint16).any(-1).mean()), float(z[..., 0][cloudy].astype(np.float32).mean()), float(z[..., 0][cloudy].min()),
             float(z[..., 0][cloudy].max()), float((o.view(np.uint16) != f.view(np.uint16))[cloudy].mean())), flush=True)
ctx.close()
