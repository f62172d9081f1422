"""The cloud shadow map's timing run (raw output: profiles/r14/).  One process, meant to run under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o shadow -- python tools/shadow_profile.py
30 warm-up launches, then eight groups of 3 + 50 launches of a 1024 x 1024, N = 64 map -- scenes A and B of tests/shadow_reference.py with the exact
end on and off, then the same four in reverse order, so that a drifting clock shows -- and 3 + 10 C3 cloud frames (2048 x 1024, 128 x 6 steps) for
scale.  Prints device-event times per group as well (profiler overhead included when run under one).
    python tools/shadow_profile.py --summarise DIR/shadow_kernel_trace.csv
prints the mean kernel time of each group from the trace (no GPU needed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GROUPS = (("A", True), ("A", False), ("B", True), ("B", False), ("B", False), ("B", True), ("A", False), ("A", True))
WARM, PER_GROUP_WARM, PER_GROUP = 30, 3, 50

if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
    import csv
    rows = list(csv.DictReader(open(sys.argv[2])))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
    sh = sorted((r for r in rows if "shadow_kernel" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    d = [us(r) for r in sh][WARM:]
    assert len(d) == len(GROUPS) * (PER_GROUP_WARM + PER_GROUP), len(sh)
    for g, (name, exact) in enumerate(GROUPS):
        x = d[g * (PER_GROUP_WARM + PER_GROUP) + PER_GROUP_WARM:(g + 1) * (PER_GROUP_WARM + PER_GROUP)]
        print("shadow_kernel scene %s exact_end=%d: %d launches, mean %.2f us, min %.2f, max %.2f" % (name, exact, len(x), sum(x) / len(x), min(x), max(x)))
    cl = sorted((r for r in rows if "clouds_kernel" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    x = [us(r) for r in cl][-10:]
    print("clouds_kernel 2048 x 1024 (C3): %d launches, mean %.2f us" % (len(x), sum(x) / len(x)))
    sys.exit(0)

import torch  # noqa: E402

import gvcd_amd  # noqa: E402
import shadow_reference as SR  # noqa: E402
from oracle import oracle as O  # noqa: E402

ctx = gvcd_amd.Context(0)
ctx.set_noise(*gvcd_amd.assets.load_default_noise())
W = H = 1024
out = torch.empty((H, W), dtype=torch.float16, device="cuda")
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    p = SR.scene(O, "A")
    for _ in range(WARM):                                    # clocks up before the first timed group
        ctx.render_cloud_shadow(p, W, H, (0.0, 0.0), (16384.0, 16384.0), 64, out=out, stream=s.cuda_stream)
    for name, exact in GROUPS:
        p = SR.scene(O, name)
        ctx.set_shadow_exact_end(exact)
        for _ in range(PER_GROUP_WARM):
            ctx.render_cloud_shadow(p, W, H, (0.0, 0.0), (16384.0, 16384.0), 64, out=out, stream=s.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(PER_GROUP):
            ctx.render_cloud_shadow(p, W, H, (0.0, 0.0), (16384.0, 16384.0), 64, out=out, stream=s.cuda_stream)
        e1.record(s)
        s.synchronize()
        m = out.cpu().numpy()
        print("scene %s exact_end=%d: %.4f ms per launch (events around 50 launches); zeros %.3f ones %.3f" %
              (name, exact, e0.elapsed_time(e1) / 50, float((m.view(np.uint16) == 0).mean()), float((m.view(np.uint16) == 0x3C00).mean())), flush=True)
    ctx.set_shadow_exact_end(True)
    sun = SR.F([1, 1, 0]) / np.sqrt(SR.F(2))
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(sun, 200, 100)
    pc = O.default_params(2048, 1024, (1, 1, 0))
    frame = torch.empty((1024, 2048, 4), dtype=torch.float16, device="cuda")
    for _ in range(3):
        ctx.render_clouds_device(pc, 2048, (8, 0, 1, 128), frame.data_ptr(), 2048 * 8, s.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(10):
        ctx.render_clouds_device(pc, 2048, (8, 0, 1, 128), frame.data_ptr(), 2048 * 8, s.cuda_stream)
    e1.record(s)
    s.synchronize()
    print("C3 cloud frame 2048x1024: %.4f ms per launch (events around 10 launches)" % (e0.elapsed_time(e1) / 10), flush=True)
ctx.close()
