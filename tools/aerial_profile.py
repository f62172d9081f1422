"""The aerial-perspective volume's timing run (raw output: profiles/r15/aerial_*).  One process, meant to run under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o aerial -- python tools/aerial_profile.py
20 warm-up launches, then 3 + 50 launches each of the default perspective volume (32 x 32 x 32, S = 2, 32 km), a 64 x 32 x 64 panorama (S = 2, 32 km)
and, as the yardstick in the same process, the 200 x 100 sky LUT with reuse off; then the first two groups again, so that a drifting clock shows.
Prints device-event times per group as well (profiler overhead included when run under one).
    python tools/aerial_profile.py --summarise DIR/aerial_kernel_trace.csv
prints the mean kernel time of each group from the trace (no GPU needed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GROUPS = ("perspective 32x32x32", "panorama 64x32x64", "sky LUT 200x100", "perspective 32x32x32", "panorama 64x32x64")
WARM, PER_GROUP_WARM, PER_GROUP = 20, 3, 50

if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
    import csv
    rows = sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
    d = [(("aerial" if "aerial_kernel" in r["Kernel_Name"] else "sky"), us(r)) for r in rows if "aerial_kernel" in r["Kernel_Name"] or "sky_lut_kernel" in r["Kernel_Name"]]
    d = d[-len(GROUPS) * (PER_GROUP_WARM + PER_GROUP):]
    assert len(d) == len(GROUPS) * (PER_GROUP_WARM + PER_GROUP), len(d)
    for g, name in enumerate(GROUPS):
        x = d[g * (PER_GROUP_WARM + PER_GROUP) + PER_GROUP_WARM:(g + 1) * (PER_GROUP_WARM + PER_GROUP)]
        assert all(k == ("sky" if name.startswith("sky") else "aerial") for k, _ in x), name
        x = [t for _, t in x]
        print("%-22s: %d launches, mean %.2f us, min %.2f, max %.2f" % (name, len(x), sum(x) / len(x), min(x), max(x)))
    sys.exit(0)

import torch  # noqa: E402

import aerial_reference as AR  # noqa: E402
import gvcd_amd  # noqa: E402

ctx = gvcd_amd.Context(0)
ctx.render_transmittance(256, 64)
ctx.set_sky_lut_reuse(False)
sun = (np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)).astype(np.float32)
view = (AR.camera_basis(30.0, 10.0), 70.0)
persp = torch.empty((32, 32, 32, 4), dtype=torch.float16, device="cuda")
pano = torch.empty((64, 32, 64, 4), dtype=torch.float16, device="cuda")
s = torch.cuda.Stream()


def launch(name):
    if name.startswith("perspective"):
        ctx.render_aerial_perspective(sun, 32, 32, 32, 32.0, 2, view, 16.0 / 9.0, out=persp, stream=s.cuda_stream)
    elif name.startswith("panorama"):
        ctx.render_aerial_perspective(sun, 64, 32, 64, 32.0, 2, out=pano, stream=s.cuda_stream)
    else:
        ctx.render_sky_lut_device(sun, 200, 100, s.cuda_stream)


with torch.cuda.stream(s):
    for _ in range(WARM):                                    # clocks up before the first timed group
        launch(GROUPS[0])
    for name in GROUPS:
        for _ in range(PER_GROUP_WARM):
            launch(name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(PER_GROUP):
            launch(name)
        e1.record(s)
        s.synchronize()
        ctx.sync()
        print("%-22s: %.4f ms per launch (events around %d launches)" % (name, e0.elapsed_time(e1) / PER_GROUP, PER_GROUP), flush=True)
    a = persp.cpu().numpy().astype(np.float32)
    print("perspective volume: last-slice alpha %.3f .. %.3f, rgb max %.3f" % (a[-1, ..., 3].min(), a[-1, ..., 3].max(), a[..., :3].max()), flush=True)
ctx.close()
