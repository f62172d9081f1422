"""The shadowed aerial-perspective volume's timing run (raw output: profiles/r16/shafts_*).  One process, meant to run under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o shafts -- python tools/shafts_profile.py
20 warm-up launches, then 3 + 50 launches each of: the plain volume (aerial_kernel, unchanged from the parent commit: the yardstick in the same
process) and the shadowed volume (shafts_kernel) with a 256 x 256 shadow map rendered once from the shipped assets, at the default perspective
volume (32 x 32 x 32, S = 2, 32 km) and at a 64 x 32 x 64 panorama (S = 2, 32 km); CloudSky.aerial_perspective(cloud_shadows=True,
shadow_size=256), the pair of launches (shadow map + volume); then the first four groups again, so that a drifting clock shows.
Prints device-event times per group as well (profiler overhead included when run under one).
    python tools/shafts_profile.py --summarise DIR/shafts_kernel_trace.csv
prints the mean kernel time of each group from the trace (no GPU needed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
VOLUMES = ("plain perspective 32x32x32", "shadowed perspective 32x32x32", "plain panorama 64x32x64", "shadowed panorama 64x32x64")
GROUPS = VOLUMES + ("CloudSky pair, 256x256 map",) + VOLUMES
WARM, PER_GROUP_WARM, PER_GROUP = 20, 3, 50
KERNELS = {"aerial_kernel": "aerial", "shafts_kernel": "shafts", "shadow_kernel": "shadow"}


def kernel_of(name):
    for k, v in KERNELS.items():
        if k in name:
            return v
    return None


if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
    import csv
    rows = sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
    d = [(kernel_of(r["Kernel_Name"]), us(r)) for r in rows if kernel_of(r["Kernel_Name"])]
    per = [2 * (PER_GROUP_WARM + PER_GROUP) if g.startswith("CloudSky") else PER_GROUP_WARM + PER_GROUP for g in GROUPS]   # the pair is two kernels a call
    d = d[-sum(per):]
    assert len(d) == sum(per), len(d)
    at = 0
    for g, name in enumerate(GROUPS):
        x = d[at:at + per[g]]
        at += per[g]
        if name.startswith("CloudSky"):
            x = x[2 * PER_GROUP_WARM:]
            assert [k for k, _ in x] == ["shadow", "shafts"] * PER_GROUP, name
            sh, vo = [t for k, t in x if k == "shadow"], [t for k, t in x if k == "shafts"]
            print("%-30s: %d calls, shadow map mean %.2f us (min %.2f, max %.2f) + volume mean %.2f us (min %.2f, max %.2f) = %.2f us"
                  % (name, len(sh), sum(sh) / len(sh), min(sh), max(sh), sum(vo) / len(vo), min(vo), max(vo), (sum(sh) + sum(vo)) / len(sh)))
            continue
        x = x[PER_GROUP_WARM:]
        assert all(k == ("shafts" if name.startswith("shadowed") else "aerial") for k, _ in x), name
        x = [t for _, t in x]
        print("%-30s: %d launches, mean %.2f us, min %.2f, max %.2f" % (name, len(x), sum(x) / len(x), min(x), max(x)))
    sys.exit(0)

import torch  # noqa: E402

import aerial_reference as AR  # noqa: E402
import gvcd_amd  # noqa: E402

sky = gvcd_amd.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), clock=lambda: 0.0, device_buffers=True)
sky.sun = gvcd_amd.cloud_sky.DirectionalLight(direction=(1.0, 1.0, 0.0))
sky.update_sky()
ctx = sky.ctx
sun = np.asarray(sky.frame_data.LIGHT_DIRECTION, np.float32)
view = (AR.camera_basis(30.0, 10.0), 70.0)
center, extent = gvcd_amd.aerial_shadow_rect(sun, 32.0)
shadow = sky.cloud_shadow_map(256, extent, center)
torch.cuda.synchronize()
m = shadow.cpu().numpy().astype(np.float32)
print("shadow map 256x256 over %.1f x %.1f km: %.1f %% of the texels below 0.9, %.1f %% fully lit" % (extent[0] / 1e3, extent[1] / 1e3, 100 * (m < 0.9).mean(), 100 * (m == 1).mean()),
      flush=True)
persp = torch.empty((32, 32, 32, 4), dtype=torch.float16, device="cuda")
pano = torch.empty((64, 32, 64, 4), dtype=torch.float16, device="cuda")
s = torch.cuda.Stream()


def launch(name):
    size, out, v, aspect = ((32, 32, 32), persp, view, 16.0 / 9.0) if "perspective" in name else ((64, 32, 64), pano, None, 0.0)
    if name.startswith("plain"):
        ctx.render_aerial_perspective(sun, size[0], size[1], size[2], 32.0, 2, v, aspect, out=out, stream=s.cuda_stream)
    elif name.startswith("shadowed"):
        ctx.render_aerial_perspective_shadowed(sun, shadow, center, extent, size[0], size[1], size[2], 32.0, 2, v, aspect, out=out, stream=s.cuda_stream)
    else:
        sky.aerial_perspective(view=view, cloud_shadows=True, shadow_size=256)      # on torch's current stream, which is s here


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
        print("%-30s: %.4f ms per call (events around %d calls)" % (name, e0.elapsed_time(e1) / PER_GROUP, PER_GROUP), flush=True)
    a = persp.cpu().numpy().astype(np.float32)
    print("perspective volume: last-slice alpha %.3f .. %.3f, rgb max %.3f" % (a[-1, ..., 3].min(), a[-1, ..., 3].max(), a[..., :3].max()), flush=True)
sky.close()
