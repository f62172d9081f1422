"""Drive the radiance cubemap for a kernel trace: `rocprofv3 --kernel-trace --stats -- python tools/radiance_profile.py`.
All layers of a 64 x 64 x 8-layer cubemap (csky_render_radiance, layer 0 from the default resource's sky), then PROCESS_MODE_INCREMENTAL
(one layer per call), then csky_prefilter_cube of the same layer 0; --reps times each after one warm-up.  Prints host wall times per call."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gvcd_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--face", type=int, default=64)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    sky = gvcd_amd.CloudSky.from_default_resource(device_id=0, texture_size=(768, 768), clock=lambda: 0.0)
    sky.sun = gvcd_amd.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
    sky.update_sky()

    def timed(name, fn):
        fn()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        print("%-34s %8.3f ms per call (host wall, blocking host form)" % (name, (time.perf_counter() - t0) * 1e3 / a.reps))

    timed("all %d layers, S = %d" % (a.layers, a.face), lambda: sky.radiance_cubemap(a.face, a.layers))
    timed("one incremental layer (cycling)", lambda: sky.update_radiance(a.face, a.layers))
    cube = np.ascontiguousarray(sky.radiance[0])
    timed("prefilter_cube, %d layers" % a.layers, lambda: sky.ctx.prefilter_cube(cube, a.layers))
    sky.close()


if __name__ == "__main__":
    main()
