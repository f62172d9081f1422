"""The timing run of the direct cloud march (raw output: profiles/r18/view_march.txt).

    python tools/view_march_profile.py [--tree DIR] [--hemisphere-only]
One process.  The C3 parameters (128 x 6 steps, sun (1, 1, 0), the default block).  csky_set_kernel_timing's events around every launch, one frame
at a time on one stream: 20 warm-up hemisphere frames (2048 x 1024), then groups of 3 + 20 launches in the order hemisphere, view, view, hemisphere so
that a drifting clock shows.  The view: 1920 x 1080, fov 70, pitched up 20 degrees.  --tree DIR imports the package from another checkout (the parent
commit's, built there, for the hemisphere number the change must not move); --hemisphere-only is all such a tree can run.

    python tools/view_march_profile.py --walk
No GPU: the in-cloud samples per marched ray of both images from the host cores (tests/rays_host, every 16th pixel of every 16th row), so that the
two Mrays/s can be read against each other."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 2048, 1024
VW, VH, FOV, PITCH = 1920, 1080, 70.0, 20.0
STEPS, LIGHT = 128, 6
GROUP_WARM, GROUP = 3, 20


def c3_params(w, h):
    s = (np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)).astype(np.float32)
    return np.array([w, h, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.270588, 0.188235, 0.027451, 1.0, s[0], s[1], s[2], 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.05, 0.2, 0.0], np.float32)


def basis(pitch_deg):
    p = np.radians(pitch_deg)
    return np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]], np.float32)


def walk():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C
    import subprocess

    import gvcd_amd
    import test_clouds_rays_host as T
    from oracle import oracle as O
    O.build()
    d = os.path.join(ROOT, "tests", "rays_host")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "librays_host.so"))
    for f in ("rays_host_grid", "rays_host_view_dirs", "rays_host_march"):
        getattr(L, f).restype = None
    L.rays_host_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.rays_host_view_dirs.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p]
    L.rays_host_march.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    large, small, weather = gvcd_amd.assets.load_default_noise()
    chains = (gvcd_amd.assets.build_mips(large, 8), gvcd_amd.assets.build_mips(small, 6), np.ascontiguousarray(weather, np.uint8))
    p = c3_params(W, H)
    sky = O.sky_lut(p[16:19], O.transmittance_lut(256, 64), 200, 100)
    hemi, _ = T.grid(L, W, H, STEPS)
    view = T.host_view_dirs(L, basis(PITCH), FOV, VW, VH)
    for name, dirs in (("hemisphere %d x %d" % (W, H), hemi), ("view %d x %d, fov %g, pitched up %g" % (VW, VH, FOV, PITCH), view)):
        sub = np.ascontiguousarray(dirs[8::16, 8::16])
        img, marched, inc = T.host_march(L, chains, p, sky, sub, STEPS, LIGHT)
        m = int(marched.sum())
        print("%s: %d of %d rays walked, %.1f %% above the horizon, alpha > 0 on %.1f %%; in-cloud samples per marched ray %.2f (per ray of the image %.2f), heaviest ray %d"
              % (name, sub.size // 3, dirs.size // 3, 100.0 * marched.mean(), 100.0 * (img[..., 3] > 0).mean(), inc.sum() / max(m, 1), inc.mean(), int(inc.max())), flush=True)


def main():
    if "--walk" in sys.argv:
        return walk()
    tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT
    sys.path.insert(0, tree)
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
        s.synchronize()

        def hemisphere():
            ctx.render_clouds_device(p, W, (8, 0, 1, H // 8), frame.data_ptr(), W * 8, s.cuda_stream)

        def direct():
            ctx.render_clouds_view(p, basis(PITCH), FOV, VW, VH, out=view, stream=s.cuda_stream)

        def timed(label, rays, n_warm, n, call):
            for _ in range(n_warm):
                call()
                s.synchronize()                              # one frame at a time
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
            print("%s: kernel %.4f ms mean of %d (min %.4f, max %.4f), %.1f Mrays/s over the image's %d rays" % (label, mean, n, min(each), max(each), rays / mean / 1e3, rays),
                  flush=True)

        timed("hemisphere 2048 x 1024, warm-up", W * H, 0, 20, hemisphere)
        groups = (("hemisphere", hemisphere),) * 2 if "--hemisphere-only" in sys.argv else (("hemisphere", hemisphere), ("view", direct), ("view", direct), ("hemisphere", hemisphere))
        for kind, call in groups:
            if kind == "view":
                timed("view 1920 x 1080, fov 70, pitched up 20", VW * VH, GROUP_WARM, GROUP, call)
            else:
                timed("hemisphere 2048 x 1024", W * H, GROUP_WARM, GROUP, call)
        f = frame.cpu().numpy()
        print("hemisphere frame: alpha > 0 on %.1f %% of the pixels" % (100.0 * (f[..., 3] > 0).mean()))
        if "--hemisphere-only" not in sys.argv:
            v = view.cpu().numpy()
            print("view frame: alpha > 0 on %.1f %% of the pixels, %.1f %% of them zero texels" % (100.0 * (v[..., 3] > 0).mean(), 100.0 * (~v.view(np.uint16).any(-1)).mean()))
    ctx.close()


if __name__ == "__main__":
    main()
