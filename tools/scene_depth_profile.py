"""The timing run of the observer's cloud march behind a per-pixel scene depth (raw output: profiles/r29/scene_depth.txt).

    python tools/scene_depth_profile.py
One process, in the manner of tools/observer_profile.py, whose parameters it takes: the C3 block (128 x 6 steps, sun (1, 1, 0)), 1920 x 1080 views
of fov 70 from `above_down` (8 000 m up, pitched down 30 degrees) and `inside` (2 750 m up, level, capped at 20 000 m).  csky_set_kernel_timing's
events around every launch, one call at a time on one stream: 20 warm-up hemisphere frames, then for each observer groups of 3 + 20 launches in
the order

    _from (clouds_observer_kernel), _from_depth with +inf everywhere (clouds_observer_depth_kernel), the same again, _from

so that a drifting clock shows: the same rays through both kernels, and the difference is what the depth kernel pays for its load and its two
clauses.  Then the depth form behind `shell` (a sphere at 2 500 m seen from above, at 3 000 m from inside) and behind `mixed` (that sphere in the
left 38 / 64 of the image, nothing in the right but for a post at 400 m), tests/scene_depths.py's surfaces at this size, with the shares of cut,
occluded and untouched rays from the restatement of the definition (tests/observer_reference.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from view_march_profile import FOV, GROUP, GROUP_WARM, LIGHT, STEPS, VH, VW, H, W, basis, c3_params  # noqa: E402

INF = float("inf")
RG = 6000000.0
F = np.float32
#            label          pitch   position              cap       the sphere's altitude
OBSERVERS = (("above_down", -30.0, (0.0, 8000.0, 0.0), INF, 2500.0), ("inside", 0.0, (0.0, 2750.0, 0.0), 20000.0, 3000.0))


def shell(pos, dirs, altitude):
    """tests/scene_depths.py shell for any image: metres along each ray to the sphere of radius RG + altitude, +inf where the ray misses it"""
    o = np.array([pos[0], RG + pos[1], pos[2]], np.float64)
    e = dirs.astype(np.float64)
    a, b, c = (e * e).sum(-1), 2.0 * (e * o).sum(-1), float((o * o).sum()) - (RG + altitude) ** 2
    D = b * b - 4.0 * a * c
    with np.errstate(all="ignore"):
        r = np.sqrt(np.where(D >= 0, D, np.nan))
        near, far = (-b - r) / (2.0 * a), (-b + r) / (2.0 * a)
        t = np.where(near > 0, near, np.where(far > 0, far, np.inf))
    return np.where(D >= 0, t, np.inf).astype(F)


def mixed(z):
    """tests/scene_depths.py mixed at the image's own size: the same fractions of a 64 x 36 image"""
    h, w = z.shape
    z = z.copy()
    z[:, 38 * w // 64:] = F(INF)
    z[20 * h // 36:31 * h // 36, 45 * w // 64:53 * w // 64] = F(400.0)
    return z


def main():
    sys.path.insert(0, ROOT)
    import torch

    import clouds_rays_reference as RR
    import gvcd_amd
    import scene_depth_reference as DR
    ctx = gvcd_amd.Context(0)
    ctx.set_noise(*gvcd_amd.assets.load_default_noise())
    ctx.set_march(STEPS, LIGHT)
    p = c3_params(W, H)
    ctx.render_transmittance(256, 64)
    ctx.render_sky_lut(p[16:19], 200, 100)
    print("library %s" % os.path.relpath(gvcd_amd.library_path(), ROOT), flush=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        frame = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
        view = torch.empty((VH, VW, 4), dtype=torch.float16, device="cuda")
        other = torch.empty((VH, VW, 4), dtype=torch.float16, device="cuda")
        s.synchronize()

        def hemisphere():
            ctx.render_clouds_device(p, W, (8, 0, 1, H // 8), frame.data_ptr(), W * 8, s.cuda_stream)

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

        timed("hemisphere 2048 x 1024, warm-up", 0, 20, hemisphere)
        for name, pitch, pos, cap, altitude in OBSERVERS:
            b = basis(pitch)
            dirs = RR.view_dirs(b, FOV, VW, VH)
            surface = shell(pos, dirs, altitude)
            buffers = {"inf": np.full((VH, VW), INF, F), "shell": surface, "mixed": mixed(surface)}
            dev = {k: torch.from_numpy(v).cuda() for k, v in buffers.items()}
            s.synchronize()

            def plain():
                ctx.render_clouds_view_from(p, b, FOV, VW, VH, pos, cap, out=view, stream=s.cuda_stream)

            def behind(k):
                return lambda: ctx.render_clouds_view_from_depth(p, b, FOV, VW, VH, pos, dev[k], "distance", cap, out=other, stream=s.cuda_stream)
            where = "view 1920 x 1080, fov 70, %s" % name
            ms = {"from": [], "inf": []}
            for kind, call in (("from", plain), ("inf", behind("inf")), ("inf", behind("inf")), ("from", plain)):
                ms[kind].append(timed("%s, %s" % (where, "clouds_observer_kernel" if kind == "from" else "clouds_observer_depth_kernel, +inf everywhere"), GROUP_WARM, GROUP, call))
            a, c = sum(ms["from"]) / 2, sum(ms["inf"]) / 2
            print("%s, the same rays: clouds_observer_kernel %.4f ms (its two groups %+.2f %% apart), clouds_observer_depth_kernel %.4f ms, %+.2f %%" %
                  (name, a, 100.0 * (ms["from"][1] / ms["from"][0] - 1.0), c, 100.0 * (c / a - 1.0)), flush=True)
            assert (view.cpu().numpy().view(np.uint16) == other.cpu().numpy().view(np.uint16)).all()
            for k in ("shell", "mixed"):
                t = timed("%s, clouds_observer_depth_kernel behind %s" % (where, k), GROUP_WARM, GROUP, behind(k))
                cut, occluded, untouched = DR.shares(pos, cap, dirs, buffers[k])
                v = other.cpu().numpy()
                print("%s behind %s: %+.2f %% against clouds_observer_kernel; cut %.1f %%, occluded %.1f %%, untouched %.1f %% of the marched rays; alpha > 0 on %.1f %% of the pixels" %
                      (name, k, 100.0 * (t / a - 1.0), 100.0 * cut, 100.0 * occluded, 100.0 * untouched, 100.0 * (v[..., 3] > 0).mean()), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
