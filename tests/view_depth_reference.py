"""The depth frame of a ray frame (include/cloudsky.h csky_render_cloud_depth_dirs / _view) restated in numpy for the tests (test
infrastructure, not product).

The definition is the hemisphere depth frame's from "T = 1, alpha = 0 ..." on, for the ray of a direction the caller gives.  So this module restates
nothing twice: it runs tests/cloud_depth_reference.depth_frame, the restatement of that definition, with its rays() replaced by the rays of the
given directions (tests/ray_reference.ray, the one restatement of the march's ray) under the accept rule (tests/clouds_rays_reference.accept)."""
import numpy as np

import cloud_depth_reference as CR
import clouds_rays_reference as RR
from ray_reference import ray

F = np.float32


def depth_frame_dirs(oracle, otex, params, dirs, steps):
    """CR.depth_frame for the directions float32 [H, W, 3]: the same dict; `above` holds the accepted directions."""
    e = np.ascontiguousarray(dirs, F)
    assert e.ndim == 3 and e.shape[2] == 3
    height, width = e.shape[:2]
    ok = RR.accept(e)

    def rays(w, h, n):
        assert (w, h, n) == (width, height, steps)
        r = ray(e, n)
        return e, ok, r["t0"], r["ss"], np.moveaxis(r["p"], -1, 0), np.moveaxis(r["inc"], -1, 0)

    saved = CR.rays, CR._cache
    CR.rays, CR._cache = rays, {}                                    # a cache of its own: CR's key does not know the directions
    try:
        return CR.depth_frame(oracle, otex, params, width, height, steps)
    finally:
        CR.rays, CR._cache = saved
