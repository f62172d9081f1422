"""The observers the direct march from a position is held at (test infrastructure, not product), beside view_cameras.py: the reference's own place, a
hill, inside the layer looking level with a distance cap and looking up, above the layer looking down, and far off the reference's axis.

An observer is (position in metres from the reference's camera, y up; camera pitch and vertical field of view in degrees; max_distance).  Every
camera is clouds_rays_reference.VIEW's (64 x 36, yaw 40, fov 70) with the pitch named here, but for `inside`, whose field of view is 20 degrees: from
2 750 m a ray is still inside the layer after 20 000 m only within asin(1250 / 20000) = 3.58 degrees of level, a band 7.2 degrees thick whatever the
camera's pitch or yaw, which is 10 % of the rows of a 70 degree view (measured: 10.1 % of the marched rays end at the cap) and can reach the 25 % asked
of it in no other way than by a narrower view.  `inside_up` is pitched up 30 degrees, not 60: scene A has little cloud above 2 750 m, and at 60
degrees alpha > 0 in 5.6 % of the pixels (at 50: 14.8 %, at 40: 22.3 %, at 30: 35.1 %; other yaws give less).

assert_conditions holds every observer to the conditions it is in the table for, on the host core alone, before anything is compared:
alpha > 0 on at least 25 % of the pixels; above_down: at least 25 % of the marched rays look down; inside: the cap is the smaller of the two ends on
at least 25 % of the marched rays.  Measured on the host core with scene A (128 x 6 steps), in % :

    name         alpha > 0   marched   e.y < 0 of marched   capped of marched
    ground         57.4       83.3            0                    0
    hill           63.2       86.1            3.2                  0
    inside         86.9      100.0           50.0                 36.2
    inside_up      35.1      100.0            8.3                  0
    above_down     63.2       87.2          100.0                  0
    offset         85.6       86.1            3.2                  0
"""
import numpy as np

import clouds_rays_reference as RR

F = np.float32
INF = float("inf")
V = RR.VIEW

#        name           position (x, altitude, z)       pitch       fov       max_distance
OBSERVERS = {
    "ground":     ((0.0, 0.0, 0.0),               V["pitch"], V["fov"], INF),
    "hill":       ((0.0, 1000.0, 0.0),            V["pitch"], V["fov"], INF),
    "inside":     ((0.0, 2750.0, 0.0),            0.0,        20.0,     20000.0),
    "inside_up":  ((0.0, 2750.0, 0.0),            30.0,       V["fov"], INF),
    "above_down": ((0.0, 8000.0, 0.0),            -30.0,      V["fov"], INF),
    "offset":     ((50000.0, 1000.0, -30000.0),   V["pitch"], V["fov"], INF),
}
NAMES = list(OBSERVERS)
MOVED = [n for n in NAMES if n != "ground"]


def observer(name):
    """(position float32 [3], max_distance, basis 3x3 float32, fov, W, H)"""
    pos, pitch, fov, cap = OBSERVERS[name]
    return np.asarray(pos, F), cap, RR.camera_basis(pitch, V["yaw"]), fov, V["width"], V["height"]


def dirs(name):
    """float32 [H, W, 3]: the view directions of the observer's camera (the numpy restatement, bit-identical to the core's: test_clouds_rays_host H5)"""
    _, _, basis, fov, w, h = observer(name)
    return RR.view_dirs(basis, fov, w, h)


def assert_conditions(name, d, alpha, marched, seg):
    """d float32 [H, W, 3], alpha [H, W] and marched bool [H, W] of the host core's march, seg float32 [H, W, 2] its capped segments"""
    cap = OBSERVERS[name][3]
    cloudy = float((alpha > 0).mean())
    down = float((d[..., 1][marched] < 0).mean()) if marched.any() else 0.0
    capped = float((seg[..., 1][marched] == F(cap)).mean()) if marched.any() and np.isfinite(cap) else 0.0
    print("%s, host core: alpha > 0 in %.1f %% of the pixels, %.1f %% marched; of the marched rays %.1f %% look down, %.1f %% end at the cap" %
          (name, 100 * cloudy, 100 * marched.mean(), 100 * down, 100 * capped))
    assert cloudy >= 0.25
    if name == "above_down":
        assert down >= 0.25
    if name == "inside":
        assert capped >= 0.25
    return cloudy, down, capped
