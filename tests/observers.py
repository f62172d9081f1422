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
import observer_reference as OR

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


# The ends of what observer_invalid accepts and the rays the six above never reach (the table of measured figures: assert_edge_conditions).  A second
# table: every test parametrized over NAMES or MOVED keeps its cases.
#        name            position (x, altitude, z)          pitch    fov    max_distance
EDGE = {
    "above_graze": ((0.0, 8000.0, 0.0),             -2.38,   1.5,   INF),      # the layer's limb from above: half the rays pass over the inner shell
    "inside_dip":  ((0.0, 2750.0, 0.0),             -0.6,    2.0,   INF),      # inside, just under level: rays that dip and rise
    "high_down":   ((0.0, 100000.0, 0.0),           -60.0,   70.0,  INF),      # OBSERVER_MAX_ALTITUDE
    "high_graze":  ((0.0, 100000.0, 0.0),           -10.24,  0.4,   INF),      # the limb from there: segments of 342 km
    "far_ground":  ((1.0e6, -83000.0, 0.0),         20.0,    70.0,  INF),      # OBSERVER_MAX_OFFSET, 907 m above the sphere, under the layer
    "far_above":   ((-1.0e6, -60000.0, 5.0e5),      -30.0,   70.0,  INF),      # as far out, above the layer
    "on_bottom":   ((0.0, 1500.0, 0.0),             20.0,    70.0,  INF),      # |o| = SKY_B_RADIUS exactly: cb == 0
    "on_top":      ((0.0, 4000.0, 0.0),             -20.0,   70.0,  INF),      # |o| = SKY_T_RADIUS exactly: ct == 0
    "capped_ring": ((0.0, 0.0, 0.0),                20.0,    70.0,  6000.0),   # the cap in front of the layer for some rays, inside it for others
}
EDGE_NAMES = list(EDGE)
CHORD = ["above_graze", "inside_dip", "high_graze"]           # a quarter of their marched rays or more leave the layer's height range downwards and come back
ALL_NAMES = NAMES + EDGE_NAMES


def observer(name):
    """(position float32 [3], max_distance, basis 3x3 float32, fov, W, H)"""
    pos, pitch, fov, cap = OBSERVERS[name] if name in OBSERVERS else EDGE[name]
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


def assert_edge_conditions(name, d, alpha, marched, seg):
    """assert_conditions for an observer of EDGE: the arrays of the host core's march of its camera's rays.  What each is in the table for, before
    anything is compared.  `chord`: the share of the marched rays that leave the layer's height range downwards and come back, by the restated
    definition's own tests (observer_reference.classify).  `capped`: the share of them whose end is the cap.  `refused`: the share of the accepted
    rays that have a segment without the cap and none with it (the cap ends them in front of the layer).  `marched`, `capped` and alpha are the host
    core's; which rays are chords and which have a segment without the cap is asked of the numpy restatement, which the core equals bit for bit
    (test_observer_edges_host E1).  Measured with scenes A (128 x 6 steps) and B (30 x 4), in % :

        name          marched   chord   capped   refused   alpha > 0, A / B
        above_graze     69.4     56.0     0         0        56.4 / 56.6
        inside_dip     100.0     58.3     0         0       100.0 / 100.0
        high_down      100.0      0       0         0        57.7 / 75.8
        high_graze      66.7     50.0     0         0        54.7 / 55.0
        far_ground      69.2      0       0         0        62.7 / 68.8
        far_above       75.1      0.5     0         0        50.9 / 64.2
        on_bottom       75.0      0       0         0        61.2 / 74.9
        on_top          75.0      2.9     0         0        56.1 / 65.8
        capped_ring     52.7      0      81.2      22.3      23.4 / 31.7
    """
    pos, _, _, cap = EDGE[name]
    where, has, chord, _ = OR.classify(pos, d)
    _, _, free = OR.segment(pos, INF, d)
    ok = OR.accept(d)
    cloudy = float((alpha > 0).mean())
    chords = float((has & chord)[marched].mean())
    capped = float((seg[..., 1][marched] == F(cap)).mean()) if np.isfinite(cap) else 0.0
    refused = float((free & ~marched)[ok].mean())
    print("%s, host core: alpha > 0 in %.1f %% of the pixels, %.1f %% marched; of the marched rays %.1f %% dip and rise, %.1f %% end at the cap; the cap refuses %.1f %% of the accepted rays" %
          (name, 100 * cloudy, 100 * marched.mean(), 100 * chords, 100 * capped, 100 * refused))
    assert ok.all()
    assert cloudy >= (0.15 if name == "capped_ring" else 0.25)
    if name in CHORD:
        assert chords >= 0.25
    if name == "capped_ring":
        assert capped >= 0.25 and refused >= 0.10
    if name in ("inside_dip", "high_down"):                  # the layer fills these two views (high_down: the limb is 79.8 degrees from the nadir, the view's corners 72.2)
        assert marched.all()
    else:
        assert not marched.all()
    o = OR.origin(pos)
    if name == "on_bottom":
        assert OR._c(o, OR.RB) == 0 and where == 1
    if name == "on_top":
        assert OR._c(o, OR.RT) == 0 and where == 1
    return cloudy, chords, capped, refused
