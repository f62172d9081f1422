"""The depth buffers the observer's march behind a scene depth is held at (test infrastructure, not product), beside observers.py: analytic surfaces
seen from the six observers' cameras (64 x 36), computed in float64 and cast to float32, metres along each pixel's ray.

    shell(name, A)   the distance from the observer along each ray to the sphere of radius G_RADIUS + A: the first root with t > 0, +inf where
                     there is none.  From under it a dome overhead, from above it the terrain below, from inside the layer a floor or a ceiling.
    mixed(name, A)   shell(A) in columns 0..37 and +inf in columns 38..63, but for a post (rows 20..30, columns 45..52) at 400 m.  No edge falls
                     on a multiple of 8: every 8 x 8 tile along an edge holds lanes of both kinds.
    quad(name)       the caps 3 000 / 9 000 / 20 000 / +inf in the four quadrants (QUAD_CAPS: top left, top right, bottom left, bottom right), split
                     at column 27 and row 13, both inside tiles.

ALTITUDE[name] is the A of `mixed` each observer is tested with, chosen from {2 000, 2 500, 3 000} on the host core so that assert_conditions
holds.  Geometry shares (of the marched rays, from observer_reference.segment alone): cut t0 < d < t1, occluded d <= t0, untouched d >= t1.
Measured on the host core with scene A (128 x 6 steps), in %; `alpha > 0` of the pixels of the capped frame, `changed` the marched pixels whose
texel differs from the uncapped frame's:

    name         A      cut   occluded  untouched   alpha > 0   changed
    ground      3000   59.4     4.2      36.5         53.6       42.3
    hill        3000   59.4     4.4      36.2         59.2       40.9
    inside      3000   31.9     0.0      68.1         83.2       20.1
    inside_up   3000   59.9     0.0      40.1         31.0       13.4
    above_down  2500   58.6     4.4      37.0         49.5       46.6
    offset      3000   59.4     4.4      36.2         81.7       61.7
"""
import numpy as np

import observers as OB
import scene_depth_reference as DR
from ray_reference import RG

F = np.float32
INF = float("inf")
POST = (20, 31, 45, 53, 400.0)                                  # rows [20, 31), columns [45, 53), metres
SPLIT_COLUMN = 38
QUAD_COLUMN, QUAD_ROW = 27, 13
QUAD_CAPS = (3000.0, 9000.0, 20000.0, INF)                      # top left, top right, bottom left, bottom right
ALTITUDE = {"ground": 3000.0, "hill": 3000.0, "inside": 3000.0, "inside_up": 3000.0, "above_down": 2500.0, "offset": 3000.0}


def shell(name, altitude):
    """float32 [H, W]: metres along each ray of the observer's camera to the sphere of radius G_RADIUS + altitude; +inf where the ray misses it"""
    pos = OB.observer(name)[0].astype(np.float64)
    o = np.array([pos[0], float(RG) + pos[1], pos[2]])
    e = OB.dirs(name).astype(np.float64)
    a = (e * e).sum(-1)
    b = 2.0 * (e * o).sum(-1)
    c = float((o * o).sum()) - (float(RG) + altitude) ** 2
    D = b * b - 4.0 * a * c
    with np.errstate(all="ignore"):
        r = np.sqrt(np.where(D >= 0, D, np.nan))
        near, far = (-b - r) / (2.0 * a), (-b + r) / (2.0 * a)
        t = np.where(near > 0, near, np.where(far > 0, far, np.inf))
    return np.where(D >= 0, t, np.inf).astype(F)


def mixed(name, altitude=None):
    z = shell(name, ALTITUDE[name] if altitude is None else altitude)
    z[:, SPLIT_COLUMN:] = F(INF)
    r0, r1, c0, c1, d = POST
    z[r0:r1, c0:c1] = F(d)
    return z


def quad_index(h, w):
    """int [h, w]: which of QUAD_CAPS each pixel takes"""
    j, i = np.mgrid[0:h, 0:w]
    return (i >= QUAD_COLUMN).astype(int) + 2 * (j >= QUAD_ROW).astype(int)


def quad(name):
    _, _, _, _, w, h = OB.observer(name)
    return np.asarray(QUAD_CAPS, F)[quad_index(h, w)]


def assert_conditions(name, z, capped, uncapped, marched_uncapped):
    """z float32 [H, W] a `mixed` buffer; capped / uncapped float16 [H, W, 4] the host core's frames behind it and without it; marched_uncapped
    bool [H, W] the rays the host core marches without it.  The conditions every test on `mixed` asserts before it compares anything."""
    pos, cap, _, _, _, _ = OB.observer(name)
    cut, occluded, untouched = DR.shares(pos, cap, OB.dirs(name), z)
    cloudy = float((capped[..., 3].astype(F) > 0).mean())
    differ = (capped.view(np.uint16) != uncapped.view(np.uint16)).any(-1)
    changed = float(differ[marched_uncapped].mean())
    print("%s, mixed: cut %.1f %%, occluded %.1f %%, untouched %.1f %% of the marched rays; alpha > 0 in %.1f %% of the pixels; %.1f %% of the marched pixels changed" %
          (name, 100 * cut, 100 * occluded, 100 * untouched, 100 * cloudy, 100 * changed))
    assert cut >= 0.25 and untouched >= 0.25
    if name not in ("inside", "inside_up"):
        assert occluded >= 0.02
    assert cloudy >= 0.25
    assert changed >= 0.10
    return cut, occluded, untouched, cloudy, changed
