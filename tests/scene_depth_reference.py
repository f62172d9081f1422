"""The definition of the observer's cloud march behind a per-pixel scene depth (include/cloudsky.h) restated in numpy for the tests
(test infrastructure, not product).  Everything not named here is observer_reference.py's.

For pixel (i, j) with direction e and depth texel z:

    d        kind 0 (distance):  d = z
             kind 1 (view-z)  :  f = -((cam[6]*e.x + cam[7]*e.y) + cam[8]*e.z);  d = z / f;  not valid unless f > 0
    valid    z > 0 and d > 0                                             (NaN, 0, -0, negatives, -inf fail; +inf passes)
    cap      t1 = min(min(t1, max_distance), d)
    marched  accepted, a segment, valid, t1 > t0, |end - start|^2 >= 2^-102 and |raystep|^2 >= 2^-102      (the two sums as `ray` forms them; the
             first implies shelldist > 0)
    ray      observer_reference.ray's lines from t0 and the capped t1

Written from the definition, one operation per line, not from csrc/scene_depth_core.h: float32 throughout, in the order written."""
import numpy as np

import observer_reference as OR

F = np.float32
DISTANCE, VIEW_Z = 0, 1
ROOT_MIN = F(2.0 ** -102)                                       # the smallest argument the ray's two square roots are specified on


def forward(cam, e):
    """f float32 [...]: the directions float32 [..., 3] along the camera's forward axis; cam: csky_view.basis, nine floats column-major"""
    cam = np.asarray(cam, F)
    e = np.asarray(e, F)
    with np.errstate(all="ignore"):
        f = cam[6] * e[..., 0]
        f = f + cam[7] * e[..., 1]
        f = f + cam[8] * e[..., 2]
        return (-f).astype(F)


def cap(kind, cam, e, z):
    """(d float32 [...], valid bool [...]) of the depth texels z float32 [...] of the directions e float32 [..., 3]"""
    z = np.asarray(z, F)
    with np.errstate(all="ignore"):
        if kind == DISTANCE:
            d = z
            ok = np.ones(z.shape, bool)
        else:
            f = forward(cam, e)
            d = (z / f).astype(F)
            ok = f > F(0.0)
        return d, ok & (z > F(0.0)) & (d > F(0.0))


def view_z(cam, e, d):
    """The view-z buffer of distances d float32 [...] along the directions e: z = d * f, formed in float32"""
    with np.errstate(all="ignore"):
        return (np.asarray(d, F) * forward(cam, e)).astype(F)


def segment(position, max_distance, e, z, kind=DISTANCE, cam=None):
    """(t0, t1 float32 [...], has bool [...]): observer_reference.segment's with the depth's cap behind max_distance's; `has` includes `valid`"""
    t0, t1, has = OR.segment(position, max_distance, e)
    d, valid = cap(kind, cam, e, z)
    with np.errstate(all="ignore"):
        t1 = np.fmin(t1, d).astype(F)
        has = has & valid & (t1 > t0)
    return t0, t1, has


def ray(position, max_distance, e, z, steps, kind=DISTANCE, cam=None):
    """float32 [..., 11] (p, inc, dir, ss, marched as 1 / 0) of directions float32 [..., 3] with depth texels z float32 [...]; all zero where the
    ray is not marched."""
    e = np.asarray(e, F)
    o = OR.origin(position)
    x, y, zz = e[..., 0], e[..., 1], e[..., 2]
    t0, t1, has = segment(position, max_distance, e, z, kind, cam)
    marched = OR.accept(e) & has
    n = F(steps)
    with np.errstate(all="ignore"):
        sx, sy, sz = o[0] + x * t0, o[1] + y * t0, o[2] + zz * t0
        ex, ey, ez = o[0] + x * t1, o[1] + y * t1, o[2] + zz * t1
        qx, qy, qz = ex - sx, ey - sy, ez - sz
        sd = qx * qx
        sd = sd + qy * qy
        sd = sd + qz * qz
        marched = marched & (sd >= ROOT_MIN)
        sd = np.sqrt(sd)
        rx, ry, rz = x * sd / n, y * sd / n, zz * sd / n
        ss = rx * rx
        ss = ss + ry * ry
        ss = ss + rz * rz
        marched = marched & (ss >= ROOT_MIN)
        ss = np.sqrt(ss)
        ux, uy, uz = rx / ss, ry / ss, rz / ss
        out = np.stack([sx, sy, sz, ux * ss, uy * ss, uz * ss, ux, uy, uz, ss, np.ones_like(ss)], -1).astype(F)
    return np.where(marched[..., None], out, F(0.0))


def shares(position, max_distance, e, d):
    """(cut, occluded, untouched) as fractions of the rays observer_reference marches, for distances d float32 [...] along the directions e, from
    observer_reference.segment alone: cut t0 < d < t1, occluded d <= t0, untouched d >= t1"""
    t0, t1, has = OR.segment(position, max_distance, e)
    m = OR.accept(e) & has
    d = np.asarray(d, F)
    n = max(1, int(m.sum()))
    return float(((d > t0) & (d < t1) & m).sum()) / n, float(((d <= t0) & m).sum()) / n, float(((d >= t1) & m).sum()) / n
