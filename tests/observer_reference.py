"""The definition of the direct cloud march from an observer's position (include/cloudsky.h) restated in numpy for the tests (test
infrastructure, not product).

For a direction e, the observer's world position o = (position[0], G_RADIUS + position[1], position[2]), N primary steps:

    accept   0.99 <= (e.x*e.x + e.y*e.y) + e.z*e.z <= 1.01                                  (NaN fails)
    isect(r) a = e.e;  b = 2*(e.x*o.x + e.y*o.y + e.z*o.z);  c = (o.x*o.x + o.y*o.y + o.z*o.z) - r*r
             D = b*b - 4*a*c;  d = sqrt(D);  near = min(-b-d, -b+d)/(2a);  far = max(-b-d, -b+d)/(2a)
    where    cb = c(B), ct = c(T):   below: cb < 0;   above: ct > 0;   inside: otherwise
    segment  below : blocked = b <= 0 and D(G) >= 0 -> no segment;   else t0 = far(B), t1 = far(T)
             inside: t0 = 0;  t1 = (b < 0 and D(B) >= 0) ? near(B) : far(T)
             above : no segment unless b < 0 and D(T) >= 0;  t0 = near(T);  t1 = D(B) >= 0 ? near(B) : far(T)
    cap      t1 = min(t1, max_distance)
    ray      start = o + e*t0, end = o + e*t1; shelldist = |end - start|; raystep = e * shelldist / N; ss = |raystep|; dir = raystep / ss;
             inc = dir * ss; p = start
    marched  accepted, a segment, t1 > t0, |end - start|^2 >= 2^-102 and |raystep|^2 >= 2^-102    (NaN fails)
             (the squares as summed for the two square roots; a segment too short to have a direction in fp32 is not marched)

Written from the definition, one operation per line, not from csrc/observer_core.h: float32 throughout, in the order written (dot products summed
left to right; numpy's float32 add, multiply, divide and sqrt are IEEE: exactly the operations of code compiled without contraction)."""
import numpy as np

from ray_reference import RB, RG, RT

F = np.float32
SQRT_EXACT_MIN = F(2.0 ** -102)                                 # cloud_core.h: both square roots of the ray's tail take at least this


def origin(position):
    p = np.asarray(position, F)
    return np.array([p[0], RG + p[1], p[2]], F)


def accept(e):
    """bool [...]: which directions float32 [..., 3] may be marched"""
    e = np.asarray(e, F)
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    with np.errstate(all="ignore"):
        l2 = x * x
        l2 = l2 + y * y
        l2 = l2 + z * z
        return (l2 >= F(0.99)) & (l2 <= F(1.01))


def _c(o, r):
    c = o[0] * o[0]
    c = c + o[1] * o[1]
    c = c + o[2] * o[2]
    return F(c - r * r)


def _isect(a, b, c):
    """(D, near, far)"""
    k = F(4.0) * a
    k = k * c
    D = b * b
    D = D - k
    d = np.sqrt(D)
    p = -b - d
    p2 = -b + d
    den = F(2.0) * a
    return D, np.minimum(p, p2) / den, np.maximum(p, p2) / den


def segment(position, max_distance, e):
    """(t0, t1 float32 [...], has bool [...]) of directions float32 [..., 3]: the capped first segment through the layer and whether there is one with
    t1 > t0.  Where `has` is False, t0 and t1 hold whatever the arithmetic gave.  Acceptance is not part of it."""
    e = np.asarray(e, F)
    o = origin(position)
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    with np.errstate(all="ignore"):
        a = x * x
        a = a + y * y
        a = a + z * z
        b = x * o[0]
        b = b + y * o[1]
        b = b + z * o[2]
        b = F(2.0) * b
        cb, ct, cg = _c(o, RB), _c(o, RT), _c(o, RG)
        Db, nb, fb = _isect(a, b, cb)
        Dt, nt, ft = _isect(a, b, ct)
        Dg, _, _ = _isect(a, b, cg)
        if cb < 0:
            has = ~((b <= 0) & (Dg >= 0))
            t0, t1 = fb, ft
        elif ct > 0:
            has = (b < 0) & (Dt >= 0)
            t0, t1 = nt, np.where(Db >= 0, nb, ft)
        else:
            has = np.ones(a.shape, bool)
            t0, t1 = np.zeros(a.shape, F), np.where((b < 0) & (Db >= 0), nb, ft)
        assert not np.isnan(np.where(has & accept(e), t1, F(0.0))).any()   # an end that is chosen exists: its discriminant was tested, or o is inside its sphere
        t1 = np.fmin(t1, F(max_distance)).astype(F)
        has = has & (t1 > t0)
    return t0.astype(F), t1, has


def classify(position, e, dtype=F):
    """(where, has, chord, t1_on_top) of directions float32 [..., 3], before the cap: where the definition puts the observer (0 below, 1 inside, 2
    above: one value, the observer's), whether the line has a segment, whether that segment leaves the layer's height range downwards and comes
    back (above: in through the top and out through it; inside: b < 0 and the inner shell missed), and whether its far end is on the outer shell.
    The definition's own tests, evaluated in `dtype`: float32 is what `segment` decides, float64 the geometry of the same fp32 inputs."""
    T = dtype
    e = np.asarray(e, F).astype(T)
    o = origin(position).astype(T)
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    with np.errstate(all="ignore"):
        a = x * x
        a = a + y * y
        a = a + z * z
        b = x * o[0]
        b = b + y * o[1]
        b = b + z * o[2]
        b = T(2.0) * b
        c0 = o[0] * o[0]
        c0 = c0 + o[1] * o[1]
        c0 = c0 + o[2] * o[2]
        cb, ct, cg = T(c0 - T(RB) * T(RB)), T(c0 - T(RT) * T(RT)), T(c0 - T(RG) * T(RG))
        k = T(4.0) * a
        Db, Dt, Dg = b * b - k * cb, b * b - k * ct, b * b - k * cg
        no = np.zeros(a.shape, bool)
        if cb < 0:
            return 0, ~((b <= 0) & (Dg >= 0)), no, ~no
        if ct > 0:
            return 2, (b < 0) & (Dt >= 0), Db < 0, Db < 0
        down = (b < 0) & (Db >= 0)
        return 1, ~no, (b < 0) & (Db < 0), ~down


def ray(position, max_distance, e, steps):
    """float32 [..., 11] (p, inc, dir, ss, marched as 1 / 0) of directions float32 [..., 3]; all zero where the ray is not marched."""
    e = np.asarray(e, F)
    o = origin(position)
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    t0, t1, has = segment(position, max_distance, e)
    marched = accept(e) & has
    n = F(steps)
    with np.errstate(all="ignore"):
        sx, sy, sz = o[0] + x * t0, o[1] + y * t0, o[2] + z * t0
        ex, ey, ez = o[0] + x * t1, o[1] + y * t1, o[2] + z * t1
        qx, qy, qz = ex - sx, ey - sy, ez - sz
        sd = qx * qx
        sd = sd + qy * qy
        sd = sd + qz * qz
        marched = marched & (sd >= SQRT_EXACT_MIN)
        sd = np.sqrt(sd)
        rx, ry, rz = x * sd / n, y * sd / n, z * sd / n
        ss = rx * rx
        ss = ss + ry * ry
        ss = ss + rz * rz
        marched = marched & (ss >= SQRT_EXACT_MIN)
        ss = np.sqrt(ss)
        ux, uy, uz = rx / ss, ry / ss, rz / ss
        out = np.stack([sx, sy, sz, ux * ss, uy * ss, uz * ss, ux, uy, uz, ss, np.ones_like(ss)], -1).astype(F)
    return np.where(marched[..., None], out, F(0.0))
