"""The cloud depth frame and the aerial perspective on a cloud frame (include/cloudsky.h) restated in numpy for the tests (test
infrastructure, not product).

Written from the definitions, not from csrc/depth_core.h or csrc/cloud_aerial_core.h: the rays (tests/ray_reference.py), positions and distances
in float32, one operation per line in the order the definition gives (dot products summed left to right, IEEE sqrt and divide: numpy's float32 ufuncs are exactly that), and
per sample the oracle's own weather tap (csko_tap_weather, clouds.glsl:174) and density() (csko_density_probe, clouds.glsl:109-137, mip 0).  The
exp of a sample is numpy's, in float64, rounded once.  The apply step's air is tests/aerial_reference.columns with D = 1, S = n and one reach per
pixel; the transmittance behind its steps, which columns() keeps to itself, is restated beside it from the same lines."""
import ctypes as C

import numpy as np

import aerial_reference as AR
import tlut_reference as TR
from oracle import numpy_restatement as NR
from ray_reference import pixel_dirs, ray  # noqa: F401  (CR.pixel_dirs: what the tests of the core's direction compare with)

F = np.float32

SIZE = dict(width=64, height=32)
STEPS = {"A": 128, "B": 30}          # B: not a multiple of four (the early exit is tried every fourth step)
THIN = F(2.0 ** -6)                  # below this alpha the mean distance is only held between front and back


def rays(width, height, steps):
    """(e [H, W, 3], above [H, W], t0 [H, W], ss [H, W], start [3, H, W], step [3, H, W]) of every pixel: tests/ray_reference.py's ray of its
    direction.  Pixels that are not above hold whatever the arithmetic gives: nothing reads them."""
    e = pixel_dirs(width, height)
    r = ray(e, steps)
    return e, e[..., 1] > 0, r["t0"], r["ss"], np.moveaxis(r["p"], -1, 0), np.moveaxis(r["inc"], -1, 0)


_cache = {}


def depth_frame(oracle, otex, params, width, height, steps):
    """The restated depth frame.  A dict: out float16 [H, W, 4]; mean, front, back (metres), alpha float32 [H, W]; incloud int [H, W] the in-cloud
    samples per pixel; hit bool [H, W] the pixels whose texel is not zero; t0, ss float32 [H, W].  Computed once per argument set and shared:
    treat the arrays as read-only."""
    prm = np.ascontiguousarray(params, F)
    key = (prm.tobytes(), width, height, steps)
    if key in _cache:
        return _cache[key]
    L = oracle.lib()
    L.csko_tap_weather.restype = None
    L.csko_tap_weather.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    e, above, t0, ss, p, st = rays(width, height, steps)
    dens = np.zeros((steps, height, width), F)                       # density() of every sample; 0 where the ray is not marched
    w3, p3 = (C.c_float * 3)(), (C.c_float * 3)()
    wptr, pptr = otex.weather.ctypes.data_as(C.c_void_p), prm.ctypes.data_as(C.c_void_p)
    tex = C.byref(otex.c)
    tap, probe = L.csko_tap_weather, L.csko_density_probe
    up = above.tolist()
    for k in range(steps):
        p = p + st                                                   # :173
        wsx = p[0] * F(0.00006) + F(0.5) + prm[8]                    # :174
        wsy = p[2] * F(0.00006) + F(0.5) + prm[9]
        assert p.dtype == F and wsx.dtype == F
        pl, wxl, wyl = p.tolist(), wsx.tolist(), wsy.tolist()        # float32 -> Python float is exact, and c_float takes it back exactly
        row = dens[k]
        for j in range(height):
            upj = up[j]
            for i in range(width):
                if not upj[i]:
                    continue
                tap(wptr, wxl[j][i], wyl[j][i], w3)
                p3[0], p3[1], p3[2] = pl[0][j][i], pl[1][j][i], pl[2][j][i]
                row[j, i] = probe(tex, pptr, p3, w3, 0.0)
    T = np.ones((height, width), F)
    alpha = np.zeros((height, width), F)
    sw = np.zeros((height, width), F)
    swd = np.zeros((height, width), F)
    front = np.full((height, width), -1.0, F)
    back = np.zeros((height, width), F)
    incloud = np.zeros((height, width), np.int64)
    for k in range(steps):
        t = dens[k]
        m = t > 0                                                    # :184
        x = -prm[25] * t
        x = x * ss
        dt = np.exp(x.astype(np.float64)).astype(F)                  # :178
        s = F(k + 1) * ss
        s = t0 + s
        om = F(1.0) - dt
        w = T * om
        ws = w * s
        oa = F(1.0) - alpha
        inc = om * oa
        assert s.dtype == F and ws.dtype == F and inc.dtype == F
        sw = np.where(m, sw + w, sw)
        swd = np.where(m, swd + ws, swd)
        alpha = np.where(m, alpha + inc, alpha)                      # :207
        T = np.where(m, T * dt, T)                                   # :210
        front = np.where(m & (front < 0), s, front)
        back = np.where(m, s, back)
        incloud += m
    hit = above & (sw > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = swd / sw
    mean = np.minimum(np.maximum(mean, front), back)
    a = np.minimum(np.maximum(alpha, F(0.0)), F(1.0))
    out = np.stack([mean / F(1000.0), front / F(1000.0), back / F(1000.0), a], -1)
    assert out.dtype == F
    out = np.where(hit[..., None], out, F(0.0)).astype(np.float16)
    _cache[key] = dict(out=out, mean=np.where(hit, mean, F(0.0)), front=np.where(hit, front, F(0.0)), back=np.where(hit, back, F(0.0)), alpha=a,
                       incloud=incloud, hit=hit, t0=t0, ss=ss, above=above)
    return _cache[key]


def passes(cloud, depth):
    """The pixels csky_apply_cloud_aerial hands through: alpha is (+-)0 as a half, or the stored distance is not > 0.  bool [H, W]"""
    c, z = np.asarray(cloud, np.float16), np.asarray(depth, np.float16)
    with np.errstate(invalid="ignore"):
        return (c[..., 3] == 0) | ~(z[..., 0].astype(F) > 0)


def _transmittance(e, far_km, n, t_stop):
    """Tr behind the n steps of AR.columns(e, ., far_km, 1, n): its lines for the ray, the midpoints, the skip rule and the step's transmittance."""
    rd = np.stack([-e[..., 0], -e[..., 2], e[..., 1]], -1)
    ro = np.broadcast_to(NR.F([0, 0, 6371.5]), rd.shape)
    dt = (np.asarray(far_km, F) / F(n)).astype(F)
    Tr = np.ones(e.shape[:-1] + (4,), F)
    for i in range(n):
        t = (F(i) + F(0.5)) * dt
        take = ~(t >= t_stop)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            x_t = ro + rd * t[..., None]
            alt = NR.length(x_t) - NR.EARTH_RADIUS
            ext = NR.collision_coefficients(alt)[2]
            stepT = np.exp(-dt[..., None] * ext)
            Tr = np.where(take[..., None], Tr * stepT, Tr).astype(F)
    return Tr


def apply(cloud, depth, sun, steps, trans, mapping=TR.REFERENCE):
    """csky_apply_cloud_aerial restated.  cloud, depth: float16 [H, W, 4].  A dict: out float16 [H, W, 4]; L float32 [H, W, 4] the spectral
    in-scattering in front of every pixel; worked bool [H, W] the pixels that do not pass."""
    c, z = np.ascontiguousarray(cloud, np.float16), np.ascontiguousarray(depth, np.float16)
    H, W = c.shape[:2]
    worked = ~passes(c, z)
    e = pixel_dirs(W, H)
    far = np.where(worked, z[..., 0].astype(F), F(1.0))              # a reach for the pixels that pass too: their columns are discarded
    col = AR.columns(e, sun, far, 1, steps, trans, mapping)
    L = col["L"][0]
    Tr = _transmittance(e, far, steps, col["t_stop"])
    rgb = NR.M[0] * L[..., 0:1] + NR.M[1] * L[..., 1:2] + NR.M[2] * L[..., 2:3] + NR.M[3] * L[..., 3:4]
    tr = (((Tr[..., 0] + Tr[..., 1]) + Tr[..., 2]) + Tr[..., 3]) * F(0.25)
    cf = c.astype(F)
    o = cf[..., :3] * tr[..., None] + cf[..., 3:4] * (rgb / F(50.0))
    assert o.dtype == F
    out = c.copy()
    out[..., :3] = np.where(worked[..., None], o.astype(np.float16), c[..., :3])
    return dict(out=out, L=np.where(worked[..., None], L, F(0.0)), worked=worked, tr=tr)
