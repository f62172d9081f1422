"""The cloud shadow map's definition (include/cloudsky.h) restated in numpy for the tests (test infrastructure, not product).

Written from the definition, not from csrc/shadow_core.h: the positions in float32, one operation per line in the order the definition gives
(dot products summed left to right, IEEE sqrt and divide: numpy's float32 ufuncs are exactly that), and per sample the oracle's own weather tap
(csko_tap_weather, clouds.glsl:174) and density() (csko_density_probe, clouds.glsl:109-137, mip 0).  tau is summed in float32; one exp at the end."""
import ctypes as C

import numpy as np

F = np.float32
RG, RB, RT = F(6000000.0), F(6001500.0), F(6004000.0)   # clouds.glsl:43-45

# the gate for values rendered from the shipped assets (tests/parity_metrics.py TIGHT), applied to the one channel
GATE = dict(max_ulp=2, within1=0.999, max_err=2e-3)

SCENE_SIZE = dict(width=64, height=64, center=(0.0, 0.0), extent=(16384.0, 16384.0), steps=32)


def scene(oracle, name):
    """The push-constant blocks of scenes A and B."""
    if name == "A":
        return oracle.default_params(64, 32, (1, 1, 0), coverage=0.2)
    p = oracle.default_params(64, 32, (-0.9, 0.26, 0.3), coverage=0.35)
    p[4:10] = (1.5, -2.25, 0.75, 3.5, 0.125, -0.375)
    p[23] = 12.5
    return p


def _intersect_sphere(px, py, pz, dx, dy, dz, r):   # clouds.glsl:97-105
    a = dx * dx
    a = a + dy * dy
    a = a + dz * dz
    b = dx * px
    b = b + dy * py
    b = b + dz * pz
    b = F(2.0) * b
    c = px * px
    c = c + py * py
    c = c + pz * pz
    c = c - r * r
    e = F(4.0) * a
    e = e * c
    d = b * b
    d = d - e
    d = np.sqrt(d)
    p = -b - d
    p2 = -b + d
    return np.maximum(p, p2) / (F(2.0) * a)


def sample_positions(params, width, height, center, extent, steps):
    """(l, p, ss): l = normalize(LIGHT_DIRECTION) (3 float32), p = float32 [steps, 3, height, width] sample positions, ss = float32 [height, width]."""
    prm = np.asarray(params, F)
    W, H, N = F(width), F(height), F(steps)
    lx, ly, lz = prm[16], prm[17], prm[18]
    n = lx * lx
    n = n + ly * ly
    n = n + lz * lz
    n = np.sqrt(n)
    lx, ly, lz = lx / n, ly / n, lz / n
    i = np.arange(width, dtype=F)[None, :] + np.zeros((height, 1), F)
    j = np.arange(height, dtype=F)[:, None] + np.zeros((1, width), F)
    u = (i + F(0.5)) / W
    v = (j + F(0.5)) / H
    gx = F(center[0]) + (u - F(0.5)) * F(extent[0])
    gz = F(center[1]) + (v - F(0.5)) * F(extent[1])
    gy = np.full_like(gx, RG)
    t0 = _intersect_sphere(gx, gy, gz, lx, ly, lz, RB)
    t1 = _intersect_sphere(gx, gy, gz, lx, ly, lz, RT)
    sx0, sy0, sz0 = gx + lx * t0, gy + ly * t0, gz + lz * t0
    ex0, ey0, ez0 = gx + lx * t1, gy + ly * t1, gz + lz * t1
    qx, qy, qz = ex0 - sx0, ey0 - sy0, ez0 - sz0
    sd = qx * qx
    sd = sd + qy * qy
    sd = sd + qz * qz
    sd = np.sqrt(sd)
    ss = sd / N
    stx, sty, stz = lx * sd / N, ly * sd / N, lz * sd / N
    px, py, pz = sx0 + stx * F(0.5), sy0 + sty * F(0.5), sz0 + stz * F(0.5)
    out = np.zeros((steps, 3, height, width), F)
    for k in range(steps):
        out[k, 0], out[k, 1], out[k, 2] = px, py, pz
        px, py, pz = px + stx, py + sty, pz + stz
    assert ss.dtype == F and out.dtype == F and px.dtype == F
    return (lx, ly, lz), out, ss


_cache = {}


def shadow_map(oracle, otex, params, width, height, center=(0.0, 0.0), extent=(16384.0, 16384.0), steps=64):
    """(map float16 [height, width], in-cloud samples).  Computed once per argument set and shared: treat the arrays as read-only."""
    prm = np.ascontiguousarray(params, F)
    key = (prm.tobytes(), width, height, tuple(center), tuple(extent), steps)
    if key in _cache:
        return _cache[key]
    L = oracle.lib()
    L.csko_tap_weather.restype = None
    L.csko_tap_weather.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    (lx, ly, lz), pos, ss = sample_positions(prm, width, height, center, extent, steps)
    if not ly > 0:                                                   # night
        _cache[key] = (np.zeros((height, width), np.float16), 0)
        return _cache[key]
    wsx = pos[:, 0] * F(0.00006) + F(0.5) + prm[8]                   # clouds.glsl:174
    wsy = pos[:, 2] * F(0.00006) + F(0.5) + prm[9]
    assert wsx.dtype == F
    tau = np.zeros((height, width), F)
    incloud = 0
    w3, p3 = (C.c_float * 3)(), (C.c_float * 3)()
    wptr, pptr = otex.weather.ctypes.data_as(C.c_void_p), prm.ctypes.data_as(C.c_void_p)
    tex = C.byref(otex.c)
    tap, probe = L.csko_tap_weather, L.csko_density_probe
    pos_l, wsx_l, wsy_l = pos.tolist(), wsx.tolist(), wsy.tolist()  # float32 -> Python float is exact, and c_float takes it back exactly
    for j in range(height):
        for i in range(width):
            t = F(0.0)
            for k in range(steps):
                tap(wptr, wsx_l[k][j][i], wsy_l[k][j][i], w3)
                pk = pos_l[k]
                p3[0], p3[1], p3[2] = pk[0][j][i], pk[1][j][i], pk[2][j][i]
                d = probe(tex, pptr, p3, w3, 0.0)
                if d > 0.0:
                    incloud += 1
                t = F(t + F(d))
            tau[j, i] = t
    x = -prm[25] * ss                                                # exp(-params.density * ss * tau)
    x = x * tau
    assert x.dtype == F
    m = np.exp(x.astype(np.float64)).astype(np.float16)
    _cache[key] = (m, incloud)
    return _cache[key]


def compare(test, ref):
    """The figures the gate is written against: (worst fp16 ulp distance, share within 1 ulp, largest absolute difference)."""
    from conftest import ulp_diff
    t, r = np.ascontiguousarray(test, np.float16), np.ascontiguousarray(ref, np.float16)
    u = ulp_diff(t, r)
    err = np.abs(t.astype(np.float64) - r.astype(np.float64))
    return int(u.max()), float((u <= 1).mean()), float(err.max())


def assert_gate(test, ref, what=""):
    worst, within1, max_err = compare(test, ref)
    print("shadow parity %s: worst ulp %d, within 1 ulp %.5f, max |d| %.3e" % (what, worst, within1, max_err))
    assert np.isfinite(np.asarray(test, np.float32)).all(), what
    assert worst <= GATE["max_ulp"] and within1 >= GATE["within1"] and max_err <= GATE["max_err"], (what, worst, within1, max_err)
