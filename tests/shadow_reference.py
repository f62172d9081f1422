"""The cloud shadow map's definition (include/cloudsky.h) restated in numpy for the tests (test infrastructure, not product).

Written from the definition, not from csrc/shadow_core.h: the positions in float32, one operation per line in the order the definition gives
(dot products summed left to right, IEEE sqrt and divide: numpy's float32 ufuncs are exactly that), and per sample the oracle's own weather tap
(csko_tap_weather, clouds.glsl:174) and density() (csko_density_probe, clouds.glsl:109-137, mip 0).  tau is summed in float32; one exp at the end.

The three kinds of texel, from the two discriminants in the order of clouds.glsl:97-105: disc(Rb) >= 0: ORDINARY, from the larger root of Rb to the
larger root of Rt; otherwise disc(Rt) >= 0: CHORD, from the smaller to the larger root of Rt; otherwise MISS: the half 1.0 and no sample.

SCENES is the scene sweep that tests/test_shadow_host.py and tests/test_gpu_cloud_shadow.py share."""
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


def _sphere_roots(px, py, pz, dx, dy, dz, r):   # clouds.glsl:97-105, both roots and the discriminant
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
    disc = b * b
    disc = disc - e
    with np.errstate(invalid="ignore"):
        d = np.sqrt(disc)
        p = -b - d
        p2 = -b + d
        return disc, np.minimum(p, p2) / (F(2.0) * a), np.maximum(p, p2) / (F(2.0) * a)


ORDINARY, CHORD, MISS = 0, 1, 2                # the three kinds of texel: the line meets the inner shell; only the outer one, on a chord; neither


def texel_kinds(params, width, height, center, extent):
    """int [height, width] of ORDINARY / CHORD / MISS"""
    return sample_positions(params, width, height, center, extent, 1)[3]


def sample_positions(params, width, height, center, extent, steps):
    """(l, p, ss, kind): l = normalize(LIGHT_DIRECTION) (3 float32), p = float32 [steps, 3, height, width] sample positions, ss = float32 [height, width],
    kind = int [height, width].  A MISS texel has no samples: its p and ss are 0."""
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
    disc_b, _, hi_b = _sphere_roots(gx, gy, gz, lx, ly, lz, RB)
    disc_t, lo_t, hi_t = _sphere_roots(gx, gy, gz, lx, ly, lz, RT)
    kind = np.where(disc_b >= 0, ORDINARY, np.where(disc_t >= 0, CHORD, MISS))
    t0 = np.where(kind == ORDINARY, hi_b, np.where(kind == CHORD, lo_t, F(0.0))).astype(F)     # the chord's near end: the smaller root of Rt
    t1 = np.where(kind == MISS, F(0.0), hi_t).astype(F)
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
    miss = kind == MISS
    out[:, :, miss] = 0
    ss = np.where(miss, F(0.0), ss).astype(F)
    assert ss.dtype == F and out.dtype == F and px.dtype == F
    return (lx, ly, lz), out, ss, kind


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
    (lx, ly, lz), pos, ss, kind = sample_positions(prm, width, height, center, extent, steps)
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
            for k in range(steps if kind[j, i] != MISS else 0):              # the line meets no cloud: no sample, and exp(-0) = 1.0 is stored
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


# ----------------------------------------------------------------------------------------------------------------------------------------------
# The scene sweep: one table for the host build (tests/test_shadow_host.py) and the GPU (tests/test_gpu_cloud_shadow.py).
# ----------------------------------------------------------------------------------------------------------------------------------------------
def helper_rect(sun, far_km=32.0):
    """The rectangle csky_aerial_shadow_rect hands out, by the contract's text (tests/shafts_reference.py has the restatement)."""
    import shafts_reference
    center, extent = shafts_reference.shadow_rect(np.asarray(sun, F), far_km)
    return (float(center[0]), float(center[1])), (float(extent[0]), float(extent[1]))


WIND = dict(offsets=(1.5, -2.25, 0.75, 3.5, 0.125, -0.375), time=12.5)      # cloud_pos, detailed_pos, weather_pos and time of scene B

# name -> sun, rect ("helper": aerial_shadow_rect(sun, 32), or (center, extent)), width, height, steps (0 = 64), weather ("shipped": cloud type all
# high; "stratus": R // 2, ct_mode 2; "white": white-noise weather with the shipped volumes, the mixed branch), coverage, density, wind,
# kinds = the number of (ordinary, chord, miss) texels the restatement finds, mixed = the number of 8 x 8 tiles that hold both of the first two.
SCENES = {
    "zenith":        dict(sun=(0, 1, 0), rect=((0.0, 0.0), (16384.0, 16384.0)), width=32, height=16, steps=17, weather="shipped", coverage=0.35, density=0.05, wind=False, kinds=(512, 0, 0), mixed=0),
    "deg45":         dict(sun=(1, 1, 0), rect=((1000.0, -3000.0), (9000.0, 3000.0)), width=37, height=5, steps=5, weather="stratus", coverage=0.5, density=0.05, wind=False, kinds=(185, 0, 0), mixed=0),
    "deg6":          dict(sun=(1, 0.1, 0), rect="helper", width=48, height=16, steps=32, weather="shipped", coverage=0.2, density=0.01, wind=False, kinds=(768, 0, 0), mixed=0),
    "deg2.7":        dict(sun=(1, 0.05, 0.3), rect="helper", width=48, height=16, steps=3, weather="shipped", coverage=0.2, density=0.01, wind=False, kinds=(768, 0, 0), mixed=0),
    "deg1.1":        dict(sun=(1, 0.02, 0), rect="helper", width=48, height=16, steps=32, weather="shipped", coverage=0.1, density=0.01, wind=True, kinds=(480, 288, 0), mixed=2),
    "deg1.1-n1":     dict(sun=(1, 0.02, 0), rect="helper", width=37, height=5, steps=1, weather="shipped", coverage=0.35, density=0.00002, wind=False, kinds=(115, 70, 0), mixed=1),
    "deg0.66-z":     dict(sun=(0.3, 0.012, 1), rect="helper", width=16, height=48, steps=17, weather="shipped", coverage=0.1, density=0.01, wind=True, kinds=(323, 415, 30), mixed=3),
    "deg0.66-str":   dict(sun=(0.3, 0.012, 1), rect="helper", width=16, height=48, steps=5, weather="stratus", coverage=0.3, density=0.001, wind=False, kinds=(323, 415, 30), mixed=3),
    "deg0.34":       dict(sun=(1, 0.006, 0), rect="helper", width=48, height=8, steps=0, weather="shipped", coverage=0.1, density=0.01, wind=False, kinds=(156, 218, 10), mixed=1),
    "deg1.1-white":  dict(sun=(1, 0.02, 0), rect="helper", width=48, height=16, steps=5, weather="white", coverage=0.1, density=0.01, wind=False, kinds=(480, 288, 0), mixed=2),
    "one-texel":     dict(sun=(1, 0.02, 0), rect=((-180000.0, 0.0), (2000.0, 2000.0)), width=1, height=1, steps=0, weather="shipped", coverage=0.1, density=0.01, wind=False, kinds=(0, 1, 0), mixed=0),
    "miss":          dict(sun=(-1, 0.364, 0), rect=((900000.0, 840000.0), (190000.0, 300000.0)), width=32, height=16, steps=5, weather="shipped", coverage=0.3, density=0.001, wind=False, kinds=(224, 18, 270), mixed=4),
}


def weather_map(weather, which):
    """The weather map of a scene, from the shipped one."""
    if which == "shipped":
        return weather
    if which == "stratus":                                          # test_stratus_only_weather_map: cloud type below 0.5 everywhere
        w2 = weather.copy()
        w2[..., 0] = w2[..., 0] // 2
        return w2
    assert which == "white"
    return np.random.default_rng(11).integers(0, 256, (512, 512, 3), dtype=np.uint8)


def sweep_scene(oracle, name):
    """(push-constant block, dict(width, height, center, extent, steps)) of a scene; steps as the C ABI takes it (0 = 64)."""
    s = SCENES[name]
    p = oracle.default_params(64, 32, s["sun"], coverage=s["coverage"], density=s["density"])
    if s["wind"]:
        p[4:10] = WIND["offsets"]
        p[23] = WIND["time"]
    center, extent = helper_rect(s["sun"]) if s["rect"] == "helper" else s["rect"]
    return p, dict(width=s["width"], height=s["height"], center=center, extent=extent, steps=s["steps"])


def tile_census(kind):
    """(ordinary, chord, miss) texel counts and the number of 8 x 8 tiles (a wavefront's texels) that hold both ordinary and chord texels."""
    H, W = kind.shape
    mixed = 0
    for j in range(0, H, 8):
        for i in range(0, W, 8):
            t = kind[j:j + 8, i:i + 8]
            mixed += bool((t == ORDINARY).any() and (t == CHORD).any())
    return (int((kind == ORDINARY).sum()), int((kind == CHORD).sum()), int((kind == MISS).sum())), mixed
