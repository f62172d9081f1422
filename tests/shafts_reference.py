"""Numpy restatement of the shadowed aerial-perspective volume (include/cloudsky.h, "light shafts").

TEST INFRASTRUCTURE ONLY, written from the contract's text -- not from csrc/shafts_core.h.  The column loop is tests/aerial_reference.py's, statement
for statement, with the one product the contract adds (t_sun' = t_sun * s); the factor s is evaluated in fp32 in the order the contract writes it,
so that its decisions (above the layer, out of the rectangle, which texels) agree with the core.  Units: km in the LUT frame, metres in the map's.
"""
import numpy as np

import aerial_reference as AR
import tlut_reference as TR
from oracle import numpy_restatement as NR

f32 = np.float32


def synthetic_map():
    """The issue's map M: 24 x 16 texels, (i, j) -> 0.25 where (i // 3 + j // 2) is even, else 1.0; with its center and extent."""
    i, j = np.meshgrid(np.arange(24), np.arange(16))
    return np.where((i // 3 + j // 2) % 2 == 0, 0.25, 1.0).astype(np.float16), (4000.0, -2000.0), (48000.0, 32000.0)


def sun_unit(sun):
    s = np.asarray(sun, f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        ll = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        return (s / ll).astype(f32)


def factor(x, y, altitude, l, shadow, center, extent):
    """The step factor s of the contract for steps at (x, y) km of the LUT frame, `altitude` km up.  shadow: float16 [H, W].
    Returns (s, info): info has h, gx, gz (float32), m (the filtered value, NaN where nothing was tapped) and tapped (bool)."""
    x, y, altitude = np.asarray(x, f32), np.asarray(y, f32), np.asarray(altitude, f32)
    one = np.ones(x.shape, f32)
    h = altitude * f32(1000.0)
    nothing = dict(h=h, gx=np.zeros(x.shape, f32), gz=np.zeros(x.shape, f32), m=np.full(x.shape, np.nan, f32), tapped=np.zeros(x.shape, bool))
    if not (l[1] > 0):
        return one, nothing
    T = np.asarray(shadow, np.float16).astype(f32)
    H, W = T.shape
    cx, cz, ex, ez = f32(center[0]), f32(center[1]), f32(extent[0]), f32(extent[1])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        wx, wz = -x * f32(1000.0), -y * f32(1000.0)
        below = ~(h >= f32(4000.0))
        k = h / l[1]
        gx, gz = wx - l[0] * k, wz - l[2] * k
        u, v = (gx - cx) / ex + f32(0.5), (gz - cz) / ez + f32(0.5)
        fx, fy = u * f32(W) - f32(0.5), v * f32(H) - f32(0.5)
        inside = (fx >= f32(-1.0)) & (fx < f32(W)) & (fy >= f32(-1.0)) & (fy < f32(H))
        tapped = below & inside
        fxs, fys = np.where(tapped, fx, f32(0.0)), np.where(tapped, fy, f32(0.0))     # no conversion to int of anything outside the test
        fi, fj = np.floor(fxs), np.floor(fys)
        ax, ay = fxs - fi, fys - fj
        i0, j0 = fi.astype(np.int64), fj.astype(np.int64)

        def tap(i, j):
            ok = (i >= 0) & (i < W) & (j >= 0) & (j < H)
            return np.where(ok, T[np.clip(j, 0, H - 1), np.clip(i, 0, W - 1)], f32(1.0)).astype(f32)

        def lerp(a, b, w):
            return a + (b - a) * w

        m = lerp(lerp(tap(i0, j0), tap(i0 + 1, j0), ax), lerp(tap(i0, j0 + 1), tap(i0 + 1, j0 + 1), ax), ay)
        w = np.minimum(np.maximum((h - f32(1500.0)) / f32(2500.0), f32(0.0)), f32(1.0))
        s = np.where(tapped, m + (f32(1.0) - m) * w, one).astype(f32)
    return s, dict(h=h, gx=np.where(below, gx, f32(0.0)), gz=np.where(below, gz, f32(0.0)), m=np.where(tapped, m, f32(np.nan)), tapped=tapped)


def columns(e, sun, far_km, D, S, trans, shadow, center, extent, mapping=TR.REFERENCE):
    """aerial_reference.columns with the shadow map inside.  Returns its dict (out, L, t_stop, taken, near) and, per step [n, ...]: take (the step
    is taken), s, h, gx, gz, m, tapped."""
    e = np.asarray(e, f32)
    sun = NR.F(sun)
    l = sun_unit(sun)
    tap = AR.tap_for(mapping, trans)
    shape = e.shape[:-1]
    rd = np.stack([-e[..., 0], -e[..., 2], e[..., 1]], -1)
    ro = np.broadcast_to(NR.F([0, 0, 6371.5]), rd.shape)
    sd = NR.F([-sun[0], -sun[2], sun[1]])
    atmos = NR.ray_sphere_intersection(ro, rd, NR.ATMOSPHERE_RADIUS)
    ground = NR.ray_sphere_intersection(ro, rd, NR.EARTH_RADIUS)
    t_stop = np.where(ground < 0, atmos, ground).astype(f32)
    n = D * S
    dt = (np.broadcast_to(np.asarray(far_km, f32), shape) / f32(n)).astype(f32)
    cos_theta = NR.dot(-rd, sd)
    mol_phase = f32((3.0 / 16.0) / NR.S_PI) * (f32(1.0) + cos_theta * cos_theta)
    den = f32(1.0 + 0.64) + f32(1.6) * cos_theta
    aer_phase = f32(0.25 / NR.S_PI) * (f32(1.0) - f32(0.64)) / (den * np.sqrt(den))
    L = np.zeros(shape + (4,), f32)
    Tr = np.ones(shape + (4,), f32)
    taken = np.zeros(shape, np.int64)
    near = np.zeros(shape, bool)
    out = np.zeros((D,) + shape + (4,), np.float16)
    Ls = np.zeros((D,) + shape + (4,), f32)
    per = {k: [] for k in ("take", "s", "h", "gx", "gz", "m", "tapped")}
    for i in range(n):
        t = (f32(i) + f32(0.5)) * dt
        take = ~(t >= t_stop)
        near |= np.abs(t.astype(np.float64) - t_stop.astype(np.float64)) <= 1e-4 * dt.astype(np.float64)
        taken += take
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):       # skipped steps lie under the ground or outside: computed, then discarded
            x_t = ro + rd * t[..., None]
            d = NR.length(x_t)
            zen = x_t / d[..., None]
            alt = d - NR.EARTH_RADIUS
            nalt = alt / NR.ATMOSPHERE_THICKNESS
            sc = NR.dot(zen, sd)
            asc, msc, ext = NR.collision_coefficients(alt)
            one, zero, rg = np.ones_like(sc), np.zeros_like(sc), np.full_like(sc, NR.EARTH_RADIUS)
            s, info = factor(x_t[..., 0], x_t[..., 1], alt, l, shadow, center, extent)
            t_sun = (tap(sc, d, nalt) * s[..., None]).astype(f32)                 # the one product
            omega = f32(2.0 * NR.S_PI) * (f32(1.0) - np.sqrt(d * d - NR.EARTH_RADIUS * NR.EARTH_RADIUS) / d)
            T_to_ground = tap(sc, rg, zero)
            T_g2s = tap(one, rg, zero) / tap(one, d, nalt)
            L_ground = (f32(0.25 / NR.S_PI) * omega * f32(0.3 / NR.S_PI))[..., None] * T_to_ground * T_g2s * sc[..., None]
            L_ms = NR.F([0.02 * 0.217, 0.02 * 0.347, 0.02 * 0.594, 0.02]) * (f32(1.0) / (f32(1.0) + f32(5.0) * np.exp(f32(-17.92) * sc)))[..., None]
            ms = L_ms + L_ground
            Src = NR.SUN_IRR * (msc * (mol_phase[..., None] * t_sun + ms) + asc * (aer_phase[..., None] * t_sun + ms))
            stepT = np.exp(-dt[..., None] * ext)
            S_int = (Src - Src * stepT) / np.maximum(ext, f32(1e-7))
            L = np.where(take[..., None], L + Tr * S_int, L).astype(f32)
            Tr = np.where(take[..., None], Tr * stepT, Tr).astype(f32)
        per["take"].append(take)
        per["s"].append(s)
        for k in ("h", "gx", "gz", "m", "tapped"):
            per[k].append(info[k])
        if (i + 1) % S == 0:
            k = (i + 1) // S - 1
            rgb = NR.M[0] * L[..., 0:1] + NR.M[1] * L[..., 1:2] + NR.M[2] * L[..., 2:3] + NR.M[3] * L[..., 3:4]
            a = (((Tr[..., 0] + Tr[..., 1]) + Tr[..., 2]) + Tr[..., 3]) * f32(0.25)
            out[k] = np.concatenate([rgb, a[..., None]], -1).astype(np.float16)
            Ls[k] = L
    r = dict(out=out, L=Ls, t_stop=t_stop, taken=taken, near=near)
    r.update({k: np.stack(v) for k, v in per.items()})
    return r


def volume(W, H, D, S, far_km, sun, trans, shadow, center, extent, mapping=TR.REFERENCE, view=None, aspect=0.0):
    """The W x H x D volume with the shadow map inside: view None = the panorama, or (basis, fov_y_degrees)."""
    e = AR.eyedir_panorama(W, H) if view is None else AR.eyedir_view(W, H, view[0], view[1], aspect)
    return columns(e, sun, far_km, D, S, trans, shadow, center, extent, mapping)


def shadow_rect(sun, far_km):
    """csky_aerial_shadow_rect by the contract's text: (center, extent) float32 pairs, or None where it reports an error."""
    l = sun_unit(sun)
    if not (l[1] > 0):
        return None
    k = f32(4000.0) / l[1]
    shift = np.array([-l[0] * k, -l[2] * k], f32)
    center, extent = shift * f32(0.5), f32(2.0) * (f32(far_km) * f32(1000.0)) + np.abs(shift)
    if ((np.abs(center) + extent * f32(0.5)) > f32(1.0e6)).any():
        return None
    return center, extent
