"""Numpy restatement of the aerial-perspective volume (include/cloudsky.h, "aerial-perspective volume").

TEST INFRASTRUCTURE ONLY, written from the contract's text and from the reference's GLSL as restated in oracle/numpy_restatement.py and
tests/tlut_reference.py (whose transmittance taps serve both mappings) -- not from csrc/aerial_core.h.

Positions, t, t_stop and the skip decision are evaluated in fp32 in the order the contract writes them, so that decisions agree with the core; the
per-step body is tlut_reference.sky_lut's, statement for statement.  Units km.
"""
import numpy as np

import tlut_reference as TR
from oracle import numpy_restatement as NR

f32 = np.float32
G_PI = f32(3.14159265358979323846)


# ----------------------------------------------------------------------------- column (i, j) -> EYEDIR
def _uv(W, H):
    i, j = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    return (i + f32(0.5)) / f32(W), (j + f32(0.5)) / f32(H)


def eyedir_panorama(W, H):
    """csky_composite_sky's panorama: u -> azimuth (2u-1) pi, v -> elevation (0.5-v) pi, e = (cos el cos az, sin el, cos el sin az).  [H, W, 3]"""
    u, v = _uv(W, H)
    az, el = (u * f32(2.0) - f32(1.0)) * G_PI, (f32(0.5) - v) * G_PI
    return np.stack([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)], -1).astype(f32)


def eyedir_view(W, H, basis, fov_y_degrees, aspect=0.0):
    """csky_composite_view's camera: pixel -> NDC -> view ray (x tan(fov/2) aspect, y tan(fov/2), -1) -> world through the basis columns
    (right, up, back) -> normalised.  basis: 3x3, columns = the camera's axes.  aspect 0 = W / H.  [H, W, 3]"""
    u, v = _uv(W, H)
    b = np.asarray(basis, f32)
    th = np.tan(f32(fov_y_degrees) * f32(0.5) * G_PI / f32(180.0)).astype(f32)
    asp = f32(W) / f32(H) if aspect == 0 else f32(aspect)
    vx, vy, vz = (u * f32(2.0) - f32(1.0)) * th * asp, (f32(1.0) - v * f32(2.0)) * th, f32(-1.0)
    w = [b[k, 0] * vx + b[k, 1] * vy + b[k, 2] * vz for k in range(3)]
    l = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    return np.stack([w[0] / l, w[1] / l, w[2] / l], -1).astype(f32)


def camera_basis(yaw_degrees, pitch_degrees):
    """A camera looking along -z, yawed about y then pitched about its own x axis (positive = up): 3x3, columns right / up / back."""
    y, p = np.radians(yaw_degrees), np.radians(pitch_degrees)
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    return (ry @ rx).astype(f32)


# ----------------------------------------------------------------------------- the volume
def tap_for(mapping, trans):
    """tap(cos, radius, normalised altitude) of tlut_reference.sky_lut for a table of `mapping`."""
    T = np.asarray(trans).astype(f32)
    if mapping == TR.BRUNETON:
        return lambda c, r, nalt: TR.lookup_bruneton(T, r, c)
    return lambda c, r, nalt: NR.tex2d(T, np.stack([NR.clamp(c * f32(0.5) + f32(0.5), 0, 1), NR.clamp(nalt, 0, 1)], -1), repeat=False)


def columns(e, sun, far_km, D, S, trans, mapping=TR.REFERENCE):
    """The columns of EYEDIRs e [..., 3] (fp32), reach far_km (a scalar or one per column), D slices of S steps, sun used as given.
    Returns a dict: out float16 [D, ..., 4]; L float32 [D, ..., 4] the spectral in-scattering behind every slice; t_stop [...]; taken [...] the
    steps taken; near [...] True where some step midpoint lies within 1e-4 dt of t_stop (the skip decision is fp32-fragile there)."""
    e = np.asarray(e, f32)
    sun = NR.F(sun)
    tap = tap_for(mapping, trans)
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
            t_sun = tap(sc, d, nalt)
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
        if (i + 1) % S == 0:
            k = (i + 1) // S - 1
            rgb = NR.M[0] * L[..., 0:1] + NR.M[1] * L[..., 1:2] + NR.M[2] * L[..., 2:3] + NR.M[3] * L[..., 3:4]
            a = (((Tr[..., 0] + Tr[..., 1]) + Tr[..., 2]) + Tr[..., 3]) * f32(0.25)
            out[k] = np.concatenate([rgb, a[..., None]], -1).astype(np.float16)
            Ls[k] = L
    return dict(out=out, L=Ls, t_stop=t_stop, taken=taken, near=near)


def volume(W, H, D, S, far_km, sun, trans, mapping=TR.REFERENCE, view=None, aspect=0.0):
    """The W x H x D volume: view None = the panorama, or (basis, fov_y_degrees)."""
    e = eyedir_panorama(W, H) if view is None else eyedir_view(W, H, view[0], view[1], aspect)
    return columns(e, sun, far_km, D, S, trans, mapping)


# ----------------------------------------------------------------------------- the sky LUT's texels as world directions
def sky_texel_eyedir(px, py, w=200, h=100):
    """The world direction e = (-cos el cos az, sin el, -cos el sin az) of sky-LUT texels (sky-lut.glsl:284-297), and their LUT-frame ray."""
    px, py = np.asarray(px, f32), np.asarray(py, f32)
    uvx, uvy = px / f32(w), py / f32(h)
    az = f32(2.0 * NR.S_PI) * uvx
    l = uvy * f32(2.0) - f32(1.0)
    el = l * l * np.sign(l) * f32(NR.S_PI) * f32(0.5)
    e = np.stack([-(np.cos(el) * np.cos(az)), np.sin(el), -(np.cos(el) * np.sin(az))], -1).astype(f32)
    return e


def ray_length(e):
    """t_d of the ray along EYEDIR e from the observer (sky-lut.glsl:299-309)."""
    e = np.asarray(e, f32)
    rd = np.stack([-e[..., 0], -e[..., 2], e[..., 1]], -1)
    ro = np.broadcast_to(NR.F([0, 0, 6371.5]), rd.shape)
    atmos = NR.ray_sphere_intersection(ro, rd, NR.ATMOSPHERE_RADIUS)
    ground = NR.ray_sphere_intersection(ro, rd, NR.EARTH_RADIUS)
    return np.where(ground < 0, atmos, ground).astype(f32), ground >= 0


# ----------------------------------------------------------------------------- the gate
def half_steps(a):
    """fp16 values on a monotone integer scale (steps of one ulp, +0 = -0 = 0): differences count ulps across zero too."""
    b = np.ascontiguousarray(a).view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def ulp_dist(a, b):
    return np.abs(half_steps(a) - half_steps(b))


def half_ulp_of(x):
    """The size of one fp16 ulp at magnitude |x| (float64)."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(x)) - 10)


def gate(test, ref, L_test=None, L_ref=None, keep=None, what=""):
    """The sky-LUT gate: every half within 1 fp16 ulp.  A half outside it passes only as cancellation in M * L: the spectral L of both sides (when
    given) agree to 1e-5 relative and the half is within 1 ulp of the texel's LARGEST channel.  keep: columns [...] that count.
    Returns (halves that differ, halves let through as cancellation)."""
    d = ulp_dist(test, ref)
    if keep is not None:
        d = np.where(keep[None, ..., None], d, 0)
    bad = d > 1
    n_cancel = 0
    if bad.any():
        assert L_test is not None and L_ref is not None, "%s: %d halves outside 1 fp16 ulp (max %d)" % (what, int(bad.sum()), int(d.max()))
        assert not bad[..., 3].any(), "%s: alpha outside 1 fp16 ulp" % what
        rel = np.abs(L_test.astype(np.float64) - L_ref) / np.maximum(np.abs(L_ref).max(-1, keepdims=True), 1e-30)
        tex = bad.any(-1)
        assert (rel[tex] <= 1e-5).all(), "%s: halves outside the gate whose spectral L differs by %.3g relative" % (what, rel[tex].max())
        a, b = np.asarray(test).astype(np.float64), np.asarray(ref).astype(np.float64)
        big = half_ulp_of(np.abs(b[..., :3]).max(-1, keepdims=True))
        assert (np.abs(a - b)[..., :3][bad[..., :3]] <= np.broadcast_to(big, bad[..., :3].shape)[bad[..., :3]]).all(), "%s: outside 1 ulp of the largest channel" % what
        n_cancel = int(bad.sum())
    return int((d > 0).sum()), n_cancel
