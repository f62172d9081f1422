"""Numpy restatement of the Bruneton parametrization of the transmittance LUT (cloudsky.h CSKY_TLUT_BRUNETON).

TEST INFRASTRUCTURE ONLY, written from the formulas of the feature's specification (Bruneton 2017, `GetTransmittanceTextureUvFromRMu` and its
inverse) and from the reference's GLSL as restated in oracle/numpy_restatement.py -- not from csrc/tlut_core.h.

  * the mapping both ways and the ground-hit test in float64 from fp32 inputs, rounded to fp32 once (the precision rule of the mode: tap
    coordinates and hit decisions are then reproducible, no tolerance needed);
  * the mapping-1 LUT integrated the way numpy_restatement.transmittance_lut integrates the reference's (fp32 arrays, GLSL order, 40 steps);
  * truth: point evaluation / tables in float64 with many midpoint steps; a ray that meets the ground is blocked (transmittance 0);
  * bilinear CLAMP look-ups in both mappings; the sky LUT of numpy_restatement.sky_lut with its transmittance tap replaced.
Units km.
"""
import numpy as np

from oracle import numpy_restatement as NR

f32 = np.float32
RG, RT = 6371.0, 6471.0
H2 = RT * RT - RG * RG
H = np.sqrt(H2)
REFERENCE, BRUNETON = 0, 1


# ----------------------------------------------------------------------------- the mapping (float64)
def clamp_inputs(r, mu):
    """fp32 (r, mu) as a caller holds them -> float64, clamped to [Rg, Rt] x [-1, 1]."""
    r = np.clip(np.asarray(r, f32).astype(np.float64), RG, RT)
    mu = np.clip(np.asarray(mu, f32).astype(np.float64), -1.0, 1.0)
    return r, mu


def hits_ground(r, mu):
    r, mu = clamp_inputs(r, mu)
    return (mu < 0.0) & (r * r * (mu * mu - 1.0) + RG * RG >= 0.0)


def uv_exact(r, mu, w, h):
    """(r, mu) float64, already clamped -> (u, v) float64."""
    rho = np.sqrt(np.maximum((r - RG) * (r + RG), 0.0))
    d = np.maximum(-r * mu + np.sqrt(np.maximum(r * r * (mu * mu - 1.0) + RT * RT, 0.0)), 0.0)
    d_min, d_max = RT - r, rho + H
    x_mu = np.clip((d - d_min) / (d_max - d_min), 0.0, 1.0)
    x_r = rho / H
    return 0.5 / w + x_mu * (1.0 - 1.0 / w), 0.5 / h + x_r * (1.0 - 1.0 / h)


def uv(r, mu, w, h):
    """What a reader computes: fp32 (r, mu) in, fp32 (u, v) out (rounded once), and the hit decision."""
    rc, mc = clamp_inputs(r, mu)
    u, v = uv_exact(rc, mc, w, h)
    return u.astype(f32), v.astype(f32), hits_ground(r, mu)


def texel_ray_exact(w, h):
    """float64 (r, mu, d) [h, w] of the rays a w x h table stores."""
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x_mu, x_r = px / (w - 1), py / (h - 1)
    rho = H * x_r
    r = np.sqrt(rho * rho + RG * RG)
    d_min, d_max = RT - r, rho + H
    d = d_min + x_mu * (d_max - d_min)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(d == 0.0, 1.0, np.clip((H2 - rho * rho - d * d) / (2.0 * r * d), -1.0, 1.0))
    return r, mu, d


def texel_ray(w, h):
    r, mu, d = texel_ray_exact(w, h)
    return r.astype(f32), mu.astype(f32), d.astype(f32)


# ----------------------------------------------------------------------------- the 40-step fp32 LUT, as the GLSL would integrate it
def transmittance_lut(w=256, h=64, steps=40):
    """numpy_restatement.transmittance_lut (T:157-196) with the texel's ray from the mapping: from (0, 0, r) along (-sqrt(1 - mu^2), 0, mu)
    over the texel's own d."""
    r, mu, d = texel_ray(w, h)
    sun_dir = np.stack([-np.sqrt(f32(1.0) - mu * mu), np.zeros_like(mu), mu], -1)
    ro = np.stack([np.zeros_like(r), np.zeros_like(r), r], -1)
    dt = d / f32(steps)
    result = np.zeros((h, w, 4), f32)
    for i in range(steps):
        t = (f32(i) + f32(0.5)) * dt
        x_t = ro + sun_dir * t[..., None]
        alt = NR.length(x_t) - NR.EARTH_RADIUS
        _, _, ext = NR.collision_coefficients(alt)
        result = result + ext * dt[..., None]
    return np.exp(-result).astype(np.float16)


# ----------------------------------------------------------------------------- look-ups (fp32 bilinear CLAMP taps of fp16 tables)
def lookup_reference(T, r, mu):
    """transmittance_from_lut (S:137-142) at radius r: the normalised altitude as sky-lut.glsl derives it."""
    T = np.asarray(T).astype(f32)
    r, mu = np.asarray(r, f32), np.asarray(mu, f32)
    nalt = (r - NR.EARTH_RADIUS) / NR.ATMOSPHERE_THICKNESS
    u = NR.clamp(mu * f32(0.5) + f32(0.5), 0, 1)
    v = NR.clamp(nalt, 0, 1)
    return NR.tex2d(T, np.stack([u, v], -1), repeat=False)


def lookup_bruneton(T, r, mu):
    T = np.asarray(T).astype(f32)
    h, w = T.shape[:2]
    u, v, hit = uv(r, mu, w, h)
    t = NR.tex2d(T, np.stack([u, v], -1), repeat=False)
    return np.where(hit[..., None], f32(0.0), t).astype(f32)


# ----------------------------------------------------------------------------- truth (float64)
_AER = np.array([2.8722e-24, 4.6168e-24, 7.9706e-24, 1.3578e-23]) + np.array([1.5908e-22, 1.7711e-22, 2.0942e-22, 2.4033e-22])
_MOL = np.array([6.605e-3, 1.067e-2, 1.842e-2, 3.156e-2])
_OZ = np.array([3.472e-21, 3.914e-21, 1.349e-21, 11.03e-23]) * 1e-4 * 350.0


def extinction64(alt):
    alt = np.maximum(alt, 0.0)
    aer = 1.3681e20 * (np.exp(-alt / 0.73) + 2e6 / 1.3681e20)
    h2 = alt + 1e-4
    t = np.log(h2) - 3.22261
    oz = 3.78547397e20 / h2 * np.exp(-t * t * 5.55555555)
    mol = np.exp(-0.07771971 * np.power(alt, 1.16364243))
    return _AER * aer[..., None] + _OZ * oz[..., None] + _MOL * mol[..., None]


def transmittance_point(r, mu, steps=4000, block_ground=True):
    """Transmittance from radius r along zenith cosine mu to the top of the atmosphere, midpoint rule in float64, evaluated at the fp32 pair
    the query holds.  block_ground: a ray that meets the ground has transmittance 0 (the mode's choice)."""
    rc, mc = clamp_inputs(r, mu)
    d = np.maximum(-rc * mc + np.sqrt(np.maximum(rc * rc * (mc * mc - 1.0) + RT * RT, 0.0)), 0.0)
    s = np.sqrt(np.maximum(1.0 - mc * mc, 0.0))
    dt = d / steps
    acc = np.zeros(rc.shape + (4,))
    for i in range(steps):
        t = (i + 0.5) * dt
        x, z = -s * t, rc + mc * t
        acc += extinction64(np.sqrt(x * x + z * z) - RG) * dt[..., None]
    out = np.exp(-acc)
    if block_ground:
        out = np.where(hits_ground(r, mu)[..., None], 0.0, out)
    return out


def transmittance_table64(w, h, steps):
    """A mapping-1 table from float64 rays and float64 integration, stored as fp16 like every table."""
    r, mu, d = texel_ray_exact(w, h)
    s = np.sqrt(np.maximum(1.0 - mu * mu, 0.0))
    dt = d / steps
    acc = np.zeros((h, w, 4))
    for i in range(steps):
        t = (i + 0.5) * dt
        x, z = -s * t, r + mu * t
        acc += extinction64(np.sqrt(x * x + z * z) - RG) * dt[..., None]
    return np.exp(-acc).astype(np.float16)


# ----------------------------------------------------------------------------- the accuracy claim's query grid
QUERY_RADII = (6371.0, 6371.2, 6371.5, 6372.0, 6373.5, 6376.0, 6381.0, 6391.0, 6411.0, 6441.0, 6465.0)


def query_grid(near_horizon):
    """(r, mu) fp32 [11, 401]: mu = mu_h + delta, delta in [0, 0.1] (near the horizon) or mu_h + delta (1 - mu_h), delta in [0.1, 1]."""
    rs = np.array(QUERY_RADII)
    deltas = np.linspace(0.0, 0.1, 401) if near_horizon else np.linspace(0.1, 1.0, 401)
    R, D = np.meshgrid(rs, deltas, indexing="ij")
    mu_h = -np.sqrt(1.0 - (RG / R) ** 2)
    MU = np.minimum(mu_h + D if near_horizon else mu_h + D * (1.0 - mu_h), 1.0)
    return R.astype(f32), MU.astype(f32)


# ----------------------------------------------------------------------------- the sky LUT with its transmittance tap replaced
def sky_lut(sun, tap, w=200, h=100):
    """numpy_restatement.sky_lut (S:278-315), statement for statement, with `tap(cos, radius, normalised altitude)` in place of its
    transmittance look-up: the radius is the sample's own distance from the planet's centre, or the ground's."""
    sun = NR.F(sun)
    px, py = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    uvx, uvy = px / f32(w), py / f32(h)
    az = f32(2.0 * NR.S_PI) * uvx
    l = uvy * f32(2.0) - f32(1.0)
    elev = l * l * np.sign(l) * f32(NR.S_PI) * f32(0.5)
    rd = np.stack([np.cos(elev) * np.cos(az), np.cos(elev) * np.sin(az), np.sin(elev)], -1).astype(f32)
    ro = np.broadcast_to(NR.F([0, 0, 6371.5]), rd.shape)
    atmos = NR.ray_sphere_intersection(ro, rd, NR.ATMOSPHERE_RADIUS)
    ground = NR.ray_sphere_intersection(ro, rd, NR.EARTH_RADIUS)
    t_d = np.where(ground < 0, atmos, ground)
    sd = NR.F([-sun[0], -sun[2], sun[1]])
    cos_theta = NR.dot(-rd, sd)
    mol_phase = f32((3.0 / 16.0) / NR.S_PI) * (f32(1.0) + cos_theta * cos_theta)
    den = f32(1.0 + 0.64) + f32(1.6) * cos_theta
    aer_phase = f32(0.25 / NR.S_PI) * (f32(1.0) - f32(0.64)) / (den * np.sqrt(den))
    dt = t_d / f32(30.0)
    L = np.zeros((h, w, 4), f32)
    Tr = np.ones((h, w, 4), f32)
    for i in range(30):
        t = (f32(i) + f32(0.5)) * dt
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
        S = NR.SUN_IRR * (msc * (mol_phase[..., None] * t_sun + ms) + asc * (aer_phase[..., None] * t_sun + ms))
        stepT = np.exp(-dt[..., None] * ext)
        S_int = (S - S * stepT) / np.maximum(ext, f32(1e-7))
        L = L + Tr * S_int
        Tr = Tr * stepT
    rgb = NR.M[0] * L[..., 0:1] + NR.M[1] * L[..., 1:2] + NR.M[2] * L[..., 2:3] + NR.M[3] * L[..., 3:4]
    return np.concatenate([rgb, np.ones((h, w, 1), f32)], -1).astype(np.float16)


def sky_lut_bruneton(sun, trans, w=200, h=100):
    T = np.asarray(trans).astype(f32)
    return sky_lut(sun, lambda c, r, nalt: lookup_bruneton(T, r, c), w, h)


def sky_lut_reference(sun, trans, w=200, h=100):
    T = np.asarray(trans).astype(f32)

    def tap(c, r, nalt):
        return NR.tex2d(T, np.stack([NR.clamp(c * f32(0.5) + f32(0.5), 0, 1), NR.clamp(nalt, 0, 1)], -1), repeat=False)
    return sky_lut(sun, tap, w, h)


SUNS = {"zenith": (0.0, 1.0, 0.0), "deg45": (1.0, 1.0, 0.0), "demo": (-0.998773, 0.0495291, 2.69869e-07),
        "deg0p5": (np.cos(np.radians(0.5)), np.sin(np.radians(0.5)), 0.0), "degm2": (np.cos(np.radians(-2.0)), np.sin(np.radians(-2.0)), 0.0)}


def norm(s):
    s = np.asarray(s, np.float64)
    return (s / np.linalg.norm(s)).astype(f32)
