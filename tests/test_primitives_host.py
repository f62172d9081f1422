"""The march's arithmetic primitives on the HOST build (csrc/primitives_core.h through tests/hostsim: the `#else` branches), held against numpy,
and the input sets tests/test_gpu_primitives.py runs through the device forms of the same functions.

On the host split_coord is floorf and a subtraction, lerp_h one correctly rounded fmaf, lerp_h2 two of them, f2h_normal the software f2h, the
divide and the square root the compiler's IEEE ones: the definitions the comments in cloud_core.h appeal to when they call a device form "the same
value".  These tests check those definitions themselves, so that what the GPU tests compare the device with is known to be right on this machine:
    floor / subtract in float32, astype(float16) for the half, and for the lerp the round-to-nearest-even float32 of the EXACT a + d f.
The exact lerp is `fma32`: the float64 product of two float32 is exact, the float64 sum is made exact by carrying its error term (two-sum), the
pair is rounded to odd and then to float32 -- a single rounding of the exact value.  It is checked against `fractions` on a few ten thousand cases.

The input generators are seeded and cached: a set is built once per session, whoever asks first."""
import ctypes
import functools
from fractions import Fraction

import numpy as np

import ray_reference as RAY

F, U, I = np.float32, np.uint32, np.int32
RAY_FRAMES = ((64, 32), (200, 104), (1000, 500))
RAY_STEPS = (1, 32, 100, 128, 1024)
RAY_FIELDS = ("px", "py", "pz", "ss", "dx", "dy", "dz", "sx", "sy", "sz")
TAP_SIZES = (1, 2, 4, 8, 16, 32, 64, 128, 512)                  # cells per side of every level the three taps address
SQRT_EXACT_MIN = F(2.0 ** -102)                                 # cloud_core.h: sqrt_exact is specified from here up
LERP_F_SPECIAL = (0.0, 2.0 ** -25, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0)


def bits(x):
    return np.ascontiguousarray(x, F).view(U)


def fl(b):
    return np.ascontiguousarray(b, U).view(F)


def step(x, d):
    """The float32 d ulp32 away from x (d an int): one step is the next float in that direction; -0 counts as +0."""
    b = bits(x).astype(np.int64)
    key = np.where(b >= 0x80000000, -(b & 0x7fffffff), b) + d
    return fl(np.where(key < 0, 0x80000000 | -key, key).astype(U))


def with_neighbours(x, k=2):
    x = np.ascontiguousarray(x, F).reshape(-1)
    return np.concatenate([step(x, d) for d in range(-k, k + 1)])


def is_normal(x):
    a = np.abs(x)
    return np.isfinite(x) & (a >= F(2.0 ** -126))


def host_primitive(hostsim, op, *arrays):
    from gvcd_amd._lib import run_primitive

    def call(code, *a):
        assert hostsim.hostsim_primitive(code, *a[:5], ctypes.c_size_t(a[5])) == 0
    return run_primitive(call, op, arrays)


def first_diff(got, ref, *inputs):
    """'' when the bit patterns agree, else the count and the first differing input (hex patterns)."""
    g, r = np.ascontiguousarray(got).view(U if got.dtype.itemsize == 4 else np.uint16), np.ascontiguousarray(ref).view(U if ref.dtype.itemsize == 4 else np.uint16)
    bad = np.flatnonzero((g != r).reshape(len(g), -1).any(axis=1)) if g.ndim > 1 else np.flatnonzero(g != r)
    if not bad.size:
        return ""
    k = int(bad[0])
    return "%d of %d differ; first at #%d: in %s got %s want %s" % (bad.size, len(g), k, [np.ascontiguousarray(x)[k].tobytes().hex() for x in inputs],
                                                                     np.atleast_1d(g[k]).tolist(), np.atleast_1d(r[k]).tolist())


# ---------------------------------------------------------------------------------------------------------------- exact fma
def fma32(a, b, c):
    """The correctly rounded float32 of the exact a * b + c, float32 arrays (finite; |values| far inside float64's range)."""
    with np.errstate(all="ignore"):                              # (inf and NaN operands give what they give: the callers mask them)
        a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
        p = a * b                                                # 24 x 24 bits: exact
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)                            # two-sum: s + err == p + c exactly
        sb = np.ascontiguousarray(s).view(np.int64)
        toward = np.where((err > 0) == (s > 0), 1, -1)           # the neighbour of s on err's side, as a step of the bit pattern
        sb = np.where((err != 0) & ((sb & 1) == 0), sb + toward, sb)   # round to odd: the exact value lies strictly between s and that neighbour
        return np.ascontiguousarray(sb).view(np.float64).astype(F)     # 53 >= 24 + 2 bits: rounding the odd-rounded value rounds the exact one


def _half(u16):
    return np.ascontiguousarray(u16, np.uint16).view(np.float16).astype(F)


def lerp_h_exact(pair, f):
    return fma32(_half(pair >> 16), f, _half(pair & 0xffff))


def lerp_h2_two_step(pair, f):
    lo, hi = _half(pair & 0xffff), _half(pair >> 16)
    return fma32(hi, f, fma32(lo, -np.asarray(f, F), lo))


# ---------------------------------------------------------------------------------------------------------------- input sets
@functools.lru_cache(None)
def ray_cases():
    """Directions, step counts, the reference's rays and the operands of every sqrt and divide of the set-up.  Directions: every pixel of RAY_FRAMES
    plus the 32 grazing directions of test_clouds_rays_host's H4, each at every count of RAY_STEPS.  Operands are recorded for the pixel directions
    and for the rays at 100 and 128 steps (the other counts change the two divisions by the count alone)."""
    rec = {"sqrt": [], "div": []}
    dirs = [RAY.pixel_dirs(w, h, rec).reshape(-1, 3) for w, h in RAY_FRAMES]
    graze = []
    for y in (1e-7, 1e-5, 1e-3, 0.05):
        for k in range(8):
            az = 2.0 * np.pi * (k + 0.3) / 8.0
            c = np.sqrt(1.0 - y * y)
            graze.append([c * np.cos(az), y, c * np.sin(az)])
    e = np.ascontiguousarray(np.concatenate(dirs + [np.asarray(graze, F)]), F)
    out, steps = [], []
    for n in RAY_STEPS:
        r = RAY.ray(e, n, rec if n in (100, 128) else None)
        out.append(np.concatenate([r["p"], r["ss"][:, None], r["dir"], r["inc"]], axis=1))
        steps.append(np.full(len(e), n, F))
    pix = []
    for w, h in RAY_FRAMES:
        j, i = np.mgrid[0:h, 0:w]
        pix.append(np.stack([i.ravel(), j.ravel(), np.full(i.size, w), np.full(i.size, h)], 1))
    pix = np.concatenate(pix)
    sq = np.concatenate(rec["sqrt"])
    da, db = np.concatenate([a for a, _ in rec["div"]]), np.concatenate([b for _, b in rec["div"]])
    return dict(e=np.tile(e, (len(RAY_STEPS), 1)), steps=np.concatenate(steps), ref=np.concatenate(out).astype(F), n_dirs=len(e), n_graze=len(graze),
                pix_ij=pix[:, :2].astype(I), pix_wh=pix[:, 2:].astype(F), pix_ref=np.concatenate(dirs), sqrt_ops=sq, div_ops=(da, db))


@functools.lru_cache(None)
def sqrt_binades():
    return fl(np.arange(0x3f800000, 0x40800000, dtype=U))        # every float in [1, 4)


@functools.lru_cache(None)
def sqrt_edges():
    """Per exponent -126..127 the mantissas 0, 1, 0x7ffffe, 0x7fffff and 4096 random ones; then the ray set-up's own (normal, positive) operands."""
    rng = np.random.default_rng(20)
    man = np.concatenate([np.tile(np.array([0, 1, 0x7ffffe, 0x7fffff], U), (254, 1)), rng.integers(0, 1 << 23, (254, 4096), dtype=U)], axis=1)
    x = fl(((np.arange(1, 255, dtype=U)[:, None] << 23) | man).reshape(-1))
    ops = ray_cases()["sqrt_ops"]
    ops = ops[is_normal(ops) & (ops > 0)]
    return np.concatenate([x, ops])


def sqrt_unspecified():
    return np.array([0.0, -0.0, 1e-45, 2.0 ** -127, 1.1754942e-38, np.inf, np.nan, -1.0], F)


@functools.lru_cache(None)
def div_pairs():
    """2^20 random normal pairs; quotients within 2 ulp of a power of two; the ray set-up's operand pairs.  Every operand and quotient is zero or normal."""
    rng = np.random.default_rng(21)

    def rnd(n):
        return fl((rng.integers(0, 2, n, dtype=U) << 31) | (rng.integers(127 - 60, 127 + 61, n, dtype=U) << 23) | rng.integers(0, 1 << 23, n, dtype=U))
    a, b = rnd(1 << 20), rnd(1 << 20)
    nb = 1 << 16
    b2 = np.repeat(rnd(nb), 5)
    q = np.concatenate([step(fl((rng.integers(127 - 20, 127 + 21, nb, dtype=U) << 23)), d) for d in range(-2, 3)]).reshape(5, nb).T.reshape(-1)
    a2 = (q.astype(np.float64) * b2.astype(np.float64)).astype(F)
    a2, b2 = with_neighbours(a2, 1), np.tile(b2, 3)
    ra, rb = ray_cases()["div_ops"]
    with np.errstate(all="ignore"):
        rq = ra / rb
    ok = np.isfinite(ra) & np.isfinite(rb) & (rb != 0) & ((ra == 0) | is_normal(ra)) & is_normal(rb) & ((rq == 0) | is_normal(rq))
    return np.concatenate([a, a2, ra[ok]]), np.concatenate([b, b2, rb[ok]])


F2H_LO, F2H_HI = F(2.0 ** -14), F(65520.0)


@functools.lru_cache(None)
def f2h_inputs():
    """Every normal half, the midpoint of every adjacent pair, 65504 and the last floats under 65520, each with its +-1 and +-2 ulp32 neighbours; 2^20
    random floats of the range.  Filtered to [2^-14, 65520), the range f2h_normal is specified on."""
    rng = np.random.default_rng(22)
    h = _half(np.arange(0x0400, 0x7c00, dtype=np.uint16))
    mid = (h[:-1] + h[1:]) * F(0.5)                              # exact: one more bit than a half
    top = step(np.full(4, 65520.0, F), -np.arange(1, 5))
    x = np.concatenate([with_neighbours(np.concatenate([h, mid, top])),
                        fl((rng.integers(127 - 14, 127 + 16, 1 << 20, dtype=U) << 23) | rng.integers(0, 1 << 23, 1 << 20, dtype=U))])
    return x[(x >= F2H_LO) & (x < F2H_HI)]


@functools.lru_cache(None)
def split_inputs():
    """Integers and half-integers of [-4096, 4096], +-2^22, +-2^23, +-2^24 and the small values around the documented case u = -2^-25, each with its
    neighbours; 2^20 random u = fl(x n - 0.5) as the taps form them.  Denormals and -0.0 are left out (split_unasserted)."""
    rng = np.random.default_rng(23)
    k = np.arange(-4096, 4097).astype(F)
    big = np.array([s * 2.0 ** e for e in (22, 23, 24) for s in (1, -1)], F)
    tiny = np.array([s * 2.0 ** e for e in (-26, -25, -24, -23, -100, -126) for s in (1, -1)], F)
    x = rng.uniform(-300.0, 300.0, 1 << 20).astype(F)
    n = np.array(TAP_SIZES, F)[rng.integers(0, len(TAP_SIZES), 1 << 20)]
    u = np.concatenate([with_neighbours(np.concatenate([k, (k + F(0.5))[:-1], big, tiny])), x * n - F(0.5)])
    return u[(u == 0) & ~np.signbit(u) | is_normal(u)]


def split_unasserted():
    return np.array([-0.0, 1e-45, -1e-45, 2.0 ** -127, -(2.0 ** -127), 1.1754942e-38, -1.1754942e-38], F)


def split_reference(u):
    fl_ = np.floor(u)
    return fl_.astype(I), (u - fl_).astype(F)


@functools.lru_cache(None)
def lerp_inputs():
    """(pair, f, full) -- pair = lo | hi << 16.  Set A: all 2^16 low halves with the high half in {0, +-1, +-2040} and 64 random others; set B: all
    2^16 high halves with the low half in {0, 255, 2040}.  f: LERP_F_SPECIAL and 16 random values of [0, 1).  The pairs with a special high (A) or any
    low (B) meet every special f; every pair also meets one of the 22 values, in rotation.  Inf and NaN halves stay in: `lerp_finite` masks them."""
    rng = np.random.default_rng(24)
    fs = np.concatenate([np.array(LERP_F_SPECIAL, F), rng.random(16, dtype=F)])
    allh = np.arange(1 << 16, dtype=U)
    special = np.array([0.0, 1.0, -1.0, 2040.0, -2040.0], np.float16).view(np.uint16).astype(U)
    others = rng.integers(0, 1 << 16, 64, dtype=U)
    others = np.where((others & 0x7c00) == 0x7c00, others ^ 0x4000, others)
    pa = (allh[None, :] | (np.concatenate([special, others])[:, None] << 16)).reshape(-1)
    pb = ((allh[None, :] << 16) | np.array([0.0, 255.0, 2040.0], np.float16).view(np.uint16).astype(U)[:, None]).reshape(-1)
    cross = np.concatenate([pa[: 5 << 16], pb])
    pair = np.concatenate([np.repeat(cross, len(LERP_F_SPECIAL)), pa, pb])
    rot = np.concatenate([pa, pb])
    f = np.concatenate([np.tile(fs[: len(LERP_F_SPECIAL)], len(cross)), fs[((rot & 0xffff) + (rot >> 16) * 7) % len(fs)]])
    return pair.astype(U), f.astype(F)


def lerp_finite(pair):
    return ((pair & 0x7c00) != 0x7c00) & (((pair >> 16) & 0x7c00) != 0x7c00)


# ---------------------------------------------------------------------------------------------------------------- the host branches
def test_exact_fma_reference_against_fractions():
    """fma32 (what the lerps are held against) equals the float32 nearest the exact rational a * b + c, ties to even, on 40 000 lerp cases drawn
    from the device test's own set plus cases built to tie."""
    pair, f = lerp_inputs()
    rng = np.random.default_rng(25)
    pick = rng.choice(np.flatnonzero(lerp_finite(pair)), 40000, replace=False)
    a, d, ff = _half(pair[pick] & 0xffff), _half(pair[pick] >> 16), f[pick]
    # ties: a = 2^12 (ulp32 2^-11), d f = 2^-12 exactly half an ulp, +- a little
    a = np.concatenate([a, np.full(6, 4096.0, F)]); d = np.concatenate([d, np.array([1, -1, 1, -1, 3, -3], F) * F(2.0 ** -11)])
    ff = np.concatenate([ff, np.array([0.5, 0.5, 0.5 + 2.0 ** -24, 0.5 + 2.0 ** -24, 0.5, 0.5], F)])
    got = fma32(d, ff, a)

    def rne32(q):
        if q == 0:
            return 0.0
        lo = float(F(float(q)))                                  # float(Fraction) is correctly rounded to float64; then the two float32 around q
        cand = sorted({lo, float(np.nextafter(F(lo), F(np.inf))), float(np.nextafter(F(lo), F(-np.inf)))}, key=lambda v: (abs(Fraction(v) - q), int(F(v).view(U)) & 1))
        return cand[0]
    want = np.array([rne32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(d, ff, a)], F)
    assert not first_diff(got, want, d, ff, a)
    assert got[-6] == 4096.0 and got[-4] == F(4096.0 + 2.0 ** -11)   # the tie goes to even, a little more goes up


def test_host_lerps_are_one_and_two_correctly_rounded_fmas(hostsim):
    pair, f = lerp_inputs()
    ok = lerp_finite(pair)
    assert ok.sum() > 6e6 and len(pair) <= 1 << 24
    d = _half(pair >> 16)
    assert (d[ok] > 0).sum() > 1e6 and (d[ok] < 0).sum() > 1e6      # both signs of the difference
    assert ((pair & 0x7c00) == 0)[ok].sum() > 1e5                   # fp16 denormals and zeros of the low half
    got = host_primitive(hostsim, "lerp_h", pair, f)
    assert not first_diff(got[ok], lerp_h_exact(pair, f)[ok], pair[ok], f[ok])
    got2 = host_primitive(hostsim, "lerp_h2", pair, f)
    assert not first_diff(got2[ok], lerp_h2_two_step(pair, f)[ok], pair[ok], f[ok])


def test_host_split_coord_is_floor_and_subtract(hostsim):
    u = np.concatenate([split_inputs(), split_unasserted()])
    i, f = host_primitive(hostsim, "split_coord", u)
    ri, rf = split_reference(u)
    assert (i == ri).all() and not first_diff(f, rf, u)
    assert (rf == 1.0).sum() >= 3 and (ri[rf == 1.0] == -1).all()   # the documented case is in the set: u = -2^-25 and smaller
    assert ((rf >= 0) & (rf <= 1)).all()


def test_host_f2h_is_numpys_half_conversion(hostsim):
    x = np.concatenate([f2h_inputs(), np.array([2.0 ** -15, 65520.0, 0.0, 1e-8, 1e6], F)])
    assert 1.3e6 < len(f2h_inputs()) < 1.4e6
    got = host_primitive(hostsim, "f2h_normal", x).astype(np.uint16)
    with np.errstate(over="ignore"):
        assert not first_diff(got, x.astype(np.float16), x)


def test_host_sqrt_and_divide_are_ieee(hostsim):
    x = np.concatenate([sqrt_binades()[:: 64], sqrt_edges()])
    for op in ("sqrt_exact", "sqrtf"):
        assert not first_diff(host_primitive(hostsim, op, x), np.sqrt(x), x)
    a, b = div_pairs()
    assert len(a) <= 1 << 24
    q = a / b
    assert not first_diff(host_primitive(hostsim, "div", a, b), q, a, b)
    m = (bits(q) & 0x7fffff).astype(np.int64)
    assert (np.minimum(m, (1 << 23) - m) <= 3).sum() >= 1 << 17                               # the quotients around powers of two are there


def test_host_ray_and_pixel_dir_equal_the_numpy_restatement(hostsim):
    c = ray_cases()
    above = c["e"][:, 1] > 0
    assert above.mean() >= 0.4 and not np.isnan(c["ref"][above]).any()
    got = host_primitive(hostsim, "ray", c["e"], c["steps"])
    assert not first_diff(got[above], c["ref"][above], c["e"][above], c["steps"][above])
    assert (got[~above].view(U) == 0).all() and (~above).sum() > 0
    assert not first_diff(host_primitive(hostsim, "pixel_dir", c["pix_ij"], c["pix_wh"]), c["pix_ref"], c["pix_ij"], c["pix_wh"])


def test_host_forms_of_the_approximations_are_the_library_functions(hostsim):
    """On the host fast_* are libm's and the reciprocals a division: what the oracle comparison of the cores rests on."""
    x = np.linspace(0.5, 2.0, 4097).astype(F)
    for op in ("fast_rcp", "rad_rcp"):
        assert not first_diff(host_primitive(hostsim, op, x), F(1.0) / x, x)
    assert np.abs(host_primitive(hostsim, "fast_log2", x).astype(np.float64) - np.log2(x.astype(np.float64))).max() < 2.0 ** -22
    t = np.linspace(-20.0, 0.0, 4097).astype(F)
    for op, ref in (("fast_exp2", np.exp2), ("fast_exp", np.exp)):
        got = host_primitive(hostsim, op, t).astype(np.float64)
        assert (np.abs(got / ref(t.astype(np.float64)) - 1.0)).max() < 2.0 ** -20
    y = np.linspace(0.5, 1.3, 4097).astype(F)
    got = host_primitive(hostsim, "fast_pow", x * F(0.5), y).astype(np.float64)
    assert np.abs(got / np.power((x * F(0.5)).astype(np.float64), y.astype(np.float64)) - 1.0).max() < 2.0 ** -20
