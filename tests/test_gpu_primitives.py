"""-m gpu: the DEVICE forms of the march's arithmetic primitives (cloud_core.h, radiance_core.h: the code inside `#if defined(__HIP_DEVICE_COMPILE__)`
and the plain divide / sqrtf of Section A as hipcc compiles them for gfx950), run over arrays by csky_test_primitive (csrc/primitives.hip, which
calls the march's own inline functions) and held against numpy at the inputs where such instructions go wrong.

The host suite never runs these branches (there they are libm and the software f2h: tests/test_primitives_host.py checks THOSE against numpy and
owns the input sets), and the launch-form identity tests compare device with device.  Exact ops: bit equality, the first differing input reported.
Hardware approximations: error against the float64 function, in ulp of the correctly rounded float32 result.

GATES.  AMD's statement of the accuracy of v_rcp_f32 / v_exp_f32 / v_log_f32 (1 ulp) is not in any document shipped with the toolchain this project
builds with, so the gates below are MEASURED, NOT DOCUMENTED: the worst error of the first run on an MI355X against float64, plus nothing (these
are fixed hardware functions: a second run gives the same bits).  MEASURED_ULP holds them.

Every test is a copy up, one launch, a copy down.

MUTATION CHECK (done once on an MI355X against scratch builds, profiles/r23/primitive_mutations.txt): sqrt_exact without its neighbour fix-up fails
4 tests here (2.5 M of the 16.7 M floats of [1, 4)); one flipped op_sel bit of lerp_h fails test_lerp[lerp_h] on 3 587 005 of the 3 587 051 cases
with a negative difference; split_coord as (int)u truncation fails test_split_coord (i on half the inputs); the library built with the fast divide
fails 5 (div: 3.2 M of 13 M pairs).  All four also fail the parent suite's oracle frame gates (21 to 31 of 38 tests): mutations that large never
were the gap.  The gap is a primitive wrong on inputs no frame reaches, and the first run found one (test_sqrt_is_correctly_rounded)."""
import numpy as np
import pytest

import test_primitives_host as P
from test_primitives_host import F, U, bits, first_diff, fl, step

pytestmark = pytest.mark.gpu

# worst error in ulp of the correctly rounded float32 result, measured on an MI355X over the sets below (see GATES above)
# v_rcp_f32 0.8818 at x = 0.51360989 (0x3f037bf0); v_exp_f32 0.7688 at x = -3.1565962 (0xc04a05ac); v_log_f32 0.99986 at x = 2.8990924e-36
# (0x0476a0a4; on [0.5, 2): 0.99850 at 1.9663044): all inside the 1 ulp usually quoted for them
MEASURED_ULP = {"fast_rcp": 0.881808677688241, "rad_rcp": 0.881808677688241, "fast_exp2": 0.7687959354370832, "fast_log2": 0.9998609777539968}


def ulp_error(got, exact):
    """|got - exact| in ulp of the correctly rounded float32 of `exact` (float64)."""
    r = np.abs(exact.astype(F))
    return np.abs(got.astype(np.float64) - exact) / np.spacing(r).astype(np.float64)


def worst(name, err, x):
    k = int(np.argmax(err))
    print("%s: worst %r at input %s (%r) over %d inputs" % (name, float(err[k]), np.atleast_1d(x[k]).view(U).tolist(), np.atleast_1d(x[k]).tolist(), len(err)))
    return float(err[k])


# ------------------------------------------------------------------------------------------------------------------------ exact ops
@pytest.mark.parametrize("inputs", ["binades", "edges"])
@pytest.mark.parametrize("op", ["sqrt_exact", "sqrtf"])
def test_sqrt_is_correctly_rounded(gpu_ctx, op, inputs):
    """sqrt_exact (v_sqrt_f32 plus the residual test of both neighbours) and the compiler's sqrtf against numpy's IEEE float32 sqrt: every float of
    [1, 4) (two binades: the mantissa behaviour repeats with the exponent pair); per exponent -126 .. 127 the mantissa edges and 4096 random
    mantissas; the operands the ray set-up itself takes roots of.
    sqrt_exact is asserted from SQRT_EXACT_MIN = 2^-102 up, the range cloud_core.h states.  FOUND BY THIS TEST: the comment used to claim every
    normal input, and the first run on an MI355X gave 1909 of the 98 400 inputs below 2^-102 one ulp low (exponents -126 .. -110; 845 of 4100 at
    -126), because the neighbours' residuals underflow there.  The claim was corrected, the frame set-up's lengths moved to the IEEE sqrtf, and the
    inputs below the range are now run and their misses printed.  The compiler's sqrtf is asserted on every exponent."""
    x = P.sqrt_binades() if inputs == "binades" else P.sqrt_edges()
    assert len(x) <= 1 << 24 and (inputs != "binades" or len(x) == 1 << 24)
    got, ref = gpu_ctx.test_primitive(op, x), np.sqrt(x)
    inside = (x >= P.SQRT_EXACT_MIN) if op == "sqrt_exact" else np.ones(len(x), bool)
    if not inside.all():
        print("sqrt_exact below 2^-102: %d of %d inputs differ from the IEEE root" % ((bits(got) != bits(ref))[~inside].sum(), (~inside).sum()))
        assert (~inside).sum() == 24 * 4100                     # exponents -126 .. -103
    assert not first_diff(got[inside], ref[inside], x[inside])


def test_sqrt_outside_the_specified_range(gpu_ctx):
    """sqrt_exact is specified for normal positive inputs; nothing in the march feeds it anything else.  What it returns for 0, denormals, inf, NaN
    and a negative is PRINTED; the compiler's sqrtf must be IEEE there too."""
    x = P.sqrt_unspecified()
    with np.errstate(invalid="ignore"):
        ref = np.sqrt(x)
    got = gpu_ctx.test_primitive("sqrtf", x)
    print("sqrt_exact outside its range:", [(float(a), float(b)) for a, b in zip(x, gpu_ctx.test_primitive("sqrt_exact", x))])
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all() and not first_diff(got[~nan], ref[~nan], x[~nan])


def test_divide_is_correctly_rounded(gpu_ctx):
    """The plain `/` of Section A (pixel_dir, intersect_sphere_cam, ray_from_dir) is the IEEE divide: pins the build's correctly rounded division
    (no flag may turn it into v_rcp_f32 and a multiply)."""
    a, b = P.div_pairs()
    assert not first_diff(gpu_ctx.test_primitive("div", a, b), a / b, a, b)


def test_f2h_normal_is_the_software_f2h_on_its_range(gpu_ctx):
    """cloud_core.h::f2h_normal == f2h for 2^-14 <= x < 65520, which ray_saturated's proof rests on.  2^-15 and 65520 (outside) are printed."""
    x = np.concatenate([P.f2h_inputs(), np.array([2.0 ** -15, 65520.0], F)])
    got = gpu_ctx.test_primitive("f2h_normal", x)
    print("f2h_normal outside its range: 2^-15 -> 0x%04x, 65520 -> 0x%04x" % (got[-2], got[-1]))
    assert (got >> 16 == 0).all()
    assert not first_diff(got[:-2].astype(np.uint16), x[:-2].astype(np.float16), x[:-2])


def test_split_coord_is_floor_and_fraction(gpu_ctx):
    """v_cvt_flr_i32_f32 + v_fract_f32 against floor / u - floor(u) in float32: i equal everywhere; f bit-equal except where the reference's f is
    exactly 1.0 (u = -2^-25 and smaller: the documented case), where the device gives 1 - 2^-24 and i = -1; under every tap's mask the same sample
    point.  Denormals and -0.0 (no tap forms them) are printed."""
    ua, ux = P.split_inputs(), P.split_unasserted()
    gi, gf = gpu_ctx.test_primitive("split_coord", np.concatenate([ua, ux]))
    print("split_coord of inputs no tap forms:", [(float(a), int(b), float(c)) for a, b, c in zip(ux, gi[len(ua):], gf[len(ua):])])
    gi, gf = gi[: len(ua)], gf[: len(ua)]
    ri, rf = P.split_reference(ua)
    assert not first_diff(gi, ri, ua)
    one = rf == 1.0
    assert one.sum() >= 3
    assert not first_diff(gf[~one], rf[~one], ua[~one])
    assert (bits(gf[one]) == 0x3f7fffff).all() and (gi[one] == -1).all(), (ua[one], gf[one], gi[one])
    for n in P.TAP_SIZES:                                       # (i & m, f) names the reference's sample point: the same cell, the same place in it
        assert ((gi & (n - 1)) == (ri & (n - 1))).all()
    assert (np.abs(gf.astype(np.float64) - rf.astype(np.float64)) <= 2.0 ** -24).all() and (gf < 1.0).all() and (gf >= 0.0).all()


@pytest.mark.parametrize("op", ["lerp_h", "lerp_h2"])
def test_lerp_is_one_rounding_of_the_exact_value(gpu_ctx, op):
    """v_fma_mix_f32 with its op_sel / op_sel_hi / neg modifiers: lerp_h against the single correctly rounded a + d f, lerp_h2 against the host
    branch's two correctly rounded steps; positive and negative differences apart, so that a wrong modifier bit cannot hide."""
    pair, f = P.lerp_inputs()
    got = gpu_ctx.test_primitive(op, pair, f)
    ref = P.lerp_h_exact(pair, f) if op == "lerp_h" else P.lerp_h2_two_step(pair, f)
    ok = P.lerp_finite(pair)
    with np.errstate(invalid="ignore"):
        d = P._half(pair >> 16) if op == "lerp_h" else P._half(pair >> 16) - P._half(pair & 0xffff)
        groups = {"negative difference": ok & (d < 0), "positive difference": ok & (d > 0), "zero difference": ok & (d == 0)}
    for name, m in groups.items():
        assert m.sum() > 50
        assert not first_diff(got[m], ref[m], pair[m], f[m]), name


def test_pixel_dir_equals_the_numpy_restatement(gpu_ctx):
    c = P.ray_cases()
    assert not first_diff(gpu_ctx.test_primitive("pixel_dir", c["pix_ij"], c["pix_wh"]), c["pix_ref"], c["pix_ij"], c["pix_wh"])


def test_ray_equals_the_numpy_restatement(gpu_ctx):
    """ray_from_dir on the device, every field bit for bit against tests/ray_reference.py: all pixels of 64 x 32, 200 x 104 and 1000 x 500, the 32
    grazing directions down to y = 1e-7, at 1, 32, 100, 128 and 1024 steps.  Rays under the horizon come back all-zero."""
    c = P.ray_cases()
    above = c["e"][:, 1] > 0
    assert above.mean() >= 0.4 and not np.isnan(c["ref"][above]).any()          # preconditions on the reference
    got = gpu_ctx.test_primitive("ray", c["e"], c["steps"])
    bad = first_diff(got[above], c["ref"][above], c["e"][above], c["steps"][above])
    assert not bad, (bad, P.RAY_FIELDS)
    assert (~above).sum() > 0 and (got[~above].view(U) == 0).all()


# ------------------------------------------------------------------------------------------------------------------------ approximations
@pytest.mark.parametrize("op", ["fast_rcp", "rad_rcp"])
def test_rcp_error(gpu_ctx, op):
    x = fl(np.arange(0x3f000000, 0x40000000, dtype=U))                           # every float in [0.5, 2); 2.0 is in test_known_answers
    err = ulp_error(gpu_ctx.test_primitive(op, x), 1.0 / x.astype(np.float64))
    assert worst(op, err, x) <= MEASURED_ULP[op]


def test_exp2_error(gpu_ctx):
    rng = np.random.default_rng(30)
    x = np.concatenate([rng.uniform(-126.0, 0.0, (1 << 20) - 2), [-126.0, 0.0], rng.uniform(0.0, 16.0, (1 << 16) - 1), [16.0]]).astype(F)
    err = ulp_error(gpu_ctx.test_primitive("fast_exp2", x), np.exp2(x.astype(np.float64)))
    assert worst("fast_exp2", err, x) <= MEASURED_ULP["fast_exp2"]


@pytest.mark.parametrize("inputs", ["sweep", "loguniform"])
def test_log2_error(gpu_ctx, inputs):
    if inputs == "sweep":
        x = fl(np.arange(0x3f000000, 0x40000000, dtype=U))                       # every float in [0.5, 2)
    else:
        rng = np.random.default_rng(31)
        x = np.concatenate([fl((rng.integers(1, 127, 1 << 20, dtype=U) << 23) | rng.integers(0, 1 << 23, 1 << 20, dtype=U)), np.array([2.0 ** -126, 1.0, 2.0], F)])
    got, ref = gpu_ctx.test_primitive("fast_log2", x), np.log2(x.astype(np.float64))
    z = ref == 0.0                                                               # log2(1) = 0 has no ulp: asserted exactly
    assert (got[z] == 0.0).all()
    err = ulp_error(got[~z], ref[~z])
    assert worst("fast_log2 " + inputs, err, x[~z]) <= MEASURED_ULP["fast_log2"]


def test_fast_exp_error(gpu_ctx):
    """fast_exp(x) = exp2(fl(x * fl(log2 e))) on [-88, 0].  The product's rounding and the constant's own (2^-24 each, relative) move the argument t by
    at most |t| 2^-23, i.e. the result by a relative ln 2 |t| 2^-23; v_exp_f32 adds its ulp, at most 2^-23 relative: bound 2^-23 + ln 2 |x log2 e| 2^-23.
    Below 2^-126 (x < -87.3) the result is denormal and only the absolute bound 2^-126 is asked, as for fast_exp2."""
    rng = np.random.default_rng(32)
    x = np.concatenate([rng.uniform(-88.0, 0.0, (1 << 20) - 2), [-88.0, 0.0]]).astype(F)
    x64 = x.astype(np.float64)
    got, ref = gpu_ctx.test_primitive("fast_exp", x).astype(np.float64), np.exp(x64)
    norm = ref >= 2.0 ** -126
    rel = np.abs(got / ref - 1.0)[norm]
    bound = (2.0 ** -23 + np.log(2.0) * np.abs(x64 * np.log2(np.e)) * 2.0 ** -23)[norm]
    k = int(np.argmax(rel / bound))
    print("fast_exp: worst relative error %.4g (bound %.4g) at x = %r; largest relative error anywhere %.4g" % (rel[k], bound[k], x[norm][k], rel.max()))
    assert (rel <= bound).all()
    assert (np.abs(got - ref)[~norm] < 2.0 ** -126).all() and (~norm).sum() > 100


def test_fast_pow_error(gpu_ctx):
    """fast_pow(x, y) = exp2(y log2 x) on x in [2^-24, 1], y in [0.5, 1.3] (density()'s (1 - hf) 0.8 + 0.5).  From 1-ulp primitives: the exponent
    y log2 x carries the logarithm's ulp and the product's rounding, at most |y log2 x| 2^-22 together, the result a relative ln 2 times that, plus
    v_exp_f32's own ulp: bound 2^-23 + ln 2 |y log2 x| 2^-22."""
    rng = np.random.default_rng(33)
    n = 1 << 20
    x = np.concatenate([fl((rng.integers(127 - 24, 127, n, dtype=U) << 23) | rng.integers(0, 1 << 23, n, dtype=U)), step(np.ones(64, F), -np.arange(64)), [2.0 ** -24]]).astype(F)
    y = np.concatenate([rng.uniform(0.5, 1.3, len(x) - 2), [0.5, 1.3]]).astype(F)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    got, ref = gpu_ctx.test_primitive("fast_pow", x, y).astype(np.float64), np.power(x64, y64)
    rel = np.abs(got / ref - 1.0)
    bound = 2.0 ** -23 + np.log(2.0) * np.abs(y64 * np.log2(x64)) * 2.0 ** -22
    k = int(np.argmax(rel / bound))
    print("fast_pow: worst relative error %.4g (bound %.4g) at x = %r, y = %r; largest relative error anywhere %.4g" % (rel[k], bound[k], x[k], y[k], rel.max()))
    assert (rel <= bound).all()


def test_known_answers(gpu_ctx):
    y = np.linspace(0.5, 1.3, 257).astype(F)
    assert (gpu_ctx.test_primitive("fast_pow", np.zeros_like(y), y) == 0.0).all()
    assert (gpu_ctx.test_primitive("fast_pow", np.ones_like(y), y) == 1.0).all()
    assert gpu_ctx.test_primitive("fast_exp2", np.array([-np.inf], F))[0] == 0.0
    for op in ("fast_rcp", "rad_rcp"):
        assert gpu_ctx.test_primitive(op, np.array([1.0, 2.0, 0.5], F)).tolist() == [1.0, 0.5, 2.0]
    assert gpu_ctx.test_primitive("fast_log2", np.array([1.0, 2.0, 0.5], F)).tolist() == [0.0, 1.0, -1.0]


def test_denormal_inputs_and_results_are_harmless(gpu_ctx):
    """The raw v_log_f32 / v_exp_f32 skip the scaling the library functions do around denormals, so device and host may differ there.  Asserted is
    the absolute bound that makes it harmless: |device - exact| < 2^-63 for fast_pow of a denormal x (x^y <= 2^-63 for y >= 0.5), < 2^-126 for
    fast_exp2 below -126.  What the hardware returns is printed."""
    rng = np.random.default_rng(34)
    xd = np.concatenate([fl(rng.integers(1, 1 << 23, 4093, dtype=U)), fl(np.array([1, 0x7fffff, 0x400000], U))])
    y = np.concatenate([rng.uniform(0.5, 1.3, len(xd) - 2), [0.5, 1.3]]).astype(F)
    got = gpu_ctx.test_primitive("fast_pow", xd, y).astype(np.float64)
    ref = np.power(xd.astype(np.float64), y.astype(np.float64))
    lg = gpu_ctx.test_primitive("fast_log2", xd)
    print("fast_log2 of denormals: %s ... ; fast_pow(denormal, y): max |device - exact| = %.3g (2^-63 = %.3g), device values %s ..." %
          (lg[-3:].tolist(), np.abs(got - ref).max(), 2.0 ** -63, got[-3:].tolist()))
    assert (np.abs(got - ref) < 2.0 ** -63).all()
    t = np.concatenate([rng.uniform(-160.0, -126.0, 4093), [-126.5, -149.0, -150.0]]).astype(F)
    g2 = gpu_ctx.test_primitive("fast_exp2", t).astype(np.float64)
    print("fast_exp2 below -126: of %s -> %s; max |device - exact| = %.3g (2^-126 = %.3g)" %
          (t[-3:].tolist(), g2[-3:].tolist(), np.abs(g2 - np.exp2(t.astype(np.float64))).max(), 2.0 ** -126))
    assert (np.abs(g2 - np.exp2(t.astype(np.float64))) < 2.0 ** -126).all()
