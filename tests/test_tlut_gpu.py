"""The Bruneton parametrization of the transmittance LUT (cloudsky.h CSKY_TLUT_BRUNETON) on the GPU, through the C ABI and the Python classes:
the HIP kernels against the host-compiled cores, the state machine of csky_set_transmittance_mapping, the rows / multi-device forms, and the
compositor and radiance layer 0.  Every test owns its contexts: the session's shared one never leaves the reference mapping."""
import numpy as np
import pytest

import radiance_reference as R
import tlut_reference as TR
from conftest import ulp_diff
from test_tlut_mapping import host_sky, host_trans, tlut_host  # noqa: F401  (tlut_host: the module-scoped fixture)

pytestmark = pytest.mark.gpu
W, Hh = 256, 64
DEMO = TR.norm(TR.SUNS["demo"])
BELOW = TR.norm((-np.cos(np.radians(1.0)), -np.sin(np.radians(1.0)), 0.0))        # 1 degree under the horizon, towards -x like the demo sun


def new_ctx(pkg, noise=None, mapping=None):
    if pkg.lib().csky_device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible (libcloudsky has no CPU fallback)")
    ctx = pkg.Context(0)
    if noise is not None:
        ctx.set_noise(*noise)
    if mapping is not None:
        ctx.set_transmittance_mapping(mapping)
    return ctx


@pytest.fixture(scope="module")
def ctx1(pkg, noise):
    ctx = new_ctx(pkg, noise, "bruneton")
    yield ctx
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------- 7. kernels vs host cores
def test_luts_match_the_host_cores(ctx1, tlut_host):  # noqa: F811
    assert ctx1.transmittance_mapping() == 1
    t = ctx1.render_transmittance(W, Hh)
    ht = host_trans(tlut_host, 1)
    d = ulp_diff(t, ht)
    print("mapping-1 transmittance LUT, GPU vs host core: max %d fp16 ulp, %.4f %% differ" % (d.max(), 100.0 * (d > 0).mean()))
    assert d.max() <= 1
    assert (t[Hh - 1, 0].astype(np.float32) == 1.0).all()
    for name, sun in TR.SUNS.items():
        s = TR.norm(sun)
        g = ctx1.render_sky_lut(s, 200, 100)
        hs = host_sky(tlut_host, 1, s, t)                           # from the GPU's own table: the sky kernel alone is compared
        d = ulp_diff(g, hs)
        print("mapping-1 sky LUT %s, GPU vs host core: max %d fp16 ulp, %.4f %% differ" % (name, d.max(), 100.0 * (d > 0).mean()))
        assert np.isfinite(g.astype(np.float32)).all() and d.max() <= 1, name


def test_default_size_table_is_rendered_on_demand(pkg, noise, ctx1):
    """A context that never called csky_render_transmittance renders the 256 x 64 table itself, in its mapping."""
    ctx = new_ctx(pkg, mapping="bruneton")
    try:
        sk = ctx.render_sky_lut(DEMO, 200, 100)
        assert np.array_equal(bits(ctx.read_transmittance()), bits(ctx1.render_transmittance(W, Hh)))
        assert np.array_equal(bits(sk), bits(ctx1.render_sky_lut(DEMO, 200, 100)))
        with pytest.raises(pkg.CloudSkyError) as e:                  # texel centres sit on the ends of both ranges: no 1-texel tables
            ctx.render_transmittance(1, 64)
        assert e.value.code == pkg._lib.ERR_INVALID
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 8. state
def test_round_trip_through_mapping_1_leaves_mapping_0_untouched(pkg, noise, oracle):
    p = oracle.default_params(512, 256, TR.SUNS["demo"])
    fresh, trip = new_ctx(pkg, noise), new_ctx(pkg, noise)
    try:
        want = (fresh.render_transmittance(W, Hh), fresh.render_sky_lut(DEMO, 200, 100), fresh.render_clouds(p))
        trip.render_sky_lut(DEMO, 200, 100)
        trip.render_clouds(p)
        trip.set_transmittance_mapping("reference")                 # the current value: nothing is dropped
        assert trip.read_sky_lut().shape == (100, 200, 4)
        trip.set_transmittance_mapping("bruneton")
        assert trip.transmittance_mapping() == 1
        for call in (lambda: trip.render_clouds(p), trip.read_sky_lut, trip.read_transmittance):
            with pytest.raises(pkg.CloudSkyError) as e:             # between the switch and the next sky LUT
                call()
            assert e.value.code == pkg._lib.ERR_STATE
        sk1 = trip.render_sky_lut(DEMO, 200, 100)
        assert not np.array_equal(bits(sk1), bits(want[1]))
        assert not np.array_equal(bits(trip.read_transmittance()), bits(want[0]))
        trip.render_clouds(p)
        trip.set_transmittance_mapping("reference")
        assert trip.transmittance_mapping() == 0
        with pytest.raises(pkg.CloudSkyError) as e:
            trip.render_clouds(p)
        assert e.value.code == pkg._lib.ERR_STATE
        with pytest.raises(pkg.CloudSkyError) as e:
            trip.set_transmittance_mapping(2)
        assert e.value.code == pkg._lib.ERR_INVALID and trip.transmittance_mapping() == 0
        got = (trip.render_transmittance(W, Hh), trip.render_sky_lut(DEMO, 200, 100), trip.render_clouds(p))
        for a, b, what in zip(got, want, ("transmittance LUT", "sky LUT", "cloud frame")):
            assert np.array_equal(bits(a), bits(b)), what
        assert float(got[2][..., 3].astype(np.float32).mean()) > 0.0
    finally:
        fresh.close(); trip.close()


# ---------------------------------------------------------------------------------------------------------------- 9. end to end
def test_rows_form_and_multi_give_the_whole_lut_frame(pkg, noise, oracle, ctx1):
    import torch
    p = oracle.default_params(512, 256, TR.SUNS["demo"])
    whole = ctx1.render_sky_lut(DEMO, 200, 100)
    frame = ctx1.render_clouds(p)
    assert float(frame[..., 3].astype(np.float32).mean()) > 0.0
    # (b) the LUT goes to the caller as rows 1::4; the frame set-up renders the texels it filters itself, through the same mapping
    rows = torch.zeros(25 * 200 * 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx1.render_sky_lut_rows_device(DEMO, 1, 4, rows.data_ptr(), rows.numel(), 200, 100, None)
    frame_rows = ctx1.render_clouds(p)
    assert np.array_equal(rows.cpu().numpy().view(np.uint16).reshape(25, 200, 4), bits(whole)[1::4])
    assert np.array_equal(bits(frame_rows), bits(frame))
    ctx1.render_sky_lut(DEMO, 200, 100)
    # the same frame in the reference mapping is another frame (the sun, ambient and ground colours hang on the table)
    ref = new_ctx(pkg, noise)
    try:
        ref.render_sky_lut(DEMO, 200, 100)
        assert not np.array_equal(bits(ref.render_clouds(p)), bits(frame))
    finally:
        ref.close()
    # two contexts on device 0 behind one handle: rows i::2 of the LUT and bands i::2 of the frame from each
    m = pkg.MultiContext([0, 0])
    try:
        m.set_noise(*noise)
        m.set_transmittance_mapping("bruneton")
        assert [m.ctx(i).transmittance_mapping() for i in range(2)] == [1, 1]
        m.render_sky_lut(DEMO, 200, 100)
        fm = m.render_clouds(p)
        assert np.array_equal(bits(m.ctx(0).read_sky_lut()), bits(whole))
        assert np.array_equal(bits(fm), bits(frame))
        with pytest.raises(pkg.CloudSkyError) as e:
            m.set_transmittance_mapping(2)
        assert e.value.code == pkg._lib.ERR_INVALID
    finally:
        m.close()


def test_python_classes_take_the_mapping(pkg, noise, ctx1):
    ctx = new_ctx(pkg)
    try:
        t = pkg.TransmittanceLut(ctx, mapping="bruneton")
        assert ctx.transmittance_mapping() == 1 and np.array_equal(bits(t.image), bits(ctx1.render_transmittance(W, Hh)))
        s = pkg.SkyLut(ctx, t)
        assert s.mapping == "bruneton"
        s.update_lut(DEMO)
        assert np.array_equal(bits(s.image), bits(ctx1.render_sky_lut(DEMO, 200, 100)))
        assert pkg.TransmittanceLut(ctx).mapping is None and ctx.transmittance_mapping() == 1          # no mapping given: the context's own stays
        assert pkg.TransmittanceLut(ctx, mapping="reference").mapping == "reference" and ctx.transmittance_mapping() == 0
    finally:
        ctx.close()
    sky = pkg.CloudSky(texture_size=(128, 64), noise=noise, mapping="bruneton")
    try:
        assert sky.ctx.transmittance_mapping() == 1 and sky.sky_lut.mapping == "bruneton"
        assert np.array_equal(bits(sky.transmittance_tex.image), bits(ctx1.render_transmittance(W, Hh)))
    finally:
        sky.ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 10. compositor, radiance layer 0
def tlut_value_for_the_compositor(table, sun):
    """getValFromTLUT's arguments are pixel-invariant (viewPos, LIGHT0_DIRECTION; clouds.gdshader:97): mu = dot(up, sun) at r = Rg + hn (Rt - Rg)
    with the shader's own normalised height, in its fp32 arithmetic.  The one value every lit pixel taps, looked up by the restatement."""
    f = np.float32
    vpy = f(6.360 + 0.0002)
    height = np.sqrt(vpy * vpy)
    mu = f(0.0) / height * f(sun[0]) + vpy / height * f(sun[1]) + f(0.0) / height * f(sun[2])
    hn = np.maximum(f(0.0), np.minimum(f(1.0), (height - f(6.360)) / f(6.460 - 6.360)))
    r = f(6371.0) + hn * f(100.0)
    return TR.lookup_bruneton(table, np.array([r], f), np.array([mu], f))[0], bool(TR.hits_ground(r, mu))


@pytest.mark.parametrize("sun_key", ["demo", "below"])
def test_compositor_and_radiance_layer_0(ctx1, oracle, sun_key):
    from test_radiance_gpu import cloud_texture
    sun = DEMO if sun_key == "demo" else BELOW
    table = ctx1.render_transmittance(W, Hh)
    val, hit = tlut_value_for_the_compositor(table, sun)
    assert hit == (sun_key == "below")
    if hit:
        assert (val == 0).all()                                      # the disc adds exactly nothing
    else:
        assert (val[:3] > 0.01).all()
    const = np.broadcast_to(val.astype(np.float16), (Hh, W, 4)).copy()   # a bilinear tap of a constant is the constant
    sk, sk2 = ctx1.render_sky_lut(sun, 200, 100), ctx1.render_sky_lut(TR.norm(sun + np.array([0.0, 0.02, 0.0], np.float32)), 200, 100)
    cl, cl2 = cloud_texture(1), cloud_texture(2)
    ref = oracle.composite(cl, cl2, sk, sk2, const, sun, 0.25, 2.0, 512, 256)
    img = ctx1.composite_sky(cl, cl2, sk, sk2, sun, 0.25, 2.0, 512, 256)
    d = ulp_diff(img, ref)
    print("compositor %s: max %d fp16 ulp, %.3f %% differ" % (sun_key, d.max(), 100.0 * (d > 0).mean()))
    assert d.max() <= 2
    if not hit:                                                      # the disc is in view and lit: a black table gives another image
        dark = oracle.composite(cl, cl2, sk, sk2, np.zeros_like(const), sun, 0.25, 2.0, 512, 256)
        assert (img.astype(np.float32) - dark.astype(np.float32)).max() > 0.05
    S = 64
    cube = ctx1.render_radiance(cl, cl2, sk, sk2, sun, 0.25, 2.0, S, 1, 0, 0, 1)
    for f in range(6):
        want = oracle.composite_view(cl, cl2, sk, sk2, const, sun, R.face_basis(f), 90.0, 0.25, 2.0, S, S)
        view = ctx1.composite_view(cl, cl2, sk, sk2, sun, R.face_basis(f), 90.0, 0.25, 2.0, S, S)
        assert ulp_diff(cube[0, f], want).max() <= 2 and ulp_diff(view, want).max() <= 2, f
