"""The sky LUT is rendered when the sun or its other inputs have changed, and only then.

The LUT is a function of the sun direction, its size, the transmittance table and that table's mapping.  csky_render_sky_lut[_device] with the
request the context's ring slot was rendered from launches nothing (csrc/sky_lut_reuse.h holds the rule, tests/test_sky_lut_reuse_host.py its
table); csky_render_sky_lut_rows_device answers the same request again with a copy of the rows it kept; csky_multi_render_sky_lut renders on no
device.  Here, on the GPU: the launch counter (csky_sky_lut_launches) moves exactly when it must, and whatever the path, the bytes are those a
fresh context renders for the same request -- LUTs, rows and the cloud frames set up from them."""
import numpy as np
import pytest

from conftest import norm

pytestmark = pytest.mark.gpu

SIZES = [(200, 100), (8, 4)]
A = norm((1, 1, 0))                                   # z is +0.0
B = norm((-0.998773, 0.0495291, 2.69869e-07))         # conftest SUNS["demo"]
POISON = -1                                           # 0xFFFF in every half, a NaN no LUT and no frame contains (tests/test_gpu_write_coverage.py)
GUARD = 512                                           # poisoned halfs before and after a rows buffer


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def ulp_up(sun, i):
    s = np.array(sun, np.float32)
    s[i] = np.nextafter(s[i], np.float32(np.inf))
    return s


_FRESH = {}


def fresh(pkg, sun, w, h, mapping=0):
    """the LUT a context that has rendered nothing else renders for (sun, w, h, mapping): uint16 [h, w, 4], once per request"""
    k = (np.asarray(sun, np.float32).tobytes(), w, h, mapping)
    if k not in _FRESH:
        ctx = pkg.Context(0)
        try:
            ctx.set_transmittance_mapping(mapping)
            assert ctx.sky_lut_launches() == 0
            _FRESH[k] = bits(ctx.render_sky_lut(sun, w, h)).copy()
            assert ctx.sky_lut_launches() == 1
        finally:
            ctx.close()
    return _FRESH[k]


@pytest.fixture
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cloud_ctx(pkg, noise):
    c = pkg.Context(0)
    c.set_noise(*noise)
    c.set_march(128, 6)
    yield c
    c.close()


def render_and_count(c, sun, w, h):
    """(bytes, launches this call made)"""
    n0 = c.sky_lut_launches()
    out = bits(c.render_sky_lut(sun, w, h))
    return out, c.sky_lut_launches() - n0


@pytest.mark.parametrize("w,h", SIZES)
def test_the_same_request_again_launches_nothing(pkg, ctx, w, h):
    first, n = render_and_count(ctx, A, w, h)
    assert n == 1
    again, n = render_and_count(ctx, A, w, h)
    assert n == 0
    assert np.array_equal(first, fresh(pkg, A, w, h)) and np.array_equal(again, fresh(pkg, A, w, h))
    n0 = ctx.sky_lut_launches()
    ctx.render_sky_lut_device(A, w, h)                           # the device form decides the same way, and what is read back is the same LUT
    assert ctx.sky_lut_launches() == n0
    assert np.array_equal(bits(ctx.read_sky_lut()), fresh(pkg, A, w, h))


def changed_suns():
    return [("sun[%d] one ulp up" % i, ulp_up(A, i)) for i in range(3)] + [("-0.0 against 0.0", np.array([A[0], A[1], -0.0], np.float32))]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name,sun", changed_suns(), ids=[n for n, _ in changed_suns()])
def test_a_sun_that_differs_in_one_bit_is_rendered(pkg, ctx, w, h, name, sun):
    assert sun.tobytes() != A.tobytes()
    _, n = render_and_count(ctx, A, w, h)
    assert n == 1
    got, n = render_and_count(ctx, sun, w, h)
    assert n == 1, name
    assert np.array_equal(got, fresh(pkg, sun, w, h)), name
    got, n = render_and_count(ctx, sun, w, h)
    assert n == 0 and np.array_equal(got, fresh(pkg, sun, w, h)), name


def test_another_size_is_rendered(pkg, ctx):
    render_and_count(ctx, A, 200, 100)
    for w, h in ((8, 4), (200, 100), (100, 200)):
        got, n = render_and_count(ctx, A, w, h)
        assert n == 1 and got.shape == (h, w, 4), (w, h)
        assert np.array_equal(got, fresh(pkg, A, w, h)), (w, h)


@pytest.mark.parametrize("w,h", SIZES)
def test_a_transmittance_table_rendered_again_renders_the_lut_again(pkg, ctx, w, h):
    ctx.render_transmittance(256, 64)
    render_and_count(ctx, A, w, h)
    ctx.render_transmittance(256, 64)                            # the same size: the same bytes, but the library does not know that
    got, n = render_and_count(ctx, A, w, h)
    assert n == 1 and np.array_equal(got, fresh(pkg, A, w, h))
    _, n = render_and_count(ctx, A, w, h)
    assert n == 0


@pytest.mark.parametrize("w,h", SIZES)
def test_the_mapping_changed_and_changed_back_renders_each_time(pkg, ctx, w, h):
    render_and_count(ctx, A, w, h)
    ctx.set_transmittance_mapping(1)
    got, n = render_and_count(ctx, A, w, h)
    assert n == 1 and np.array_equal(got, fresh(pkg, A, w, h, mapping=1))
    ctx.set_transmittance_mapping(0)
    got, n = render_and_count(ctx, A, w, h)
    assert n == 1 and np.array_equal(got, fresh(pkg, A, w, h, mapping=0))
    assert not np.array_equal(fresh(pkg, A, w, h, mapping=1), fresh(pkg, A, w, h, mapping=0))


@pytest.mark.parametrize("w,h", SIZES)
def test_after_a_rows_form_call_the_whole_lut_is_rendered(pkg, ctx, w, h):
    import torch
    render_and_count(ctx, A, w, h)
    rows = torch.zeros(h * w * 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_sky_lut_rows_device(A, 1, 3, rows.data_ptr(), rows.numel(), w, h, None)
    got, n = render_and_count(ctx, A, w, h)
    assert n == 1 and np.array_equal(got, fresh(pkg, A, w, h))


@pytest.mark.parametrize("w,h", SIZES)
def test_after_the_multi_device_form_the_whole_lut_is_rendered(pkg, w, h):
    m = pkg.MultiContext([0, 0])
    try:
        c0, c1 = m.ctx(0), m.ctx(1)
        render_and_count(c0, A, w, h)
        m.render_sky_lut(A, w, h)                                # rows of both contexts into the first one's ring
        m.sync()
        assert np.array_equal(bits(c0.read_sky_lut()), fresh(pkg, A, w, h))
        got, n = render_and_count(c0, A, w, h)
        assert n == 1 and np.array_equal(got, fresh(pkg, A, w, h))
        # the handle's own reuse: the same request again renders on no device; a context's own call in between makes the handle render again
        m.render_sky_lut(A, w, h)
        n0, n1 = c0.sky_lut_launches(), c1.sky_lut_launches()
        m.render_sky_lut(A, w, h)
        assert (c0.sky_lut_launches(), c1.sky_lut_launches()) == (n0, n1)
        m.sync()
        assert np.array_equal(bits(c0.read_sky_lut()), fresh(pkg, A, w, h))
        m.render_sky_lut(B, w, h)
        assert (c0.sky_lut_launches(), c1.sky_lut_launches()) == (n0 + 1, n1 + 1)
        m.sync()
        assert np.array_equal(bits(c0.read_sky_lut()), fresh(pkg, B, w, h))
        render_and_count(c0, B, w, h)
        m.render_sky_lut(B, w, h)
        assert (c0.sky_lut_launches(), c1.sky_lut_launches()) == (n0 + 3, n1 + 2)
        m.sync()
        assert np.array_equal(bits(c0.read_sky_lut()), fresh(pkg, B, w, h))
    finally:
        m.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_a_b_a_goes_round_the_two_slot_ring(pkg, ctx, w, h):
    for k, sun in enumerate((A, B, A)):
        got, n = render_and_count(ctx, sun, w, h)
        assert n == 1, k
        assert np.array_equal(got, fresh(pkg, sun, w, h)), k
    assert not np.array_equal(fresh(pkg, A, w, h), fresh(pkg, B, w, h))


@pytest.mark.parametrize("w,h", SIZES)
def test_with_reuse_off_every_call_launches(pkg, ctx, w, h):
    import torch
    ctx.set_sky_lut_reuse(False)
    for k in range(3):
        got, n = render_and_count(ctx, A, w, h)
        assert n == 1 and np.array_equal(got, fresh(pkg, A, w, h)), k
    rows = torch.zeros(h * w * 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k in range(2):
        n0 = ctx.sky_lut_launches()
        ctx.render_sky_lut_rows_device(A, 1, 3, rows.data_ptr(), rows.numel(), w, h, None)
        assert ctx.sky_lut_launches() == n0 + 1, k
    ctx.set_sky_lut_reuse(True)
    _, n = render_and_count(ctx, A, w, h)
    assert n == 1                                               # nothing rendered while the switch was off is taken for stored
    _, n = render_and_count(ctx, A, w, h)
    assert n == 0


def frame_params(oracle, k, sun):
    """64 x 32, another frame every k: the wind offsets and the time move as they do in the demo"""
    p = oracle.default_params(64, 32, sun)
    p[4:10] = np.float32(0.37 * k) * np.array([1.0, -0.5, 0.25, 2.0, -1.0, 0.5], np.float32)
    p[23] = np.float32(1.5 * k)
    return p


def six_frames(c, oracle, reuse, lut_size):
    """six frames on two alternating streams with two in flight, the LUT asked for before each one; suns A A A B B A"""
    import torch
    c.set_sky_lut_reuse(reuse)
    c.set_frames_in_flight(2)
    suns = [A, A, A, B, B, A]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [torch.full((32, 64, 4), POISON, dtype=torch.int16, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    n0 = c.sky_lut_launches()
    try:
        for k in range(6):
            st = streams[k & 1].cuda_stream
            c.render_sky_lut_device(suns[k], lut_size[0], lut_size[1], st)
            c.render_clouds_device(frame_params(oracle, k, suns[k]), 64, (32, 0, 1, 1), outs[k].data_ptr(), 64 * 8, st)
    finally:
        torch.cuda.synchronize()
        c.sync()
        c.set_frames_in_flight(1)
        c.set_sky_lut_reuse(True)
    return [bits(o.cpu().numpy()) for o in outs], c.sky_lut_launches() - n0


@pytest.mark.parametrize("w,h", SIZES)
def test_six_frames_in_flight_are_the_same_with_and_without_reuse(cloud_ctx, oracle, w, h):
    on, n_on = six_frames(cloud_ctx, oracle, True, (w, h))
    off, n_off = six_frames(cloud_ctx, oracle, False, (w, h))
    assert n_off == 6 and n_on == 3, (n_on, n_off)              # A, B and A again
    for k in range(6):
        assert not (on[k] == 0xFFFF).any(), k
        assert np.array_equal(on[k], off[k]), k
    assert not np.array_equal(on[0], on[1]) and not np.array_equal(on[2], on[3])
    assert float(on[0].view(np.float16)[..., 3].astype(np.float32).mean()) > 0.0


class RowsBuffer:
    """rows first_row::row_stride of a w x h LUT, compact, between two poisoned guards"""

    def __init__(self, w, h, first_row, row_stride):
        import torch
        self.n_rows, self.w = len(range(first_row, h, row_stride)), w
        self.halfs = self.n_rows * w * 4
        self.t = torch.full((GUARD + self.halfs + GUARD,), POISON, dtype=torch.int16, device="cuda")
        self.ptr, self.bytes = self.t.data_ptr() + GUARD * 2, self.halfs * 2

    def read(self):
        """(rows as uint16 [n_rows, w, 4], whether both guards are untouched)"""
        a = bits(self.t.cpu().numpy())
        return a[GUARD:GUARD + self.halfs].reshape(self.n_rows, self.w, 4), bool((a[:GUARD] == 0xFFFF).all() and (a[GUARD + self.halfs:] == 0xFFFF).all())


def rows_then_frame(c, oracle, reuse, w, h):
    """sun A twice, then sun B twice, rows 1::3 into two buffers on two streams in turn; then one frame.  -> (rows x 4, guards x 4, launches x 4, frame)"""
    import torch
    c.set_sky_lut_reuse(reuse)
    streams = [torch.cuda.Stream() for _ in range(2)]
    bufs = [RowsBuffer(w, h, 1, 3) for _ in range(4)]
    frame = torch.full((32, 64, 4), POISON, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    launches = []
    try:
        for k, sun in enumerate((A, A, B, B)):
            n0 = c.sky_lut_launches()
            c.render_sky_lut_rows_device(sun, 1, 3, bufs[k].ptr, bufs[k].bytes, w, h, streams[k & 1].cuda_stream)
            launches.append(c.sky_lut_launches() - n0)
        c.render_clouds_device(frame_params(oracle, 1, B), 64, (32, 0, 1, 1), frame.data_ptr(), 64 * 8, streams[0].cuda_stream)
    finally:
        torch.cuda.synchronize()
        c.sync()
        c.set_sky_lut_reuse(True)
    got = [b.read() for b in bufs]
    return [g[0] for g in got], [g[1] for g in got], launches, bits(frame.cpu().numpy())


@pytest.mark.parametrize("w,h", SIZES)
def test_the_rows_form_copies_the_rows_it_kept(pkg, cloud_ctx, oracle, w, h):
    rows, guards, launches, frame = rows_then_frame(cloud_ctx, oracle, True, w, h)
    assert launches == [1, 0, 1, 0], launches
    assert all(guards), guards
    for k, sun in enumerate((A, A, B, B)):
        assert rows[k].shape[0] == len(range(1, h, 3)) > 0
        assert np.array_equal(rows[k], fresh(pkg, sun, w, h)[1::3]), k
    rows_off, guards_off, launches_off, frame_off = rows_then_frame(cloud_ctx, oracle, False, w, h)
    assert launches_off == [1, 1, 1, 1] and all(guards_off)
    for k in range(4):
        assert np.array_equal(rows[k], rows_off[k]), k
    assert not (frame == 0xFFFF).any() and np.array_equal(frame, frame_off)
    # the frame set up from the rows' sun is the frame set up from the whole LUT of that sun
    import torch
    whole = torch.full((32, 64, 4), POISON, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    cloud_ctx.render_sky_lut_device(B, w, h)
    cloud_ctx.render_clouds_device(frame_params(oracle, 1, B), 64, (32, 0, 1, 1), whole.data_ptr(), 64 * 8, None)
    cloud_ctx.sync()
    assert np.array_equal(bits(whole.cpu().numpy()), frame)
