"""-m gpu: the atmosphere LUT path and the compositor off their default sizes, through the C ABI.

The transmittance table (transmittance_kernel, 4 texels per block), the sky LUT in its whole and rows form (sky_lut_kernel, sky_lut_rows_kernel,
8 texels per block), the frame set-ups that filter it (frame_setup_kernel, frame_setup_taps_kernel), the state that hangs on a size (ensure_sky,
the size inside sky_lut_key, RowsCache::fill re-growing, the read-backs and copies out) and composite_kernel, at the sizes, suns and cases of
tests/test_lut_sizes_host.py -- where the same references are first held to the host-compiled cores on the CPU.

Gates: LUT vs oracle (mapping 0) or host core (mapping 1) <= 1 fp16 ulp; compositor vs oracle <= 2 ulp; cloud frames parity_metrics.cloud_tight;
everything described as "the same" byte equality.  The share of differing halves is printed pooled over a size list (one half of a 1 x 1 LUT is
25 % of it) and gated, at the 0.02 of test_gpu_parity.test_sky_lut, for the sky LUTs over the default table only.  Every test owns its contexts:
the session's shared one is not touched."""
import ctypes as C

import numpy as np
import pytest

import shadow_reference as SR
from conftest import cloud_tight, ulp_diff
from test_gpu_clouds_rays import MARCH
from test_gpu_sky_lut_reuse import GUARD, POISON, RowsBuffer
from test_lut_sizes_host import (DEFAULT_TABLE, LUT_SUNS, PANORAMA_CASES, SKY_SIZES, SMALL_TABLE, SUNS, TRANS_SIZES, VIEW_CASES, Pool, bits, composite_inputs,
                                 oracle_composite, right_angle_basis)
from test_tlut_gpu import new_ctx
from test_tlut_mapping import host_sky, host_trans, tlut_host  # noqa: F401  (tlut_host: the module-scoped fixture)

pytestmark = pytest.mark.gpu
DEFAULT_SKY = (200, 100)


@pytest.fixture(scope="module")
def ctxs(pkg, noise):
    """a context per mapping, with the noise bound"""
    c = {0: new_ctx(pkg, noise, "reference"), 1: new_ctx(pkg, noise, "bruneton")}
    yield c
    for x in c.values():
        x.close()


def reference_trans(oracle, L, mapping, w, h):
    return oracle.transmittance_lut(w, h) if mapping == 0 else host_trans(L, 1, w, h)


def reference_sky(oracle, L, mapping, sun, table, w, h):
    return oracle.sky_lut(sun, table, w, h) if mapping == 0 else host_sky(L, 1, sun, table, w, h)


def poisoned(halfs):
    """(tensor of GUARD + halfs + GUARD int16, all 0xFFFF; device pointer of its middle)"""
    import torch
    t = torch.full((GUARD + halfs + GUARD,), POISON, dtype=torch.int16, device="cuda")
    return t, t.data_ptr() + GUARD * 2


def split(t, halfs):
    """(middle as uint16, whether both guards are untouched)"""
    a = bits(t.cpu().numpy())
    return a[GUARD:GUARD + halfs], bool((a[:GUARD] == 0xFFFF).all() and (a[GUARD + halfs:] == 0xFFFF).all())


# ---------------------------------------------------------------------------------------------------------------- 1. transmittance sizes
@pytest.mark.parametrize("mapping", [0, 1])
def test_transmittance_sizes(pkg, ctxs, oracle, tlut_host, mapping):  # noqa: F811
    """render_transmittance at sizes whose w * h is no multiple of the kernel's 4 texels per block, down to one texel (mapping 0) and 2 x 2
    (mapping 1), against the oracle / the host core.  Measured on the GPU: mapping 0 the oracle's bytes (0 of 1 804 halves differ), mapping 1
    the host core's (0 of 1 540)."""
    ctx = ctxs[mapping]
    fresh = new_ctx(pkg, mapping=mapping)
    try:
        want_default = bits(fresh.render_transmittance(*DEFAULT_TABLE)).copy()
    finally:
        fresh.close()
    pool = Pool()
    try:
        for w, h in TRANS_SIZES[mapping]:
            t = ctx.render_transmittance(w, h)
            assert t.shape == (h, w, 4) and np.isfinite(t.astype(np.float32)).all(), (w, h)
            d = pool.add(t, reference_trans(oracle, tlut_host, mapping, w, h))
            assert d.max() <= 1, (mapping, w, h, int(d.max()))
            back = ctx.read_transmittance()
            assert back.shape == (h, w, 4) and np.array_equal(bits(back), bits(t)), (w, h)
        print("mapping-%d transmittance LUT over %s, GPU vs reference: %s" % (mapping, TRANS_SIZES[mapping], pool))
        if mapping == 1:
            for w, h in ((1, 64), (64, 1), (1, 1)):                 # texel centres sit on the ends of both ranges: no 1-texel rows or columns
                with pytest.raises(pkg.CloudSkyError) as e:
                    ctx.render_transmittance(w, h)
                assert e.value.code == pkg._lib.ERR_INVALID, (w, h)
    finally:
        after = ctx.render_transmittance(*DEFAULT_TABLE)
    assert np.array_equal(bits(after), want_default)                # a size change leaves nothing behind
    assert np.array_equal(bits(ctx.read_transmittance()), want_default)


# ---------------------------------------------------------------------------------------------------------------- 2. sky LUT sizes
@pytest.mark.parametrize("table", ["default-table", "small-table"])
@pytest.mark.parametrize("mapping", [0, 1])
def test_sky_lut_sizes(ctxs, oracle, tlut_host, mapping, table):  # noqa: F811
    """render_sky_lut at sizes whose w * h leaves every residue of the kernel's 8 texels per block, three suns, over the default table and a
    small one; the reference is given the GPU's own table read back, so the sky kernel alone is compared.  Then the read-back and the device copy,
    which must write w * h * 8 bytes and nothing else.  Measured on the GPU over the 7 sizes x 3 suns (38 112 halves), worst ulp and share of
    differing halves: mapping 0 over 256 x 64 0 ulp, 0 %; mapping 0 over 31 x 9 1 ulp, 0.0052 % (2 halves); mapping 1 over 256 x 64 1 ulp,
    0.0105 % (4 halves); mapping 1 over 33 x 9 0 ulp, 0 %."""
    import torch
    ctx = ctxs[mapping]
    tw, th = DEFAULT_TABLE if table == "default-table" else SMALL_TABLE[mapping]
    stream = torch.cuda.Stream()
    pool = Pool()
    try:
        ctx.render_transmittance(tw, th)
        t = ctx.read_transmittance()
        assert t.shape == (th, tw, 4)
        for w, h in SKY_SIZES:
            for name in LUT_SUNS:
                g = ctx.render_sky_lut(SUNS[name], w, h)
                assert g.shape == (h, w, 4) and np.isfinite(g.astype(np.float32)).all(), (w, h, name)
                d = pool.add(g, reference_sky(oracle, tlut_host, mapping, SUNS[name], t, w, h))
                assert d.max() <= 1, (mapping, table, w, h, name, int(d.max()))
                back = ctx.read_sky_lut()
                assert back.shape == (h, w, 4) and np.array_equal(bits(back), bits(g)), (w, h, name)
                for s in (stream.cuda_stream, None):
                    buf, ptr = poisoned(w * h * 4)
                    torch.cuda.synchronize()                       # the fill ran on torch's stream
                    ctx.copy_sky_lut_device(ptr, s)
                    stream.synchronize()
                    ctx.sync()
                    got, guards = split(buf, w * h * 4)
                    assert guards, (w, h, name, s)
                    assert np.array_equal(got.reshape(h, w, 4), bits(g)), (w, h, name, s)
        print("mapping-%d sky LUT over the %d x %d table, %s x %s, GPU vs reference: %s" % (mapping, tw, th, SKY_SIZES, LUT_SUNS, pool))
        if table == "default-table":
            assert pool.share < 0.02
    finally:
        ctx.render_transmittance(*DEFAULT_TABLE)
        ctx.render_sky_lut(SUNS["deg45"], *DEFAULT_SKY)


# ---------------------------------------------------------------------------------------------------------------- 3. rows at ragged sizes
@pytest.mark.parametrize("reuse", [True, False], ids=["reuse", "no-reuse"])
@pytest.mark.parametrize("mapping", [0, 1])
def test_rows_at_ragged_sizes(pkg, mapping, reuse):
    """csky_render_sky_lut_rows_device where w * n_rows is no multiple of 8 and where a rank owns no row (first_row >= h: no launch, nothing
    written, still OK).  Every call goes into a poisoned buffer between guards and is repeated into a fresh one: with reuse on the repeat is the
    rows cache's copy.  The sizes grow, so the cache re-grows; the first size is asked for again at the end."""
    import torch
    ctx = new_ctx(pkg, mapping=mapping)                             # its own: the rows cache starts empty
    sun = SUNS["demo"]
    st = torch.cuda.Stream()
    try:
        ctx.set_sky_lut_reuse(reuse)
        sizes = [(7, 5), (13, 7), (201, 3)]
        whole = {size: bits(ctx.render_sky_lut(sun, *size)).copy() for size in sizes}
        largest = 0
        regrown = 0
        for w, h in sizes + sizes[:1]:
            for stride in (2, 3, 8):
                got = np.full((h, w, 4), 0xFFFF, np.uint16)
                for r in range(stride):
                    n_rows = len(range(r, h, stride))
                    assert (n_rows == 0) == (r >= h)
                    if reuse and n_rows * w > largest:
                        largest, regrown = n_rows * w, regrown + 1
                    first = None
                    for k in range(2):
                        buf = RowsBuffer(w, h, r, stride)
                        assert buf.bytes == n_rows * w * 8
                        torch.cuda.synchronize()                   # the fill ran on torch's stream
                        n0 = ctx.sky_lut_launches()
                        ctx.render_sky_lut_rows_device(sun, r, stride, buf.ptr, buf.bytes, w, h, st.cuda_stream)
                        launched = ctx.sky_lut_launches() - n0
                        st.synchronize()
                        rows, guards = buf.read()
                        assert guards, (w, h, stride, r, k)
                        assert rows.shape == (n_rows, w, 4) and not (rows == 0xFFFF).any(), (w, h, stride, r, k)
                        assert launched == (0 if n_rows == 0 or (reuse and k == 1) else 1), (w, h, stride, r, k, launched)
                        if k == 0:
                            first = rows
                        else:
                            assert np.array_equal(rows, first), (w, h, stride, r)
                    got[r::stride] = first
                assert np.array_equal(got, whole[(w, h)]), (w, h, stride)          # the interleaved rows are the whole LUT of that size
        assert regrown >= 3 or not reuse
        # one byte short of n_rows * w * 8
        w, h, r, stride = 13, 7, 1, 3
        buf = RowsBuffer(w, h, r, stride)
        torch.cuda.synchronize()
        assert buf.n_rows == 2
        with pytest.raises(pkg.CloudSkyError) as e:
            ctx.render_sky_lut_rows_device(sun, r, stride, buf.ptr, buf.bytes - 1, w, h, st.cuda_stream)
        assert e.value.code == pkg._lib.ERR_INVALID
        st.synchronize()
        rows, guards = buf.read()
        assert guards and (rows == 0xFFFF).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 4. frame set-up over other sky sizes
@pytest.mark.parametrize("table", ["default-table", "small-table"])
def test_frame_setup_over_other_sky_sizes(ctxs, oracle, otex, table):
    """frame_setup_kernel filtering sky LUTs of (1, 1), (7, 5), (64, 33) and (200, 100): where its three taps fall depends on sw, sh.  Scenes A and
    B of shadow_reference.scene at 64 x 32 against the oracle marching over the context's own LUT read back.  Measured on the GPU: alpha > 0 in
    64.1 % (scene A) and 76.5 % (scene B) of the pixels at every sky size, as on the oracle; over the 16 frames at least 99.74 % of the values are
    the oracle's, the worst is 1.00 ulp-equivalent."""
    ctx = ctxs[0]
    tw, th = DEFAULT_TABLE if table == "default-table" else SMALL_TABLE[0]
    try:
        ctx.render_transmittance(tw, th)
        for name in ("A", "B"):
            p = SR.scene(oracle, name)
            N, ls = MARCH[name]
            ctx.set_march(N, ls)
            frames = {}
            for w, h in ((1, 1), (7, 5), (64, 33), DEFAULT_SKY):
                ctx.render_sky_lut(np.asarray(p[16:19], np.float32), w, h)
                sky = ctx.read_sky_lut()
                assert sky.shape == (h, w, 4)
                frame = ctx.render_clouds(p)
                cloudy = float((frame[..., 3] > 0).mean())
                ok, info = cloud_tight(frame, oracle.clouds(otex, p, sky, primary_steps=N, light_steps=ls))
                print("scene %s over the %d x %d table and a %d x %d sky: alpha > 0 in %.1f %% of the pixels; within0 %.4f, max %.2f ulp-equivalents" %
                      (name, tw, th, w, h, 100 * cloudy, info["within0"], info["max_ulp"]))
                assert cloudy >= 0.25, (name, w, h)
                assert ok, (name, w, h, info)
                frames[(w, h)] = bits(frame).copy()
            assert not np.array_equal(frames[(7, 5)], frames[DEFAULT_SKY]), name
    finally:
        ctx.set_march(128, 6)
        ctx.render_transmittance(*DEFAULT_TABLE)
        ctx.render_sky_lut(SUNS["deg45"], *DEFAULT_SKY)


# ---------------------------------------------------------------------------------------------------------------- 5. the taps kernel at other sizes
@pytest.mark.parametrize("table", ["default-table", "small-table"])
@pytest.mark.parametrize("mapping", [0, 1])
def test_taps_kernel_at_other_sizes(ctxs, oracle, mapping, table):
    """test_gpu_round4.test_frames_marched_on_a_rows_only_lut_are_byte_identical at sky sizes (1, 1), (7, 5) and (64, 33): frame_setup_taps_kernel
    renders the <= 12 texels its three taps filter itself, and which texels those are depends on sw, sh.  The light is the LUT's sun, one below the
    horizon (v clamps at row 0) and one straight up (atan2f(0, 0), top row)."""
    import torch
    ctx = ctxs[mapping]
    tw, th = DEFAULT_TABLE if table == "default-table" else SMALL_TABLE[mapping]
    W, H = 256, 128
    bands = (8, 3, 8, H // 8 // 8)
    sun = SUNS["deg45"]
    other = np.asarray(SUNS["demo"], np.float32)                   # both slots of the LUT ring hold ANOTHER sun's texels when the rows-only frame is marched
    st = torch.cuda.Stream()
    try:
        ctx.render_transmittance(tw, th)
        for w, h in ((1, 1), (7, 5), (64, 33)):
            n_rows = len(range(3, h, 8))
            for light in (None, (-0.3, -0.8, 0.5), (0.0, 1.0, 0.0)):
                params = oracle.default_params(W, H, light if light is not None else sun)
                out = [torch.zeros((bands[3] * 8, W, 4), dtype=torch.int16, device="cuda") for _ in range(2)]
                rows = torch.zeros(max(1, n_rows) * w * 8, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()                           # the fills above run on torch's stream, the renders on `st`
                ctx.render_sky_lut_device(sun, w, h, st.cuda_stream)
                ctx.render_clouds_device(params, W, bands, out[0].data_ptr(), W * 8, st.cuda_stream)
                ctx.render_sky_lut_device(other, w, h, st.cuda_stream)
                ctx.render_sky_lut_device(other, w, h, st.cuda_stream)
                ctx.render_sky_lut_rows_device(sun, 3, 8, rows.data_ptr(), n_rows * w * 8, w, h, st.cuda_stream)
                ctx.render_clouds_device(params, W, bands, out[1].data_ptr(), W * 8, st.cuda_stream)
                st.synchronize()
                ctx.sync()
                assert bool((out[0] == out[1]).all().item()), (w, h, light)
                assert float(out[0].view(torch.float16)[..., 3].float().mean().item()) > 0.0, (w, h, light)
    finally:
        ctx.render_transmittance(*DEFAULT_TABLE)
        ctx.render_sky_lut(sun, *DEFAULT_SKY)


# ---------------------------------------------------------------------------------------------------------------- 6. a size change with work in flight
def test_size_change_in_flight_and_the_reuse_key(pkg, noise, oracle):
    """ensure_sky re-allocates both ring slots when the LUT's size changes; here it does so with a frame marched on the old size still in flight on
    the caller's stream.  The size is part of the reuse key, and a size change drops what was held: going back to the first size renders again.
    Measured on the GPU: the 200 x 100 LUT over the 31 x 9 table max 1 ulp from the oracle, 0.055 % of the halves differ."""
    import torch
    W, H = 512, 256
    sun = SUNS["deg45"]
    p = oracle.default_params(W, H, sun)
    whole = (H, 0, 1, 1)

    def fresh_frame(size):
        c = new_ctx(pkg, noise)
        try:
            out = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            c.render_sky_lut_device(sun, *size)
            c.render_clouds_device(p, W, whole, out.data_ptr(), W * 8, None)
            c.sync()
            return bits(out.cpu().numpy())
        finally:
            c.close()
    want = {size: fresh_frame(size) for size in (DEFAULT_SKY, (64, 33))}
    assert not np.array_equal(want[DEFAULT_SKY], want[(64, 33)]) and float((want[DEFAULT_SKY].view(np.float16)[..., 3] > 0).mean()) >= 0.25
    ctx = new_ctx(pkg, noise)
    try:
        st = torch.cuda.Stream()
        outs = [torch.full((H, W, 4), POISON, dtype=torch.int16, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        n0 = ctx.sky_lut_launches()
        counts = []
        for out, size in zip(outs, (DEFAULT_SKY, (64, 33), DEFAULT_SKY)):           # no host synchronisation between the steps
            ctx.render_sky_lut_device(sun, size[0], size[1], st.cuda_stream)
            counts.append(ctx.sky_lut_launches() - n0)
            ctx.render_clouds_device(p, W, whole, out.data_ptr(), W * 8, st.cuda_stream)
        ctx.render_sky_lut_device(sun, DEFAULT_SKY[0], DEFAULT_SKY[1], st.cuda_stream)     # the last request again
        counts.append(ctx.sky_lut_launches() - n0)
        st.synchronize()
        ctx.sync()
        assert counts == [1, 2, 3, 3], counts
        got = [bits(o.cpu().numpy()) for o in outs]
        assert np.array_equal(got[0], want[DEFAULT_SKY]) and np.array_equal(got[2], want[DEFAULT_SKY])
        assert np.array_equal(got[1], want[(64, 33)])
        table = ctx.render_transmittance(31, 9)                    # another table: the same sun and size are rendered again, over it
        lut = ctx.render_sky_lut(sun, *DEFAULT_SKY)
        assert ctx.sky_lut_launches() - n0 == 4
        d = ulp_diff(lut, oracle.sky_lut(sun, table, *DEFAULT_SKY))
        print("sky LUT 200 x 100 over the 31 x 9 table, GPU vs oracle: max %d fp16 ulp, %.4f %% differ" % (d.max(), 100.0 * (d > 0).mean()))
        assert d.max() <= 1
        assert not np.array_equal(bits(lut), bits(oracle.sky_lut(sun, oracle.transmittance_lut(*DEFAULT_TABLE), *DEFAULT_SKY)))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 7. compositor off the default shapes
class GpuInputs:
    """composite_inputs with the context as the provider: the table, the skies and the cloud frames are the context's own renders"""

    def __init__(self, ctx):
        self.ctx, self.memo = ctx, {}

    def table(self, w, h):
        return self.ctx.render_transmittance(w, h)

    def sky(self, sun, table, w, h):
        self.set_table(table.shape[1], table.shape[0])
        return self.ctx.render_sky_lut(sun, w, h)

    def clouds(self, params, sky):
        again = self.ctx.render_sky_lut(np.asarray(params[16:19], np.float32), sky.shape[1], sky.shape[0])      # the frame set-up filters the context's LUT
        assert np.array_equal(bits(again), bits(sky))
        return self.ctx.render_clouds(params)

    def set_table(self, w, h):
        if self.ctx.read_transmittance().shape != (h, w, 4):
            self.ctx.render_transmittance(w, h)

    def __call__(self, case):
        self.set_table(*case["table"])
        inputs = composite_inputs(case, self.table, self.sky, self.clouds, self.memo)
        self.set_table(*case["table"])                             # the table the compositor taps
        assert np.array_equal(bits(self.ctx.read_transmittance()), bits(inputs[4]))
        return inputs


def gpu_composite(ctx, case, inputs):
    cf, ct, sf, st, _, sun = inputs
    w, h = case["out"]
    if "fov" in case:
        return ctx.composite_view(cf, ct, sf, st, sun, right_angle_basis(case["yaw"], case["pitch"]), case["fov"], case["blend"], case["disk"], w, h)
    return ctx.composite_sky(cf, ct, sf, st, sun, case["blend"], case["disk"], w, h)


def test_compositor_off_the_default_shapes(pkg, ctxs, oracle):
    """composite_kernel with outputs narrower than one 32 x 8 block, one pixel high and one pixel wide, cloud frames of 8 x 8, 9 x 5 and 33 x 17,
    skies down to one texel, a 31 x 9 table, blend 0 and 1, disk scale 0, a sun under the horizon and at the zenith, cameras looking straight up
    (atan2f(0, 0) at the centre pixel) and straight down, fov 1 and 179: every input the context's own render.  Measured on the GPU:
    the six panorama cases max 1 ulp, 10 of 150 424 halves differ (0.0066 %); the five view cases are the oracle's bytes (14 804 halves)."""
    ctx = ctxs[0]
    make = GpuInputs(ctx)
    pools = {"panorama": Pool(), "view": Pool()}
    try:
        for case in PANORAMA_CASES + VIEW_CASES:
            inputs = make(case)
            assert not np.array_equal(bits(inputs[0]), bits(inputs[1])) and not np.array_equal(bits(inputs[2]), bits(inputs[3])), case
            img = gpu_composite(ctx, case, inputs)
            ref = oracle_composite(oracle, case, inputs)
            assert img.shape == ref.shape == (case["out"][1], case["out"][0], 4) and np.isfinite(img.astype(np.float32)).all(), case
            d = pools["view" if "fov" in case else "panorama"].add(img, ref)
            assert d.max() <= 2, (case, int(d.max()))
        for k, pool in pools.items():
            print("compositor, %s cases, GPU vs oracle: %s" % (k, pool))
        # grow-only scratch: a small call after a larger one writes the bytes it wrote before it, and those of a context that never grew
        small, large = PANORAMA_CASES[0], PANORAMA_CASES[-1]
        assert small["table"] == large["table"] == DEFAULT_TABLE
        ins, inl = make(small), make(large)
        grown, never = new_ctx(pkg), new_ctx(pkg)
        try:
            a = bits(gpu_composite(grown, small, ins)).copy()
            big = bits(gpu_composite(grown, large, inl)).copy()
            b = bits(gpu_composite(grown, small, ins)).copy()
            assert np.array_equal(a, b) and np.array_equal(a, bits(gpu_composite(never, small, ins)))
            assert np.array_equal(big, bits(gpu_composite(ctx, large, inl)))
        finally:
            grown.close(); never.close()
    finally:
        ctx.render_transmittance(*DEFAULT_TABLE)
        ctx.render_sky_lut(SUNS["deg45"], *DEFAULT_SKY)


# ---------------------------------------------------------------------------------------------------------------- 8. error paths
def test_error_paths(pkg):
    """Every CSKY_ERR_INVALID case of csky_composite_sky and csky_composite_view, and the one state they need nothing for: a context that has
    rendered nothing renders the default table itself."""
    L, lib = pkg.lib(), pkg._lib
    INV, OK = lib.ERR_INVALID, lib.OK
    nan = float("nan")
    ctx = new_ctx(pkg)
    try:
        h = ctx._h
        cloud, sky, out = np.zeros((4, 6, 4), np.uint16), np.zeros((3, 5, 4), np.uint16), np.zeros((7, 9, 4), np.uint16)
        cp, sp, op = (a.ctypes.data_as(C.c_void_p) for a in (cloud, sky, out))
        fields = dict(out_w=9, out_h=7, cloud_w=6, cloud_h=4, sky_w=5, sky_h=3)

        def params(**kw):
            f = dict(fields, **kw)
            q = lib.CompositeParams(f["out_w"], f["out_h"], f["cloud_w"], f["cloud_h"], f["sky_w"], f["sky_h"], 0.25, 2.0)
            q.light_direction[0], q.light_direction[1], q.light_direction[2] = 0.6, 0.8, 0.0
            return q

        def view(fov=70.0):
            return lib.View((C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), fov)

        def ref(x):
            return C.byref(x) if x is not None else None

        def pano(c=h, q=None, cf=cp, ct=cp, sf=sp, st=sp, o=op):
            return L.csky_composite_sky(c, ref(q), cf, ct, sf, st, o)

        def cam(c=h, q=None, v=None, cf=cp, ct=cp, sf=sp, st=sp, o=op):
            return L.csky_composite_view(c, ref(q), C.c_void_p(C.addressof(v)) if v is not None else None, cf, ct, sf, st, o)

        assert pano(q=params()) == OK                              # nothing rendered before: the context renders the default table itself
        assert ctx.read_transmittance().shape == (DEFAULT_TABLE[1], DEFAULT_TABLE[0], 4)
        assert cam(q=params(), v=view()) == OK
        assert pano(c=None, q=params()) == INV and cam(c=None, q=params(), v=view()) == INV
        assert pano(q=None) == INV and cam(q=None, v=view()) == INV
        assert cam(q=params(), v=None) == INV and cam(c=None, q=params(), v=None) == INV
        for arg in ("cf", "ct", "sf", "st", "o"):
            assert pano(q=params(), **{arg: None}) == INV and cam(q=params(), v=view(), **{arg: None}) == INV, arg
        for name in fields:
            for bad in (0, -1):
                assert pano(q=params(**{name: bad})) == INV and cam(q=params(**{name: bad}), v=view()) == INV, (name, bad)
        for name in ("out_w", "out_h"):
            assert pano(q=params(**{name: 16385})) == INV and cam(q=params(**{name: 16385}), v=view()) == INV, name
        assert b"size" in L.csky_last_error(h)
        for fov in (0.0, 180.0, -1.0, nan):
            assert cam(q=params(), v=view(fov)) == INV, fov
        assert b"fov" in L.csky_last_error(h)
        assert pano(q=params()) == OK and cam(q=params(), v=view(179.0)) == OK
        bare = new_ctx(pkg)
        try:
            assert cam(c=bare._h, q=params(), v=view()) == OK      # the view form on a context that has rendered nothing
            assert bare.read_transmittance().shape == (DEFAULT_TABLE[1], DEFAULT_TABLE[0], 4)
        finally:
            bare.close()
    finally:
        ctx.close()
