"""-m gpu: every buffer the once-per-texture-set kernels write (csrc/bake_kernels.hip, csrc/bc7enc.hip), read back and compared with a reference
that shares no code with them.

  mip_level_kernel, bake_{shape,detail,weather}_kernel, their fp32 "exact" forms, the unpacked fp16 detail chain, the weather map's range
  reduction and the inexact counter                              against tests/bake_reference.py (numpy; held against the host bake in
                                                                 tests/test_bake_reference.py), on white noise and on ramps that jump at every seam
  shape_noise_kernel / detail_noise_kernel at their smallest n   against oracle/noise_restatement.py, computed here
  bc7_encode_kernel at quality 0 and 1, 1x1 to 65 blocks         against the host build of its per-block code (tests/hostsim)

All integer or fp16 / fp32-bit work: every comparison is equality of bytes.  One context of this module's own; the session's gpu_ctx keeps the shipped
textures bound and is only read."""
import ctypes as C

import numpy as np
import pytest

import bake_reference as BR

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -5                                    # cloudsky.h


@pytest.fixture(scope="module")
def ctx(pkg):
    if pkg.lib().csky_device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible (libcloudsky has no CPU fallback)")
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(hostsim):
    """name -> (textures, reference Bake), computed once."""
    rank = hostsim.hostsim_shape_poly()
    return {name: (tex, BR.Bake(*tex, rank=rank)) for name, tex in (("W", BR.white_noise_set()), ("S", BR.seam_set()))}


def same(got, want, what):
    """Byte equality, reporting where it first breaks instead of two 150 MB arrays."""
    assert got.dtype == np.uint8 and got.size == want.size, (what, got.size, want.size)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail("%s: %d of %d bytes differ, first at %s: device %s, reference %s" % (what, bad.size, got.size, bad[:6], got[bad[:6]], want[bad[:6]]))


def check_held(ctx, ref, what):
    held = ctx.read_baked_texture(9)
    rec = held.view(np.dtype([("inexact", "<u8"), ("rmin", "<i4"), ("rmax", "<i4"), ("bmax", "<i4"), ("lod5", "<u4")]))[0]
    print("%s: device inexact %d range (%d, %d, %d) lod5 bits %#x; reference %d %s %#x" % (what, rec["inexact"], rec["rmin"], rec["rmax"], rec["bmax"], rec["lod5"],
                                                                                          ref.inexact, ref.range, np.float32(ref.lod5).view(np.uint32)))
    same(held, ref.held(), what + " which 9")
    assert ctx.noise_inexact_coeffs() == ref.inexact, what


def check_layouts(ctx, ref, what, exact):
    for which, want in ((3, ref.large_chain), (4, ref.small_chain), (0, ref.shape), (1, ref.detail), (2, ref.weather), (5, ref.detail_h)):
        same(ctx.read_baked_texture(which), want, "%s which %d" % (what, which))
    check_held(ctx, ref, what)
    if exact:
        for which, want in ((6, ref.shape32), (7, ref.detail32), (8, ref.weather32)):
            same(ctx.read_baked_texture(which), want, "%s which %d" % (what, which))
    else:
        for which in (6, 7, 8):
            with pytest.raises(Exception) as e:
                ctx.read_baked_texture(which)
            assert getattr(e.value, "code", None) == ERR_STATE and "exact cells" in str(e.value), (what, which, e.value)


def test_white_noise_set_bakes_to_the_reference(ctx, sets):
    """Set W: 105498 coefficients do not fit fp16, so the context builds the exact cells unasked and says so."""
    tex, ref = sets["W"]
    ctx.set_exact_cells(0)
    ctx.set_noise(*tex)
    assert ref.inexact == 105498
    check_layouts(ctx, ref, "W", exact=True)
    assert "exact fp32 cells" in ctx.last_warning() and str(ref.inexact) in ctx.last_warning()


def test_seam_set_after_white_noise_on_the_same_context(ctx, sets):
    """Set S after W: every layout again (the seam cells are where a clamp, or a neighbouring level's texels, would show), the range set by three
    single texels -- first lane of the first wave, last lane of the last, a lane 63 -- and a counter that restarts with the bind."""
    (wtex, wref), (stex, sref) = sets["W"], sets["S"]
    ctx.set_exact_cells(0)
    ctx.set_noise(*wtex)
    assert ctx.noise_inexact_coeffs() == wref.inexact
    ctx.set_exact_cells(1)
    ctx.set_noise(*stex)
    assert sref.range == (3, 250, 201) and 0 < sref.inexact < wref.inexact   # S's own count is told from W's and from the sum
    check_layouts(ctx, sref, "S, exact cells requested", exact=True)
    ctx.set_exact_cells(0)
    ctx.set_noise(*stex)
    check_layouts(ctx, sref, "S, exact cells not requested", exact=sref.inexact != 0)


def test_a_set_that_fits_fp16_has_no_exact_cells_to_read(gpu_ctx):
    """The shipped textures bake exactly and nobody asked for exact cells: 6..8 are refused by name, not read from a released buffer."""
    assert gpu_ctx.noise_inexact_coeffs() == 0
    for which in (6, 7, 8):
        with pytest.raises(Exception) as e:
            gpu_ctx.read_baked_texture(which)
        assert getattr(e.value, "code", None) == ERR_STATE and "exact cells" in str(e.value), (which, e.value)
    with pytest.raises(Exception) as e:
        gpu_ctx.read_baked_texture(10)
    assert getattr(e.value, "code", None) == ERR_INVALID and "0..9" in str(e.value)
    assert gpu_ctx.read_baked_texture(9).view(np.uint64)[0] == 0


@pytest.mark.parametrize("r,b", [(128, 0), (127, 255), (0, 0)])
def test_constant_weather_maps_pin_the_range_reduction(ctx, sets, r, b):
    """No texel differs from another: the result is the reduction's start values {255, 0, 0} met by atomics that change nothing or everything.
    (128, 0) is the ct_mode 1 side of the cloud-type branch, (127, 255) ct_mode 2."""
    stex, sref = sets["S"]
    weather = BR.seam_weather(r, 9, b, spikes=False)
    ctx.set_exact_cells(0)
    ctx.set_noise(stex[0], stex[1], weather)
    rec = ctx.read_baked_texture(9).view(np.int32)
    print("constant map R %d B %d: device range %s" % (r, b, tuple(rec[2:5])))
    assert tuple(int(v) for v in rec[2:5]) == (r, r, b)
    want, bad = BR.halves(BR.weather_cells(weather))
    assert bad == 0
    same(ctx.read_baked_texture(2), want.reshape(-1).view(np.uint8), "constant weather which 2")
    same(ctx.read_baked_texture(0), sref.shape, "constant weather which 0")


@pytest.mark.parametrize("n,ch,levels", BR.MIP_SHAPES)
def test_device_mips_equal_the_reference(ctx, n, ch, levels):
    inputs = BR.mip_inputs(n, ch)
    for name in ("random", "all255", "half_up"):
        same(ctx.build_mips(inputs[name], levels), BR.chain(BR.mips(inputs[name], levels)), "mips %s n %d ch %d levels %d" % (name, n, ch, levels))


def test_device_mips_refuse_a_level_without_a_texel(ctx):
    """n = 4 has three levels.  (Level counts of 32 and more, where the old check's shift was undefined, are asked of the shared rule on the CPU:
    tests/test_bake_reference.py.  They are not handed to a GPU.)"""
    buf = np.zeros(4096, np.uint8)
    rc = ctx._L.csky_build_mips_device(ctx._h, buf.ctypes.data_as(C.c_void_p), 4, 1, 4)
    assert rc == ERR_INVALID and not buf.any()


@pytest.mark.parametrize("seed,n", [(1, 8), (7, 16)])
def test_detail_generator_equals_the_restatement(ctx, seed, n):
    from oracle import noise_restatement as NR
    got = ctx.generate_detail_noise(seed, n)
    assert got.shape == (n, n, n, 3) and np.array_equal(got, NR.detail_volume(seed, n))


@pytest.mark.parametrize("seed,n", [(1, 8), (7, 16), (3, 32)])
def test_shape_generator_equals_the_restatement(ctx, seed, n):
    """n = 8 is the entry points' minimum: 512 voxels, two blocks of 256."""
    from oracle import noise_restatement as NR
    got = ctx.generate_shape_noise(seed, n)
    assert got.shape == (n, n, n, 4) and np.array_equal(got, NR.shape_volume(seed, n, min(8, n)))


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 4, 4), (3, 3, 5), (1, 52, 20), (2, 16, 16)])
def test_bc7_encoder_equals_its_host_build(ctx, hostsim, quality, n, h, w):
    """One block per lane, 64 lanes per workgroup: one block, ragged edges (texels repeated past them), 65 blocks = one lane of a second workgroup.
    Quality 1 (more partitions, end-point coordinate descent) had never run on the GPU."""
    rng = np.random.default_rng(1000 * n + 10 * h + w)
    img = np.clip(rng.normal(128, 30, size=(n, h, w, 4)), 0, 255).astype(np.uint8)
    want = np.zeros((n, (h + 3) // 4, (w + 3) // 4, 16), np.uint8)
    hostsim.hostsim_bc7_encode_quality.restype = None
    hostsim.hostsim_bc7_encode_quality.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    hostsim.hostsim_bc7_encode_quality(img.ctypes.data, w, h, n, quality, want.ctypes.data)
    got = ctx.encode_bc7(img, quality)
    assert got.shape == want.shape and want.any()
    bad = np.flatnonzero((got != want).reshape(-1, 16).any(1))
    assert bad.size == 0, "quality %d, %d x %d x %d: %d of %d blocks differ, first %s: device %s host %s" % (
        quality, n, h, w, bad.size, want.size // 16, bad[:4], got.reshape(-1, 16)[bad[:2]], want.reshape(-1, 16)[bad[:2]])
