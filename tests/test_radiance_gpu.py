"""The sky's radiance cubemap on the GPU (csky_render_radiance*, csky_prefilter_cube): layer 0 against the oracle's compositor through the
six face cameras, the filtered layers against the numpy restatement (tests/radiance_reference.py), known answers, invariants, error paths
and the CloudSky methods."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import radiance_reference as R
from conftest import norm, ulp_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUNS = {"in_view": norm((-0.6, 0.35, 0.3)), "below": norm((0.3, -0.2, 0.9))}


def cloud_texture(seed):
    """A smooth synthetic 128 x 64 cloud texture (premultiplied colour + coverage): any RGBA16F image is a valid input of sky()."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, 64), np.linspace(0, 1, 128), indexing="ij")
    a = np.clip(0.5 + 0.45 * np.sin(6 * x + 3 * seed) * np.cos(5 * y) + 0.05 * rng.random((64, 128)), 0, 1)
    return np.stack([0.8 * a, 0.75 * a, 0.7 * a, a], -1).astype(np.float16)


@pytest.fixture(scope="module")
def rscene(gpu_ctx, oracle, o_trans):
    """Cloud textures and oracle sky LUTs for the two suns (one above the horizon, its disk in view; one below it)."""
    gpu_ctx.render_transmittance(256, 64)
    out = {}
    for k, sun in SUNS.items():
        sk = oracle.sky_lut(sun, o_trans)
        sk2 = oracle.sky_lut(norm(sun + np.array([0.0, 0.05, 0.0], np.float32)), o_trans)
        out[k] = dict(sun=sun, cl=cloud_texture(1), cl2=cloud_texture(2), sky=sk, sky2=sk2, tr=o_trans)
    return out


def radiance(ctx, s, S, L=8, Ss=0, first=0, n=None, out=None):
    return ctx.render_radiance(s["cl"], s["cl2"], s["sky"], s["sky2"], s["sun"], 0.25, 2.0, S, L, Ss, first, n, out)


smooth_cube = R.smooth_cube


@pytest.mark.gpu
@pytest.mark.parametrize("S", [8, 16, 64, 256])
@pytest.mark.parametrize("sun", sorted(SUNS))
def test_layer0_faces_match_the_view_compositor(gpu_ctx, oracle, rscene, S, sun):
    """Layer 0, face f == csky_composite_view through the camera of face f (header table), fov 90, S x S: the compositor's gate."""
    s = rscene[sun]
    cube = radiance(gpu_ctx, s, S, L=1)
    assert cube.shape == (1, 6, S, S, 4) and (cube[..., 3] == 1).all()
    d = np.stack([ulp_diff(cube[0, f], oracle.composite_view(s["cl"], s["cl2"], s["sky"], s["sky2"], s["tr"], s["sun"], R.face_basis(f), 90.0, 0.25, 2.0, S, S))
                  for f in range(6)])
    assert d.max() <= 2 and (d > 0).mean() < 0.02, (d.max(), (d > 0).mean())


def check_filtered(gpu, ref):
    d = ulp_diff(gpu.astype(np.float16), ref.astype(np.float16))
    assert d.max() <= 2 and (d <= 1).mean() >= 0.99, (d.max(), (d <= 1).mean())


@pytest.mark.gpu
@pytest.mark.parametrize("S", [16, 32])
def test_filtered_layers_match_numpy_every_texel(gpu_ctx, rscene, S):
    cube = radiance(gpu_ctx, rscene["in_view"], S, L=8, Ss=S)
    assert np.isfinite(cube.astype(np.float32)).all() and (cube[..., 3] == 1).all()
    ref = R.prefilter(cube[0].astype(np.float64), 8, S).reshape(7, 6, S, S, 3)
    check_filtered(cube[1:, ..., :3], ref)


@pytest.mark.gpu
def test_filtered_layers_match_numpy_sampled_64(gpu_ctx, rscene):
    S = 64
    cube = radiance(gpu_ctx, rscene["in_view"], S, L=8)                 # source_size 0 = min(S, 64)
    rng = np.random.default_rng(7)
    f, j, i = rng.integers(0, 6, 2000), rng.integers(0, S, 2000), rng.integers(0, S, 2000)
    ref = R.prefilter(cube[0].astype(np.float64), 8, 0, texels=(f, j, i))
    check_filtered(cube[1:, f, j, i, :3], ref)


@pytest.mark.gpu
def test_prefilter_known_answers(gpu_ctx):
    S = 16
    d = R.face_dirs(S)
    # a constant cube comes back exactly constant in every layer (any source size)
    const = np.broadcast_to(np.array([0.75, 1.5, 3.0, 1.0], np.float16), (6, S, S, 4)).copy()
    for Ss in (16, 8, 1):
        out = gpu_ctx.prefilter_cube(const, layers=8, source_size=Ss)
        assert (out.view(np.uint16) == const.view(np.uint16)[None]).all(), Ss
    # 1 + 0.5 y: the r = 1 layer is the cosine-weighted mean 1 + N_y / 3
    S2 = 32
    d2 = R.face_dirs(S2)
    lin = np.ones((6, S2, S2, 4), np.float16)
    lin[..., :3] = (1.0 + 0.5 * d2[..., 1:2]).astype(np.float16)
    top = gpu_ctx.prefilter_cube(lin, layers=8, source_size=S2)[-1].astype(np.float64)
    assert np.abs(top[..., :3] / (1.0 + d2[..., 1:2] / 3.0) - 1.0).max() < 5e-3
    # one hot texel: the r = 1 layer is proportional to max(N.L0, 0)
    hot = np.zeros((6, S, S, 4), np.float16)
    hot[..., 3] = 1.0
    hot[4, 7, 9, :3] = 1000.0
    top = gpu_ctx.prefilter_cube(hot, layers=8, source_size=S)[-1, ..., 0].astype(np.float64)
    c = d @ d[4, 7, 9]
    assert (top[c < -1e-4] == 0).all()
    ratio = top[c > 0.05] / c[c > 0.05]
    assert ratio.min() / ratio.max() > 0.99, (ratio.min(), ratio.max())
    # layer 0 is the input, byte for byte
    cube = smooth_cube(S, 3)
    out = gpu_ctx.prefilter_cube(cube, layers=4, source_size=S)
    assert (out[0].view(np.uint16) == cube.view(np.uint16)).all()


@pytest.mark.gpu
def test_prefilter_matches_numpy_with_a_smaller_source(gpu_ctx):
    cube = smooth_cube(32, 5)
    out = gpu_ctx.prefilter_cube(cube, layers=10, source_size=8)
    ref = R.prefilter(cube.astype(np.float64), 10, 8).reshape(9, 6, 32, 32, 3)
    check_filtered(out[1:, ..., :3], ref)


@pytest.mark.gpu
def test_incremental_equals_all_layers_and_calls_repeat(gpu_ctx, rscene):
    s = rscene["in_view"]
    whole = radiance(gpu_ctx, s, 64, L=8)
    again = radiance(gpu_ctx, s, 64, L=8)
    assert (whole.view(np.uint16) == again.view(np.uint16)).all()
    inc = np.zeros_like(whole)
    for k in range(8):
        radiance(gpu_ctx, s, 64, L=8, first=k, n=1, out=inc)
    assert (inc.view(np.uint16) == whole.view(np.uint16)).all()
    part = np.zeros_like(whole)
    radiance(gpu_ctx, s, 64, L=8, first=0, n=3, out=part)
    radiance(gpu_ctx, s, 64, L=8, first=3, n=5, out=part)
    assert (part.view(np.uint16) == whole.view(np.uint16)).all()
    only = np.zeros_like(whole)
    radiance(gpu_ctx, s, 64, L=8, first=5, n=2, out=only)                 # only the requested layers are written
    assert (only[[0, 1, 2, 3, 4, 7]].view(np.uint16) == 0).all() and (only[5:7].view(np.uint16) == whole[5:7].view(np.uint16)).all()


CULL_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import gvcd_amd
from radiance_reference import smooth_cube
ctx = gvcd_amd.Context(0)
np.save(sys.argv[1], ctx.prefilter_cube(smooth_cube(64, 11), layers=8).view(np.uint16))
ctx.close()
""" % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.gpu
def test_culling_off_gives_identical_bytes(gpu_ctx, tmp_path):
    on = gpu_ctx.prefilter_cube(smooth_cube(64, 11), layers=8).view(np.uint16)
    path = str(tmp_path / "nocull.npy")
    r = subprocess.run([sys.executable, "-c", CULL_CHILD, path], env=dict(os.environ, CSKY_RADIANCE_CULL="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert (np.load(path) == on).all()


# ------------------------------------------------------------------------------------------------ the header's whole range
# (S, Ss, L): together S in {8, 16, 64, 128, 256, 512}, Ss in {1, 2, 4, ..., 256} and every L in 2..10 (filter kernel NL = 1..9); the
# expensive source sizes (numpy cost ~ receivers x 6 Ss^2) get few layers
SWEEP = [(8, 1, 4), (8, 8, 10), (16, 2, 9), (16, 16, 8), (64, 4, 7), (64, 64, 3), (128, 32, 6), (128, 128, 2), (256, 8, 5), (256, 256, 2),
         (512, 16, 3)]
DISC = [(512, 1, 3), (512, 2, 3), (512, 4, 3), (512, 64, 3)]        # hdr_cube(512): the block mean over up to 512 x 512 texels


def ref_chunk(Ss):
    """Receivers per chunk of R.prefilter: about 32 MB per float64 [chunk, 6 Ss^2] temporary."""
    return max(1, (1 << 22) // (6 * Ss * Ss))


def sampled_receivers(S, seed, extra=None):
    """(face, row, col) of 2000 random receivers, the four corner texels of every face, row 0 of every face (a seam with a neighbouring face)
    and the texels `extra`."""
    rng = np.random.default_rng(seed)
    f, j, i = [rng.integers(0, 6, 2000)], [rng.integers(0, S, 2000)], [rng.integers(0, S, 2000)]
    c = np.array([0, S - 1])
    F, J, I = np.meshgrid(np.arange(6), c, c, indexing="ij")
    f.append(F.ravel()); j.append(J.ravel()); i.append(I.ravel())
    F, I = np.meshgrid(np.arange(6), np.arange(S), indexing="ij")
    f.append(F.ravel()); j.append(np.zeros(F.size, int)); i.append(I.ravel())
    if extra is not None:
        f.append(extra[0]); j.append(extra[1]); i.append(extra[2])
    return np.concatenate(f), np.concatenate(j), np.concatenate(i)


def check_prefiltered(out, cube, L, Ss, seed=0, extra=None):
    """prefilter_cube's result against numpy: every texel where that is cheap (S <= 32 or Ss <= 4), else sampled_receivers."""
    S = cube.shape[1]
    assert out.shape == (L, 6, S, S, 4)
    assert np.isfinite(out.astype(np.float32)).all() and (out[1:, ..., 3] == 1).all()
    assert (out[0].view(np.uint16) == cube.view(np.uint16)).all()
    c64 = cube.astype(np.float64)
    if S <= 32 or Ss <= 4:
        check_filtered(out[1:, ..., :3], R.prefilter(c64, L, Ss, chunk=ref_chunk(Ss)).reshape(L - 1, 6, S, S, 3))
    else:
        f, j, i = sampled_receivers(S, seed, extra)
        check_filtered(out[1:, f, j, i, :3], R.prefilter(c64, L, Ss, texels=(f, j, i), chunk=ref_chunk(Ss)))


@pytest.mark.gpu
@pytest.mark.parametrize("S,Ss,L", SWEEP)
def test_prefilter_geometry_sweep_matches_numpy(gpu_ctx, S, Ss, L):
    cube = smooth_cube(S, 100 + S + Ss)
    check_prefiltered(gpu_ctx.prefilter_cube(cube, layers=L, source_size=Ss), cube, L, Ss, seed=S + Ss)


@pytest.mark.gpu
@pytest.mark.parametrize("S,Ss,L", DISC)
def test_prefilter_bright_disc_matches_numpy(gpu_ctx, S, Ss, L):
    """A 30000 sun disc: every texel where Ss <= 4 (512 x 512 down to 1 x 1 is where an fp32 block mean drifted by 4 ulp), else sampled
    receivers plus every texel within 0.1 rad of the disc."""
    cube = R.hdr_cube(S, 30000.0)
    out = gpu_ctx.prefilter_cube(cube, layers=L, source_size=Ss)
    check_prefiltered(out, cube, L, Ss, seed=Ss, extra=np.nonzero(R.disc_angle(S) < 0.1))


@pytest.mark.gpu
@pytest.mark.parametrize("S,Ss,L", [(64, 16, 5), (16, 1, 6)])
def test_prefilter_three_black_faces(gpu_ctx, S, Ss, L):
    cube = smooth_cube(S, 21)
    cube[[0, 2, 4], ..., :3] = 0                                       # +X, +Y, +Z black
    out = gpu_ctx.prefilter_cube(cube, layers=L, source_size=Ss)
    # black outputs where every weighted source texel is black (at Ss = 1 the six face centres), lit ones elsewhere: numpy decides which
    assert (out[1:, ..., :3].astype(np.float32) > 0).any()
    check_filtered(out[1:, ..., :3], R.prefilter(cube.astype(np.float64), L, Ss).reshape(L - 1, 6, S, S, 3))
    assert np.isfinite(out.astype(np.float32)).all() and (out[1:, ..., 3] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("S,Ss,L", [(32, 4, 6), (32, 32, 4)])
def test_prefilter_subnormal_cube(gpu_ctx, S, Ss, L):
    """Values ~1e-6, fp16 subnormals in and out: f2h must round them, not flush them."""
    cube = smooth_cube(S, 22)
    cube[..., :3] = (cube[..., :3].astype(np.float32) * 1e-6).astype(np.float16)
    rgb = np.abs(cube[..., :3].astype(np.float32))
    assert (rgb > 0).all() and (rgb < 6.1e-5).all()
    out = gpu_ctx.prefilter_cube(cube, layers=L, source_size=Ss)
    f = out[1:, ..., :3].astype(np.float32)
    assert (f > 0).all() and (f < 6.1e-5).all()
    check_prefiltered(out, cube, L, Ss)


@pytest.mark.gpu
@pytest.mark.parametrize("S,Ss,L", SWEEP + DISC)
def test_culling_leaves_bytes_unchanged_at_every_geometry(gpu_ctx, monkeypatch, S, Ss, L):
    """rad_filter reads CSKY_RADIANCE_CULL at every call: source blocks that are whole faces (Ss <= 8) and the smallest receiver cones
    (S = 512) included."""
    cube = R.hdr_cube(S, 30000.0) if (S, Ss, L) in DISC else smooth_cube(S, 100 + S + Ss)
    on = gpu_ctx.prefilter_cube(cube, layers=L, source_size=Ss)
    monkeypatch.setenv("CSKY_RADIANCE_CULL", "0")
    off = gpu_ctx.prefilter_cube(cube, layers=L, source_size=Ss)
    assert (off.view(np.uint16) == on.view(np.uint16)).all()


# one context through geometries that grow and shrink every buffer of rad_prepare and rebuild both cone tables of both sets
SEQUENCE = [(512, 8, 64), (8, 2, 1), (128, 5, 128), (16, 9, 2), (512, 8, 64)]


@pytest.mark.gpu
def test_geometry_sequence_on_one_context_matches_fresh_contexts(pkg, rscene):
    s = rscene["in_view"]
    fresh = {}

    def run(ctx, kind, S, L, Ss):
        if kind == "render":
            return radiance(ctx, s, S, L=L, Ss=Ss)
        return ctx.prefilter_cube(smooth_cube(S, 300 + S), layers=L, source_size=Ss)

    def expected(kind, S, L, Ss):
        if (kind, S, L, Ss) not in fresh:
            c = pkg.Context(0)
            try:
                fresh[kind, S, L, Ss] = run(c, kind, S, L, Ss)
            finally:
                c.close()
        return fresh[kind, S, L, Ss]

    ctx = pkg.Context(0)
    try:
        for step, (S, L, Ss) in enumerate(SEQUENCE):
            got = {}
            for kind in (("render", "prefilter") if step % 2 == 0 else ("prefilter", "render")):
                got[kind] = run(ctx, kind, S, L, Ss)
                assert (got[kind].view(np.uint16) == expected(kind, S, L, Ss).view(np.uint16)).all(), (step, kind)
            whole = got["render"]
            # the snapshot survives prefilter_cube calls: layers 1..L-1 again from it, and they are the filter of its own layer 0
            inc = np.zeros_like(whole)
            radiance(ctx, s, S, L=L, Ss=Ss, first=1, n=L - 1, out=inc)
            assert (inc[1:].view(np.uint16) == whole[1:].view(np.uint16)).all(), step
            again = ctx.prefilter_cube(whole[0], layers=L, source_size=Ss)
            assert (again.view(np.uint16) == whole.view(np.uint16)).all(), step
    finally:
        ctx.close()


@pytest.mark.gpu
def test_incremental_equals_all_layers_at_a_non_default_geometry(gpu_ctx, rscene):
    s = rscene["below"]
    whole = radiance(gpu_ctx, s, 128, L=10, Ss=16)
    inc = np.zeros_like(whole)
    for k in range(10):
        radiance(gpu_ctx, s, 128, L=10, Ss=16, first=k, n=1, out=inc)
    assert (inc.view(np.uint16) == whole.view(np.uint16)).all()


@pytest.mark.gpu
def test_radiance_error_paths(pkg, noise, rscene):
    L, lib = pkg.lib(), pkg._lib
    ctx = pkg.Context(0)
    try:
        h = ctx._h
        cube = np.zeros((6, 16, 16, 4), np.uint16)
        out = np.zeros((10, 6, 32, 32, 4), np.uint16)
        P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        for S, nl, Ss, first, n in ((12, 8, 0, 0, 8), (4, 8, 0, 0, 8), (1024, 8, 0, 0, 8), (16, 0, 0, 0, 1), (16, 11, 0, 0, 11), (16, 8, 3, 0, 8),
                                    (16, 8, 32, 0, 8), (16, 8, -8, 0, 8), (16, 8, 0, -1, 2), (16, 8, 0, 0, 0), (16, 8, 0, 7, 2), (16, 8, 0, 8, 1)):
            assert L.csky_prefilter_cube(h, P(cube), S, nl, Ss, first, n, P(out)) == lib.ERR_INVALID, (S, nl, Ss, first, n)
        assert L.csky_prefilter_cube(h, None, 16, 8, 0, 0, 8, P(out)) == lib.ERR_INVALID
        assert L.csky_prefilter_cube(h, P(cube), 16, 8, 0, 0, 8, None) == lib.ERR_INVALID
        assert L.csky_prefilter_cube(None, P(cube), 16, 8, 0, 0, 8, P(out)) == lib.ERR_INVALID
        s = rscene["in_view"]
        u = [np.ascontiguousarray(s[k]).view(np.uint16) for k in ("cl", "cl2", "sky", "sky2")]
        sp = lib.CompositeParams(16, 16, 128, 64, 200, 100, 0.25, 2.0)
        rp = lib.RadianceParams(16, 8, 0)
        args = lambda sp, rp, first, n, o: (h, C.byref(sp) if sp else None, C.byref(rp) if rp else None, P(u[0]), P(u[1]), P(u[2]), P(u[3]), first, n, o)  # noqa: E731
        assert L.csky_render_radiance(*args(sp, None, 0, 8, P(out))) == lib.ERR_INVALID
        assert L.csky_render_radiance(*args(None, rp, 0, 8, P(out))) == lib.ERR_INVALID
        assert L.csky_render_radiance(*args(sp, rp, 0, 8, None)) == lib.ERR_INVALID
        assert L.csky_render_radiance(h, C.byref(sp), C.byref(rp), None, P(u[1]), P(u[2]), P(u[3]), 0, 8, P(out)) == lib.ERR_INVALID
        assert L.csky_render_radiance(*args(lib.CompositeParams(16, 32, 128, 64, 200, 100, 0.25, 2.0), rp, 0, 8, P(out))) == lib.ERR_INVALID   # out_h != S
        assert L.csky_render_radiance_device(h, C.byref(sp), C.byref(rp), None, None, None, None, 0, 8, None, None) == lib.ERR_INVALID
        # no snapshot yet (a fresh context): layers >= 1 are a state error
        assert L.csky_render_radiance(*args(sp, rp, 1, 1, P(out))) == lib.ERR_STATE
        assert L.csky_render_radiance(*args(sp, rp, 0, 1, P(out))) == lib.OK
        assert L.csky_render_radiance(*args(sp, rp, 1, 7, P(out))) == lib.OK
        assert L.csky_render_radiance(h, None, C.byref(rp), None, None, None, None, 1, 2, P(out)) == lib.OK     # layers >= 1 read no sky input
        for other in (lib.RadianceParams(32, 8, 0), lib.RadianceParams(16, 9, 0), lib.RadianceParams(16, 8, 8)):   # geometry change
            assert L.csky_render_radiance(*args(lib.CompositeParams(other.face_size, other.face_size, 128, 64, 200, 100, 0.25, 2.0), other, 1, 1, P(out))) == lib.ERR_STATE
        # csky_prefilter_cube leaves the snapshot alone
        assert L.csky_prefilter_cube(h, P(np.zeros((6, 32, 32, 4), np.uint16)), 32, 4, 0, 0, 4, P(out)) == lib.OK
        assert L.csky_render_radiance(*args(sp, rp, 1, 1, P(out))) == lib.OK
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cloudsky_radiance_cubemap_and_incremental_updates(pkg, noise):
    sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0)
    sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
    sky.update_sky()
    whole = sky.radiance_cubemap().copy()
    assert whole.shape == (8, 6, 64, 64, 4) and whole.dtype == np.float16
    assert np.isfinite(whole.astype(np.float32)).all() and (whole[..., 3] == 1).all() and whole[0, ..., :3].max() > 0.05
    sky.radiance[...] = 0
    for _ in range(8):
        sky.update_radiance()
    assert (sky.radiance.view(np.uint16) == whole.view(np.uint16)).all()
    sky.close()


@pytest.mark.gpu
def test_cloudsky_radiance_device_buffers(pkg, noise):
    import torch
    sky = pkg.CloudSky.from_default_resource(device_id=0, texture_size=(128, 64), noise=noise, clock=lambda: 0.0, device_buffers=True)
    sky.sun = pkg.cloud_sky.DirectionalLight(direction=(-0.6, 0.35, 0.3))
    sky.update_sky()
    whole = sky.radiance_cubemap(32, 6).clone()
    assert isinstance(whole, torch.Tensor) and whole.is_cuda and tuple(whole.shape) == (6, 6, 32, 32, 4)
    sky.radiance.zero_()
    for _ in range(6):
        sky.update_radiance(32, 6)
    torch.cuda.synchronize()
    assert torch.equal(sky.radiance.view(torch.int16), whole.view(torch.int16))
    assert torch.isfinite(whole.float()).all() and bool((whole[..., 3] == 1).all())
    sky.close()
