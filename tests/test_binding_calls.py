"""What the Python binding (_lib.py Context) hands libcloudsky for given arrays: the symbol, every struct byte for byte, every pointer, integer and
pitch, and what the method returns.  No GPU and no library call: the context's library is replaced by a recorder whose every export appends
(name, args) and returns 0, and torch CPU tensors stand for device tensors (the binding reads only data_ptr, stride, shape, element_size, dtype,
is_contiguous and .device).  The structs are packed here field by field from include/cloudsky.h's layout.  Inputs are the smallest that can go
wrong: a ragged 5 x 3 image, rows of 8 texels sliced to 5 (pitch 64), one row, one column, a basis of nine distinct values, a sun of (3, 4, 12).
Every refusal is a ValueError raised before any library call."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

HANDLE = 0x5EED
W, H = 5, 3
SUN = (3.0, 4.0, 12.0)                                           # not a unit vector: used as given
BASIS = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]]
FOV = 70.0
PARAMS = np.arange(28, dtype=np.float32) * 0.5 + 1.0
PARAMS[0:2] = (7, 4)                                             # texture_size: the defaulted frame size
STREAM = 0x77
F16, F32 = np.float16, np.float32


class Recorder:
    """Stands for the loaded library.  A call is held to the real export's argtypes (a numpy integer that reached a c_int would fail there too)."""

    def __init__(self, symbols):
        self.argtypes = {name: args for name, _, args in symbols}
        self.calls = []
        self.during = None                                       # called inside the export, while the binding's temporaries are alive

    def __getattr__(self, name):
        types = self.__dict__["argtypes"][name]                  # KeyError: the binding called something the headers do not declare

        def export(*args):
            assert len(args) == len(types), (name, len(args), len(types))
            for t, a in zip(types, args):
                t.from_param(a)
            if self.during:
                self.during(name, args)
            self.calls.append((name, args))
            return 0
        return export


@pytest.fixture
def bound(pkg):
    ctx = pkg.Context(0, _borrowed=HANDLE)                       # loads the library; creates and destroys no context
    rec = Recorder(pkg._lib.SYMBOLS)
    ctx._L = rec
    yield ctx, rec
    ctx._h = None


# ---- the C header's layouts
def s_cloud(p=PARAMS):
    return struct.pack("28f", *[float(x) for x in p])


def s_sky(w, h, sun=SUN):
    return struct.pack("8f", w, h, 0, 0, sun[0], sun[1], sun[2], 0)


def s_view(basis=BASIS, fov=FOV):
    return struct.pack("10f", *([basis[k % 3][k // 3] for k in range(9)] + [fov]))   # column-major: element k is row k % 3 of column k // 3


def s_composite(out_w, out_h, cloud_w, cloud_h, sky_w, sky_h, blend, disk, light=SUN):
    return struct.pack("6i2f3f", out_w, out_h, cloud_w, cloud_h, sky_w, sky_h, blend, disk, *light)


def s_shadow(w, h, center, extent, steps):
    return struct.pack("2i2f2fi", w, h, *center, *extent, steps)


def s_aerial(w, h, d, steps, far_km, aspect, sun=SUN):
    return struct.pack("4i2f3f", w, h, d, steps, far_km, aspect, *sun)


def s_depth(w, h, steps):
    return struct.pack("3i", w, h, steps)


def s_cloud_aerial(w, h, steps, sun=SUN):
    return struct.pack("3i3f", w, h, steps, *sun)


def test_the_layouts_are_the_bindings(pkg):
    L = pkg._lib
    for cls, n in ((L.CloudParams, 112), (L.SkyParams, 32), (L.View, 40), (L.CompositeParams, 44), (L.ShadowParams, 28), (L.AerialParams, 36),
                   (L.DepthParams, 12), (L.CloudAerialParams, 24), (L.RadianceParams, 12)):
        assert C.sizeof(cls) == n, cls


# ---- reading a recorded call
def num(a):
    if a is None:
        return 0
    if hasattr(a, "value"):
        return a.value or 0
    assert type(a) is int, type(a)
    return a


def blob(a, n):
    if hasattr(a, "_obj"):                                       # byref(struct)
        assert C.sizeof(a._obj) == n
        return bytes(a._obj)
    return C.string_at(a.value, n)                               # the same bytes handed over as void*


def at(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def one_call(rec, name, *want):
    """The recorder holds exactly this call: ctx first, a bytes item is a struct, an int is an integer, a pitch or a pointer."""
    assert [c[0] for c in rec.calls] == [name]
    args = rec.calls.pop()[1]
    assert len(args) == len(want) + 1 and num(args[0]) == HANDLE
    for k, (a, w) in enumerate(zip(args[1:], want), 1):
        if isinstance(w, bytes):
            assert blob(a, len(w)) == w, (name, k)
        else:
            assert num(a) == w, (name, k, num(a), w)


def is_new(a, shape, dtype=F16):
    return isinstance(a, np.ndarray) and a.shape == tuple(shape) and a.dtype == dtype and a.flags.c_contiguous


def is_new_tensor(t, shape):
    return isinstance(t, torch.Tensor) and tuple(t.shape) == tuple(shape) and t.dtype == torch.float16 and t.is_contiguous() and t.device.type == "cpu"


def refuses(rec, fn, *a, **kw):
    with pytest.raises(ValueError):
        fn(*a, **kw)
    assert rec.calls == []


# ---- the image arguments the cases share
def frame_tensors():
    """(name, tensor [h, w, 4] of 2-byte elements with contiguous texels, the pitch it must give)"""
    return [("contiguous", torch.zeros(H, W, 4, dtype=torch.float16), W * 8),
            ("rows of 8 sliced to 5", torch.zeros(H, 8, 4, dtype=torch.float16)[:, :W], 64),
            ("int16", torch.zeros(H, 8, 4, dtype=torch.int16)[:, :W], 64)]


def one_row_tensor():
    t = torch.zeros(1, 8, 4, dtype=torch.float16)[:, :W]
    assert t.stride(0) == 32                                     # what the pitch must not be read from
    return t


def one_column_tensor():
    t = torch.zeros(H, 2, 8, dtype=torch.float16)[:, :1, :4]
    assert tuple(t.stride()) == (16, 8, 1)                       # stride(1) is not 4: the test of it is skipped for one column
    return t


def bad_frame_tensors(shape=(H, W, 4)):
    h, w, c = shape
    return {"wrong shape": torch.zeros(w, h, c, dtype=torch.float16),
            "two dimensions": torch.zeros(h, w * c, dtype=torch.float16),
            "4-byte elements": torch.zeros(h, w, c, dtype=torch.float32),
            "texels not contiguous": torch.zeros(h, w, 2 * c, dtype=torch.float16)[:, :, ::2],
            "texels apart": torch.zeros(h, w, 2 * c, dtype=torch.float16)[:, :, :c]}


def bad_host_outs(shape):
    wrong = (shape[0] + 1,) + tuple(shape[1:])
    wide = tuple(shape[:-1]) + (2 * shape[-1],)
    return {"wrong shape": np.zeros(wrong, F16), "float32": np.zeros(shape, F32), "not contiguous": np.zeros(wide, F16)[..., ::2]}


# ---------------------------------------------------------------------------------------------------------------- sky LUT
def test_sky_lut(bound):
    ctx, rec = bound
    out = ctx.render_sky_lut(SUN, W, H)
    assert is_new(out, (H, W, 4))
    one_call(rec, "csky_render_sky_lut", s_sky(W, H), at(out))
    assert ctx.render_sky_lut(SUN, readback=False) is None
    one_call(rec, "csky_render_sky_lut", s_sky(200, 100), 0)
    assert ctx.render_sky_lut_device(SUN, W, H, stream=STREAM) is None
    one_call(rec, "csky_render_sky_lut_device", s_sky(W, H), STREAM)
    ctx.render_sky_lut_device(SUN)
    one_call(rec, "csky_render_sky_lut_device", s_sky(200, 100), 0)
    assert ctx.render_sky_lut_rows_device(SUN, np.int64(1), 2, 0x1000, 4096, w=W, h=H, stream=STREAM) is None
    one_call(rec, "csky_render_sky_lut_rows_device", s_sky(W, H), 1, 2, 0x1000, 4096, STREAM)


# ---------------------------------------------------------------------------------------------------------------- hemisphere frame
def test_render_and_submit_clouds(bound):
    ctx, rec = bound
    out = ctx.render_clouds(PARAMS)
    assert is_new(out, (4, 7, 4))
    one_call(rec, "csky_render_clouds", s_cloud(), 7, 4, at(out), 56)
    out = ctx.render_clouds(PARAMS, np.int64(W), H)
    assert is_new(out, (H, W, 4))
    one_call(rec, "csky_render_clouds", s_cloud(), W, H, at(out), W * 8)
    assert ctx.submit_clouds(PARAMS) == -1                       # the ticket as initialised: the recorder writes none
    one_call(rec, "csky_submit_clouds", s_cloud(), 7, 4, struct.pack("q", -1))
    assert ctx._shapes == {-1: (4, 7)}
    assert ctx.submit_clouds(PARAMS, np.int64(W), H) == -1
    one_call(rec, "csky_submit_clouds", s_cloud(), W, H, struct.pack("q", -1))
    assert ctx._shapes == {-1: (H, W)}
    refuses(rec, ctx.render_clouds, PARAMS[:27])


# ---------------------------------------------------------------------------------------------------------------- shadow map
CENTER, EXTENT = (10.0, 20.0), (300.0, 400.0)


def map_tensors():
    """(tensor [h, w] of 2-byte elements, pitch)"""
    one_col = torch.zeros(H, 4, dtype=torch.float16)[:, ::2][:, :1]
    assert tuple(one_col.stride()) == (4, 2)
    return [(torch.zeros(H, W, dtype=torch.float16), W * 2), (torch.zeros(H, 8, dtype=torch.float16)[:, :W], 16),
            (torch.zeros(1, 8, dtype=torch.float16)[:, :W], W * 2), (one_col, 8), (torch.zeros(H, 8, dtype=torch.int16)[:, :W], 16)]


def test_render_cloud_shadow(bound):
    ctx, rec = bound
    sp = s_shadow(W, H, CENTER, EXTENT, 9)
    out = ctx.render_cloud_shadow(PARAMS, np.int64(W), H, CENTER, EXTENT, 9)
    assert is_new(out, (H, W))
    one_call(rec, "csky_render_cloud_shadow", s_cloud(), sp, at(out))
    mine = np.zeros((H, W), F16)
    assert ctx.render_cloud_shadow(PARAMS, W, H, CENTER, EXTENT, 9, out=mine) is mine
    one_call(rec, "csky_render_cloud_shadow", s_cloud(), sp, at(mine))
    out = ctx.render_cloud_shadow(PARAMS, W, H)
    one_call(rec, "csky_render_cloud_shadow", s_cloud(), s_shadow(W, H, (0.0, 0.0), (16384.0, 16384.0), 64), at(out))
    for t, pitch in map_tensors():
        h, w = t.shape
        assert ctx.render_cloud_shadow(PARAMS, np.int64(w), h, CENTER, EXTENT, 9, out=t, stream=STREAM) is t
        one_call(rec, "csky_render_cloud_shadow_device", s_cloud(), s_shadow(w, h, CENTER, EXTENT, 9), at(t), pitch, STREAM)
    for why, bad in bad_host_outs((H, W)).items():
        refuses(rec, ctx.render_cloud_shadow, PARAMS, W, H, out=bad)
    for bad in (torch.zeros(W, H, dtype=torch.float16), torch.zeros(H, W, 1, dtype=torch.float16), torch.zeros(H, W, dtype=torch.float32),
                torch.zeros(H, 2 * W, dtype=torch.float16)[:, ::2]):
        refuses(rec, ctx.render_cloud_shadow, PARAMS, W, H, out=bad)


# ---------------------------------------------------------------------------------------------------------------- aerial volume
D = 2
VOL = (D, H, W, 4)


@pytest.mark.parametrize("view", [None, (BASIS, FOV)])
def test_render_aerial_perspective(bound, view):
    ctx, rec = bound
    ap = s_aerial(W, H, D, 3, 16.0, 1.5)
    v = 0 if view is None else s_view()
    kw = dict(width=np.int64(W), height=H, depth=D, far_km=16.0, steps_per_slice=3, view=view, aspect=1.5)
    out = ctx.render_aerial_perspective(SUN, **kw)
    assert is_new(out, VOL)
    one_call(rec, "csky_render_aerial_perspective", ap, v, at(out))
    mine = np.zeros(VOL, F16)
    assert ctx.render_aerial_perspective(SUN, out=mine, **kw) is mine
    one_call(rec, "csky_render_aerial_perspective", ap, v, at(mine))
    for t in (torch.zeros(VOL, dtype=torch.float16), torch.zeros(VOL, dtype=torch.int16)):
        assert ctx.render_aerial_perspective(SUN, out=t, stream=STREAM, **kw) is t
        one_call(rec, "csky_render_aerial_perspective_device", ap, v, at(t), STREAM)
    for bad in bad_host_outs(VOL).values():
        refuses(rec, ctx.render_aerial_perspective, SUN, out=bad, **kw)
    for bad in (torch.zeros((D, W, H, 4), dtype=torch.float16), torch.zeros(VOL, dtype=torch.float32), torch.zeros((D, H, 8, 4), dtype=torch.float16)[:, :, :W]):
        refuses(rec, ctx.render_aerial_perspective, SUN, out=bad, **kw)


def test_render_aerial_perspective_defaults(bound):
    ctx, rec = bound
    out = ctx.render_aerial_perspective(SUN)
    assert is_new(out, (32, 32, 32, 4))
    one_call(rec, "csky_render_aerial_perspective", s_aerial(32, 32, 32, 2, 32.0, 0.0), 0, at(out))


@pytest.mark.parametrize("view", [None, (BASIS, FOV)])
def test_render_aerial_perspective_shadowed(bound, view):
    ctx, rec = bound
    ap = s_aerial(W, H, D, 3, 16.0, 1.5)
    v = 0 if view is None else s_view()
    kw = dict(width=W, height=np.int64(H), depth=D, far_km=16.0, steps_per_slice=3, view=view, aspect=1.5)
    MW, MH = 5, 3                                                # the map's own size, read from the map
    sp = s_shadow(MW, MH, CENTER, EXTENT, 0)
    m = np.arange(MH * MW, dtype=F16).reshape(MH, MW)
    out = ctx.render_aerial_perspective_shadowed(SUN, m, CENTER, EXTENT, **kw)
    assert is_new(out, VOL)
    one_call(rec, "csky_render_aerial_perspective_shadowed", ap, v, sp, at(m), at(out))   # a contiguous float16 map is read where it lies
    mine = np.zeros(VOL, F16)
    seen = []
    rec.during = lambda name, args: seen.append(C.string_at(args[4].value, MH * MW * 2))
    strided = np.arange(MH * 8, dtype=F16).reshape(MH, 8)[:, :MW]
    assert ctx.render_aerial_perspective_shadowed(SUN, strided, CENTER, EXTENT, out=mine, **kw) is mine
    rec.during = None
    assert seen == [np.ascontiguousarray(strided).tobytes()]     # a strided one through a contiguous copy
    assert num(rec.calls[0][1][4]) != at(strided)
    one_call(rec, "csky_render_aerial_perspective_shadowed", ap, v, sp, num(rec.calls[0][1][4]), at(mine))
    for t, pitch in map_tensors():
        mh, mw = t.shape
        spt = s_shadow(mw, mh, CENTER, EXTENT, 0)
        out = ctx.render_aerial_perspective_shadowed(SUN, t, CENTER, EXTENT, stream=STREAM, **kw)
        assert is_new_tensor(out, VOL)
        one_call(rec, "csky_render_aerial_perspective_shadowed_device", ap, v, spt, at(t), pitch, at(out), STREAM)
        mine_t = torch.zeros(VOL, dtype=torch.int16)
        assert ctx.render_aerial_perspective_shadowed(SUN, t, CENTER, EXTENT, out=mine_t, **kw) is mine_t
        one_call(rec, "csky_render_aerial_perspective_shadowed_device", ap, v, spt, at(t), pitch, at(mine_t), 0)
    f = ctx.render_aerial_perspective_shadowed
    for bad in list(bad_host_outs(VOL).values()) + [torch.zeros(VOL, dtype=torch.float16), [0.0]]:   # a host map with a tensor, or with no array at all
        refuses(rec, f, SUN, m, CENTER, EXTENT, out=bad, **kw)
    for bad_map in (m.astype(F32), np.zeros((MH, MW, 1), F16), np.zeros(MW, F16)):
        refuses(rec, f, SUN, bad_map, CENTER, EXTENT, **kw)
    t = map_tensors()[1][0]
    for bad in (np.zeros(VOL, F16), torch.zeros((D, W, H, 4), dtype=torch.float16), torch.zeros(VOL, dtype=torch.float32),
                torch.zeros((D, H, 8, 4), dtype=torch.float16)[:, :, :W]):
        refuses(rec, f, SUN, t, CENTER, EXTENT, out=bad, **kw)
    for bad_map in (torch.zeros(MH, MW, dtype=torch.float32), torch.zeros(MH, MW, 1, dtype=torch.float16), torch.zeros(MH, 2 * MW, dtype=torch.float16)[:, ::2]):
        refuses(rec, f, SUN, bad_map, CENTER, EXTENT, **kw)


# ---------------------------------------------------------------------------------------------------------------- frames from a push-constant block
def frame_calls(ctx):
    """(method, symbol, what stands between the push-constant block and the image in the host call, leading arguments, keyword arguments)"""
    size = (W, H)
    return [(ctx.render_cloud_depth, "csky_render_cloud_depth", (s_depth(W, H, 11),), (PARAMS, np.int64(W), H), dict(steps=11)),
            (ctx.render_clouds_view, "csky_render_clouds_view", (s_view(),) + size, (PARAMS, BASIS, FOV, np.int64(W), H), {}),
            (ctx.render_cloud_depth_view, "csky_render_cloud_depth_view", (s_view(),) + size + (11,), (PARAMS, BASIS, FOV, W, np.int64(H)), dict(steps=11))]


def test_frames_of_the_hemisphere_and_of_a_view(bound):
    ctx, rec = bound
    for f, sym, mid, a, kw in frame_calls(ctx):
        out = f(*a, **kw)
        assert is_new(out, (H, W, 4)), sym
        one_call(rec, sym, s_cloud(), *mid, at(out))
        mine = np.zeros((H, W, 4), F16)
        assert f(*a, out=mine, **kw) is mine
        one_call(rec, sym, s_cloud(), *mid, at(mine))
        for why, t, pitch in frame_tensors():
            assert f(*a, out=t, stream=STREAM, **kw) is t
            one_call(rec, sym + "_device", s_cloud(), *mid, at(t), pitch, STREAM)
        for why, bad in bad_host_outs((H, W, 4)).items():
            refuses(rec, f, *a, out=bad, **kw)
        for why, bad in bad_frame_tensors().items():
            refuses(rec, f, *a, out=bad, **kw)


def test_one_row_and_one_column(bound):
    ctx, rec = bound
    row, col = one_row_tensor(), one_column_tensor()
    assert ctx.render_cloud_depth(PARAMS, W, 1, out=row) is row
    one_call(rec, "csky_render_cloud_depth_device", s_cloud(), s_depth(W, 1, 0), at(row), W * 8, 0)     # not stride(0) * 2
    assert ctx.render_cloud_depth(PARAMS, 1, H, out=col) is col
    one_call(rec, "csky_render_cloud_depth_device", s_cloud(), s_depth(1, H, 0), at(col), 32, 0)
    assert ctx.render_clouds_view(PARAMS, BASIS, FOV, W, 1, out=row) is row
    one_call(rec, "csky_render_clouds_view_device", s_cloud(), s_view(), W, 1, at(row), W * 8, 0)
    assert ctx.render_clouds_view(PARAMS, BASIS, FOV, 1, H, out=col) is col
    one_call(rec, "csky_render_clouds_view_device", s_cloud(), s_view(), 1, H, at(col), 32, 0)
    assert ctx.render_cloud_depth_view(PARAMS, BASIS, FOV, W, 1, out=row) is row
    one_call(rec, "csky_render_cloud_depth_view_device", s_cloud(), s_view(), W, 1, 0, at(row), W * 8, 0)
    assert ctx.render_cloud_depth_view(PARAMS, BASIS, FOV, 1, H, out=col) is col
    one_call(rec, "csky_render_cloud_depth_view_device", s_cloud(), s_view(), 1, H, 0, at(col), 32, 0)
    d_row, d_col = torch.zeros(1, W, 3), torch.zeros(H, 1, 3)
    assert ctx.render_clouds_dirs(PARAMS, d_row, out=row) is row
    one_call(rec, "csky_render_clouds_dirs_device", s_cloud(), W, 1, at(d_row), at(row), W * 8, 0)
    assert ctx.render_cloud_depth_dirs(PARAMS, d_col, out=col) is col
    one_call(rec, "csky_render_cloud_depth_dirs_device", s_cloud(), 1, H, 0, at(d_col), at(col), 32, 0)
    col_apart = torch.zeros(H, 2, 8, dtype=torch.float16)[:, :1, ::2]
    refuses(rec, ctx.render_cloud_depth, PARAMS, 1, H, out=col_apart)   # one column skips the test of stride(1), not that of the texel


def test_frames_of_caller_given_rays(bound):
    ctx, rec = bound
    for f, sym, mid, kw in ((ctx.render_clouds_dirs, "csky_render_clouds_dirs", (W, H), {}),
                            (ctx.render_cloud_depth_dirs, "csky_render_cloud_depth_dirs", (W, H, 11), dict(steps=11))):
        d = np.arange(H * W * 3, dtype=F32).reshape(H, W, 3)
        out = f(PARAMS, d, **kw)
        assert is_new(out, (H, W, 4))
        one_call(rec, sym, s_cloud(), *mid, at(d), at(out))      # contiguous float32 directions are read where they lie
        mine = np.zeros((H, W, 4), F16)
        seen = []
        rec.during = lambda name, args: seen.append(C.string_at(args[-2].value, H * W * 12))
        assert f(PARAMS, d.astype(np.float64), out=mine, **kw) is mine
        rec.during = None
        assert seen == [d.tobytes()]                             # others through a float32 copy
        one_call(rec, sym, s_cloud(), *mid, num(rec.calls[0][1][-2]), at(mine))
        t = torch.zeros(H, W, 3)
        out = f(PARAMS, t, stream=STREAM, **kw)
        assert is_new_tensor(out, (H, W, 4))
        one_call(rec, sym + "_device", s_cloud(), *mid, at(t), at(out), W * 8, STREAM)
        for why, o, pitch in frame_tensors():
            assert f(PARAMS, t, out=o, **kw) is o
            one_call(rec, sym + "_device", s_cloud(), *mid, at(t), at(o), pitch, 0)
        refuses(rec, f, PARAMS, t, out=mine)                     # device dirs with a numpy out
        refuses(rec, f, PARAMS, d, out=frame_tensors()[0][1])    # and the reverse
        for bad in (np.zeros((H, W, 4), F32), np.zeros((H, W), F32), torch.zeros(H, W, 4), torch.zeros(H, W, 3, dtype=torch.float64),
                    torch.zeros(H, W, 6)[:, :, ::2], torch.zeros(H, 8, 3)[:, :W]):
            refuses(rec, f, PARAMS, bad, **kw)
        for why, bad in bad_host_outs((H, W, 4)).items():
            refuses(rec, f, PARAMS, d, out=bad, **kw)
        for why, bad in bad_frame_tensors().items():
            refuses(rec, f, PARAMS, t, out=bad, **kw)


# ---------------------------------------------------------------------------------------------------------------- the aerial step on a frame
def apply_calls(ctx):
    """(method, symbol, what stands between the struct and the frames: host, device; leading arguments as a function of the kind)"""
    d_host, d_dev = np.zeros((H, W, 3), F32), torch.zeros(H, W, 3)
    return [(ctx.apply_cloud_aerial, "csky_apply_cloud_aerial", (), (), lambda dev: (SUN,)),
            (ctx.apply_cloud_aerial_dirs, "csky_apply_cloud_aerial_dirs", (at(d_host),), (at(d_dev),), lambda dev: (SUN, d_dev if dev else d_host)),
            (ctx.apply_cloud_aerial_view, "csky_apply_cloud_aerial_view", (s_view(),), (s_view(),), lambda dev: (SUN, BASIS, FOV))]


def test_apply_cloud_aerial_and_its_ray_forms(bound):
    ctx, rec = bound
    ca = s_cloud_aerial(W, H, 5)
    for f, sym, mid_h, mid_d, lead in apply_calls(ctx):
        c, z = np.zeros((H, W, 4), F16), np.ones((H, W, 4), F16)
        out = f(*lead(False), c, z, steps=5)
        assert is_new(out, (H, W, 4)), sym
        one_call(rec, sym, ca, *mid_h, at(c), at(z), at(out))    # contiguous float16 frames are read where they lie
        assert f(*lead(False), c, z, steps=5, out=c) is c        # out may be the cloud frame
        one_call(rec, sym, ca, *mid_h, at(c), at(z), at(c))
        out = f(*lead(False), c, z)
        one_call(rec, sym, s_cloud_aerial(W, H, 16), *mid_h, at(c), at(z), at(out))
        tc, tz = torch.zeros(H, W, 4, dtype=torch.float16), torch.zeros(H, W, 4, dtype=torch.int16)
        out = f(*lead(True), tc, tz, steps=5, stream=STREAM)
        assert is_new_tensor(out, (H, W, 4))
        one_call(rec, sym + "_device", ca, *mid_d, at(tc), at(tz), at(out), STREAM)
        assert f(*lead(True), tc, tz, steps=5, out=tc) is tc
        one_call(rec, sym + "_device", ca, *mid_d, at(tc), at(tz), at(tc), 0)
        # refusals
        refuses(rec, f, *lead(False), c, np.zeros((H, W + 1, 4), F16))                   # cloud and depth of different sizes
        refuses(rec, f, *lead(False), np.zeros((H, W, 3), F16), np.zeros((H, W, 3), F16))
        refuses(rec, f, *lead(False), np.zeros((H, W * 4), F16), np.zeros((H, W * 4), F16))
        refuses(rec, f, *lead(False), c.astype(F32), z)
        refuses(rec, f, *lead(False), c, z.astype(F32))
        refuses(rec, f, *lead(False), c, z, out=torch.zeros(H, W, 4, dtype=torch.float16))   # a host cloud with a tensor out
        for why, bad in bad_host_outs((H, W, 4)).items():
            refuses(rec, f, *lead(False), c, z, out=bad)
        refuses(rec, f, *lead(True), tc, z)                                              # a device cloud with a host depth
        refuses(rec, f, *lead(True), tc, tz, out=np.zeros((H, W, 4), F16))
        pitched = torch.zeros(H, 8, 4, dtype=torch.float16)[:, :W]
        for bad in (pitched, torch.zeros(H, W, 4, dtype=torch.float32)):                 # these frames have no pitch: contiguous or refused
            refuses(rec, f, *lead(True), bad, tz)
            refuses(rec, f, *lead(True), tc, bad)
            refuses(rec, f, *lead(True), tc, tz, out=bad)


def test_apply_cloud_aerial_dirs_refuses_other_dirs(bound):
    ctx, rec = bound
    c, z = np.zeros((H, W, 4), F16), np.zeros((H, W, 4), F16)
    tc, tz = torch.zeros(H, W, 4, dtype=torch.float16), torch.zeros(H, W, 4, dtype=torch.float16)
    f = ctx.apply_cloud_aerial_dirs
    seen = []
    rec.during = lambda name, args: seen.append(C.string_at(args[2].value, H * W * 12))
    d64 = np.arange(H * W * 3, dtype=np.float64).reshape(H, W, 3)
    f(SUN, d64, c, z)
    rec.during = None
    assert seen == [d64.astype(F32).tobytes()]                   # host directions of another type through a float32 copy
    rec.calls.clear()
    refuses(rec, f, SUN, np.zeros((H, W + 1, 3), F32), c, z)     # dirs of another size than the frames
    refuses(rec, f, SUN, np.zeros((H, W, 4), F32), c, z)
    refuses(rec, f, SUN, torch.zeros(H + 1, W, 3), tc, tz)
    refuses(rec, f, SUN, torch.zeros(H, W, 3), c, z)             # device dirs with host frames
    refuses(rec, f, SUN, np.zeros((H, W, 3), F32), tc, tz)       # and the reverse
    refuses(rec, f, SUN, torch.zeros(H, W, 3, dtype=torch.float64), tc, tz)
    refuses(rec, f, SUN, torch.zeros(H, W, 6)[:, :, ::2], tc, tz)


# ---------------------------------------------------------------------------------------------------------------- compositor and radiance
SW, SH = 7, 2


def four_frames():
    return [np.zeros((H, W, 4), F16), np.ones((H, W, 4), F16), np.zeros((SH, SW, 4), F16), np.ones((SH, SW, 4), F16)]


def test_composites(bound):
    ctx, rec = bound
    fr = four_frames()
    ptrs = [at(x) for x in fr]                                   # contiguous frames are read where they lie
    out = ctx.composite_sky(*fr, SUN, 0.25, 3.0, np.int64(6), 2)
    assert is_new(out, (2, 6, 4))
    one_call(rec, "csky_composite_sky", s_composite(6, 2, W, H, SW, SH, 0.25, 3.0), *ptrs, at(out))
    out = ctx.composite_sky(*fr, SUN)
    one_call(rec, "csky_composite_sky", s_composite(2048, 1024, W, H, SW, SH, 0.0, 2.0), *ptrs, at(out))
    out = ctx.composite_view(*fr, SUN, BASIS, FOV, 0.25, 3.0, 6, 2)
    assert is_new(out, (2, 6, 4))
    one_call(rec, "csky_composite_view", s_composite(6, 2, W, H, SW, SH, 0.25, 3.0), s_view(), *ptrs, at(out))
    out = ctx.composite_view(*fr, SUN, BASIS, FOV)
    assert is_new(out, (648, 1152, 4))
    one_call(rec, "csky_composite_view", s_composite(1152, 648, W, H, SW, SH, 0.0, 2.0), s_view(), *ptrs, at(out))
    out = ctx.composite_view_frames(*fr, SUN, BASIS, FOV, 0.25, 3.0)
    assert is_new(out, (H, W, 4))                                # the view frames' own size
    one_call(rec, "csky_composite_view_frames", s_composite(W, H, W, H, SW, SH, 0.25, 3.0), s_view(), *ptrs, at(out))
    seen = []
    rec.during = lambda name, args: seen.append(C.string_at(args[2].value, H * W * 8))   # cloud_from
    strided = np.arange(H * 8 * 4, dtype=F16).reshape(H, 8, 4)[:, :W]
    ctx.composite_sky(strided, *fr[1:], SUN, out_w=6, out_h=2)
    rec.during = None
    assert seen == [np.ascontiguousarray(strided).tobytes()]
    rec.calls.clear()


def test_render_radiance(bound):
    ctx, rec = bound
    fr = four_frames()
    ptrs = [at(x) for x in fr]
    S, L = 2, 3
    cp = s_composite(S, S, W, H, SW, SH, 0.25, 3.0)
    out = ctx.render_radiance(*fr, SUN, 0.25, 3.0, face_size=np.int64(S), layers=L, source_size=1, first_layer=1)
    assert is_new(out, (L, 6, S, S, 4))
    one_call(rec, "csky_render_radiance", cp, struct.pack("3i", S, L, 1), *ptrs, 1, 2, at(out))   # n_layers None: the layers from first_layer on
    mine = np.zeros((L, 6, S, S, 4), F16)
    assert ctx.render_radiance(*fr, SUN, 0.25, 3.0, S, L, 0, 0, np.int64(1), out=mine) is mine
    one_call(rec, "csky_render_radiance", cp, struct.pack("3i", S, L, 0), *ptrs, 0, 1, at(mine))
    for why, bad in bad_host_outs((L, 6, S, S, 4)).items():
        refuses(rec, ctx.render_radiance, *fr, SUN, face_size=S, layers=L, out=bad)
    assert ctx.render_radiance_device(0x1000, 0, 0x3000, None, (np.int64(W), H), (SW, SH), SUN, 0.25, 3.0, S, L, 1, 1, np.int64(2), 0x9000, stream=STREAM) is None
    one_call(rec, "csky_render_radiance_device", cp, struct.pack("3i", S, L, 1), 0x1000, 0, 0x3000, 0, 1, 2, 0x9000, STREAM)
