"""What Context.render_clouds_view_from_depth / render_clouds_dirs_from_depth and CloudSky.cloud_view(scene_depth=...) hand libcloudsky
(tests/test_binding_calls.py's recorder and inputs; no GPU and no library call): the four symbols, csky_scene_depth's bytes, the depth buffer's
pointer and its own pitch, that a numpy depth selects the host form and a tensor the device form, and every refusal as a ValueError before any
library call."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from test_binding_calls import (BASIS, F16, F32, FOV, H, PARAMS, STREAM, W, at, bad_frame_tensors, bad_host_outs, bound, frame_tensors, is_new,  # noqa: F401
                                is_new_tensor, one_call, refuses, s_cloud, s_view)
from test_binding_observer import POS, s_observer

INF = float("inf")
VIEW, VIEW_DEV = "csky_render_clouds_view_from_depth", "csky_render_clouds_view_from_depth_device"
DIRS, DIRS_DEV = "csky_render_clouds_dirs_from_depth", "csky_render_clouds_dirs_from_depth_device"


def s_scene_depth(ptr, pitch, kind=0):
    return struct.pack("PNi4x", ptr, pitch, kind)                # const void*, size_t, int, padded to the pointer's alignment


def depth_tensors():
    """(tensor float32 [H, W] with contiguous texels, the pitch it must give)"""
    return [(torch.zeros(H, W), W * 4), (torch.zeros(H, 8)[:, :W], 32), (torch.zeros(2 * H, 8)[::2, :W], 64)]


def bad_depths(tensor):
    z = (lambda *s, **k: torch.zeros(*s, **k)) if tensor else (lambda *s, **k: np.zeros(s, **k))
    f64, i32 = (torch.float64, torch.int32) if tensor else (np.float64, np.int32)
    return {"float64": z(H, W, dtype=f64), "int32": z(H, W, dtype=i32), "transposed shape": z(W, H), "three dimensions": z(H, W, 1), "one row short": z(H - 1, W),
            "texels apart": z(H, 2 * W)[:, ::2], "rows backwards": z(H, W)[::-1] if not tensor else z(H, W).t().contiguous().t()}


def test_the_symbols_and_the_struct(pkg):
    names = {n: a for n, _, a in pkg._lib.SYMBOLS}
    S = pkg._lib.SceneDepth
    assert C.sizeof(S) == 24 and S.texels.offset == 0 and S.pitch_bytes.offset == 8 and S.kind.offset == 16
    assert pkg._lib.DEPTH_KINDS == {"distance": 0, "view_z": 1}
    for n in (VIEW, VIEW_DEV, DIRS, DIRS_DEV):
        assert C.POINTER(S) in names[n] and hasattr(pkg.lib(), n)
    assert names[VIEW].index(C.POINTER(S)) == 6 and names[VIEW_DEV].index(C.POINTER(S)) == 6           # behind w, h
    assert names[DIRS].index(C.POINTER(S)) == 6 and names[DIRS_DEV].index(C.POINTER(S)) == 6           # behind the observer
    z = np.zeros((H, 8), F32)[:, :W]
    d, device = pkg._lib._scene_depth("f", z, "view_z", W, H, True)
    assert bytes(d) == s_scene_depth(z.ctypes.data, 32, 1) and device is False


def test_view_from_depth(bound):  # noqa: F811
    ctx, rec = bound
    f = ctx.render_clouds_view_from_depth
    z = np.zeros((H, W), F32)
    out = f(PARAMS, BASIS, FOV, np.int64(W), H, POS, z)
    assert is_new(out, (H, W, 4))
    one_call(rec, VIEW, s_cloud(), s_view(), s_observer(), W, H, s_scene_depth(at(z), W * 4), at(out))
    zs = np.zeros((H, 8), F32)[:, :W]                                # a row-sliced host buffer keeps its own pitch
    mine = np.zeros((H, W, 4), F16)
    assert f(PARAMS, BASIS, FOV, W, H, POS, zs, "view_z", 20000.0, out=mine) is mine
    one_call(rec, VIEW, s_cloud(), s_view(), s_observer(POS, 20000.0), W, H, s_scene_depth(at(zs), 32, 1), at(mine))
    for zt, zpitch in depth_tensors():                               # the depth's pitch and the image's are independent
        for _, t, pitch in frame_tensors():
            assert f(PARAMS, BASIS, FOV, W, H, POS, zt, max_distance=7.5, out=t, stream=STREAM) is t
            one_call(rec, VIEW_DEV, s_cloud(), s_view(), s_observer(POS, 7.5), W, H, s_scene_depth(at(zt), zpitch), at(t), pitch, STREAM)
    zt = depth_tensors()[1][0]
    out = f(PARAMS, BASIS, FOV, W, H, POS, zt, depth_kind="view_z")  # a tensor depth alone selects the device form: a new tensor beside it
    assert is_new_tensor(out, (H, W, 4))
    one_call(rec, VIEW_DEV, s_cloud(), s_view(), s_observer(), W, H, s_scene_depth(at(zt), 32, 1), at(out), W * 8, 0)
    one = torch.zeros(1, 8)[:, :W]                                    # one row: the pitch is the row's own size, whatever stride(0) says
    out = f(PARAMS, BASIS, FOV, W, 1, POS, one)
    one_call(rec, VIEW_DEV, s_cloud(), s_view(), s_observer(), W, 1, s_scene_depth(at(one), W * 4), at(out), W * 8, 0)
    for tensor in (False, True):
        for bad in bad_depths(tensor).values():
            refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, bad)
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, z, "reversed_z")
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, z, out=torch.zeros(H, W, 4, dtype=torch.float16))     # a host depth beside a device out
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, torch.zeros(H, W), out=np.zeros((H, W, 4), F16))      # and the other way round
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, [[0.0] * W] * H)                                      # no array at all
    for bad in bad_host_outs((H, W, 4)).values():
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, z, out=bad)
    for bad in bad_frame_tensors().values():
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, torch.zeros(H, W), out=bad)
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, (1.0, 2.0), z)
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, z, max_distance=0.0)


def test_dirs_from_depth(bound):  # noqa: F811
    ctx, rec = bound
    f = ctx.render_clouds_dirs_from_depth
    d, z = np.zeros((H, W, 3), F32), np.zeros((H, 8), F32)[:, :W]
    out = f(PARAMS, d, POS, z, max_distance=20000.0)
    assert is_new(out, (H, W, 4))
    one_call(rec, DIRS, s_cloud(), W, H, at(d), s_observer(POS, 20000.0), s_scene_depth(at(z), 32), at(out))
    dt = torch.zeros(H, W, 3)
    for zt, zpitch in depth_tensors():
        for _, t, pitch in frame_tensors():
            assert f(PARAMS, dt, POS, zt, out=t, stream=STREAM) is t
            one_call(rec, DIRS_DEV, s_cloud(), W, H, at(dt), s_observer(), s_scene_depth(at(zt), zpitch), at(t), pitch, STREAM)
    zt = depth_tensors()[2][0]
    out = f(PARAMS, dt, POS, zt)
    assert is_new_tensor(out, (H, W, 4))
    one_call(rec, DIRS_DEV, s_cloud(), W, H, at(dt), s_observer(), s_scene_depth(at(zt), 64), at(out), W * 8, 0)
    refuses(rec, f, PARAMS, d, POS, z, "view_z")                      # view-z has no meaning without a camera
    refuses(rec, f, PARAMS, dt, POS, zt, "view_z")
    refuses(rec, f, PARAMS, d, POS, zt)                               # host directions beside a device depth
    refuses(rec, f, PARAMS, dt, POS, z)
    refuses(rec, f, PARAMS, d, POS, z, out=torch.zeros(H, W, 4, dtype=torch.float16))
    refuses(rec, f, PARAMS, dt, POS, zt, out=np.zeros((H, W, 4), F16))
    for tensor in (False, True):
        for bad in bad_depths(tensor).values():
            refuses(rec, f, PARAMS, dt if tensor else d, POS, bad)
    refuses(rec, f, PARAMS, d, (0.0, 0.0), z)


@pytest.mark.parametrize("device_buffers", [False, True])
def test_cloud_view_with_a_scene_depth(pkg, bound, device_buffers):  # noqa: F811
    ctx, rec = bound
    sky = pkg.CloudSky.__new__(pkg.CloudSky)
    sky.ctx, sky.device_buffers = ctx, device_buffers
    sky._fill_push_constant = lambda: PARAMS
    sky.frame_data = type("FD", (), {"LIGHT_DIRECTION": (0.0, 1.0, 0.0)})()
    sky._march_stream = lambda: (STREAM, lambda: None)
    ctx.device_id = 0
    z, zt = np.zeros((H, 8), F32)[:, :W], torch.zeros(H, 8)[:, :W]
    if device_buffers:
        real, torch_device = torch.empty, torch.device
        torch.empty = lambda shape, dtype=None, device=None: real(shape, dtype=dtype)
        torch.device = lambda *a: "cpu"
        try:
            out = sky.cloud_view(BASIS, FOV, W, H, scene_depth=zt)    # no position beside a depth: (0, 0, 0)
            one_call(rec, VIEW_DEV, s_cloud(), s_view(), s_observer((0.0, 0.0, 0.0)), W, H, s_scene_depth(at(zt), 32), at(out), W * 8, STREAM)
            out = sky.cloud_view(BASIS, FOV, W, H, position=POS, max_distance=5.0, scene_depth=zt, depth_kind="view_z")
            one_call(rec, VIEW_DEV, s_cloud(), s_view(), s_observer(POS, 5.0), W, H, s_scene_depth(at(zt), 32, 1), at(out), W * 8, STREAM)
            out = sky.cloud_view(BASIS, FOV, W, H, position=POS)     # without a depth: the call it was
            one_call(rec, "csky_render_clouds_view_from_device", s_cloud(), s_view(), s_observer(), W, H, at(out), W * 8, STREAM)
        finally:
            torch.empty, torch.device = real, torch_device
    else:
        out = sky.cloud_view(BASIS, FOV, W, H, scene_depth=z)
        one_call(rec, VIEW, s_cloud(), s_view(), s_observer((0.0, 0.0, 0.0)), W, H, s_scene_depth(at(z), 32), at(out))
        out = sky.cloud_view(BASIS, FOV, W, H, position=POS, max_distance=5.0, scene_depth=z, depth_kind="view_z")
        one_call(rec, VIEW, s_cloud(), s_view(), s_observer(POS, 5.0), W, H, s_scene_depth(at(z), 32, 1), at(out))
        out = sky.cloud_view(BASIS, FOV, W, H)
        one_call(rec, "csky_render_clouds_view", s_cloud(), s_view(), W, H, at(out))
    mine, other = (zt, z) if device_buffers else (z, zt)
    refuses(rec, sky.cloud_view, BASIS, FOV, W, H, scene_depth=other)                       # a depth of the other kind
    refuses(rec, sky.cloud_view, BASIS, FOV, W, H, aerial=True, scene_depth=mine)
    refuses(rec, sky.cloud_view, BASIS, FOV, W, H, scene_depth=mine, depth_kind="z")
    refuses(rec, sky.cloud_view, BASIS, FOV, W, H, scene_depth=np.zeros((H, W), np.float64))
    refuses(rec, sky.cloud_view, BASIS, FOV, W, H, scene_depth=mine, max_distance=0.0)
