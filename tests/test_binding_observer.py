"""What Context.render_clouds_view_from / render_clouds_dirs_from and CloudSky.cloud_view(position=...) hand libcloudsky (tests/test_binding_calls.py's
recorder and inputs; no GPU and no library call): the four symbols, csky_observer's sixteen bytes, the observer behind the view or the directions,
`position=None` as today's call, and every refusal as a ValueError before any library call."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from test_binding_calls import (BASIS, F16, F32, FOV, H, PARAMS, STREAM, W, at, bad_frame_tensors, bad_host_outs, bound, frame_tensors, is_new,  # noqa: F401
                                is_new_tensor, one_call, refuses, s_cloud, s_view)

POS = (50000.0, 1000.0, -30000.0)
INF = float("inf")
VIEW, VIEW_DEV = "csky_render_clouds_view_from", "csky_render_clouds_view_from_device"
DIRS, DIRS_DEV = "csky_render_clouds_dirs_from", "csky_render_clouds_dirs_from_device"


def s_observer(pos=POS, cap=INF):
    return struct.pack("4f", pos[0], pos[1], pos[2], cap)


def test_the_symbols_and_the_struct(pkg):
    names = {n: a for n, _, a in pkg._lib.SYMBOLS}
    O = pkg._lib.Observer
    assert C.sizeof(O) == 16 and O.position.offset == 0 and O.max_distance.offset == 12
    for n in (VIEW, VIEW_DEV, DIRS, DIRS_DEV):
        assert C.POINTER(O) in names[n] and hasattr(pkg.lib(), n)
    assert names[VIEW].index(C.POINTER(O)) == 3 and names[VIEW_DEV].index(C.POINTER(O)) == 3          # behind the view
    assert names[DIRS].index(C.POINTER(O)) == 5 and names[DIRS_DEV].index(C.POINTER(O)) == 5          # behind the directions
    assert bytes(pkg._lib._observer("f", POS, 20000.0)) == s_observer(POS, 20000.0)
    assert bytes(pkg._lib._observer("f", np.asarray(POS, F32), INF)) == s_observer()


def test_view_from(bound):  # noqa: F811
    ctx, rec = bound
    f = ctx.render_clouds_view_from
    out = f(PARAMS, BASIS, FOV, np.int64(W), H, POS)
    assert is_new(out, (H, W, 4))
    one_call(rec, VIEW, s_cloud(), s_view(), s_observer(), W, H, at(out))
    mine = np.zeros((H, W, 4), F16)
    assert f(PARAMS, BASIS, FOV, W, H, np.asarray(POS), 20000.0, out=mine) is mine
    one_call(rec, VIEW, s_cloud(), s_view(), s_observer(POS, 20000.0), W, H, at(mine))
    for _, t, pitch in frame_tensors():
        assert f(PARAMS, BASIS, FOV, W, H, POS, max_distance=7.5, out=t, stream=STREAM) is t
        one_call(rec, VIEW_DEV, s_cloud(), s_view(), s_observer(POS, 7.5), W, H, at(t), pitch, STREAM)
    for bad in bad_host_outs((H, W, 4)).values():
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, out=bad)
    for bad in bad_frame_tensors().values():
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, out=bad)
    for pos in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), (float("nan"), 0.0, 0.0), (0.0, INF, 0.0), (0.0, 0.0, -INF)):
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, pos)
    for cap in (0.0, -1.0, float("nan"), -INF):
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, POS, cap)


def test_dirs_from(bound):  # noqa: F811
    ctx, rec = bound
    f = ctx.render_clouds_dirs_from
    d = np.zeros((H, W, 3), F32)
    out = f(PARAMS, d, POS, 20000.0)
    assert is_new(out, (H, W, 4))
    one_call(rec, DIRS, s_cloud(), W, H, at(d), s_observer(POS, 20000.0), at(out))
    dt = torch.zeros(H, W, 3)
    for _, t, pitch in frame_tensors():
        assert f(PARAMS, dt, POS, out=t, stream=STREAM) is t
        one_call(rec, DIRS_DEV, s_cloud(), W, H, at(dt), s_observer(), at(t), pitch, STREAM)
    out = f(PARAMS, dt, POS)
    assert is_new_tensor(out, (H, W, 4))
    one_call(rec, DIRS_DEV, s_cloud(), W, H, at(dt), s_observer(), at(out), W * 8, 0)
    refuses(rec, f, PARAMS, np.zeros((H, W, 4), F32), POS)
    refuses(rec, f, PARAMS, d, POS, out=torch.zeros(H, W, 4, dtype=torch.float16))
    refuses(rec, f, PARAMS, dt, POS, out=np.zeros((H, W, 4), F16))
    refuses(rec, f, PARAMS, d, (0.0, 0.0))
    refuses(rec, f, PARAMS, d, POS, 0.0)


@pytest.mark.parametrize("device_buffers", [False, True])
def test_cloud_view_without_a_position_makes_todays_call(pkg, bound, device_buffers):  # noqa: F811
    ctx, rec = bound
    sky = pkg.CloudSky.__new__(pkg.CloudSky)
    sky.ctx, sky.device_buffers = ctx, device_buffers
    sky._fill_push_constant = lambda: PARAMS
    sky.frame_data = type("FD", (), {"LIGHT_DIRECTION": (0.0, 1.0, 0.0)})()
    sky._march_stream = lambda: (STREAM, lambda: None)
    ctx.device_id = 0
    if device_buffers:
        made = []
        real = torch.empty

        def empty(shape, dtype=None, device=None):
            made.append(real(shape, dtype=dtype))
            return made[-1]
        torch.empty, torch_device = empty, torch.device
        torch.device = lambda *a: "cpu"
        try:
            out = sky.cloud_view(BASIS, FOV, W, H)
            one_call(rec, "csky_render_clouds_view_device", s_cloud(), s_view(), W, H, at(out), W * 8, STREAM)
            out = sky.cloud_view(BASIS, FOV, W, H, position=None, max_distance=5.0)     # no position: the cap has nothing to act on
            one_call(rec, "csky_render_clouds_view_device", s_cloud(), s_view(), W, H, at(out), W * 8, STREAM)
            out = sky.cloud_view(BASIS, FOV, W, H, position=POS, max_distance=5.0)
            one_call(rec, VIEW_DEV, s_cloud(), s_view(), s_observer(POS, 5.0), W, H, at(out), W * 8, STREAM)
        finally:
            torch.empty, torch.device = real, torch_device
    else:
        out = sky.cloud_view(BASIS, FOV, W, H)
        one_call(rec, "csky_render_clouds_view", s_cloud(), s_view(), W, H, at(out))
        out = sky.cloud_view(BASIS, FOV, W, H, position=None)
        one_call(rec, "csky_render_clouds_view", s_cloud(), s_view(), W, H, at(out))
        out = sky.cloud_view(BASIS, FOV, W, H, position=POS)
        one_call(rec, VIEW, s_cloud(), s_view(), s_observer(), W, H, at(out))
    refuses(rec, sky.cloud_view, BASIS, FOV, W, H, aerial=True, position=POS)
    refuses(rec, sky.cloud_view, BASIS, FOV, W, H, position=(0.0, 1.0))
    refuses(rec, sky.cloud_view, BASIS, FOV, W, H, position=POS, max_distance=0.0)
