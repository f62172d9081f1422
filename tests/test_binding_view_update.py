"""What Context.render_clouds_view_update hands libcloudsky (tests/test_binding_calls.py's recorder and inputs; no GPU and no library call): the
symbol, both views byte for byte, the size, block and phase, the previous frame and the output each with its own pitch, NULL for a missing history,
and every refusal as a ValueError before any library call."""
import numpy as np
import torch

from test_binding_calls import (BASIS, F16, F32, FOV, H, PARAMS, STREAM, W, at, bad_frame_tensors, bad_host_outs, bound, frame_tensors, is_new,  # noqa: F401
                                is_new_tensor, one_call, one_row_tensor, refuses, s_cloud, s_view)

PREV_BASIS = [[9.0, 8.0, 7.0], [6.0, 5.0, 4.0], [3.0, 2.0, 1.0]]
PREV_FOV = 50.0
HOST, DEVICE = "csky_render_clouds_view_update", "csky_render_clouds_view_update_device"


def test_host_form(bound):  # noqa: F811
    ctx, rec = bound
    f = ctx.render_clouds_view_update
    out = f(PARAMS, BASIS, FOV, np.int64(W), H, 4, np.int64(7))
    assert is_new(out, (H, W, 4))
    one_call(rec, HOST, s_cloud(), s_view(), 0, W, H, 4, 7, 0, at(out))             # no history: prev_view and prev are NULL
    prev = np.ones((H, W, 4), F16)
    mine = np.zeros((H, W, 4), F16)
    assert f(PARAMS, BASIS, FOV, W, H, 2, 3, prev=prev, prev_basis=PREV_BASIS, prev_fov=PREV_FOV, out=mine) is mine
    one_call(rec, HOST, s_cloud(), s_view(), s_view(PREV_BASIS, PREV_FOV), W, H, 2, 3, at(prev), at(mine))
    for bad in bad_host_outs((H, W, 4)).values():
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, out=bad)
    for bad in (np.ones((H + 1, W, 4), F16), np.ones((H, W, 4), F32)):
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, prev=bad, prev_basis=PREV_BASIS, prev_fov=PREV_FOV)
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, prev=prev)                      # a previous frame without its camera
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, prev=prev, prev_basis=PREV_BASIS)
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, prev=prev, prev_basis=PREV_BASIS, prev_fov=PREV_FOV, out=torch.zeros(H, W, 4, dtype=torch.float16))


def test_device_form_takes_each_image_with_its_own_pitch(bound):  # noqa: F811
    ctx, rec = bound
    f = ctx.render_clouds_view_update
    for _, t, pitch in frame_tensors():                                              # no history: the output alone decides the form
        assert f(PARAMS, BASIS, FOV, W, H, 4, 7, out=t, stream=STREAM) is t
        one_call(rec, DEVICE, s_cloud(), s_view(), 0, W, H, 4, 7, 0, 0, at(t), pitch, STREAM)
    for _, prev, prev_pitch in frame_tensors():
        for _, t, pitch in frame_tensors():
            assert f(PARAMS, BASIS, FOV, W, H, 8, 63, prev=prev, prev_basis=PREV_BASIS, prev_fov=PREV_FOV, out=t) is t
            one_call(rec, DEVICE, s_cloud(), s_view(), s_view(PREV_BASIS, PREV_FOV), W, H, 8, 63, at(prev), prev_pitch, at(t), pitch, 0)
        out = f(PARAMS, BASIS, FOV, W, H, 1, 0, prev=prev, prev_basis=PREV_BASIS, prev_fov=PREV_FOV, stream=STREAM)   # a new output beside prev
        assert is_new_tensor(out, (H, W, 4))
        one_call(rec, DEVICE, s_cloud(), s_view(), s_view(PREV_BASIS, PREV_FOV), W, H, 1, 0, at(prev), prev_pitch, at(out), W * 8, STREAM)
    row = one_row_tensor()
    assert f(PARAMS, BASIS, FOV, W, 1, 4, 0, prev=row, prev_basis=PREV_BASIS, prev_fov=PREV_FOV, out=torch.zeros(1, W, 4, dtype=torch.float16)) is not row
    assert rec.calls.pop()[1][9].value == W * 8                                   # one row: its own size, not stride(0) * 2
    good = torch.zeros(H, W, 4, dtype=torch.float16)
    for bad in bad_frame_tensors().values():
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, out=bad)
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, prev=bad, prev_basis=PREV_BASIS, prev_fov=PREV_FOV, out=good)
        refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, prev=good, prev_basis=PREV_BASIS, prev_fov=PREV_FOV, out=bad)
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, prev=good, prev_basis=PREV_BASIS, prev_fov=PREV_FOV, out=np.zeros((H, W, 4), F16))   # a numpy out beside a device prev
    refuses(rec, f, PARAMS, BASIS, FOV, W, H, 4, 0, prev=good)
