"""What Context.set_weather, set_weather_generated, generate_weather and CloudSky.set_weather hand libcloudsky (tests/test_binding_calls.py's recorder;
no GPU and no library call): the symbol each argument selects, the pointer, the struct's bytes, and every refusal as a ValueError before any
library call.  A device tensor is stood for by an object with the attributes the binding reads (data_ptr, shape, dtype, is_contiguous, device):
torch.device('cuda', n) can be named without a GPU, a tensor on it cannot be made."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from test_binding_calls import HANDLE, Recorder, at, bound, num, one_call, refuses  # noqa: F401

HOST, DEV, GEN = "csky_set_weather", "csky_set_weather_device", "csky_set_weather_generated"
SHAPE = (512, 512, 3)


class DeviceTensor:
    def __init__(self, shape=SHAPE, dtype=torch.uint8, contiguous=True, device=("cuda", 0), ptr=0x7000):
        self.shape, self.dtype, self._c, self.device, self._p = torch.Size(shape), dtype, contiguous, torch.device(*device), ptr

    def data_ptr(self):
        return self._p

    def is_contiguous(self):
        return self._c


def s_weather(**k):
    d = dict(coverage_freq=2, coverage_octaves=5, type_freq=6, type_octaves=3, phase=0.0, coverage_gain=0.9, dilate=0.55, coverage_centre=0.38,
             coverage_contrast=2.0, coverage_offset=0.06, coverage_floor=0.07, type_mean=0.748, type_spread=0.32)
    d.update(k)
    return struct.pack("4i9f", *[d[n] for n in ("coverage_freq", "coverage_octaves", "type_freq", "type_octaves", "phase", "coverage_gain", "dilate",
                                                "coverage_centre", "coverage_contrast", "coverage_offset", "coverage_floor", "type_mean", "type_spread")])


def test_the_symbols_and_the_struct(pkg):
    names = {n: a for n, _, a in pkg._lib.SYMBOLS}
    for n in (HOST, DEV, GEN, "csky_generate_weather", "csky_generate_weather_device", "csky_check_weather_params", "csky_weather_default_params"):
        assert n in names and hasattr(pkg.lib(), n)
    assert C.sizeof(pkg._lib.WeatherParams) == 52 and pkg._lib.WeatherParams.phase.offset == 16 and pkg._lib.WeatherParams.type_spread.offset == 48
    assert bytes(pkg._lib.weather_params()) == s_weather()
    assert bytes(pkg._lib.weather_params(phase=0.375, type_freq=4)) == s_weather(phase=0.375, type_freq=4)


def test_a_host_map_and_a_device_map_select_their_forms(bound):  # noqa: F811
    ctx, rec = bound
    w = np.zeros(SHAPE, np.uint8)
    assert ctx.set_weather(w) is None
    one_call(rec, HOST, at(w))
    t = DeviceTensor()
    ctx.set_weather(t)
    one_call(rec, DEV, 0x7000)


def test_w6_every_other_argument_is_refused_before_any_library_call(bound):  # noqa: F811
    ctx, rec = bound
    big = np.zeros((512, 512, 6), np.uint8)
    bad = [np.zeros((512, 512, 4), np.uint8), np.zeros((512, 512), np.uint8), np.zeros((256, 512, 3), np.uint8), np.zeros(512 * 512 * 3, np.uint8),     # shape
           np.zeros(SHAPE, np.int8), np.zeros(SHAPE, np.float32), np.zeros(SHAPE, np.uint16),                                                            # dtype
           big[..., ::2], np.zeros((512, 3, 512), np.uint8).transpose(0, 2, 1), np.zeros(SHAPE, np.uint8, order="F"),                                   # not contiguous
           torch.zeros(SHAPE, dtype=torch.uint8),                                                                                                       # a CPU tensor
           DeviceTensor(device=("cuda", 1)), DeviceTensor(device=("cpu",)),                                                                              # another device
           DeviceTensor(shape=(512, 512, 4)), DeviceTensor(dtype=torch.int8), DeviceTensor(dtype=torch.float16), DeviceTensor(contiguous=False),
           None, [[0, 0, 0]], b"\0" * (512 * 512 * 3)]
    assert bad[7].shape == SHAPE and bad[8].shape == SHAPE and bad[9].shape == SHAPE and not bad[7].flags.c_contiguous
    for b in bad:
        refuses(rec, ctx.set_weather, b)
    other = type(ctx)(1, _borrowed=HANDLE)                       # a context of device 1 takes the tensor of device 1 and refuses device 0's
    other._L = rec
    try:
        other.set_weather(DeviceTensor(device=("cuda", 1)))
        one_call(rec, DEV, 0x7000)
        refuses(rec, other.set_weather, DeviceTensor())
    finally:
        other._h = None


def test_the_generated_forms(bound, pkg):  # noqa: F811
    ctx, rec = bound
    ctx.set_weather_generated()
    one_call(rec, GEN, 1, s_weather())
    ctx.set_weather_generated(np.int64(9), phase=0.25, coverage_floor=0.5)
    one_call(rec, GEN, 9, s_weather(phase=0.25, coverage_floor=0.5))
    out = ctx.generate_weather(3, type_octaves=2)
    assert out.shape == SHAPE and out.dtype == np.uint8
    one_call(rec, "csky_generate_weather_device", 3, s_weather(type_octaves=2), at(out))
    out = ctx.generate_weather(3, device=False)
    assert [c[0] for c in rec.calls] == ["csky_generate_weather"]  # the host form takes no context
    name, args = rec.calls.pop()
    assert num(args[0]) == 3 and bytes(args[1]._obj) == s_weather() and num(args[2]) == at(out)
    with pytest.raises(TypeError):
        ctx.set_weather_generated(1, coverage=0.5)
    assert rec.calls == []


class FakeContext:
    def __init__(self):
        self.calls = []

    def set_weather(self, w):
        self.calls.append(("map", w))

    def set_weather_generated(self, seed, **knobs):
        self.calls.append(("seed", seed, knobs))


def test_cloud_sky_takes_a_map_or_a_seed(pkg):
    sky = pkg.CloudSky.__new__(pkg.CloudSky)                     # no context is created: set_weather reads ctx and _temporal alone
    sky.ctx, sky._temporal = FakeContext(), object()
    w = np.zeros(SHAPE, np.uint8)
    sky.set_weather(w)
    assert sky.ctx.calls == [("map", w)] and sky._temporal is None
    sky.set_weather(seed=3, phase=0.5)
    assert sky.ctx.calls[1] == ("seed", 3, dict(phase=0.5))
    for a, k in (((), {}), ((w,), dict(seed=3)), ((w,), dict(phase=0.5))):
        with pytest.raises(ValueError):
            sky.set_weather(*a, **k)
    assert len(sky.ctx.calls) == 2
