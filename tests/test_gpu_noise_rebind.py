"""A rebind of the noise textures leaves nothing of the set before it behind: what tests/test_noise_set_host.py walks on the host (csrc/noise_set.h),
seen through the frames of one context that binds the shipped set, a weather map with another height window and another cloud-type mode, and the
shipped set again.  Every frame equals, bit for bit, the frame of a context that has only ever bound that set."""
import ctypes as C

import numpy as np
import pytest

from conftest import norm

pytestmark = pytest.mark.gpu

SUN = (1, 1, 0)
TILE = (512, 352, 64, 32)        # x, y, width, height inside the 2048 x 1024 frame: in cloud under both weather maps (asserted below)


def test_every_rebind_renders_like_a_fresh_context(pkg, noise, oracle):
    large, small, weather = noise
    stratus = weather.copy(); stratus[..., 0] //= 2; stratus[..., 2] = np.minimum(stratus[..., 2], 200)   # R all <= 127: ct_mode 2; another max B: another window
    assert stratus[..., 0].max() <= 127 and stratus[..., 2].max() != weather[..., 2].max() and weather[..., 0].min() >= 128
    p = oracle.default_params(2048, 1024, SUN)
    p[2], p[3] = TILE[0], TILE[1]
    made = []

    def context(w):
        ctx = pkg.Context(0)
        made.append(ctx)
        ctx.set_noise(large, small, w)
        ctx.render_transmittance(256, 64)
        ctx.render_sky_lut(norm(SUN), 200, 100)
        return ctx

    def render(ctx):
        img = ctx.render_clouds(p, TILE[2], TILE[3]).view(np.uint16).copy()
        n = int(ctx.cloud_stats()["incloud_samples"])
        assert n > 0                                         # an all-sky tile would compare equal whatever the context holds
        return img, n

    def same(a, b):
        return a[1] == b[1] and (a[0] == b[0]).all()

    try:
        fresh_shipped, fresh_stratus = render(context(weather)), render(context(stratus))
        assert not same(fresh_shipped, fresh_stratus)

        ctx = context(weather)
        assert same(render(ctx), fresh_shipped)
        ctx.set_noise(large, small, stratus)
        assert same(render(ctx), fresh_stratus)
        ctx.set_noise(large, small, weather)
        assert same(render(ctx), fresh_shipped)
        # arguments are checked before anything of the bound set is given up: a refused call leaves it bound
        ptr = lambda a: np.ascontiguousarray(a, np.uint8).ctypes.data_as(C.c_void_p)
        assert ctx._L.csky_set_noise(ctx._h, ptr(large), None, ptr(stratus)) == pkg._lib.ERR_INVALID
        assert same(render(ctx), fresh_shipped)
    finally:
        for c in made:
            c.close()
