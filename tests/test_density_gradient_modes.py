"""cloud_core.h::density_height_gradient takes the cloud-type mode either from FrameConsts::ct_mode (the generic form, template value 0) or as a
template value (1: every cloud-type texel of the bound map >= 128, 2: every texel <= 127), which the persistent cloud kernels are compiled with.  A
specialised form must be the generic form's branch for that mode, bit for bit: the host build of the cores (tests/gradient_host) evaluates both over a grid
of height fractions and cloud types inside the mode's range.  The generic form itself, over the mixed range, picks mode 1's branch at and above 127.5 and
mode 2's below it: the three bodies are one function."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import _make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gradient():
    d = os.path.join(ROOT, "tests", "gradient_host")
    _make(d)
    lib = C.CDLL(os.path.join(d, "libgradient_host.so"))
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    lib.gradient_forms.argtypes = [C.c_int, C.c_int, fp, fp, C.c_int, up, up]
    lib.gradient_forms.restype = C.c_int

    def forms(mode, ct, hf, typ):
        hf, typ = np.ascontiguousarray(hf, np.float32), np.ascontiguousarray(typ, np.float32)
        a, b = np.empty(hf.size, np.uint32), np.empty(hf.size, np.uint32)
        assert lib.gradient_forms(mode, ct, hf.ctypes.data_as(fp), typ.ctypes.data_as(fp), hf.size, a.ctypes.data_as(up), b.ctypes.data_as(up)) == 0
        return a, b
    return forms


def grid(lo, hi):
    """height fractions over [0, 1] with the ramps' corners and their fp32 neighbours, x cloud types on the texel scale: every integer texel of [lo, hi],
    bilinear mixes between them and the ends' fp32 neighbours inside the range"""
    hf = np.concatenate([np.linspace(0.0, 1.0, 1001, dtype=np.float32), np.float32([0.02, 0.03, 0.05, 0.09, 0.11, 0.18, 0.25, 0.3375, 0.48, 0.78])])
    hf = np.unique(np.concatenate([hf, np.nextafter(hf, np.float32(2.0)), np.nextafter(hf, np.float32(-1.0))]).clip(0.0, 1.0))
    typ = np.concatenate([np.arange(lo, hi + 1, dtype=np.float32), np.random.default_rng(5).uniform(lo, hi, 257).astype(np.float32),
                          np.float32([np.nextafter(np.float32(lo), np.float32(300.0)), np.nextafter(np.float32(hi), np.float32(-1.0))])])
    H, T = np.meshgrid(hf, typ, indexing="ij")
    return H.ravel(), T.ravel()


@pytest.mark.parametrize("mode,lo,hi", [(1, 128, 255), (2, 0, 127)])
def test_specialised_form_is_the_generic_branch(gradient, mode, lo, hi):
    hf, typ = grid(lo, hi)
    generic, compiled = gradient(mode, mode, hf, typ)
    assert np.array_equal(generic, compiled), int((generic != compiled).sum())
    g = generic.view(np.float32)
    assert np.isfinite(g).all() and g.min() >= 0.0 and g.max() <= 1.0 and g.max() > 0.9 and len(np.unique(generic)) > 1000     # a real gradient, not a constant
    # inside its range the mode's branch is also what the mixed form picks per sample
    mixed, again = gradient(0, 0, hf, typ)
    assert np.array_equal(mixed, again) and np.array_equal(mixed, generic), int((mixed != generic).sum())


def test_modes_differ_where_they_should(gradient):
    """the two branches are different functions (a form wired to the wrong mode would show): on each mode's own range the other branch gives other bits"""
    for mode, other, lo, hi in ((1, 2, 128, 255), (2, 1, 0, 127)):
        hf, typ = grid(lo, hi)
        want, wrong = gradient(mode, other, hf, typ)
        assert (want != wrong).mean() > 0.05, (mode, float((want != wrong).mean()))
