"""The scenes the saturation skip (csrc/cloud_core.h ray_saturated, exact reject (4)) is walked on, in one place for the three files that use them:
tests/test_saturation_skip.py (tests/satwalk: the earliest possible freeze), tests/test_tile_walk.py (tests/tilewalk: the flush / replay / latch sequence in
both TALLY forms) and tests/test_gpu_saturation_range.py (the kernel itself, skip on against skip off).  They go where the proof's bound is tight and where its
guards bind: light energies from 0 to past the largest half, one colour channel dark, a bright ground, a dense and an empty medium, suns below the horizon
(the lower guard L >= 2^-14), and march lengths from 1 to 1024 steps.

`fired` is the number of rays tests/satwalk saw fire on this scene when the table was written (x86-64, libm transcendentals; the device's v_exp_f32 /
v_rcp_f32 may move it by a few rays).  A scene with fired > 0 must fire on at least a third of that (`floor`), the convention of the two CPU files, so that
no comparison passes by never firing; a scene with fired == 0 is a control and must not fire at all.  `empty` marks the scenes whose full march is allowed
to be (nearly) transparent."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

DEFAULT_SUN = (1, 1, 0)
LOW_SUN = (1.0, -0.2, 0.3)           # below the horizon, the sky LUT still lit: L is small
DARK_SUN = (0.3, -0.9, 0.3)          # far below: L under 2^-14 or zero, the lower guard keeps every ray marching
# indices into the 28-float push-constant block (oracle.default_params)
GROUND, ENERGY, COLOR = 12, 19, 20

# over: (index, value) pairs written into the block after default_params (the density is a field of its own: default_params takes it).
# early_out: csky_set_early_out for the GPU renders; the CPU walks have no early-out, so such a scene's `fired` is that of the scene without it.
Scene = namedtuple("Scene", "name size sun coverage density primary light over fired empty early_out")


def scene(name, fired, size=(256, 128), sun=DEFAULT_SUN, coverage=0.5, density=0.05, primary=128, light=6, over=(), empty=False, early_out=0.0):
    return Scene(name, size, sun, coverage, density, primary, light, tuple(over), fired, empty, early_out)


def load_satwalk(root):
    """builds and loads tests/satwalk (the fixture of the files that walk with it)"""
    d = os.path.join(root, "tests", "satwalk")
    subprocess.check_call(["make", "-C", d, "-s"])
    return C.CDLL(os.path.join(d, "libsatwalk.so"))


def mip_chains(pkg, noise):
    """the raw mip chains the CPU walks bake their cells from, and the weather map"""
    large, small, weather = noise
    return pkg.assets.build_mips(large, 8), pkg.assets.build_mips(small, 6), weather


def energy(e):
    return ((ENERGY, e),)


def ground(v):
    return tuple((GROUND + k, v) for k in range(3))


def floor(sc):
    """the least number of rays that must fire: a third of the measured count (None for a control, which must not fire at all)"""
    return None if sc.fired == 0 else -(-sc.fired // 3)


def params(oracle, sc):
    p = np.ascontiguousarray(oracle.default_params(sc.size[0], sc.size[1], sc.sun, coverage=sc.coverage, density=sc.density), np.float32).copy()
    for idx, val in sc.over:
        p[idx] = val
    return p


def stratus(weather):
    """the stratus-only weather map of test_stratus_only_weather_map: cloud type below 0.5 everywhere (ct_mode 2)"""
    w2 = weather.copy(); w2[..., 0] = w2[..., 0] // 2
    return w2


def check_fired(sc, fired):
    """`fired`: the rays a CPU walk of the scene saw fire (or latch)"""
    if sc.fired == 0:
        assert fired == 0, (sc.name, fired)
    else:
        assert fired >= floor(sc), (sc.name, fired, floor(sc))


# 256 x 128, coverage 0.5, sun (1, 1, 0), 128 x 6 steps unless said; 32 385 rays above the horizon (128 x 64: 8 001)
TABLE = [
    scene("energy-0", 20600, over=energy(0.0)),                     # the ambient term does not scale with the energy: these three are lit by it alone
    scene("energy-1e-4", 20599, over=energy(1e-4)),
    scene("energy-3e-3", 20560, over=energy(3e-3)),
    scene("energy-30", 20311, over=energy(30.0)),
    scene("energy-1e3", 19817, over=energy(1e3)),
    scene("energy-1e5", 19678, over=energy(1e5)),
    scene("energy-1e6", 19493, over=energy(1e6)),
    scene("energy-1e7", 12864, over=energy(1e7)),                   # part of the frame is past hi < 65504
    scene("energy-1e30", 0, over=energy(1e30)),                       # all of it is: nothing may fire
    scene("red-light", 20569, over=((COLOR + 1, 0.0), (COLOR + 2, 0.0))),
    scene("bright-ground", 20632, over=energy(0.0) + ground(0.9)),
    scene("density-5", 27358, density=5.0),
    scene("density-0", 0, density=0.0, empty=True),                  # dt = exp(0) = 1 for every sample: alpha stays 0
    scene("low-sun-1", 690, sun=LOW_SUN, over=ground(0.0)),
    scene("low-sun-1e-2", 653, sun=LOW_SUN, over=ground(0.0) + energy(1e-2)),
    scene("low-sun-1e-3", 666, sun=LOW_SUN, over=ground(0.0) + energy(1e-3)),
    scene("low-sun-1e-4", 658, sun=LOW_SUN, over=ground(0.0) + energy(1e-4)),
    scene("dark-sun", 0, sun=DARK_SUN, over=ground(0.0)),
    scene("16x0", 5198, size=(128, 64), primary=16, light=0),
    scene("1024x3", 2989, size=(128, 64), primary=1024, light=3),
    scene("2x0", 0, size=(128, 64), primary=2, light=0, empty=True),
    scene("1x6", 0, size=(128, 64), primary=1, light=6, empty=True),
]

# ---- scenes of tests/test_gpu_saturation_range.py alone
# (b) the two edges of the stored range at other coverages
EDGES = [
    scene("energy-1e7-cov-0.2", 129, coverage=0.2, over=energy(1e7)),
    scene("energy-1e7-cov-0.8", 22729, coverage=0.8, over=energy(1e7)),
    scene("dark-sun-cov-0.2", 0, coverage=0.2, sun=DARK_SUN, over=ground(0.0)),
    scene("dark-sun-cov-0.8", 0, coverage=0.8, sun=DARK_SUN, over=ground(0.0)),
]
# the ragged frame of tests/test_gpu_small_detail_lds.py (200 = 6 * 32 + 8 columns, 13 slabs): invalid lanes share wavefronts with rays that latch
RAGGED = [
    scene("ragged-energy-30", 12785, size=(200, 104), over=energy(30.0)),
    scene("ragged-energy-1e7", 8125, size=(200, 104), over=energy(1e7)),
    scene("ragged-red-light", 12996, size=(200, 104), over=((COLOR + 1, 0.0), (COLOR + 2, 0.0))),
    scene("ragged-density-5", 17340, size=(200, 104), density=5.0),
]
# (c) a dead lane and an early-out lane share `live`.  At 1e-3 a ray that could latch (alpha >= 1 - 2^-12, transmittance about 2.4e-4) is taken by the
# early-out at the same flush, so the skip is inert; at 1e-5 rays latch first.  The walks know no early-out: `fired` is the count of the same scene
# without it (energy 1).
EARLY_OUT = scene("early-out-1e-3", 20529, early_out=1e-3)
EARLY_OUT_DEEP = scene("early-out-1e-5", 20529, early_out=1e-5)
# (d) ct_mode 2: walked and rendered with stratus() of the shipped weather map
STRATUS = scene("stratus-cov-0.6", 17125, coverage=0.6)
# (e) blocks that break an assumption of the proof (tests/test_saturation_skip.py::test_negative_colour_switches_the_skip_off) and an infinite energy: the
# guard is evaluated by frame_setup_kernel on the device.  With a negative density every dt = exp(-density t ss) is above 1 and alpha only falls from 0:
# that frame is stored with alpha 0 everywhere (`empty`); the other seven change a colour or the energy, which alpha does not depend on.
REFUSED = [scene("refused-%s" % name, 0, over=over) for name, over in
           (("ground-r--0.2", ((GROUND, -0.2),)), ("ground-g--1e-3", ((GROUND + 1, -1e-3),)), ("ground-b--5", ((GROUND + 2, -5.0),)), ("light-r--1", ((COLOR, -1.0),)),
            ("light-g--0.01", ((COLOR + 1, -0.01),)), ("energy--1", ((ENERGY, -1.0),)), ("energy-inf", ((ENERGY, float("inf")),)))]
REFUSED.append(scene("refused-density--0.05", 0, density=-0.05, empty=True))
