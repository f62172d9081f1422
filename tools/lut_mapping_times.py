"""Render the transmittance LUT (256 x 64) and the sky LUT (200 x 100, the demo scene's sun) 50 times in every transmittance-LUT mapping the
given library knows (cloudsky.h CSKY_TLUT_*), for a kernel trace:

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o lut -- python tools/lut_mapping_times.py PATH/libcloudsky.so

Raw ctypes against the .so, so that a library built from a commit without the mapping entry points runs the same script (mapping 0 only):
DESIGN.md 12 compares the two (profiles/r10/lut_kernel_stats_{change,parent}.csv)."""
import ctypes as C
import sys

import numpy as np

L = C.CDLL(sys.argv[1])
ctx = C.c_void_p()
assert L.csky_create(C.byref(ctx), 0) == 0
tp = (C.c_float * 4)(256.0, 64.0, 0.0, 0.0)
sp = (C.c_float * 8)(200.0, 100.0, 0.0, 0.0, -0.998773, 0.0495291, 2.69869e-07, 0.0)
t = np.zeros((64, 256, 4), np.uint16)
s = np.zeros((100, 200, 4), np.uint16)
P = lambda a: a.ctypes.data_as(C.c_void_p)
maps = [0, 1] if hasattr(L, "csky_set_transmittance_mapping") else [0]
for m in maps:
    if len(maps) > 1:
        assert L.csky_set_transmittance_mapping(ctx, m) == 0
    for i in range(50):
        assert L.csky_render_transmittance(ctx, tp, P(t)) == 0
    for i in range(50):
        assert L.csky_render_sky_lut(ctx, sp, P(s)) == 0
    print("mapping", m, "transmittance checksum", int(t.astype(np.uint64).sum()), "sky checksum", int(s.astype(np.uint64).sum()), flush=True)
L.csky_destroy(ctx)
print("lut_times ok")
