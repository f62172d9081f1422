"""The launch orders on the host: csrc/order_core.h, compiled with g++ by tests/hostsim, against a numpy restatement of what each order MEANS
(order_kernels.hip, "static workgroup orders" and "cost-feedback schedule"; cloud_kernels.hip clouds_kernel_persistent).  The restatement builds every table from the
sequences the eight XCDs are meant to walk, not from the C expressions, and the properties the launch relies on are asserted on their own:
every footprint exactly once, idle entries everywhere else, the grid the launch code uses.

Physical workgroup b runs on XCD b % 8, so "the sequence of XCD x" is the entries at b = x, x + 8, x + 16, ... read in that order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDLE = 0xFFFFFFFF
MODES = (1, 2, 5)

# (tiles_x, slabs) of the project's launches: a footprint is bw x 8 pixels, bw = 32 for whole rays, 16 / 8 for 2 / 4 and interleaved segments, 128 for "lds"
REAL = [(64, 128), (64, 64), (64, 32), (64, 16),               # the C3 frame (2048 x 1024) and its 1/2, 1/4, 1/8 band shares
        (128, 256),                                            # the C5 frame (4096 x 2048)
        (128, 128), (128, 64), (128, 32), (128, 16),           # bw = 16
        (256, 128), (256, 64), (256, 32), (256, 16),           # bw = 8
        (16, 128), (16, 16)]                                   # the 128-wide "lds" strip


def _table(hostsim, mode, tiles_x, slabs):
    grid = hostsim.hostsim_static_order_grid(mode, tiles_x, slabs)
    out = np.full(grid + 8, 0x5A5A5A5A, np.uint32)             # 8 guard entries behind the table
    assert hostsim.hostsim_static_order(mode, tiles_x, slabs, out.ctypes.data_as(C.c_void_p), grid) == grid
    assert (out[grid:] == 0x5A5A5A5A).all()
    return out[:grid]


def reference_grid(mode, tiles_x, slabs):
    """Workgroups of the launch: mode 2 has no padding, mode 1 gives every XCD ceil(nblocks / 8) places, mode 5 gives every XCD ceil(slabs / 8) whole rows."""
    nblocks = tiles_x * slabs
    if mode == 2:
        return nblocks
    if mode == 1:
        return 8 * -(-nblocks // 8)
    return 8 * tiles_x * -(-slabs // 8)


def reference_sequences(mode, tiles_x, slabs):
    """The footprints each of the eight XCDs renders, in its order (modes 1 and 5)."""
    nblocks = tiles_x * slabs
    if mode == 1:                                              # contiguous eighths of the launch
        per = -(-nblocks // 8)
        return [np.arange(min(x * per, nblocks), min((x + 1) * per, nblocks)) for x in range(8)]
    seqs = []                                                  # mode 5: slab rows dealt round-robin, each walked left to right
    for x in range(8):
        rows = np.arange(x, slabs, 8)
        seqs.append((rows[:, None] * tiles_x + np.arange(tiles_x)[None, :]).reshape(-1))
    return seqs


def reference_table(mode, tiles_x, slabs):
    if mode == 2:
        return np.arange(tiles_x * slabs, dtype=np.uint32)
    t = np.full(reference_grid(mode, tiles_x, slabs), IDLE, np.uint32)
    for x, seq in enumerate(reference_sequences(mode, tiles_x, slabs)):
        t[x + 8 * np.arange(seq.size)] = seq
    return t


def check_static_order(table, mode, tiles_x, slabs):
    """The assertions of one (mode, tiles_x, slabs) on a table, wherever it comes from (the host's here, the device's in test_gpu_launch_order.py)."""
    nblocks = tiles_x * slabs
    where = (mode, tiles_x, slabs)
    assert table.size == reference_grid(mode, tiles_x, slabs), where
    busy = table[table != IDLE]
    assert busy.size == nblocks and np.array_equal(np.sort(busy), np.arange(nblocks)), where     # every footprint exactly once, all else idle
    if mode == 2:
        assert np.array_equal(table, np.arange(nblocks)), where
        return
    per = -(-nblocks // 8)
    for x in range(8):
        seq = table[x::8]
        seq = seq[seq != IDLE].astype(np.int64)
        if mode == 1:
            assert np.array_equal(seq, np.arange(min(x * per, nblocks), min((x + 1) * per, nblocks))), where + (x,)
        else:
            rows, cols = seq // tiles_x, seq % tiles_x
            assert (rows % 8 == x).all(), where + (x,)
            assert seq.size == tiles_x * len(range(x, slabs, 8)), where + (x,)
            assert (np.diff(seq) > 0).all(), where + (x,)      # rows ascend, and inside a row the columns do
            assert np.array_equal(cols, np.tile(np.arange(tiles_x), seq.size // tiles_x)), where + (x,)
    assert np.array_equal(table, reference_table(mode, tiles_x, slabs)), where


@pytest.mark.parametrize("mode", MODES)
def test_static_orders_sweep(hostsim, mode):
    for tiles_x in range(1, 71):
        for slabs in range(1, 141):
            check_static_order(_table(hostsim, mode, tiles_x, slabs), mode, tiles_x, slabs)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", REAL)
def test_static_orders_of_the_real_geometries(hostsim, mode, geom):
    check_static_order(_table(hostsim, mode, *geom), mode, *geom)


def test_static_order_grid_is_what_the_launch_code_uses(hostsim):
    """clouds_launch.cpp::ensure_order and the test hook take the grid from order_core.h::static_order_grid and nowhere else."""
    csrc = os.path.join(ROOT, "godot-volumetric-cloud-demo-v2_amd", "csrc")
    launch = open(os.path.join(csrc, "clouds_launch.cpp")).read()
    assert "const int grid = static_order_grid(mode, tiles_x, slabs);" in launch
    assert ">> 3) * 8" not in launch and ">> 3) * tiles_x" not in launch
    order_kern, kern = (open(os.path.join(csrc, f)).read() for f in ("order_kernels.hip", "cloud_kernels.hip"))
    assert "out[b] = static_order_entry(mode, tiles_x, slabs, b);" in order_kern and "persistent_pop_index(j, y, n_items, i)" in kern
    for mode in MODES:
        for tiles_x, slabs in REAL + [(1, 1), (3, 7), (70, 140)]:
            assert hostsim.hostsim_static_order_grid(mode, tiles_x, slabs) == reference_grid(mode, tiles_x, slabs)


def _buckets(hostsim, cost, shift):
    cost = np.ascontiguousarray(cost, np.uint32)
    out = np.zeros(cost.size, np.int32)
    hostsim.hostsim_lpt_bucket(cost.ctypes.data_as(C.c_void_p), cost.size, shift, out.ctypes.data_as(C.c_void_p))
    return out


def reference_bucket(cost, shift):
    """1024 buckets of 2^shift costs each, the heaviest first; everything from 1023 * 2^shift up shares bucket 0."""
    return 1023 - np.minimum(np.asarray(cost, np.uint64) // np.uint64(1 << shift), np.uint64(1023)).astype(np.int64)


@pytest.mark.parametrize("shift", range(32))
def test_lpt_bucket(hostsim, shift):
    rng = np.random.default_rng(shift)
    edges = (np.arange(1026, dtype=np.uint64) << np.uint64(shift))
    cost = np.concatenate([edges, edges + 1, edges - 1, rng.integers(0, 1 << 32, 4096, dtype=np.uint64), (rng.integers(0, 1 << 12, 4096, dtype=np.uint64) << np.uint64(shift)) >> np.uint64(1),
                           np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF], np.uint64)])
    cost = np.unique(cost[cost <= 0xFFFFFFFF])                 # ascending; edges - 1 wraps at 0 and is dropped here
    assert cost[0] == 0 and cost[-1] == 0xFFFFFFFF
    b = _buckets(hostsim, cost, shift)
    assert (np.diff(b) <= 0).all()                             # non-increasing in cost
    assert ((b >= 0) & (b <= 1023)).all()
    top, one = 1023 << shift, 1 << shift                       # Python integers: 1023 << shift may exceed 32 bits, then no cost reaches bucket 0
    assert np.array_equal(b == 0, cost.astype(object) >= top)
    if top <= 0xFFFFFFFF:
        assert b[-1] == 0                                      # 0xffffffff included
    assert np.array_equal(b == 1023, cost.astype(object) < one)
    assert np.array_equal(b, reference_bucket(cost, shift))


def test_lpt_shift_rule(hostsim):
    """Every primary_steps csky_set_march accepts: the largest cost of a workgroup, 4 wavefronts x 64 rays x (steps + 16), lands below 1024 buckets, and
    with one shift fewer it would not (at shift 0 there is no fewer)."""
    api = open(os.path.join(ROOT, "godot-volumetric-cloud-demo-v2_amd", "csrc", "api.cpp")).read()
    assert "primary_steps < 1 || primary_steps > 1024" in api   # the range swept below is the range the library accepts
    for steps in range(1, 1025):
        s = hostsim.hostsim_lpt_shift(steps)
        largest = 256 * (steps + 16)
        assert 0 <= s <= 31 and (largest >> s) < 1024, (steps, s)
        if s > 0:
            assert (largest >> (s - 1)) >= 1024, (steps, s)
        assert _buckets(hostsim, [largest], s)[0] == 1023 - (largest >> s)   # so the clamp of lpt_bucket never acts on a cost a launch can record
    assert hostsim.hostsim_lpt_shift(128) == 6


@pytest.mark.parametrize("n_items", list(range(0, 301)) + [1023, 1024, 1025, 8192, 16384, 32768, 65537, (1 << 24) + 3])
def test_persistent_pop_mapping(hostsim, n_items):
    """Pop j of sequence y reaches order entry 8 j + y: over all j < per_xcd every entry exactly once, and nothing at or beyond per_xcd, where 8 j wraps
    around 32 bits included."""
    per_xcd = (n_items + 7) // 8
    fn = hostsim.hostsim_persistent_pops
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    out = np.zeros(max(per_xcd, 1) * 8, np.uint32)
    fn(n_items, 0, per_xcd, out.ctypes.data_as(C.c_void_p))
    got = out[: per_xcd * 8]
    hit = got[got != IDLE]
    assert hit.size == n_items and np.array_equal(np.sort(hit), np.arange(n_items))
    jj, yy = np.divmod(np.arange(per_xcd * 8), 8)
    assert np.array_equal(got[got != IDLE], (8 * jj + yy)[got != IDLE])
    for j0 in (per_xcd, per_xcd + 1, 1 << 29, (1 << 29) + 1, (1 << 30), (1 << 32) - 8):
        tail = np.zeros(64, np.uint32)
        fn(n_items, j0, 8, tail.ctypes.data_as(C.c_void_p))
        assert (tail == IDLE).all(), (n_items, j0)


def test_ring_depth_the_gpu_tests_assume():
    """tests/test_gpu_write_coverage.py runs every launch form three times per ring slot: the rings of a context are this deep."""
    ctxh = open(os.path.join(ROOT, "godot-volumetric-cloud-demo-v2_amd", "csrc", "context.h")).read()
    assert re.search(r"constexpr int RING = (\d+);", ctxh).group(1) == "8"
