"""The order kernels on the device (order_kernels.hip: static_order_kernel, lpt_hist / lpt_scan / lpt_scatter) through the two lab-bench hooks
csky_test_static_order and csky_test_lpt_order: the static tables entry for entry against the host's (tests/hostsim, which tests/test_launch_order.py
checks against a numpy restatement on the CPU), the counting sort against numpy."""
import numpy as np
import pytest

from test_launch_order import IDLE, MODES, REAL, _buckets, _table, check_static_order, reference_bucket

pytestmark = pytest.mark.gpu

# slabs 1, 7, 8, 9 at several widths; nblocks not a multiple of 8 (3 x 7, 5 x 9, 33 x 3, 1 x 1); grids not a multiple of 256 (nearly all of them);
# the edges of the CPU sweep; one table larger than a 256-thread workgroup in every mode
SUBSET = [(tx, sl) for tx in (1, 2, 3, 5, 8, 17, 33, 64, 70) for sl in (1, 7, 8, 9)] + [(1, 140), (70, 140), (7, 13), (33, 3), (31, 127), (65, 25)]


@pytest.mark.parametrize("mode", MODES)
def test_static_order_kernel_equals_the_host_table(gpu_ctx, hostsim, mode):
    seen_ragged_blocks = seen_ragged_grid = False
    for tiles_x, slabs in SUBSET + REAL:
        got = gpu_ctx.test_static_order(mode, tiles_x, slabs)
        want = _table(hostsim, mode, tiles_x, slabs)
        assert got.size == want.size, (mode, tiles_x, slabs, got.size, want.size)
        assert np.array_equal(got, want), (mode, tiles_x, slabs, np.flatnonzero(got != want)[:8])
        check_static_order(got, mode, tiles_x, slabs)
        seen_ragged_blocks |= (tiles_x * slabs) % 8 != 0
        seen_ragged_grid |= got.size % 256 != 0
    assert seen_ragged_blocks and seen_ragged_grid


def test_static_order_hook_refuses_what_the_launch_never_asks(pkg, gpu_ctx):
    for bad in ((0, 4, 4), (3, 4, 4), (7, 4, 4), (5, 0, 4), (5, 4, 0), (2, 1 << 13, 1 << 13)):
        with pytest.raises(pkg.CloudSkyError):
            gpu_ctx.test_static_order(*bad)


NS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4099, 8192, 32768)
LARGEST = 256 * (128 + 16)                                     # the largest cost of a workgroup at 128 primary steps


def _costs(kind, n, rng):
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "largest":
        return np.full(n, LARGEST, np.uint32)                  # one bucket: every lane on one atomic
    if kind == "ones":
        return np.full(n, 0xFFFFFFFF, np.uint32)
    if kind == "ascending":
        return (np.arange(n, dtype=np.uint64) * (LARGEST // max(n, 1) + 1)).astype(np.uint32)
    if kind == "descending":
        return (np.arange(n, dtype=np.uint64) * (LARGEST // max(n, 1) + 1)).astype(np.uint32)[::-1].copy()
    if kind == "uniform":
        return rng.integers(0, LARGEST + 1, n, dtype=np.uint64).astype(np.uint32)
    if kind == "heavy_tail":                                   # nine in ten within 3 buckets' worth of costs, the others up to 2^32
        c = rng.integers(0, 3 << 6, n, dtype=np.uint64)
        tail = rng.random(n) < 0.1
        c[tail] = (2.0 ** rng.uniform(0, 32, int(tail.sum()))).astype(np.uint64)
        return np.minimum(c, 0xFFFFFFFF).astype(np.uint32)
    raise ValueError(kind)


KINDS = ("zero", "largest", "ones", "ascending", "descending", "uniform", "heavy_tail")


def _check_sort(order, left, scratch, cost, shift, where):
    n = cost.size
    assert order.size == n and np.array_equal(np.sort(order), np.arange(n)), where              # a permutation of range(n)
    want = reference_bucket(cost, shift)
    along = want[order.astype(np.int64)]
    assert (np.diff(along) >= 0).all(), where                                                      # heaviest (bucket 0) first
    # the set of indices placed in each bucket is numpy's: a stable sort by bucket puts the same indices on the same stretch of places
    ref = np.argsort(want, kind="stable")
    bounds = np.flatnonzero(np.diff(want[ref])) + 1
    for got_part, ref_part in zip(np.split(order.astype(np.int64), bounds), np.split(ref, bounds)):
        assert np.array_equal(np.sort(got_part), ref_part), where
    assert not left.any(), where                                                                   # cost comes back zeroed
    assert not scratch[:1024].any(), where                                                         # and so does the histogram


@pytest.mark.parametrize("kind", KINDS)
def test_lpt_sort_against_numpy(gpu_ctx, hostsim, kind):
    shift128 = hostsim.hostsim_lpt_shift(128)
    assert shift128 == 6
    for n in NS:
        for shift in (0, shift128, 31):
            cost = _costs(kind, n, np.random.default_rng(n * 37 + shift))
            if kind in ("ascending", "descending") and n > 1:
                assert (np.diff(cost.astype(np.int64)) != 0).all()
            assert np.array_equal(_buckets(hostsim, cost, shift), reference_bucket(cost, shift))  # the host's lpt_bucket is the reference's
            for rounds in (1, 3):                              # 3: the histogram is cleared by the kernels themselves, never by a memset per frame
                order, left, scratch = gpu_ctx.test_lpt_order(cost, shift, rounds)
                _check_sort(order, left, scratch, cost, shift, (kind, n, shift, rounds))


def test_lpt_hook_refuses_bad_arguments(pkg, gpu_ctx):
    one = np.ones(4, np.uint32)
    for shift, rounds in ((-1, 1), (32, 1), (0, 0), (0, 65)):
        with pytest.raises(pkg.CloudSkyError):
            gpu_ctx.test_lpt_order(one, shift, rounds)
    assert IDLE == 0xFFFFFFFF
