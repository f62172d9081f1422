"""The owner types of csrc/owners.h (DevBuf, PinnedBuf, Event, Stream) and the destruction of a csky_ctx, on the CPU: tests/owners_host defines the
HIP entry points the owners use as counting stubs, populates every owning member of a real csky_ctx through them and deletes it.  This is the leak and
double-release check of the host layer; nothing here touches a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "owners_host")


@pytest.fixture(scope="module")
def report():
    subprocess.check_call(["make", "-C", DIR, "-s"])
    r = subprocess.run([os.path.join(DIR, "owners_host")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    figures = {}
    for line in r.stdout.splitlines():
        name, _, value = line.partition(" ")
        figures.setdefault(name, []).append(value)
    return r.returncode, r.stdout, figures


def one(figures, name):
    assert name in figures, "the tool did not report %s" % name
    assert len(figures[name]) == 1
    return figures[name][0]


def test_every_expectation_of_the_tool_holds(report):
    code, out, figures = report
    assert "FAIL:" not in out, out
    assert code == 0, out
    assert int(one(figures, "failures")) == 0


def test_each_owner_releases_once_and_never_after_a_move(report):
    _, _, figures = report
    # two handles made per owner type (the moved one and the one the move assignment overwrote), two releases, none of them twice
    assert figures["owner_dev_released"] == ["2"] and figures["owner_pinned_released"] == ["2"] and figures["owner_stream_released"] == ["2"]
    assert figures["owner_event_released"] == ["2", "2"]            # with and without the timing flag: hipEventCreateWithFlags, hipEventCreate
    assert int(one(figures, "double_releases")) == 0


def test_alloc_frees_first_and_grow_is_free_within_capacity(report):
    _, _, figures = report
    assert int(one(figures, "alloc_order_free_then_malloc")) == 1
    assert int(one(figures, "grow_within_capacity_calls")) == 0


def test_failed_malloc_leaves_an_empty_owner_and_an_error_text(report):
    _, out, figures = report
    text = one(figures, "failed_malloc_error_text")
    assert "hipMalloc" in text and "out of memory" in text
    assert "failed hipMalloc" not in out                               # the tool's own expectations on the owner's state (empty, count 0)


def test_a_full_context_returns_every_handle_once(report):
    _, _, figures = report
    # 8 ring slots, 8 pinned host slots, two radiance sets, a timing pool grown from 2 to 70 events (context.h)
    want = {"dev": 56, "pinned": 8, "event": 4 + 16 + 70 + 8, "stream": 9}
    for kind, n in want.items():
        assert int(one(figures, "context_%s_made" % kind)) == n
        assert int(one(figures, "context_%s_released" % kind)) == n
    assert int(one(figures, "double_releases")) == 0
    assert int(one(figures, "live_handles_at_exit")) == 0


def test_the_context_stream_dies_last(report):
    _, _, figures = report
    assert int(one(figures, "context_stream_destroyed_last")) == 1
    assert int(one(figures, "context_stream_after_every_event")) == 1


def test_an_empty_context_releases_nothing(report):
    _, _, figures = report
    assert int(one(figures, "empty_context_calls")) == 0


def test_order_tables_grow_together_after_one_device_wide_wait(report):
    _, _, figures = report
    # tables of 8, 8, 64, 8, 8, 8, 8, 8 entries, every key recorded, grown to 32 by the ring's own code (context.h FrameRing::grow_order_tables)
    assert int(one(figures, "order_growth_device_syncs")) == 1
    assert int(one(figures, "order_growth_calls_in_order")) == 1           # the wait first, then seven times hipFree before hipMalloc
    assert int(one(figures, "order_growth_allocations_of_32")) == 7
    assert int(one(figures, "order_growth_keys_forgotten")) == 7
    assert int(one(figures, "order_growth_large_table_kept")) == 1         # the 64-entry table keeps its memory and its key


def test_a_failed_growth_of_the_timing_pool_is_all_or_nothing(report):
    _, _, figures = report
    # a pool of 4 events grown to 10 by the pool's own grow, the third new event refused
    assert int(one(figures, "pool_growth_failure_is_error")) == 1
    assert int(one(figures, "pool_growth_failure_size")) == 4
    assert int(one(figures, "pool_growth_failure_events_made")) == 2
    assert int(one(figures, "pool_growth_failure_events_released")) == 2
    assert "hipEventCreate" in one(figures, "pool_growth_failure_error_text")


def test_the_timing_pool_starts_at_512_events_and_doubles(report):
    _, _, figures = report
    assert int(one(figures, "pool_events_after_256_pairs")) == 512
    assert int(one(figures, "pool_events_after_257_pairs")) == 1024
