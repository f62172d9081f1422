"""The owner types of csrc/owners.h (DevBuf, PinnedBuf, Event, Stream) and the destruction of a csky_ctx, on the CPU: tests/owners_host defines the
HIP entry points the owners use as counting stubs, populates every owning member of a real csky_ctx through them and deletes it.  This is the leak and
double-release check of the host layer.  The same tool walks the blocking host forms' staging (csrc/host_stage.h) over the stubs: the layout of a
call's regions, and the one way through them.  Nothing here touches a GPU."""
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
    # counts of the owning members of context.h, with 8 ring slots, 8 pinned host slots and a timing pool grown from 2 to 70 events.
    # device buffers: the stage 1, the noise set 12, the transmittance LUT 2, the sky LUT's ring 4, the rows cache 1, the frame ring 8 + 8 + 4,
    #   d_stats and d_frame 2, two radiance sets of 3, d_rays_fc 1, the host slots 8
    # events: ev0 ev1 ev_copy 3, the rows cache 1 + 8, the frame slots 16, the timing pool 70, ev_rad ev_aerial ev_rays 3, the host slots 8
    want = {"dev": 1 + 12 + 2 + 4 + 1 + 20 + 2 + 6 + 1 + 8, "pinned": 8, "event": 3 + 9 + 16 + 70 + 3 + 8, "stream": 9}
    assert want["dev"] == 57 and want["event"] == 109
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


def test_the_stage_layout_is_aligned_gapless_and_refuses_overflow(report):
    _, _, figures = report
    # an 8192 x 8192 RGBA16F image; an 8192 x 8192 R16F map in front of a 512 x 512 x 256 volume: sizes that are multiples of 256 leave no gap
    assert int(one(figures, "stage_layout_image_total")) == 8192 * 8192 * 8
    assert int(one(figures, "stage_layout_shafts_total")) == 8192 * 8192 * 2 + 512 * 512 * 256 * 8
    assert int(one(figures, "stage_layout_ragged_total")) == 5 * 256 + 2             # regions of 1, 255, 256, 257 and 2 bytes
    assert int(one(figures, "stage_layout_zero_regions_total")) == 2560 + 7         # 0, 2376, 0, 0 and 7 bytes: the empty ones cost nothing
    assert int(one(figures, "stage_overflow_refused")) == 1
    assert int(one(figures, "stage_overflow_is_invalid")) == 1                      # CSKY_ERR_INVALID, nothing reserved (the tool's own expectation)
    assert "some_entry_point" in one(figures, "stage_overflow_error_text")
    assert int(one(figures, "stage_layout_hip_calls")) == 0


def test_a_blocking_call_goes_one_way_through_the_stage(report):
    _, _, figures = report
    assert int(one(figures, "host_call_success_in_order")) == 1                     # allocation, uploads, the step, the download, one wait
    assert int(one(figures, "host_call_copies_in_their_regions")) == 1
    assert int(one(figures, "host_call_smaller_allocates_nothing")) == 1
    assert int(one(figures, "host_call_larger_frees_then_allocates")) == 1


def test_a_blocking_call_waits_for_what_it_enqueued_whatever_failed(report):
    _, _, figures = report
    assert int(one(figures, "host_call_step_failure_waits_once")) == 1              # no download, one wait, the step's code
    assert one(figures, "host_call_step_failure_error_text") == "the step's own text"
    assert int(one(figures, "host_call_first_upload_failure_waits_never")) == 1     # nothing was enqueued: no step, no wait
    assert "hipMemcpyAsync" in one(figures, "host_call_upload_failure_error_text")
    assert int(one(figures, "host_call_second_upload_failure_waits_once")) == 1     # the first upload is in flight: no step, one wait
    assert int(one(figures, "host_call_reserve_failure_enqueues_nothing")) == 1
