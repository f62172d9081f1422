"""Every launch writes its whole share and nothing else.

The cloud march is tested against the oracle from many angles, but always into buffers that already hold the right answer (the context's
reused frame, a tensor the previous pass filled) or zeros, which whole rows of a cloud frame are.  Here every launch marches into a tensor
whose every half is the bit pattern 0xFFFF before the launch, a NaN no frame contains, filled on the launch's own stream.  The tensor is
larger than the share: GUARD rows before and after it, and in every other buffer 64 bytes of padding behind each row.  After the launch

  (a) no 0xFFFF half is left at any pixel of the share: a footprint the launch order left out shows, whatever the scene;
  (b) every half outside the share is still 0xFFFF: guard rows, pitch padding;

and the share's bytes are compared with a reference rendered once per scene by a fresh context (variant 3, whole rays, schedule 2, one frame
in flight, into a poisoned buffer of its own; cloud_tight holds that reference against the CPU oracle).  Whole-ray launches of variant 3 do the
same arithmetic in any order, plain or persistent, and must equal it byte for byte; the other variants and the segmented forms agree with it
under the tolerance of test_gpu_parity.py::test_variants_and_schedules_agree, and launch after launch with themselves byte for byte (a ray's
arithmetic does not depend on where and when its workgroup runs).  The host form's in-cloud tally must equal the reference's: a footprint
rendered twice shows there.

A launch form runs three times on every ring slot of the context (the rings are CTX_RING deep and advance with every launch): the second
launch on a slot is the first that finds the slot's order table, its feedback order and its re-armed pop counters."""
import collections

import numpy as np
import pytest

from conftest import cloud_close, cloud_tight, norm

pytestmark = pytest.mark.gpu

SUN = (1, 1, 0)                     # conftest SUNS["deg45"]
GUARD = 8                           # guard rows before and after the share
CTX_RING = 8                        # csrc/context.h RING (tests/test_launch_order.py pins it)
RUNS = 3 * CTX_RING
CLOSE = dict(frac=0.9999, atol=5e-4, rtol=2e-3)

# tex: texture_size; upd: update_position; tile_w x (band_rows * n_bands) pixels are rendered; bands = (band_rows, first_band, band_stride, n_bands)
Scene = collections.namedtuple("Scene", "name tex upd tile_w bands")
SCENES = [
    Scene("8x8", (8, 8), (0, 0), 8, (8, 0, 1, 1)),
    Scene("9x5", (9, 5), (0, 0), 9, (5, 0, 1, 1)),
    Scene("31x17", (31, 17), (0, 0), 31, (17, 0, 1, 1)),
    Scene("33x64", (33, 64), (0, 0), 33, (8, 0, 1, 8)),
    Scene("96x24", (96, 24), (0, 0), 96, (8, 0, 1, 3)),
    Scene("520x200", (520, 200), (0, 0), 520, (8, 0, 1, 25)),                # 17 x 25 whole-ray footprints: not a multiple of 8
    Scene("40x66_nine_slabs", (40, 66), (0, 0), 40, (66, 0, 1, 1)),          # 9 slabs, the last of 2 rows
    Scene("48x15_bands_of_5", (48, 32), (0, 0), 48, (5, 1, 2, 3)),           # rows 5-9, 15-19, 25-29: band borders inside an 8-row slab
    Scene("64x16_band_3_stride_8", (64, 128), (0, 0), 64, (8, 3, 8, 2)),     # rows 24-31 and 88-95
    Scene("50x20_at_96_40", (256, 128), (96, 40), 50, (20, 0, 1, 1)),        # a tile inside a larger texture
]
BY_NAME = {s.name: s for s in SCENES}
ids = [s.name for s in SCENES]

# (variant, segments, schedule)
PLAIN_FORMS = [(0, 1, s) for s in (1, 2, 5)] + [(v, seg, s) for v in (1, 3) for seg in (1, 2, 4, 5) for s in (2, 5, 7)] + [(2, 0, -1)]


def rows_of(scene):
    return scene.bands[0] * scene.bands[3]


def params_of(oracle, scene):
    p = oracle.default_params(scene.tex[0], scene.tex[1], SUN)
    p[2:4] = scene.upd
    return p


def whole_tile(scene):
    """the host form (csky_render_clouds: rows 0 .. tile_h - 1) renders the same pixels"""
    return scene.bands[1] == 0 and (scene.bands[2] == 1 or scene.bands[3] == 1)


class Canvas:
    """The share of a launch inside a poisoned allocation of the test's own."""

    def __init__(self, tile_w, rows, ragged):
        import torch
        self.tile_w, self.rows = tile_w, rows
        self.pitch = tile_w * 8 + (64 if ragged else 0)
        self.t = torch.empty((rows + 2 * GUARD, self.pitch // 2), dtype=torch.int16, device="cuda")
        self.share = self.t[GUARD:GUARD + rows, :tile_w * 4]
        self.ptr = self.t.data_ptr() + GUARD * self.pitch
        self.outside = self.t.numel() - rows * tile_w * 4

    def poison(self):
        self.t.fill_(-1)                                       # 0xFFFF in every half, on the current stream

    def flags(self, ref):
        """enqueued behind the launch: halfs still poisoned in the whole allocation, in the share, and halfs of the share that differ from ref"""
        import torch
        left = (self.t == -1).sum()
        left_in = (self.share == -1).sum()
        diff = (self.share != ref).sum() if ref is not None else torch.zeros((), dtype=left.dtype, device=left.device)
        return torch.stack([left, left_in, diff])

    def verdict(self, flags, where, exact=True):
        """conditions (a), (b) and the byte comparison; what is wrong is read from this buffer, which still holds the launch's result"""
        left, left_in, diff = [int(v) for v in flags.tolist()]
        if left_in or left - left_in != self.outside or (exact and diff):
            t = self.t.cpu().numpy()
            inside = np.zeros(t.shape, bool)
            inside[GUARD:GUARD + self.rows, :self.tile_w * 4] = True
            missed = np.argwhere(inside & (t == -1))
            spilled = np.argwhere(~inside & (t != -1))
            msg = "%s: (a) %d poisoned halfs left in the share, first at pixel (row, column) %s; (b) %d halfs outside the share overwritten, first at (allocation row, half) %s = %s; %d halfs differ from the reference" % (
                where, len(missed), [(int(r) - GUARD, int(c) // 4) for r, c in missed[:4]], len(spilled), [(int(r), int(c)) for r, c in spilled[:4]],
                [hex(int(t[r, c]) & 0xFFFF) for r, c in spilled[:4]], diff)
            pytest.fail(msg)

    def image(self):
        return self.share.cpu().numpy().view(np.float16).reshape(self.rows, self.tile_w, 4)


def launch(ctx, scene, p, canvas, stream):
    ctx.render_clouds_device(p, scene.tile_w, scene.bands, canvas.ptr, canvas.pitch, stream.cuda_stream)


_REFS = {}


def reference(pkg, noise, oracle, scene):
    """(device tensor of the share, its float16 image, stats of the reference context's host-form launch or None), once per scene by a fresh context"""
    import torch
    if scene.name not in _REFS:
        p = params_of(oracle, scene)
        ctx = pkg.Context(0)
        try:
            ctx.set_noise(*noise); ctx.set_march(128, 6)
            ctx.set_variant(3); ctx.set_segments(1); ctx.set_schedule(2); ctx.set_frames_in_flight(1)
            ctx.render_transmittance(256, 64)
            ctx.render_sky_lut(norm(SUN), 200, 100)
            s = torch.cuda.Stream()
            cv = Canvas(scene.tile_w, rows_of(scene), ragged=True)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                cv.poison()
                launch(ctx, scene, p, cv, s)
                cv.verdict(cv.flags(None), ("reference", scene.name))
                ref = cv.share.clone()
                img = cv.image()
            stats = None
            if whole_tile(scene):
                host = ctx.render_clouds(p, scene.tile_w, rows_of(scene))
                assert np.array_equal(host.view(np.uint16), img.view(np.uint16)), scene.name
                stats = ctx.cloud_stats()
            torch.cuda.synchronize()
        finally:
            ctx.close()
        _REFS[scene.name] = (ref, img, stats)
    return _REFS[scene.name]


def run_form(ctx, scene, p, ref, exact, where, fif=1, runs=RUNS):
    """`runs` launches of the context's current form into two poisoned canvases in turn (one with ragged pitch), on `fif` streams; the verdict of a
    launch is read before its canvas is poisoned again.  Returns the float16 image of the first launch."""
    import torch
    ref_dev, ref_img, _ = ref
    streams = [torch.cuda.Stream() for _ in range(fif)]
    canvases = [Canvas(scene.tile_w, rows_of(scene), ragged=(i == 0)) for i in range(2)]
    torch.cuda.synchronize()
    pending = [None, None]
    first_img, want = None, (ref_dev if exact else None)
    try:
        for k in range(runs):
            i = k & 1
            s = streams[i % fif]
            with torch.cuda.stream(s):
                if pending[i] is not None:
                    canvases[i].verdict(pending[i], where + (k - 2,))
                canvases[i].poison()
                launch(ctx, scene, p, canvases[i], s)
                if k == 0:
                    canvases[0].verdict(canvases[0].flags(want), where + (0,))
                    if not exact:                              # the form's own bytes are what every later launch must repeat
                        want = canvases[0].share.clone()
                    first_img = canvases[0].image()            # (waits for the stream: the clone is there before another stream reads it)
                    if not exact:
                        ok, info = cloud_close(first_img, ref_img, **CLOSE)
                        assert ok, (where, info)
                else:
                    pending[i] = canvases[i].flags(want)
        for i in range(2):
            with torch.cuda.stream(streams[i % fif]):
                if pending[i] is not None:
                    canvases[i].verdict(pending[i], where + ("drain", i))
    finally:
        torch.cuda.synchronize()
    return first_img


def check_host_form(ctx, scene, p, ref, exact, where):
    """the host form of the current launch form: the only one with a tally.  Bytes as above, and the in-cloud and primary sample counts of the reference."""
    _, ref_img, ref_stats = ref
    if ref_stats is None:
        return
    host = ctx.render_clouds(p, scene.tile_w, rows_of(scene))
    if exact:
        assert np.array_equal(host.view(np.uint16), ref_img.view(np.uint16)), where
    else:
        ok, info = cloud_close(host, ref_img, **CLOSE)
        assert ok, (where, info)
    assert ctx.cloud_stats() == ref_stats, (where, ctx.cloud_stats(), ref_stats)


def restore(ctx):
    ctx.set_variant(-1); ctx.set_segments(0); ctx.set_schedule(-1); ctx.set_frames_in_flight(1); ctx.set_march(128, 6)


@pytest.mark.parametrize("name", ids)
def test_reference_launch_is_the_oracles(pkg, noise, oracle, otex, o_skies, name):
    scene = BY_NAME[name]
    _, img, stats = reference(pkg, noise, oracle, scene)
    want, _ = oracle.clouds_bands(otex, params_of(oracle, scene), o_skies["deg45"], scene.tile_w, scene.bands, nthreads=min(8, oracle.max_threads()))
    ok, info = cloud_tight(img, want)
    print(name, info)
    assert ok, (name, info)
    if stats is not None:
        assert stats["rays"] == scene.tile_w * rows_of(scene), (name, stats)


@pytest.mark.parametrize("name", ids)
def test_plain_launch_forms_write_their_share_and_nothing_else(pkg, noise, oracle, gpu_ctx, name):
    scene = BY_NAME[name]
    ref, p = reference(pkg, noise, oracle, scene), params_of(oracle, scene)
    gpu_ctx.set_march(128, 6); gpu_ctx.set_frames_in_flight(1)
    gpu_ctx.render_sky_lut(norm(SUN), 200, 100)
    try:
        for variant, seg, sched in PLAIN_FORMS:
            gpu_ctx.set_variant(variant); gpu_ctx.set_segments(seg); gpu_ctx.set_schedule(sched)
            exact = variant == 3 and seg == 1
            where = (name, "variant", variant, "segments", seg, "schedule", sched)
            run_form(gpu_ctx, scene, p, ref, exact, where)
            check_host_form(gpu_ctx, scene, p, ref, exact, where)
    finally:
        restore(gpu_ctx)


@pytest.mark.parametrize("name", ids)
def test_persistent_form_writes_its_share_and_nothing_else(pkg, noise, oracle, monkeypatch, name):
    """CSKY_PERSISTENT=2: every whole-ray launch of variant 3 pops its footprints; one frame in flight, and two on two streams"""
    scene = BY_NAME[name]
    ref, p = reference(pkg, noise, oracle, scene), params_of(oracle, scene)
    monkeypatch.setenv("CSKY_PERSISTENT", "2")
    ctx = pkg.Context(0)
    try:
        ctx.set_noise(*noise); ctx.set_march(128, 6); ctx.set_variant(3); ctx.set_segments(1)
        ctx.render_transmittance(256, 64)
        ctx.render_sky_lut(norm(SUN), 200, 100)
        for fif in (1, 2):
            ctx.set_frames_in_flight(fif)
            for sched in (5, 7):
                ctx.set_schedule(sched)
                where = (name, "persistent", "frames in flight", fif, "schedule", sched)
                run_form(ctx, scene, p, ref, True, where, fif=fif)
                check_host_form(ctx, scene, p, ref, True, where)
    finally:
        ctx.close()


def test_exact_cells_write_their_share_and_nothing_else(pkg, noise, oracle):
    """set_exact_cells(1): the compact whole-ray kernel on the fp32-coefficient texture set, another kernel instantiation with its own launch"""
    scene = BY_NAME["520x200"]
    ref, p = reference(pkg, noise, oracle, scene), params_of(oracle, scene)
    ctx = pkg.Context(0)
    try:
        ctx.set_exact_cells(1)
        ctx.set_noise(*noise); ctx.set_march(128, 6)
        ctx.render_transmittance(256, 64)
        ctx.render_sky_lut(norm(SUN), 200, 100)
        where = (scene.name, "exact cells")
        run_form(ctx, scene, p, ref, False, where)
        check_host_form(ctx, scene, p, ref, False, where)
    finally:
        ctx.close()


def test_the_policys_own_form_of_the_headline_frame(pkg, noise, oracle, oracle_frames):
    """2048 x 1024 with two frames in flight and every knob at its default: launch_policy.h picks the persistent form (32 Ki wavefronts)"""
    scene = Scene("2048x1024", (2048, 1024), (0, 0), 2048, (8, 0, 1, 128))
    ref, p = reference(pkg, noise, oracle, scene), params_of(oracle, scene)
    want, _ = oracle_frames(2048, 1024, "deg45")
    ok, info = cloud_tight(ref[1], want)
    assert ok, info
    ctx = pkg.Context(0)
    try:
        ctx.set_noise(*noise); ctx.set_march(128, 6)
        ctx.render_transmittance(256, 64)
        ctx.render_sky_lut(norm(SUN), 200, 100)
        ctx.set_frames_in_flight(2)
        assert not ctx.last_warning(), ctx.last_warning()      # two frames do overlap here, so the policy plans for them
        run_form(ctx, scene, p, ref, True, (scene.name, "policy", "frames in flight", 2), fif=2)
        check_host_form(ctx, scene, p, ref, True, (scene.name, "policy, host form"))
    finally:
        ctx.close()


def test_feedback_order_is_dropped_when_the_tile_moves(pkg, noise, oracle, gpu_ctx):
    """Schedule 7 keeps costs per ring slot and view.  The same footprint count at another update_position on the same slot must not run in the
    other view's order table slot as if it were its own: whatever order it runs in, every footprint is rendered, at both positions, whichever
    position the slot saw last."""
    import torch
    scenes = [Scene("64x32_at_%d_%d" % u, (256, 128), u, 64, (8, 0, 1, 4)) for u in ((0, 0), (160, 24), (32, 8))]          # all above the horizon: three different images
    refs = [reference(pkg, noise, oracle, s) for s in scenes]
    ps = [params_of(oracle, s) for s in scenes]
    assert not torch.equal(refs[0][0], refs[1][0]) and not torch.equal(refs[1][0], refs[2][0])
    gpu_ctx.set_march(128, 6); gpu_ctx.set_frames_in_flight(1)
    gpu_ctx.render_sky_lut(norm(SUN), 200, 100)
    try:
        for variant, seg in ((3, 1), (3, 2), (1, 1)):
            gpu_ctx.set_variant(variant); gpu_ctx.set_segments(seg); gpu_ctx.set_schedule(7)
            exact = variant == 3 and seg == 1
            # a block of launches per position (every slot sees A twice, then B twice), then the positions in turn (3 does not divide the ring:
            # every slot meets another position than its last)
            seq = [0] * (2 * CTX_RING) + [1] * (2 * CTX_RING) + [k % 3 for k in range(3 * CTX_RING + 1)]
            s = torch.cuda.Stream()
            cv = Canvas(64, 32, ragged=True)
            torch.cuda.synchronize()
            firsts = {}
            with torch.cuda.stream(s):
                for k, which in enumerate(seq):
                    cv.poison()
                    launch(gpu_ctx, scenes[which], ps[which], cv, s)
                    where = ("variant", variant, "segments", seg, "launch", k, scenes[which].name)
                    if exact:
                        cv.verdict(cv.flags(refs[which][0]), where)
                    elif which not in firsts:
                        cv.verdict(cv.flags(None), where)
                        ok, info = cloud_close(cv.image(), refs[which][1], **CLOSE)
                        assert ok, (where, info)
                        firsts[which] = cv.share.clone()
                    else:
                        cv.verdict(cv.flags(firsts[which]), where)
            torch.cuda.synchronize()
    finally:
        restore(gpu_ctx)


def test_order_table_of_a_slot_follows_the_footprint_width(pkg, noise, oracle, gpu_ctx):
    """In mode 1 a 33-pixel-wide launch of one slab has a grid of 8 workgroups whether it is 2 whole-ray footprints, 3 of two segments or 5 of four:
    the slot's order table must be rewritten when the footprint width changes and nothing else does."""
    scene = Scene("33x8", (66, 16), (0, 0), 33, (8, 0, 1, 1))
    ref, p = reference(pkg, noise, oracle, scene), params_of(oracle, scene)
    gpu_ctx.set_march(128, 6); gpu_ctx.set_frames_in_flight(1)
    gpu_ctx.render_sky_lut(norm(SUN), 200, 100)
    try:
        gpu_ctx.set_variant(1); gpu_ctx.set_schedule(1)
        for seg in (1, 2, 4, 1, 5, 2):
            gpu_ctx.set_segments(seg)
            where = (scene.name, "variant", 1, "segments", seg, "schedule", 1)
            run_form(gpu_ctx, scene, p, ref, False, where, runs=CTX_RING + 2)
            check_host_form(gpu_ctx, scene, p, ref, False, where)
    finally:
        restore(gpu_ctx)


@pytest.mark.parametrize("members", [2, 3])
def test_multi_device_frame_is_covered_by_its_members(pkg, noise, oracle, members):
    """csky_multi on one device: member k renders the 8-row bands k, k + n, ... into ONE poisoned frame with ragged pitch (in place: out_full) or into
    its own band buffer and copies them over (staged).  Together the members cover the frame, none touches the guards or the padding.  Whole rays on
    every member, so the bytes are the single context's."""
    import torch
    sizes = [(100, 56, RUNS), (40, 8, RUNS), (2048, 1000, CTX_RING + 2)]     # 7 bands, 1 band (members without any), 125 bands
    m = pkg.MultiContext([0] * members)
    try:
        m.set_noise(*noise); m.set_march(128, 6)
        for i in range(members):
            m.ctx(i).set_segments(1)
        m.render_sky_lut(norm(SUN))
        s = torch.cuda.Stream()
        for w, h, runs in sizes:
            scene = Scene("%dx%d" % (w, h), (w, h), (0, 0), w, (8, 0, 1, h // 8))
            ref, p = reference(pkg, noise, oracle, scene), params_of(oracle, scene)
            for staged in (False, True):
                m.set_staged(staged)
                for ragged in (True, False):
                    cv = Canvas(w, h, ragged)
                    torch.cuda.synchronize()
                    with torch.cuda.stream(s):
                        for k in range(runs if ragged else 2):
                            cv.poison()
                            m.render_clouds_device(p, w, h, cv.ptr, cv.pitch, s.cuda_stream)
                            cv.verdict(cv.flags(ref[0]), (scene.name, "members", members, "staged", staged, "ragged", ragged, "launch", k))
                    m.sync(); torch.cuda.synchronize()
    finally:
        m.close()
