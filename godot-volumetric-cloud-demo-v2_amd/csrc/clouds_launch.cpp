// clouds_launch.cpp -- one launch of the cloud kernel (clouds_dev): frame set-up on the context's stream into the next slot of the frame ring, the
// workgroup order of the launch (the slot's static table, or the order cost feedback left there), per-launch timing events, and the launch itself.
// Which kernel runs and how is launch_policy.h's decision; what a ring slot owns and how the ring's steps order the streams is context.h's
// (FrameRing); when a cached order may be used is frame_ring.h's.
#include <cstring>
#include "context.h"
#include "launch_policy.h"
#include "order_core.h"

namespace csky {

TexSet texset(const csky_ctx* c) {
    const NoiseSet& n = c->noise;
    TexSet t;
#ifdef CSKY_BRICK_BOUND
    t.brick = n.d_brick;
#endif
    t.shape = n.d_shape; t.detail = n.d_detail; t.weather = n.d_weather; t.sky = c->lut.cur_f(); t.sky_w = c->lut.aw; t.sky_h = c->lut.ah; t.detail_lod5 = n.st.detail_lod5(); t.detail_h = n.d_detail_h; t.detail_lds = nullptr;
    return t;
}

TexSet32 texset32(const csky_ctx* c) {
    TexSet32 t;
    static_cast<TexSet&>(t) = texset(c);
    t.shape32 = c->noise.d_shape32; t.detail32 = c->noise.d_detail32; t.weather32 = c->noise.d_weather32;
    return t;
}

namespace {

// The static workgroup order of ring slot `slot` for this launch, on stream s (order_kernels.hip::static_order_kernel; modes 1, 2, 5).  Measured on
// the headline frame (queue kernel, round 1): 5 (slab rows round-robin over the XCDs) 3.93 ms, 1 (contiguous eighths) 4.80 ms, 2 (natural) 4.92 ms;
// azimuth-wedge and horizon-first orders (5.3-5.8 / 4.77 ms) were dropped in round 2.  The table depends on the launch geometry
// only (not on update_position: the reference's tile walk re-uses it) and is written by a kernel on the launch's stream.
int ensure_order(csky_ctx* c, int slot, int mode, int tiles_x, int slabs, hipStream_t s) {
    const int grid = static_order_grid(mode, tiles_x, slabs);                    // order_core.h
    const OrderKey key = order_key(tiles_x, slabs, mode, grid);
    FrameSlot& f = c->ring.slot[slot];
    if (f.order_st.hit(f.order != nullptr, key)) return CSKY_OK;
    if (f.order.count() < (size_t)grid) { int rc; if ((rc = c->ring.grow_order_tables(c, (size_t)grid))) return rc; }
    // the last reader of this slot's table is the march RING frames ago; the caller has already ordered `s` behind it (ev_clouds -> the context's stream ->
    // ev_setup -> s), exactly like the frame constants of the slot
    HIPCHK(c, launch_static_order(mode, tiles_x, slabs, grid, f.order, s));
    f.order_st.written(key);
    return CSKY_OK;
}

// What the set-up of a frame with these push constants is given.  The launch asks again for the same frame (clouds_dev), so that the march it
// picks by SetupArgs::ct_mode is the one compiled for the mode in the slot's FrameConsts; a launch without a set-up of its own (csky_time_clouds)
// follows one of the same call, with the same noise set and switches.
SetupArgs setup_args(csky_ctx* c, const CloudParams& cp) {
    const ExactRejects rej = c->noise.st.rejects(cp.cloud_coverage, c->use_window);
    return {c->primary_steps, c->light_steps, c->early_eps, rej.hf_lo, rej.hf_hi, rej.ct_mode, c->use_window ? 1 : 0};
}

// Frame set-up on the context's stream (beside the caller's: context.h) into the next slot of the ring; the launch stream s waits for it.
int frame_setup(csky_ctx* c, const CloudParams& cp, hipStream_t s) {
    const SetupArgs sa = setup_args(c, cp);
    int f, rc; if ((rc = c->ring.next_slot(c, c->stream, f))) return rc;
    const SkyLut& l = c->lut;
    if (l.st.own_taps())                             // the set-up renders the texels of its three taps (clouds.glsl:163-167) itself
        HIPCHK(c, launch_frame_setup_taps(cp, l.st.sun, c->d_trans_f, c->tw, c->th, l.st.w, l.st.h, sa, c->ring.slot[f].fc, c->stream, c->tlut));
    else
        HIPCHK(c, launch_frame_setup(cp, l.cur_f(), l.aw, l.ah, sa, c->ring.slot[f].fc, c->stream));
    return c->ring.setup_enqueued(c, f, c->stream, s);
}

}  // namespace

int check_bands(csky_ctx* c, const csky_bands* b, int tile_w) {
    if (tile_w < 1 || !b || b->band_rows < 1 || b->n_bands < 0 || b->first_band < 0 || b->band_stride < 1)
        return fail(c, CSKY_ERR_INVALID, "render_clouds: bad tile/bands description");
    return CSKY_OK;
}

int clouds_dev(csky_ctx* c, const csky_cloud_params* p, int tile_w, const csky_bands* b, uint2* d_out, size_t pitch_bytes, hipStream_t s,
               unsigned long long* d_stats, bool setup, bool out_full) {
    if (!p) return fail(c, CSKY_ERR_INVALID, "render_clouds: params is NULL");
    if (!c->noise.st.have()) return fail(c, CSKY_ERR_STATE, "render_clouds: csky_set_noise has not been called");
    if (c->lut.st.holds == SkyLutHolds::None) return fail(c, CSKY_ERR_STATE, "render_clouds: no sky LUT yet (call csky_render_sky_lut first; cloud_sky.gd:187,242)");
    if (!(p->texture_size[0] >= 1.0f) || !(p->texture_size[1] >= 1.0f)) return fail(c, CSKY_ERR_INVALID, "render_clouds: texture_size must be >= 1");
    int rc; if ((rc = check_bands(c, b, tile_w))) return rc;
    if (pitch_bytes % 8 || pitch_bytes < (size_t)tile_w * 8) return fail(c, CSKY_ERR_INVALID, "render_clouds: row pitch must be a multiple of 8 and >= tile_w*8");
    if (b->n_bands == 0) return CSKY_OK;
    CloudParams cp; memcpy(&cp, p, sizeof cp);
    if (setup && (rc = frame_setup(c, cp, s))) return rc;
    RenderGeom g; g.tile_w = tile_w; g.band_rows = b->band_rows; g.first_band = b->first_band; g.band_stride = b->band_stride; g.n_bands = b->n_bands;
    g.pitch_px = (uint32_t)(pitch_bytes / 8); g.out_full = out_full ? 1 : 0;
    const long long waves = ((long long)(tile_w + 7) / 8) * (((long long)b->n_bands * b->band_rows + 7) / 8);
    // the policy is told how many frames CAN overlap (csky_set_frames_in_flight): where the hardware queues cannot keep the frames' streams apart the launches
    // run one after the other, and the forms chosen for overlapping launches (the persistent one above all) are the slower ones alone
    const LaunchPlan pl = plan_launch({c->variant, c->noise.st.cell32(), c->segments, c->sched_mode, c->frames_overlapping, c->persistent}, waves);
    const int tiles_x = (g.tile_w + pl.bw - 1) / pl.bw, slabs = (g.n_bands * g.band_rows + 7) >> 3, nblocks = tiles_x * slabs;
    FrameRing& ring = c->ring;
    const int slot = ring.cur;                                   // without set-up (the warm-up and timed launches of csky_time_clouds): the current slot again
    uint32_t* const heads = pl.persist ? ring.heads(slot) : nullptr;
    TexSet32 t32; const TexSet32* t32p = nullptr;
    if (c->noise.st.cell32()) { t32 = texset32(c); t32p = &t32; }
    // timing pair of this launch (csky_set_kernel_timing).  Taken BEFORE the order table on purpose: next_pair may create events and may fail, and
    // either after ensure_order would change the order of the HIP calls a launch makes
    const Event* kt = nullptr;
    if (c->kt.on && (rc = c->kt.next_pair(c, kt))) return rc;
    if ((rc = ensure_order(c, slot, pl.static_mode, tiles_x, slabs, s))) return rc;
    const uint32_t* order = ring.slot[slot].order;
    int grid = ring.slot[slot].order_st.grid();
    uint32_t* cost = nullptr;                                    // per-workgroup costs this launch records (cost feedback only)
    if (pl.feedback) {
        // mode 7: this launch runs in the order derived from the costs of the previous launch ON THE SAME RING SLOT (same geometry and
        // view), records its own costs and derives the next order from them.  The first launch of a geometry uses the static order.  Costs,
        // order and sort scratch are per ring slot (= per frame parity, like the frame constants), so two frames in flight on two
        // streams never share them; reuse of a slot is ordered by ev_clouds, recorded below after the sort.
        if ((rc = ring.reserve_feedback(c, (size_t)(grid > nblocks ? grid : nblocks)))) return rc;
        cost = ring.cost(slot);
        const FeedbackKey fkey = feedback_key(g.tile_w, g.band_rows, g.first_band, g.band_stride, g.n_bands, cp.texture_size, cp.update_position, pl.mode, pl.static_mode, pl.seg);
        if (ring.slot[slot].feedback.begin(fkey)) { order = ring.feedback_order(slot); grid = nblocks; }
    }
    if (kt) HIPCHK(c, hipEventRecord(kt[0], s));
    // (Round 6, measured and removed, profiles/r06/split_tail_ab.txt: a feedback launch as TWO -- the heaviest 60-90 % of the feedback order here, the lightest 10-40 % on a
    // second stream at equal or lowest priority to back-fill the tail: one frame at a time 2.00 -> 2.00-2.05 ms, frames identical.  The tail is the last wavefronts'
    // serial chains, not idle slots; the next frame fills it.)
    {   // a failed persistent launch may leave the slot's pop counters armed: re-zero them so that the next launch on this slot starts clean
        const hipError_t le = launch_clouds(pl.variant, pl.seg, texset(c), ring.fc(), g, order, grid, d_out, d_stats, cost, s, heads, c->resident_wgs, t32p, c->census_lean,
                                                setup_args(c, cp).ct_mode, c->resident_wgs_slim);
        if (le != hipSuccess) { if (heads) (void)hipMemsetAsync(heads, 0, 16 * sizeof(uint32_t), s); return fail(c, CSKY_ERR_HIP, "cloud kernel launch failed: %s", hipGetErrorString(le)); }
    }
    if (kt) HIPCHK(c, hipEventRecord(kt[1], s));
    if (pl.feedback) {
        HIPCHK(c, launch_lpt_order(cost, nblocks, lpt_shift(c->primary_steps), ring.sort_scratch(slot), ring.feedback_order(slot), s));   // order_core.h: the largest cost lands below 1024 buckets
        ring.slot[slot].feedback.sort_enqueued();
    }
    return ring.march_enqueued(c, slot, s);
}

}  // namespace csky
