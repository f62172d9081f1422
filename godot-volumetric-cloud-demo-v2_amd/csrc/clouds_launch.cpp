// clouds_launch.cpp -- one launch of the cloud kernel (clouds_dev): frame set-up on the context's stream, the workgroup order of the launch
// (static tables, cost feedback), per-launch timing events, and the launch itself.  Which kernel runs and how is launch_policy.h's decision.
#include <cstring>
#include "context.h"
#include "bake.h"
#include "launch_policy.h"
#include "order_core.h"

namespace csky {

TexSet texset(const csky_ctx* c) {
    TexSet t;
#ifdef CSKY_BRICK_BOUND
    t.brick = c->d_brick;
#endif
    t.shape = c->d_shape; t.detail = c->d_detail; t.weather = c->d_weather; t.sky = c->lut.cur_f(); t.sky_w = c->lut.aw; t.sky_h = c->lut.ah; t.detail_lod5 = c->detail_lod5; t.detail_h = c->d_detail_h; t.detail_lds = nullptr;
    return t;
}

TexSet32 texset32(const csky_ctx* c) {
    TexSet32 t;
    static_cast<TexSet&>(t) = texset(c);
    t.shape32 = c->d_shape32; t.detail32 = c->d_detail32; t.weather32 = c->d_weather32;
    return t;
}

namespace {

// Static workgroup order for ring slot `slot` (cloud_kernels.hip::static_order_kernel; modes 1, 2, 5).  Measured on the headline frame
// (queue kernel, round 1): 5 (slab rows round-robin over the XCDs) 3.93 ms, 1 (contiguous eighths) 4.80 ms, 2 (natural) 4.92 ms;
// azimuth-wedge and horizon-first orders (5.3-5.8 / 4.77 ms) were dropped in round 2.  The table depends on the launch geometry
// only (not on update_position: the reference's tile walk re-uses it) and is written by a kernel on the launch's stream.
int ensure_order(csky_ctx* c, int slot, int mode, int tiles_x, int slabs, hipStream_t s) {
    const int grid = static_order_grid(mode, tiles_x, slabs);                    // order_core.h
    // everything the table is a function of.  (Until the launch-order tests the key held tile_w in place of tiles_x: in mode 1 a 33-pixel-wide launch of one slab
    // has a grid of 8 as whole rays, 2 footprints, and as two segments, 3 footprints, and the second form found the first one's table and left a footprint out.)
    const long long key[4] = {tiles_x, slabs, mode, grid};
    if (c->d_order_ring[slot] && memcmp(key, c->order_key_ring[slot], sizeof key) == 0) return CSKY_OK;
    if (c->d_order_ring[slot].count() < (size_t)grid) {
        // growing is rare and costs a device-wide wait (an older launch may still read the old table): grow EVERY slot's table now, so that it
        // happens once, at the first frame of a geometry, and not again at the first use of each of the other ring slots (with rings eight deep
        // and a five-frame warm-up that was three synchronisations inside a timed region)
        HIPCHK(c, hipDeviceSynchronize());
        for (int k = 0; k < RING; k++) {
            if (c->d_order_ring[k].count() >= (size_t)grid) continue;
            int rc; if ((rc = c->d_order_ring[k].alloc(c, (size_t)grid))) return rc;
            for (long long& v : c->order_key_ring[k]) v = -1;
        }
    }
    // the last reader of this slot's table is the march of two frames ago; the caller has already ordered `s` behind it (ev_clouds -> the context's stream ->
    // ev_setup -> s), exactly like the frame constants of the slot
    HIPCHK(c, launch_static_order(mode, tiles_x, slabs, grid, c->d_order_ring[slot], s));
    c->order_grid_ring[slot] = grid;
    memcpy(c->order_key_ring[slot], key, sizeof key);
    return CSKY_OK;
}

}  // namespace

void exact_rejects(csky_ctx* c, float coverage, float& hf_lo, float& hf_hi, int& ct_mode) {
    if (c->win_cov != coverage) {                       // height window of the exact reject (bake.h), cached per coverage value
        height_window((double)coverage, c->w_rmin, c->w_rmax, c->w_bmax, c->win_lo, c->win_hi);
        c->win_cov = coverage;
    }
    hf_lo = c->use_window ? c->win_lo : -1.0f; hf_hi = c->use_window ? c->win_hi : 2.0f;
    // cloud-type range of the weather map (texel values 0..255): all >= 128 or all <= 127 fixes the branch of the height gradient
    ct_mode = !c->use_window ? 0 : (c->w_rmin * 255.0 >= 127.5 ? 1 : (c->w_rmax * 255.0 <= 127.5 ? 2 : 0));
}

int check_bands(csky_ctx* c, const csky_bands* b, int tile_w) {
    if (tile_w < 1 || !b || b->band_rows < 1 || b->n_bands < 0 || b->first_band < 0 || b->band_stride < 1)
        return fail(c, CSKY_ERR_INVALID, "render_clouds: bad tile/bands description");
    return CSKY_OK;
}

// The event pool of csky_set_kernel_timing grows to `want` events.  All or nothing: an event that cannot be made part-way used to leave
// null entries in the pool for later timed launches to record on; now the new events made so far go with the resize and the pool keeps its old size.
int grow_timing_pool(csky_ctx* c, size_t want) {
    const size_t old_n = c->kt_ev.size();
    if (want <= old_n) return CSKY_OK;
    c->kt_ev.resize(want);
    for (size_t i = old_n; i < want; i++)
        if (const int rc = c->kt_ev[i].create(c, hipEventDefault)) { c->kt_ev.resize(old_n); return rc; }
    return CSKY_OK;
}

int clouds_dev(csky_ctx* c, const csky_cloud_params* p, int tile_w, const csky_bands* b, uint2* d_out, size_t pitch_bytes, hipStream_t s,
               unsigned long long* d_stats, bool setup, bool out_full) {
    if (!p) return fail(c, CSKY_ERR_INVALID, "render_clouds: params is NULL");
    if (!c->have_noise) return fail(c, CSKY_ERR_STATE, "render_clouds: csky_set_noise has not been called");
    if (c->lut.st.holds == SkyLutHolds::None) return fail(c, CSKY_ERR_STATE, "render_clouds: no sky LUT yet (call csky_render_sky_lut first; cloud_sky.gd:187,242)");
    if (!(p->texture_size[0] >= 1.0f) || !(p->texture_size[1] >= 1.0f)) return fail(c, CSKY_ERR_INVALID, "render_clouds: texture_size must be >= 1");
    int rc; if ((rc = check_bands(c, b, tile_w))) return rc;
    if (pitch_bytes % 8 || pitch_bytes < (size_t)tile_w * 8) return fail(c, CSKY_ERR_INVALID, "render_clouds: row pitch must be a multiple of 8 and >= tile_w*8");
    if (b->n_bands == 0) return CSKY_OK;
    CloudParams cp; memcpy(&cp, p, sizeof cp);
    if (setup) {
        float lo, hi; int ctm;
        exact_rejects(c, cp.cloud_coverage, lo, hi, ctm);
        // frame set-up on the context's stream (beside the caller's: context.h) into the other constants slot (its last reader, the march two frames ago, must be done)
        const int f = (c->fc_cur + 1) % RING;
        if (c->clouds_pending[f]) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_clouds[f], 0));
        const SetupArgs sa = {c->primary_steps, c->light_steps, c->early_eps, lo, hi, ctm, c->use_window ? 1 : 0};
        const SkyLut& l = c->lut;
        if (l.st.own_taps())                             // the set-up renders the texels of its three taps (clouds.glsl:163-167) itself
            HIPCHK(c, launch_frame_setup_taps(cp, l.st.sun, c->d_trans_f, c->tw, c->th, l.st.w, l.st.h, sa, c->fc_ring[f], c->stream, c->tlut));
        else
            HIPCHK(c, launch_frame_setup(cp, l.cur_f(), l.aw, l.ah, sa, c->fc_ring[f], c->stream));
        HIPCHK(c, hipEventRecord(c->ev_setup[f], c->stream));
        c->fc_cur = f; c->d_fc = c->fc_ring[f];
        // (Round 5 bounded what folding the set-up INTO the march launch could return by simply not waiting here -- legal in a timing run with constant
        // parameters: whole frame one at a time 2.014 -> 2.000 ms, a 1/8 share 0.408 -> 0.404, eight in flight 0.224 -> 0.227: the prologue of frame k + 1
        // already runs under the march of frame k; profiles/r05/rows_overlap_ab.txt.)
        HIPCHK(c, hipStreamWaitEvent(s, c->ev_setup[f], 0));
    }
    RenderGeom g; g.tile_w = tile_w; g.band_rows = b->band_rows; g.first_band = b->first_band; g.band_stride = b->band_stride; g.n_bands = b->n_bands;
    g.pitch_px = (uint32_t)(pitch_bytes / 8); g.out_full = out_full ? 1 : 0;
    const long long waves = ((long long)(tile_w + 7) / 8) * (((long long)b->n_bands * b->band_rows + 7) / 8);
    // the policy is told how many frames CAN overlap (csky_set_frames_in_flight): where the hardware queues cannot keep the frames' streams apart the launches
    // run one after the other, and the forms chosen for overlapping launches (the persistent one above all) are the slower ones alone
    const LaunchPlan pl = plan_launch({c->variant, c->cell32, c->segments, c->sched_mode, c->frames_overlapping, c->persistent}, waves);
    const int tiles_x = (g.tile_w + pl.bw - 1) / pl.bw, slabs = (g.n_bands * g.band_rows + 7) >> 3, nblocks = tiles_x * slabs;
    const int slot = c->fc_cur;
    uint32_t* const heads = pl.persist ? c->d_heads + slot * 16 : nullptr;
    TexSet32 t32; const TexSet32* t32p = nullptr;
    if (c->cell32) { t32 = texset32(c); t32p = &t32; }
    const Event* kt = nullptr;                                   // timing pair of this launch (csky_set_kernel_timing)
    if (c->kt_on) {
        if ((size_t)c->kt_count * 2 + 2 > c->kt_ev.size()) {    // the pool grows on demand: no launch is ever dropped from the sum
            if ((rc = grow_timing_pool(c, c->kt_ev.empty() ? 512 : c->kt_ev.size() * 2))) return rc;
        }
        kt = &c->kt_ev[(size_t)c->kt_count * 2]; c->kt_count++;
    }
    if ((rc = ensure_order(c, slot, pl.static_mode, tiles_x, slabs, s))) return rc;
    const uint32_t* order = c->d_order_ring[slot];
    int grid = c->order_grid_ring[slot];
    uint32_t* cost = nullptr;                                    // per-workgroup costs this launch records (cost feedback only)
    uint32_t* lorder = nullptr;
    if (pl.feedback) {
        // mode 7: this launch runs in the order derived from the costs of the previous launch ON THE SAME RING SLOT (same geometry and
        // view), records its own costs and derives the next order from them.  The first launch of a geometry uses the static order.  Costs,
        // order and sort scratch are per ring slot (= per frame parity, like the frame constants), so two frames in flight on two
        // streams never share them; reuse of a slot is ordered by ev_clouds, recorded below after the sort.
        const size_t need = (size_t)(grid > nblocks ? grid : nblocks);
        if (c->d_lpt_order.count() < RING * need) {
            HIPCHK(c, hipDeviceSynchronize());                   // (re)allocation is rare; frames may be in flight on other streams
            c->d_wg_cost.reset(); c->d_lpt_order.reset();        // the order, allocated last, carries the capacity of the pair: a failure on the way leaves it empty
            for (int k = 0; k < RING; k++) c->lpt_valid[k] = false;
            if ((rc = c->d_wg_cost.alloc(c, RING * need))) return rc;
            if (!c->d_lpt_hist) {
                if ((rc = c->d_lpt_hist.alloc(c, RING * 2048))) return rc;
                HIPCHK(c, hipMemset(c->d_lpt_hist, 0, RING * 2048 * sizeof(uint32_t)));
            }
            HIPCHK(c, hipMemset(c->d_wg_cost, 0, RING * need * sizeof(uint32_t)));       // the sort kernels leave both zeroed afterwards
            if ((rc = c->d_lpt_order.alloc(c, RING * need))) return rc;
        }
        const size_t per_slot = c->d_lpt_order.count() / RING;
        cost = c->d_wg_cost + (size_t)slot * per_slot;
        lorder = c->d_lpt_order + (size_t)slot * per_slot;
        // the costs belong to one view of one tile: same launch geometry AND same place in the texture (a tile walk never reuses them)
        const long long fkey[11] = {g.tile_w, g.band_rows, g.first_band, g.band_stride, g.n_bands, (long long)cp.texture_size[0], (long long)cp.texture_size[1],
                                    (long long)cp.update_position[0], (long long)cp.update_position[1], pl.mode * 16 + pl.static_mode, pl.seg};
        if (memcmp(c->lpt_key[slot], fkey, sizeof fkey) != 0) { c->lpt_valid[slot] = false; memcpy(c->lpt_key[slot], fkey, sizeof fkey); }
        if (c->lpt_valid[slot]) { order = lorder; grid = nblocks; }
    }
    if (kt) HIPCHK(c, hipEventRecord(kt[0], s));
    // (Round 6, measured and removed, profiles/r06/split_tail_ab.txt: a feedback launch as TWO -- the heaviest 60-90 % of the feedback order here, the lightest 10-40 % on a
    // second stream at equal or lowest priority to back-fill the tail: one frame at a time 2.00 -> 2.00-2.05 ms, frames identical.  The tail is the last wavefronts'
    // serial chains, not idle slots; the next frame fills it.)
    {   // a failed persistent launch may leave the slot's pop counters armed: re-zero them so that the next launch on this slot starts clean
        const hipError_t le = launch_clouds(pl.variant, pl.seg, texset(c), c->d_fc, g, order, grid, d_out, d_stats, cost, s, heads, c->resident_wgs, t32p, c->census_lean);
        if (le != hipSuccess) { if (heads) (void)hipMemsetAsync(heads, 0, 16 * sizeof(uint32_t), s); return fail(c, CSKY_ERR_HIP, "cloud kernel launch failed: %s", hipGetErrorString(le)); }
    }
    if (kt) HIPCHK(c, hipEventRecord(kt[1], s));
    if (pl.feedback) {
        HIPCHK(c, launch_lpt_order(cost, nblocks, lpt_shift(c->primary_steps), c->d_lpt_hist + slot * 2048, lorder, s));   // order_core.h: the largest cost lands below 1024 buckets
        c->lpt_valid[slot] = true;
    }
    HIPCHK(c, hipEventRecord(c->ev_clouds[slot], s)); c->clouds_pending[slot] = true;
    return CSKY_OK;
}

}  // namespace csky
