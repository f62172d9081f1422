/*
 * cloudsky_lut_hooks.h -- the A/B switch and the launch counter of the sky LUT's reuse.  Part of the lab bench (cloudsky_internal.h includes it;
 * include that one), never of the product surface: a host needs neither, it may call csky_render_sky_lut* every pass and pays a launch only
 * when the sun, the LUT's size or the transmittance table has changed.
 */
#ifndef CLOUDSKY_LUT_HOOKS_H
#define CLOUDSKY_LUT_HOOKS_H
#include "cloudsky.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 1 (the default): csky_render_sky_lut / csky_render_sky_lut_device launch nothing when asked for the LUT the context holds (same sun direction
 * bit for bit, same size, same transmittance table and mapping, a whole LUT this context rendered alone); csky_render_sky_lut_rows_device
 * answers the same request again with one device copy of the rows it kept; csky_multi_render_sky_lut (the switch of the handle's first
 * context) renders on no device.  0: a launch per call, as before the reuse existed.  Results are identical either way. */
int csky_set_sky_lut_reuse(csky_ctx* ctx, int enabled);
/* Sky-LUT kernels this context has launched since it was created, the whole and the rows form together (a csky_multi handle counts each
 * device's rows on that device's context). */
int64_t csky_sky_lut_launches(const csky_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDSKY_LUT_HOOKS_H */
