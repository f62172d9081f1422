/*
 * cloudsky_shadow_hooks.h -- the A/B switch of the cloud shadow map's exact end.  Part of the lab bench (cloudsky_internal.h includes it; include
 * that one), never of the product surface: the maps are byte-identical either way.
 */
#ifndef CLOUDSKY_SHADOW_HOOKS_H
#define CLOUDSKY_SHADOW_HOOKS_H
#include "cloudsky.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 1 (the default): a texel of csky_render_cloud_shadow* whose exponent density * ss * tau has reached 18 stops sampling, its stored half is 0
 * whatever follows (csrc/shadow_core.h shadow_march).  0: every texel takes all its samples.  The bytes are identical. */
int csky_set_shadow_exact_end(csky_ctx* ctx, int enabled);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDSKY_SHADOW_HOOKS_H */
