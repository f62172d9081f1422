// radiance_core.h -- the sky's radiance cubemap: cube-face geometry, the source-cube table and the GGX prefilter sum of
// include/cloudsky.h (csky_render_radiance*, csky_prefilter_cube).  Host+device like the other cores: radiance.hip instantiates
// it for gfx950, tests/radiance_host compiles it with g++ for the CPU tests.
//
// Layer k >= 1 of L (roughness r = k/(L-1), alpha = r^2, split-sum N = V = R) is the exact discrete form of the integral the engine's
// GGX importance sampler estimates:
//     P_k(N) = sum_t w(N,t) C_t / sum_t w(N,t),   w = c Omega_t / (c (a2-1)/2 + (a2+1)/2)^2 for c = N.L_t > 0, else 0,   a2 = alpha^2
// over every texel t of the source cube.  With e2 = |N - L_t|^2 = 2 (1 - c) for unit vectors the denominator is
//     d = a2 + e2 (1 - a2) / 4
// which has no cancellation when N ~ L_t (where a rough-0.1 lobe puts nearly all of its weight), unlike c (a2-1)/2 + (a2+1)/2.
#pragma once
#include "csky_common.h"

namespace csky {

constexpr int RAD_MAX_LAYERS = 10;        // L = 1..10
constexpr int RAD_WAVES = 8;              // waves of one filter workgroup: they share one 8x8 output block and split the source blocks

// Face f, face coordinates (sc, tc) in [-1, 1] -> unnormalised direction (Vulkan major-axis rule; faces +X, -X, +Y, -Y, +Z, -Z)
CSKY_HD void rad_face_vec(int f, double sc, double tc, double& x, double& y, double& z) {
    switch (f) {
        case 0: x = 1.0; y = -tc; z = -sc; break;
        case 1: x = -1.0; y = -tc; z = sc; break;
        case 2: x = sc; y = 1.0; z = tc; break;
        case 3: x = sc; y = -1.0; z = -tc; break;
        case 4: x = sc; y = -tc; z = 1.0; break;
        default: x = -sc; y = -tc; z = -1.0; break;
    }
}

// Texel-centre direction of texel (i = col, j = row) of face f of an n x n face, computed in double and rounded once: the same bits
// for the output texel N and the source texel L_t whenever the two faces have the same size
CSKY_HD void rad_texel_dir(int f, int i, int j, int n, float& x, float& y, float& z) {
    double dx, dy, dz;
    rad_face_vec(f, 2.0 * (i + 0.5) / n - 1.0, 2.0 * (j + 0.5) / n - 1.0, dx, dy, dz);
    const double l = sqrt(dx * dx + dy * dy + dz * dz);
    x = (float)(dx / l); y = (float)(dy / l); z = (float)(dz / l);
}

// Exact solid angle of texel (i, j) of an n x n face: A(x0,y0) - A(x0,y1) - A(x1,y0) + A(x1,y1), A(x,y) = atan2(xy, sqrt(x^2+y^2+1))
// (in double: in float the four O(1) terms cancel to a 1e-3 result at n = 64)
CSKY_HD double rad_area_term(double x, double y) { return atan2(x * y, sqrt(x * x + y * y + 1.0)); }
CSKY_HD double rad_solid_angle(int i, int j, int n) {
    const double x0 = 2.0 * i / n - 1.0, x1 = 2.0 * (i + 1) / n - 1.0, y0 = 2.0 * j / n - 1.0, y1 = 2.0 * (j + 1) / n - 1.0;
    return rad_area_term(x0, y0) - rad_area_term(x0, y1) - rad_area_term(x1, y0) + rad_area_term(x1, y1);
}

// Source texels are grouped in blocks of bs x bs (bs = min(n, 8)) of one face; the table is block-major so that a block is contiguous:
// block b = (f * nb + by) * nb + bx (nb = n / bs), texel t of the block = ty * bs + tx.  Record = two float4:
// {L.x, L.y, L.z, Omega}, {Omega R, Omega G, Omega B, 0}.
CSKY_HD int rad_block_size(int n) { return n < 8 ? n : 8; }
CSKY_HD int rad_block_count(int n) { const int nb = n / rad_block_size(n); return 6 * nb * nb; }

// Source texel (f, i, j) of an ns x ns source cube: the mean of its k x k texels of the n x n layer 0 (RGBA16F, faces back to back),
// k = n / ns, summed row by row in double and rounded once to fp32 (an fp32 sum drifts by several fp16 ulp at k = 512 with HDR texels;
// k = 1 gives the texel itself); the record goes to rec[2 * (block index * bs^2 + texel in block)]
CSKY_HD void rad_source_texel(const uint16_t* layer0, int n, int ns, int f, int i, int j, float4* tab) {
    const int k = n / ns;
    double sr = 0.0, sg = 0.0, sb = 0.0;
    for (int y = 0; y < k; y++)
        for (int x = 0; x < k; x++) {
            const uint16_t* p = layer0 + (((size_t)f * n + (size_t)j * k + y) * n + (size_t)i * k + x) * 4;
            sr += h2f(p[0]); sg += h2f(p[1]); sb += h2f(p[2]);
        }
    const double inv = 1.0 / ((double)k * k);                      // a power of two: exact
    const float r = (float)(sr * inv), g = (float)(sg * inv), b = (float)(sb * inv);
    float lx, ly, lz;
    rad_texel_dir(f, i, j, ns, lx, ly, lz);
    const float om = (float)rad_solid_angle(i, j, ns);
    const int bs = rad_block_size(ns), nb = ns / bs;
    const size_t idx = ((size_t)(f * nb + j / bs) * nb + i / bs) * (bs * bs) + (size_t)(j % bs) * bs + (i % bs);
    tab[2 * idx] = float4{lx, ly, lz, om};
    tab[2 * idx + 1] = float4{om * r, om * g, om * b, 0.0f};
}

// Bounding cone of block b of an n x n face over its texel-centre directions: {axis, half-angle + a small margin} (double, rounded once)
CSKY_HD float4 rad_block_cone(int n, int b) {
    const int bs = rad_block_size(n), nb = n / bs;
    const int f = b / (nb * nb), by = (b / nb) % nb, bx = b % nb;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int t = 0; t < bs * bs; t++) {
        float x, y, z;
        rad_texel_dir(f, bx * bs + t % bs, by * bs + t / bs, n, x, y, z);
        ax += x; ay += y; az += z;
    }
    const double l = sqrt(ax * ax + ay * ay + az * az);
    ax /= l; ay /= l; az /= l;
    double mind = 1.0;
    for (int t = 0; t < bs * bs; t++) {
        float x, y, z;
        rad_texel_dir(f, bx * bs + t % bs, by * bs + t / bs, n, x, y, z);
        const double d = ax * x + ay * y + az * z;
        mind = d < mind ? d : mind;
    }
    const double th = acos(mind < -1.0 ? -1.0 : (mind > 1.0 ? 1.0 : mind)) + 1e-4;
    return float4{(float)ax, (float)ay, (float)az, (float)th};
}

// Conservative back-face cull of a (receiver block, source block) pair: true only when every pair of directions in the two cones is more
// than 90 degrees + 2e-3 rad apart, so every c = N.L of the pair is below -1e-3 and every weight of the pair is exactly zero (the sum
// is byte-identical with and without the cull: adding +0 changes no accumulator)
CSKY_HD bool rad_cull(const float4& a, const float4& b) {
    const float d = a.x * b.x + a.y * b.y + a.z * b.z;
    const float ang = acosf(fminf(fmaxf(d, -1.0f), 1.0f));
    return ang > 1.57079637f + a.w + b.w + 2e-3f;
}

// Per-layer constants: d = fmaf(e2, k1, a2) with a2 = alpha^2, k1 = (1 - a2) / 4
struct RadLayer { float a2, k1; };
CSKY_HD RadLayer rad_layer(int k, int L) {
    const double r = (double)k / (double)(L - 1), al = r * r, a2 = al * al;
    return RadLayer{(float)a2, (float)((1.0 - a2) * 0.25)};
}

// v_rcp_f32: at most 0.882 ulp on [0.5, 2), 1 / 2^k exact (measured; tests/test_gpu_primitives.py::test_rcp_error[rad_rcp], test_known_answers)
CSKY_HD float rad_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// One source record into the NL accumulators {sum w R, sum w G, sum w B, sum w} of receiver direction (nx, ny, nz).  Shared by the
// layers: e2, c, c Omega, c Omega RGB (12 VALU); per layer 1 fma, 1 mul, 1 rcp, 4 fma.
template <int NL>
CSKY_HD void rad_accumulate(float nx, float ny, float nz, const float4& r0, const float4& r1, const RadLayer* ly, float4* acc) {
    const float dx = nx - r0.x, dy = ny - r0.y, dz = nz - r0.z;
    const float e2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const float c = fmaxf(fmaf(e2, -0.5f, 1.0f), 0.0f);            // N.L, clamped: no weight behind the receiver
    const float cw = c * r0.w, cr = c * r1.x, cg = c * r1.y, cb = c * r1.z;
#pragma unroll
    for (int l = 0; l < NL; l++) {
        const float d = fmaf(e2, ly[l].k1, ly[l].a2);
        const float q = rad_rcp(d * d);
        acc[l].x = fmaf(q, cr, acc[l].x);
        acc[l].y = fmaf(q, cg, acc[l].y);
        acc[l].z = fmaf(q, cb, acc[l].z);
        acc[l].w = fmaf(q, cw, acc[l].w);
    }
}

}  // namespace csky
