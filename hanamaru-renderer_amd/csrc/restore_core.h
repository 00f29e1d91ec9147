// The restored robust resolve R' (DESIGN.md §4.14): the robust radiance of robust_core.h plus what its trimmed hot buckets held above the highest
// kept bucket, spread over the neighbourhood along the guide planes.  Per pixel, all f64, host-compilable like robust_core.h and denoise_core.h.
// THIS HEADER IS THE DEFINITION: every operation is a single IEEE f64 operation in the order written (+ - x / max and comparisons only, no FMA —
// contraction is off), so the device, a host build and any restatement of these lines agree bit for bit.
//   the excess of a pixel, robust_pixel_excess_k<K>(B, n) -> cx[6] = {C_r, C_g, C_b, X_r, X_g, X_b} and trim
//       n == 0     C = 0, X = 0, trim = 0
//       n <  K     C_c = ((B[0][c] + .. + B[K-1][c]) / (double)n) / 4.0 — robust_pixel_k's plain mean before its rounding —, X = 0, trim = 0
//       otherwise  the sorted bucket means m_(1) .. m_(K) and the trim t of robust_sorted_means_k<K>: the same lines, the same bits
//                  C_c   = (m_(t+1),c + .. + m_(K-t),c) / (double)(K - 2 t)           robust_channel_cv_k: (float)C_c is robust_pixel's R_c
//                  top_c = m_(K-t),c
//                  X_c   = max(0, ((m_(K-t+1),c - top_c) + .. + (m_(K),c - top_c)) / (double)K)     ascending, from the first term; t = 0: X_c = 0
//   X is what the hot buckets hold above the highest kept one, per channel, in the order the keys y give: never negative, zero where nothing is trimmed.
//   the spread, one level with step s: the 5 x 5 taps q = p + s (i, j), i, j = -2 .. 2, rows first; a tap outside the image is skipped
//       w(p, q) = denoise_guide_weight(denoise_tap_h(i, j), g_p, g_q)                  denoise_core.h's h, K, x_n, x_a, x_z, x_h: no colour term
//       N_p     = sum_q w(p, q)               restore_norm: from 0.0, one tap at a time (every w >= +0; the centre tap is 9/64)
//       S_p,c   = X_p,c / N_p
//       X'_q,c  = sum_p w(q, p) S_p,c         restore_gather: from 0.0, one tap at a time, each term one product
//   w(q, p) computed at q is w(p, q) to the bit, so the gather IS the scatter "p gives X_p w(p, q) / N_p to q": in real numbers sum X' = sum X.
//   output     R'_c = (float)(base_c + X_L,c), base = C, or (double)D_c of a denoised robust radiance D
#pragma once
#include "robust_core.h"

namespace hr {

constexpr uint32_t RESTORE_MAX_LEVELS = 5;

// a pixel's 8 guides by value.  On the device they come as two 16-byte loads (a pixel's guides are 32 bytes of a 32-byte-aligned plane)
struct RestoreGuides { float g[8]; };
HR_ROBUST_HD RestoreGuides restore_guides(const float *guides, size_t pixel) {
    RestoreGuides r;
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 *v = reinterpret_cast<const float4 *>(guides + pixel * 8);
    const float4 a = v[0], b = v[1];
    r.g[0] = a.x; r.g[1] = a.y; r.g[2] = a.z; r.g[3] = a.w; r.g[4] = b.x; r.g[5] = b.y; r.g[6] = b.z; r.g[7] = b.w;
#else
    for (int k = 0; k < 8; k++) r.g[k] = guides[pixel * 8 + k];
#endif
    return r;
}

// one channel's sorted means m and the trim t: what the t hot buckets hold above the highest kept one, over K, never negative
template <uint32_t K>
HR_ROBUST_HD double robust_channel_excess_k(const double (&m)[K], uint32_t t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    // element i (0-based) is a trimmed hot bucket iff i >= K - t; the highest kept one is K - 1 - t >= (K - 1) / 2
    double top = m[K - 1];
    HR_ROBUST_UNROLL
    for (uint32_t i = (K - 1) / 2; i < K - 1; i++) top = i == K - 1 - t ? m[i] : top;
    double s = 0.0;
    HR_ROBUST_UNROLL
    for (uint32_t i = (K + 1) / 2; i < K; i++) {
        const double d = m[i] - top;
        s = i == K - t ? d : (i > K - t ? s + d : s);
    }
    const double q = s / (double)K;
    return t != 0u && q > 0.0 ? q : 0.0;   // (a NaN is clamped too)
}

// B[K][3]: the pixel's buckets; n: its samplings; cx[6] = {C, X}; trim: the buckets dropped at either end
template <uint32_t K>
HR_ROBUST_HD void robust_pixel_excess_k(const double *B, uint64_t n, double *cx, uint8_t *trim) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    *trim = 0;
    cx[3] = cx[4] = cx[5] = 0.0;
    if (n == 0) { cx[0] = cx[1] = cx[2] = 0.0; return; }
    if (n < K) {
        const double nd = (double)n;
        HR_ROBUST_UNROLL
        for (int c = 0; c < 3; c++) {
            double s = B[c];
            HR_ROBUST_UNROLL
            for (uint32_t b = 1; b < K; b++) s = s + B[b * 3 + c];
            const double q = s / nd;
            cx[c] = q / 4.0;
        }
        return;
    }
    double m0[K], m1[K], m2[K];
    const uint32_t t = robust_sorted_means_k<K>(B, n, m0, m1, m2);
    robust_channel_cv_k<K, false>(m0, t, cx + 0, nullptr);
    robust_channel_cv_k<K, false>(m1, t, cx + 1, nullptr);
    robust_channel_cv_k<K, false>(m2, t, cx + 2, nullptr);
    cx[3] = robust_channel_excess_k<K>(m0, t);
    cx[4] = robust_channel_excess_k<K>(m1, t);
    cx[5] = robust_channel_excess_k<K>(m2, t);
    *trim = (uint8_t)t;
}

// the same for a run-time K (robust_valid_k(K); anything else: cx = 0, trim = 0)
HR_ROBUST_HD void robust_pixel_excess(const double *B, uint32_t K, uint64_t n, double *cx, uint8_t *trim) {
    switch (K) {
    case 3: robust_pixel_excess_k<3>(B, n, cx, trim); break;
    case 5: robust_pixel_excess_k<5>(B, n, cx, trim); break;
    case 7: robust_pixel_excess_k<7>(B, n, cx, trim); break;
    case 9: robust_pixel_excess_k<9>(B, n, cx, trim); break;
    case 11: robust_pixel_excess_k<11>(B, n, cx, trim); break;
    case 13: robust_pixel_excess_k<13>(B, n, cx, trim); break;
    case 15: robust_pixel_excess_k<15>(B, n, cx, trim); break;
    default: for (int c = 0; c < 6; c++) cx[c] = 0.0; *trim = 0; break;
    }
}

// One level's first half for the pixel (x, y) of a w x h image: S[3] = X_p / N_p.  X: the excess of pixel 0, xs doubles from one pixel to the next
// (the init plane holds it at cx + 3 with xs = 6, a level's output with xs = 3); guides[h][w][8].  Only sg.n2, sg.a2 and sg.z2 are read.
HR_ROBUST_HD void restore_norm(const double *X, uint32_t xs, const float *guides, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t step, const DenoiseSigmas &sg, double *S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t p = (size_t)y * w + x;
    const RestoreGuides gp = restore_guides(guides, p);
    double N = 0.0;
    for (int j = -2; j <= 2; j++) {
        const int64_t qy = (int64_t)y + (int64_t)step * j;
        if (qy < 0 || qy >= (int64_t)h) continue;
        for (int i = -2; i <= 2; i++) {
            const int64_t qx = (int64_t)x + (int64_t)step * i;
            if (qx < 0 || qx >= (int64_t)w) continue;
            const RestoreGuides gq = restore_guides(guides, (size_t)qy * w + (size_t)qx);
            N = N + denoise_guide_weight(denoise_tap_h(i, j), gp.g, gq.g, sg);
        }
    }
    const double *xp = X + p * xs;
    for (int c = 0; c < 3; c++) S[c] = xp[c] / N;
}

// One level's second half for the pixel (x, y): out[3] = sum over the taps p of w(q, p) S_p; S[h][w][3]
HR_ROBUST_HD void restore_gather(const double *S, const float *guides, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t step, const DenoiseSigmas &sg, double *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const RestoreGuides gq = restore_guides(guides, (size_t)y * w + x);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = -2; j <= 2; j++) {
        const int64_t py = (int64_t)y + (int64_t)step * j;
        if (py < 0 || py >= (int64_t)h) continue;
        for (int i = -2; i <= 2; i++) {
            const int64_t px = (int64_t)x + (int64_t)step * i;
            if (px < 0 || px >= (int64_t)w) continue;
            const size_t p = (size_t)py * w + (size_t)px;
            const RestoreGuides gp = restore_guides(guides, p);
            const double wt = denoise_guide_weight(denoise_tap_h(i, j), gq.g, gp.g, sg);
            const double *sp = S + p * 3;
            for (int c = 0; c < 3; c++) acc[c] = acc[c] + wt * sp[c];
        }
    }
    for (int c = 0; c < 3; c++) out[c] = acc[c];
}

// C[3]: the pixel's base as doubles, or D != nullptr: its denoised radiance; X[3]: its spread excess
HR_ROBUST_HD void restore_final(const double *C, const float *D, const double *X, float *r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int c = 0; c < 3; c++) {
        const double base = D ? (double)D[c] : C[c];
        r[c] = (float)(base + X[c]);
    }
}

// the whole thing over a w x h image on one thread (the host side of the tests and of tools/restore_quality.py; the device runs one thread per pixel:
// restore_init_kernel, spread_norm_kernel, spread_gather_kernel, restore_final_kernel, post_kernels.h).  counts == nullptr: every pixel has n_all
// samplings.  D == nullptr: base C; else base D[h][w][3].  work: w*h*15 doubles.  x_out (may be nullptr): X_L of every pixel, w*h*3 doubles.
inline void restore_image(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, const float *guides, uint32_t w, uint32_t h, uint32_t levels,
                          const DenoiseSigmas &sg, const float *D, double *work, float *r, double *x_out = nullptr) {
    const size_t pixels = (size_t)w * h;
    double *cx = work, *S = work + pixels * 6, *xa = work + pixels * 9, *xb = work + pixels * 12;
    uint8_t t;
    for (size_t p = 0; p < pixels; p++) robust_pixel_excess(buckets + p * K * 3, K, counts ? (uint64_t)counts[p] : n_all, cx + p * 6, &t);
    const double *X = cx + 3;
    uint32_t xs = 6;
    for (uint32_t l = 0; l < levels; l++) {
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) restore_norm(X, xs, guides, w, h, x, y, 1u << l, sg, S + ((size_t)y * w + x) * 3);
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) restore_gather(S, guides, w, h, x, y, 1u << l, sg, xa + ((size_t)y * w + x) * 3);
        X = xa; xs = 3;
        double *s = xa; xa = xb; xb = s;
    }
    for (size_t p = 0; p < pixels; p++) {
        restore_final(cx + p * 6, D ? D + p * 3 : nullptr, X + p * xs, r + p * 3);
        if (x_out) for (int c = 0; c < 3; c++) x_out[p * 3 + c] = X[p * xs + c];
    }
}

}  // namespace hr
