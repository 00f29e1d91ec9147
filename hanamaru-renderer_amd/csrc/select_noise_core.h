// The error estimate of the image hr_denoise_select makes, all f64, host-compilable like select_core.h.
// THIS HEADER IS THE DEFINITION: every operation is a single IEEE f64 operation in the order written (+ - x /, comparisons and integer arithmetic
// only; no FMA — contraction is switched off below, a host compiler that contracts by default wants -ffp-contract=off), so the device, a host
// build and any restatement of these lines agree bit for bit.  The one exception is the square root of select_noise_error, which is outside the
// definition of the plane M.
//   inputs of a pixel   per level l = 0 .. levels its three states F_A,l, F_B,l, F_W,l (fa, fb, fw: 6 doubles each, {C, V}) and the halves' level-0
//                       radiance A0, B0 of select_core.h; va0_c, vb0_c: component 3 + c of F_A,0 and F_B,0 — the variances of the raw halves, already
//                       divided with `demodulate`; its guides g[8]; dem = demodulate && levels
//   k_c                 dem: a = (double)g[c] + DENOISE_EPS, k_c = a a — what takes a demodulated square back to radiance units.  Without dem the
//                       products by k_c below are not performed at all
//   held-out error      dA_c = fa[c] - b0[c]    dB_c = fb[c] - a0[c]
//                       j_c = (dA_c dA_c + dB_c dB_c) - (va0_c + vb0_c)        h_c = j_c / 2.0 (then x k_c)
//                       m_l = (h_r + h_g) + h_b — the raw held-out MSE of a half filter; it may be negative
//   smoothing           m^_l: m_l through exactly the `smooth` passes of select_smooth that the pick's e_l goes through
//   variances           vh_c = (fa[3 + c] + fb[3 + c]) / 2.0 (x k_c)    vh = (vh_r + vh_g) + vh_b     the half filters' propagated variance
//                       vw_c = fw[3 + c] (x k_c)                        vw = (vw_r + vw_g) + vw_b     the whole-buffer filter's
//   estimate            x = m^_l - vh;  b2 = x > 0.0 ? x : 0.0 (a NaN is clamped too);  mse_l = vw + b2
//   M                   written exactly when select_pick takes level l (l == 0 || e^_l < best): M(p) = mse_L(p)(p).  The pick is select_core.h's
//   e_S                 den = (((double)S_r + (double)S_g) + (double)S_b) + 3.0 floor;  e_S = den > 0 ? sqrt(M) / den : 0 — robust_pixel_error's convention
// Half A is independent of B0, so E[dA^2] = MSE(F_A,l) + Var(B0): m^ - vh is the half filters' squared bias, which the whole-buffer filter keeps
// beside its own propagated variance vw.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "select_core.h"

namespace hr {

// m_l of a pixel: fa[6], fb[6] its filtered halves, a0[3], b0[3] the halves' level-0 radiance, va0[3], vb0[3] their level-0 variances
HR_DENOISE_HD double select_noise_m(const double *fa, const double *fb, const double *a0, const double *b0, const double *va0, const double *vb0, const float *g, int dem) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double hc[3];
    HR_ROBUST_UNROLL
    for (int c = 0; c < 3; c++) {
        const double dA = fa[c] - b0[c], dB = fb[c] - a0[c];
        const double j = (dA * dA + dB * dB) - (va0[c] + vb0[c]);
        double hh = j / 2.0;
        if (dem) {
            const double a = (double)g[c] + DENOISE_EPS;
            const double k = a * a;
            hh = hh * k;
        }
        hc[c] = hh;
    }
    return (hc[0] + hc[1]) + hc[2];
}

// mse_l of a pixel from its smoothed m^_l: va[3], vb[3], vw[3] the V of F_A,l, F_B,l, F_W,l
HR_DENOISE_HD double select_noise_mse(double mbar, const double *va, const double *vb, const double *vw, const float *g, int dem) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double vhc[3], vwc[3];
    HR_ROBUST_UNROLL
    for (int c = 0; c < 3; c++) {
        double h2 = (va[c] + vb[c]) / 2.0;
        double w2 = vw[c];
        if (dem) {
            const double a = (double)g[c] + DENOISE_EPS;
            const double k = a * a;
            h2 = h2 * k;
            w2 = w2 * k;
        }
        vhc[c] = h2;
        vwc[c] = w2;
    }
    const double vh = (vhc[0] + vhc[1]) + vhc[2];
    const double vwsum = (vwc[0] + vwc[1]) + vwc[2];
    const double x = mbar - vh;
    const double b2 = x > 0.0 ? x : 0.0;
    return vwsum + b2;
}

// the pick at level l with M beside it: M takes mse exactly when select_pick takes the level; best, L, S as select_pick leaves them
HR_DENOISE_HD void select_noise_pick(double e, double mse, uint32_t l, const double *fw, const float *g, int demodulate, double *best, uint8_t *L, float *S, double *M) {
    if (l == 0u || e < *best) *M = mse;
    select_pick(e, l, fw, g, demodulate, best, L, S);
}

// e_S of a pixel from M and S[3]
HR_DENOISE_HD double select_noise_error(double M, const float *S, double floor) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double den = (((double)S[0] + (double)S[1]) + (double)S[2]) + 3.0 * floor;
    return den > 0.0 ? sqrt(M) / den : 0.0;
}

// select_image with M beside S and L, on one thread: the same arguments, the same S and L bits (the same calls in the same order), and M[h][w].
// work: w*h*53 doubles (select_image's 45, the six planes {va0, vb0} and two planes of m).
inline void select_noise_image(const double *buckets, uint32_t K, const uint32_t *counts, uint32_t n_all, const float *acc, const double *mom, const float *guides, uint32_t w, uint32_t h,
                               uint32_t levels, int demodulate, const DenoiseSigmas &sg, uint32_t smooth, double *work, float *S, uint8_t *L, double *states, double *M) {
    const size_t pixels = (size_t)w * h;
    const int dem = demodulate && levels ? 1 : 0;
    double *st[2][3];
    for (int k = 0; k < 2; k++)
        for (int s = 0; s < 3; s++) st[k][s] = work + (size_t)(k * 3 + s) * pixels * 6;
    double *raw = work + pixels * 36, *e[2] = {work + pixels * 42, work + pixels * 43}, *best = work + pixels * 44;
    double *var0 = work + pixels * 45, *m[2] = {work + pixels * 51, work + pixels * 52};
    for (size_t p = 0; p < pixels; p++) {
        select_init(buckets + p * K * 3, K, counts ? counts[p] : n_all, acc + p * 3, mom + p * 6, guides + p * 8, dem, st[0][0] + p * 6, st[0][1] + p * 6, st[0][2] + p * 6);
        for (int c = 0; c < 3; c++) {
            raw[p * 6 + c] = st[0][0][p * 6 + c]; raw[p * 6 + 3 + c] = st[0][1][p * 6 + c];
            var0[p * 6 + c] = st[0][0][p * 6 + 3 + c]; var0[p * 6 + 3 + c] = st[0][1][p * 6 + 3 + c];
        }
    }
    for (uint32_t l = 0; l <= levels; l++) {
        double **cur = st[l & 1u], **nxt = st[(l + 1u) & 1u];
        for (size_t p = 0; p < pixels; p++) {
            e[0][p] = select_error(cur[0] + p * 6, cur[1] + p * 6, raw + p * 6, raw + p * 6 + 3);
            m[0][p] = select_noise_m(cur[0] + p * 6, cur[1] + p * 6, raw + p * 6, raw + p * 6 + 3, var0 + p * 6, var0 + p * 6 + 3, guides + p * 8, dem);
        }
        for (uint32_t t = 0; t < smooth; t++) {
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) {
                    e[1][(size_t)y * w + x] = select_smooth(e[0], w, h, x, y, 1u << t);
                    m[1][(size_t)y * w + x] = select_smooth(m[0], w, h, x, y, 1u << t);
                }
            double *sw = e[0]; e[0] = e[1]; e[1] = sw;
            sw = m[0]; m[0] = m[1]; m[1] = sw;
        }
        for (size_t p = 0; p < pixels; p++) {
            const double mse = select_noise_mse(m[0][p], cur[0] + p * 6 + 3, cur[1] + p * 6 + 3, cur[2] + p * 6 + 3, guides + p * 8, dem);
            select_noise_pick(e[0][p], mse, l, cur[2] + p * 6, guides + p * 8, dem, best + p, L + p, S + p * 3, M + p);
        }
        if (l < levels) {
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) {
                    const size_t p = (size_t)y * w + x;
                    double out[3][6];
                    select_level3(SelectStatesAoS{{cur[0], cur[1], cur[2]}}, guides, w, h, x, y, 1u << l, sg, out);
                    for (int s = 0; s < 3; s++)
                        for (int c = 0; c < 6; c++) nxt[s][p * 6 + c] = out[s][c];
                }
        }
    }
    if (states)
        for (int s = 0; s < 3; s++)
            for (size_t i = 0; i < pixels * 6; i++) states[(size_t)s * pixels * 6 + i] = st[levels & 1u][s][i];
}

}  // namespace hr
