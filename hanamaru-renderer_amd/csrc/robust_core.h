// The firefly-robust resolve: an adaptive median of means over a pixel's K sample buckets, per pixel, all f64, host-compilable
// like denoise_core.h.  THIS HEADER IS THE DEFINITION: every operation is a single IEEE f64 operation in the order written (+ - x /, comparisons and
// one (int) truncation of a non-negative double; no FMA — contraction is switched off below, a host compiler that contracts by default wants
// -ffp-contract=off), so the device, a host build and any restatement of these lines agree bit for bit.
//   a pixel's buckets   B[K][3]: bucket b holds the sum of the per-sampling values x_j of the pixel's samplings j = b, b + K, ..
//                       (j = 0, 1, .. counted per pixel in the order rendered); K odd, 3 .. 15
//   n == 0              R = 0, trim = 0
//   n <  K              R_c = ((B[0][c] + B[1][c]) + .. + B[K-1][c]) / (double)n / 4.0 — the plain mean; trim = 0
//   otherwise           n_b   = (n - b + K - 1) / K (integer: the samplings bucket b holds)
//                       m_b,c = B[b][c] / (double)n_b / 4.0                  y_b = (m_b,r + m_b,g) + m_b,b
//                       the buckets in ascending order of (y_b, b): a stable insertion sort, ties by bucket index
//                       T  = y_(1) + y_(2) + .. + y_(K)                      Gn = (double)(2 - K - 1) y_(1) + .. + (double)(2 K - K - 1) y_(K)
//                       trim = 0 if T <= 0; else G = Gn / ((double)K T) — the Gini coefficient of the bucket means —,
//                       trim = G > 0 ? min((K - 1) / 2, (int)(G (double)K / 2.0)) : 0
//                       R_c = (m_(trim+1),c + .. + m_(K-trim),c) / (double)(K - 2 trim)
//                       Every sum starts with its first term and adds the others one at a time, ascending.
//   output              (float)R_c, and trim as uint8
// Equal buckets: G = 0, trim = 0, the mean of the bucket means.  One bucket holding everything: G = (K - 1) / K, trim = (K - 1) / 2, the median bucket.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "denoise_core.h"

#if defined(__HIPCC__)
#define HR_ROBUST_HD __host__ __device__ __forceinline__
#else
#define HR_ROBUST_HD inline
#endif
#if defined(__clang__)
#define HR_ROBUST_UNROLL _Pragma("unroll")
#else
#define HR_ROBUST_UNROLL
#endif

namespace hr {

constexpr uint32_t ROBUST_MAX_K = 15;

// option "robust_buckets": an odd number of buckets, 3 .. 15
HR_ROBUST_HD bool robust_valid_k(double k) { return k == 3 || k == 5 || k == 7 || k == 9 || k == 11 || k == 13 || k == 15; }

// B[K][3]: the pixel's buckets; n: its samplings; R[3]: the radiance; trim: the buckets dropped at either end
HR_ROBUST_HD void robust_pixel(const double *B, uint32_t K, uint64_t n, float *R, uint8_t *trim) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    *trim = 0;
    if (n == 0) { R[0] = R[1] = R[2] = 0.0f; return; }
    if (n < K) {
        const double nd = (double)n;
        for (int c = 0; c < 3; c++) {
            double s = B[c];
            for (uint32_t b = 1; b < K; b++) s = s + B[b * 3 + c];
            const double q = s / nd;
            R[c] = (float)(q / 4.0);
        }
        return;
    }
    double m[ROBUST_MAX_K][3], y[ROBUST_MAX_K];
    uint32_t ord[ROBUST_MAX_K];
    for (uint32_t b = 0; b < K; b++) {
        const double nb = (double)((n - b + K - 1) / K);
        for (int c = 0; c < 3; c++) {
            const double q = B[b * 3 + c] / nb;
            m[b][c] = q / 4.0;
        }
        y[b] = (m[b][0] + m[b][1]) + m[b][2];
    }
    // stable insertion sort of the bucket indices, ascending by y: an element moves past those that are strictly greater only
    for (uint32_t i = 0; i < K; i++) {
        uint32_t j = i;
        while (j > 0 && y[ord[j - 1]] > y[i]) { ord[j] = ord[j - 1]; j--; }
        ord[j] = i;
    }
    double T = y[ord[0]];
    double Gn = (double)(1 - (int)K) * y[ord[0]];
    for (uint32_t i = 2; i <= K; i++) {
        T = T + y[ord[i - 1]];
        Gn = Gn + (double)(2 * (int)i - (int)K - 1) * y[ord[i - 1]];
    }
    uint32_t t = 0;
    if (T > 0.0) {
        const double G = Gn / ((double)K * T);
        if (G > 0.0) {
            const int want = (int)(G * (double)K / 2.0);
            const int most = (int)((K - 1) / 2);
            t = (uint32_t)(want < most ? want : most);
        }
    }
    const double kept = (double)(K - 2 * t);
    for (int c = 0; c < 3; c++) {
        double s = m[ord[t]][c];
        for (uint32_t i = t + 1; i < K - t; i++) s = s + m[ord[i]][c];
        R[c] = (float)(s / kept);
    }
    *trim = (uint8_t)t;
}

// the whole image on one thread (the host side of the tests and of tools/robust_quality.py; the device runs one thread per pixel: robust_kernel,
// post_kernels.h).  counts == nullptr: every pixel has n_all samplings.
inline void robust_image(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, size_t pixels, float *R, uint8_t *trim) {
    for (size_t p = 0; p < pixels; p++) robust_pixel(buckets + p * K * 3, K, counts ? (uint64_t)counts[p] : n_all, R + p * 3, trim + p);
}

// The robust noise estimate: the relative standard error of the robust radiance's channel sum, from the spread of the pixel's
// own bucket means — the Tukey–McLaughlin (winsorized) standard error of the t-trimmed mean, t the trim robust_pixel takes.  The conventions
// above hold (f64, one IEEE operation per step in the order written, no contraction, ascending sums that start from their first term); one
// correctly rounded sqrt is added to the allowed operations.  n >= K (the caller guarantees it), floor > 0 (radiance units):
//   n_b, m_b,c, y_b, the order (y_b, b), T, Gn, G, trim t     exactly as robust_pixel: the same lines, the same bits
//   kept = (double)(K - 2 t)
//   Ry   = (y_(t+1) + .. + y_(K-t)) / kept                    the t-trimmed mean of the channel sums
//   lo = y_(t+1), hi = y_(K-t);  w_i = lo for i <= t, hi for i > K - t, y_(i) otherwise   (i = 1 .. K)   the winsorized sample
//   wbar = (w_1 + .. + w_K) / (double)K
//   ss   = sum_i (w_i - wbar) (w_i - wbar)
//   se   = sqrt(ss / (double)(K - 1) / (double)K) (double)K / kept
//   den  = Ry + 3.0 floor
//   e    = den > 0 ? se / den : 0
// It is an error of the channel SUM y, not §4.7's se_r + se_g + se_b of the three channels taken apart.  With t = (K - 1) / 2 — the median
// bucket — every w_i is the median and se is 0 by construction: no special case, such a pixel reports e = 0.
// Only the sorted keys y_(i) enter, never the per-channel means, and buckets with equal keys are interchangeable in every line above: the order
// of the keys is that of ANY correct ascending sort.  K is a template parameter and every index below a constant, so on the device the K keys
// live in registers (robust_noise_kernel<K>, post_kernels.h): the sort is the definition's stable insertion sort written out as adjacent
// compare-exchanges that swap on strictly greater only, and what depends on the run-time t is a select, not an indexed load.
template <uint32_t K>
HR_ROBUST_HD void robust_pixel_error_k(const double *B, uint64_t n, double floor, double *e, uint8_t *trim) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    static_assert(K >= 3 && K <= ROBUST_MAX_K && (K & 1u), "an odd number of buckets, 3 .. 15");
    const uint64_t nq = n / K, nr = n % K;                    // (n - b + K - 1) / K == n / K + (b < n % K)
    double y[K];
    HR_ROBUST_UNROLL
    for (uint32_t b = 0; b < K; b++) {
        const double nb = (double)(nq + (b < nr ? 1u : 0u));
        const double q0 = B[b * 3] / nb, q1 = B[b * 3 + 1] / nb, q2 = B[b * 3 + 2] / nb;
        const double m0 = q0 / 4.0, m1 = q1 / 4.0, m2 = q2 / 4.0;
        y[b] = (m0 + m1) + m2;
    }
    HR_ROBUST_UNROLL
    for (uint32_t i = 1; i < K; i++) {
    HR_ROBUST_UNROLL
        for (uint32_t j = i; j > 0; j--) {
            const double a = y[j - 1], b = y[j];
            const bool swap = a > b;
            y[j - 1] = swap ? b : a;
            y[j] = swap ? a : b;
        }
    }
    double T = y[0];
    double Gn = (double)(1 - (int)K) * y[0];
    HR_ROBUST_UNROLL
    for (uint32_t i = 2; i <= K; i++) {
        T = T + y[i - 1];
        Gn = Gn + (double)(2 * (int)i - (int)K - 1) * y[i - 1];
    }
    uint32_t t = 0;
    if (T > 0.0) {
        const double G = Gn / ((double)K * T);
        if (G > 0.0) {
            const int want = (int)(G * (double)K / 2.0);
            const int most = (int)((K - 1) / 2);
            t = (uint32_t)(want < most ? want : most);
        }
    }
    const double kept = (double)(K - 2 * t);
    // lo, hi and the kept sum: element i (0-based) is kept iff t <= i < K - t
    double lo = y[0], hi = y[K - 1], s = y[0];
    HR_ROBUST_UNROLL
    for (uint32_t i = 1; i < K; i++) {
        lo = i == t ? y[i] : lo;
        hi = i == K - 1 - t ? y[i] : hi;
        s = i == t ? y[i] : (i > t && i < K - t ? s + y[i] : s);
    }
    const double Ry = s / kept;
    double w[K];
    HR_ROBUST_UNROLL
    for (uint32_t i = 0; i < K; i++) w[i] = i < t ? lo : (i >= K - t ? hi : y[i]);
    double ws = w[0];
    HR_ROBUST_UNROLL
    for (uint32_t i = 1; i < K; i++) ws = ws + w[i];
    const double wbar = ws / (double)K;
    double ss = (w[0] - wbar) * (w[0] - wbar);
    HR_ROBUST_UNROLL
    for (uint32_t i = 1; i < K; i++) {
        const double d = w[i] - wbar;
        ss = ss + d * d;
    }
    const double v = ss / (double)(K - 1);
    const double q = v / (double)K;
    const double r = sqrt(q) * (double)K;
    const double se = r / kept;
    const double den = Ry + 3.0 * floor;
    *e = den > 0.0 ? se / den : 0.0;
    *trim = (uint8_t)t;
}

// the same for a run-time K (robust_valid_k(K); anything else: e = 0, trim = 0)
HR_ROBUST_HD void robust_pixel_error(const double *B, uint32_t K, uint64_t n, double floor, double *e, uint8_t *trim) {
    switch (K) {
    case 3: robust_pixel_error_k<3>(B, n, floor, e, trim); break;
    case 5: robust_pixel_error_k<5>(B, n, floor, e, trim); break;
    case 7: robust_pixel_error_k<7>(B, n, floor, e, trim); break;
    case 9: robust_pixel_error_k<9>(B, n, floor, e, trim); break;
    case 11: robust_pixel_error_k<11>(B, n, floor, e, trim); break;
    case 13: robust_pixel_error_k<13>(B, n, floor, e, trim); break;
    case 15: robust_pixel_error_k<15>(B, n, floor, e, trim); break;
    default: *e = 0.0; *trim = 0; break;
    }
}

// the whole image on one thread, like robust_image (every pixel n >= K: the caller guarantees it)
inline void robust_error_image(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, double floor, size_t pixels, double *e, uint8_t *trim) {
    for (size_t p = 0; p < pixels; p++) robust_pixel_error(buckets + p * K * 3, K, counts ? (uint64_t)counts[p] : n_all, floor, e + p, trim + p);
}

// The robust radiance WITH its variance: what the à-trous denoiser (denoise_core.h) reads in place of the accumulator and the raw
// moments, both of which are dominated by exactly the few paths R drops.  The conventions above hold (f64, one IEEE operation per step in the order
// written, no contraction, ascending sums that start from their first term, every index a compile-time constant) and there is NO sqrt: the device,
// this header under a host compiler and a numpy restatement agree bit for bit.  B[K][3], n >= K (the caller guarantees it):
//   n_b, m_b,c, y_b, the order (y_b, b), T, Gn, G, trim t     exactly as robust_pixel: the same lines, the same bits
//   kept = (double)(K - 2 t)
//   C_c  = (m_(t+1),c + .. + m_(K-t),c) / kept               (float)C_c is robust_pixel's R_c, bit for bit
//   w_i,c = m_(t+1),c for i <= t;  m_(K-t),c for i > K - t;  m_(i),c otherwise   (i = 1 .. K)   winsorized by the RANK in y, per channel
//   wbar_c = (w_1,c + .. + w_K,c) / (double)K
//   ss_c   = sum_i (w_i,c - wbar_c) (w_i,c - wbar_c)
//   f = (double)K / kept;  v = ss_c / (double)(K - 1);  q = v / (double)K;  r = q f;  V_c = r f
//   output cv[6] = {C_r, C_g, C_b, V_r, V_g, V_b} and trim
// V_c is the Tukey–McLaughlin variance of the t-trimmed mean (the square of §4.11's se), per channel, on the order the keys y give; with
// t = (K - 1) / 2 every w_i,c is the median bucket's and V_c is 0 by construction.  Unlike robust_pixel_error_k the per-channel means enter, so the
// order of buckets with EQUAL keys matters: it is the stable order (y_b, b), as robust_pixel's.  The sort is robust_pixel_error_k's network —
// adjacent compare-exchanges that swap on strictly greater only, hence stable — carrying (y, m_r, m_g, m_b) together through every exchange; what
// depends on the run-time t is a select, no array is indexed at run time.

// the pixel's bucket means in ascending order of (y_b, b) — m0, m1, m2: the channels — and the trim; n >= K
template <uint32_t K>
HR_ROBUST_HD uint32_t robust_sorted_means_k(const double *B, uint64_t n, double (&m0)[K], double (&m1)[K], double (&m2)[K]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    static_assert(K >= 3 && K <= ROBUST_MAX_K && (K & 1u), "an odd number of buckets, 3 .. 15");
    const uint64_t nq = n / K, nr = n % K;                    // (n - b + K - 1) / K == n / K + (b < n % K)
    double y[K];
    HR_ROBUST_UNROLL
    for (uint32_t b = 0; b < K; b++) {
        const double nb = (double)(nq + (b < nr ? 1u : 0u));
        const double q0 = B[b * 3] / nb, q1 = B[b * 3 + 1] / nb, q2 = B[b * 3 + 2] / nb;
        m0[b] = q0 / 4.0; m1[b] = q1 / 4.0; m2[b] = q2 / 4.0;
        y[b] = (m0[b] + m1[b]) + m2[b];
    }
    HR_ROBUST_UNROLL
    for (uint32_t i = 1; i < K; i++) {
    HR_ROBUST_UNROLL
        for (uint32_t j = i; j > 0; j--) {
            const bool swap = y[j - 1] > y[j];
            const double ya = y[j - 1], yb = y[j], a0 = m0[j - 1], b0 = m0[j], a1 = m1[j - 1], b1 = m1[j], a2 = m2[j - 1], b2 = m2[j];
            y[j - 1] = swap ? yb : ya;  y[j] = swap ? ya : yb;
            m0[j - 1] = swap ? b0 : a0; m0[j] = swap ? a0 : b0;
            m1[j - 1] = swap ? b1 : a1; m1[j] = swap ? a1 : b1;
            m2[j - 1] = swap ? b2 : a2; m2[j] = swap ? a2 : b2;
        }
    }
    double T = y[0];
    double Gn = (double)(1 - (int)K) * y[0];
    HR_ROBUST_UNROLL
    for (uint32_t i = 2; i <= K; i++) {
        T = T + y[i - 1];
        Gn = Gn + (double)(2 * (int)i - (int)K - 1) * y[i - 1];
    }
    uint32_t t = 0;
    if (T > 0.0) {
        const double G = Gn / ((double)K * T);
        if (G > 0.0) {
            const int want = (int)(G * (double)K / 2.0);
            const int most = (int)((K - 1) / 2);
            t = (uint32_t)(want < most ? want : most);
        }
    }
    return t;
}

// one channel's sorted means m and the trim t: the t-trimmed mean C, and with WITH_V its variance V
template <uint32_t K, bool WITH_V>
HR_ROBUST_HD void robust_channel_cv_k(const double (&m)[K], uint32_t t, double *C, double *V) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double kept = (double)(K - 2 * t);
    // lo, hi and the kept sum: element i (0-based) is kept iff t <= i < K - t
    double lo = m[0], hi = m[K - 1], s = m[0];
    HR_ROBUST_UNROLL
    for (uint32_t i = 1; i < K; i++) {
        lo = i == t ? m[i] : lo;
        hi = i == K - 1 - t ? m[i] : hi;
        s = i == t ? m[i] : (i > t && i < K - t ? s + m[i] : s);
    }
    *C = s / kept;
    if (!WITH_V) return;
    double w[K];
    HR_ROBUST_UNROLL
    for (uint32_t i = 0; i < K; i++) w[i] = i < t ? lo : (i >= K - t ? hi : m[i]);
    double ws = w[0];
    HR_ROBUST_UNROLL
    for (uint32_t i = 1; i < K; i++) ws = ws + w[i];
    const double wbar = ws / (double)K;
    double ss = (w[0] - wbar) * (w[0] - wbar);
    HR_ROBUST_UNROLL
    for (uint32_t i = 1; i < K; i++) {
        const double d = w[i] - wbar;
        ss = ss + d * d;
    }
    const double f = (double)K / kept;
    const double v = ss / (double)(K - 1);
    const double q = v / (double)K;
    const double r = q * f;
    *V = r * f;
}

// B[K][3]: the pixel's buckets; n >= K: its samplings; cv[6] = {C, V}; trim: the buckets dropped at either end
template <uint32_t K>
HR_ROBUST_HD void robust_pixel_cv_k(const double *B, uint64_t n, double *cv, uint8_t *trim) {
    double m0[K], m1[K], m2[K];
    const uint32_t t = robust_sorted_means_k<K>(B, n, m0, m1, m2);
    robust_channel_cv_k<K, true>(m0, t, cv + 0, cv + 3);
    robust_channel_cv_k<K, true>(m1, t, cv + 1, cv + 4);
    robust_channel_cv_k<K, true>(m2, t, cv + 2, cv + 5);
    *trim = (uint8_t)t;
}

// robust_pixel with K a template parameter (robust_kernel<K>, post_kernels.h): the same operations in the same order — n == 0, n < K and
// R_c = (float)C_c — so R and trim are robust_pixel's bit for bit, without its run-time indexed arrays
template <uint32_t K>
HR_ROBUST_HD void robust_pixel_k(const double *B, uint64_t n, float *R, uint8_t *trim) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    *trim = 0;
    if (n == 0) { R[0] = R[1] = R[2] = 0.0f; return; }
    if (n < K) {
        const double nd = (double)n;
        HR_ROBUST_UNROLL
        for (int c = 0; c < 3; c++) {
            double s = B[c];
            HR_ROBUST_UNROLL
            for (uint32_t b = 1; b < K; b++) s = s + B[b * 3 + c];
            const double q = s / nd;
            R[c] = (float)(q / 4.0);
        }
        return;
    }
    double m0[K], m1[K], m2[K], C0, C1, C2;
    const uint32_t t = robust_sorted_means_k<K>(B, n, m0, m1, m2);
    robust_channel_cv_k<K, false>(m0, t, &C0, nullptr);
    robust_channel_cv_k<K, false>(m1, t, &C1, nullptr);
    robust_channel_cv_k<K, false>(m2, t, &C2, nullptr);
    R[0] = (float)C0; R[1] = (float)C1; R[2] = (float)C2;
    *trim = (uint8_t)t;
}

// the denoiser's initial state of a pixel from its buckets: {C, V} above, demodulated exactly as denoise_init does — C / (A + eps),
// V / (A + eps)^2 with the pixel's guide albedo A = g[0 .. 2] (g[8]: its guides)
template <uint32_t K>
HR_ROBUST_HD void robust_denoise_init_k(const double *B, uint64_t n, const float *g, int demodulate, double *cv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    uint8_t t;
    robust_pixel_cv_k<K>(B, n, cv, &t);
    if (demodulate) {
        HR_ROBUST_UNROLL
        for (int c = 0; c < 3; c++) {
            const double a = (double)g[c] + DENOISE_EPS;
            const double a2 = a * a;
            cv[c] = cv[c] / a;
            cv[3 + c] = cv[3 + c] / a2;
        }
    }
}

// the same for a run-time K (robust_valid_k(K); anything else: cv = 0)
HR_ROBUST_HD void robust_denoise_init(const double *B, uint32_t K, uint64_t n, const float *g, int demodulate, double *cv) {
    switch (K) {
    case 3: robust_denoise_init_k<3>(B, n, g, demodulate, cv); break;
    case 5: robust_denoise_init_k<5>(B, n, g, demodulate, cv); break;
    case 7: robust_denoise_init_k<7>(B, n, g, demodulate, cv); break;
    case 9: robust_denoise_init_k<9>(B, n, g, demodulate, cv); break;
    case 11: robust_denoise_init_k<11>(B, n, g, demodulate, cv); break;
    case 13: robust_denoise_init_k<13>(B, n, g, demodulate, cv); break;
    case 15: robust_denoise_init_k<15>(B, n, g, demodulate, cv); break;
    default: for (int c = 0; c < 6; c++) cv[c] = 0.0; break;
    }
}
// {C, V} and the trim without the demodulation, for a run-time K (what the host tests compare with robust_pixel and robust_pixel_error)
HR_ROBUST_HD void robust_pixel_cv(const double *B, uint32_t K, uint64_t n, double *cv, uint8_t *trim) {
    switch (K) {
    case 3: robust_pixel_cv_k<3>(B, n, cv, trim); break;
    case 5: robust_pixel_cv_k<5>(B, n, cv, trim); break;
    case 7: robust_pixel_cv_k<7>(B, n, cv, trim); break;
    case 9: robust_pixel_cv_k<9>(B, n, cv, trim); break;
    case 11: robust_pixel_cv_k<11>(B, n, cv, trim); break;
    case 13: robust_pixel_cv_k<13>(B, n, cv, trim); break;
    case 15: robust_pixel_cv_k<15>(B, n, cv, trim); break;
    default: for (int c = 0; c < 6; c++) cv[c] = 0.0; *trim = 0; break;
    }
}

// the whole robust filter over a w x h image on one thread (the host side of the tests and of tools/robust_denoise_quality.py): this init, then
// denoise_level and denoise_final unchanged.  counts == nullptr: every pixel has n_all samplings; every pixel n >= K.  work: 2 x w*h*6 doubles.
inline void robust_denoise_image(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, const float *guides, uint32_t w, uint32_t h, uint32_t levels,
                                 int demodulate, const DenoiseSigmas &sg, double *work, float *d) {
    const size_t pixels = (size_t)w * h;
    double *a = work, *b = work + pixels * 6;
    for (size_t p = 0; p < pixels; p++) robust_denoise_init(buckets + p * K * 3, K, counts ? (uint64_t)counts[p] : n_all, guides + p * 8, demodulate, a + p * 6);
    for (uint32_t l = 0; l < levels; l++) {
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) denoise_level(a, guides, w, h, x, y, 1u << l, sg, b + ((size_t)y * w + x) * 6);
        double *t = a; a = b; b = t;
    }
    for (size_t p = 0; p < pixels; p++) denoise_final(a + p * 6, guides + p * 8, demodulate, d + p * 3);
}

}  // namespace hr
