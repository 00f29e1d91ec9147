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

}  // namespace hr
