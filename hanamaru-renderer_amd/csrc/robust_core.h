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
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HR_ROBUST_HD __host__ __device__ __forceinline__
#else
#define HR_ROBUST_HD inline
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

}  // namespace hr
