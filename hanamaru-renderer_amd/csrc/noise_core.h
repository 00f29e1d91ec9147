// The noise estimate of a pixel from the moments of its per-sampling values, per lane, all f64, host-compilable like
// post_core.h.  x_s = a sampling's contribution to the pixel (the 2x2 sub-sample sum of calc_pixel, renderer.rs:33-38,48-60), n samplings:
//     S1 = sum x_s, S2 = sum x_s^2                       the moments (accumulate_kernel<true>, trace_kernel.h)
//     m   = S1 / n                                       mean of x
//     var = max(0, (S2 - S1 m) / (n - 1))                unbiased sample variance of x (cancellation may leave a small negative: clamped)
//     se  = sqrt(var / n) / 4                            standard error of the pixel's radiance mu = m / 4
//     e   = (se_r + se_g + se_b) / (mu_r + mu_g + mu_b + 3 floor)
// Every operation is a single IEEE f64 operation in the order written (no FMA: contraction is switched off below; a host compiler that
// contracts by default wants -ffp-contract=off), so two implementations differ by what their sqrt differs, and no more.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HR_NOISE_HD __host__ __device__ __forceinline__
#else
#define HR_NOISE_HD inline
#endif

namespace hr {

// standard error of one channel's radiance
HR_NOISE_HD double noise_channel_se(double s1, double s2, double n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double m = s1 / n;
    const double p = s1 * m;
    const double d = s2 - p;
    const double v = d / (n - 1.0);
    const double var = v > 0.0 ? v : 0.0;   // (a NaN is clamped too)
    const double q = var / n;
    return sqrt(q) / 4.0;
}

// mom = {S1r, S1g, S1b, S2r, S2g, S2b} of a pixel, n >= 2 samplings behind them, floor > 0 (radiance units)
HR_NOISE_HD double noise_pixel_error(const double *mom, uint64_t samplings, double floor) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double n = (double)samplings;
    const double se_r = noise_channel_se(mom[0], mom[3], n), se_g = noise_channel_se(mom[1], mom[4], n), se_b = noise_channel_se(mom[2], mom[5], n);
    const double mu_r = mom[0] / n / 4.0, mu_g = mom[1] / n / 4.0, mu_b = mom[2] / n / 4.0;
    const double num = (se_r + se_g) + se_b;
    const double den = ((mu_r + mu_g) + mu_b) + 3.0 * floor;
    return num / den;
}

}  // namespace hr
