// The edge-avoiding à-trous denoiser, per pixel, all f64, host-compilable like noise_core.h.  THIS HEADER IS THE DEFINITION:
// every operation is a single IEEE f64 operation in the order written (+ - x / and comparisons only: no exp, pow or sqrt; no FMA — contraction is
// switched off below, a host compiler that contracts by default wants -ffp-contract=off), so the device, a host build and any restatement of
// these lines agree bit for bit.
//   a pixel's state   cv[6] = {C_r, C_g, C_b, V_r, V_g, V_b}: the radiance estimate and the variance of that estimate
//   a pixel's guides  g[8]  = {A_r, A_g, A_b, N_x, N_y, N_z, Z, H}: first-hit albedo, normal, depth, coverage (fp32; guide_primary, pt_core.h)
//   denoise_init      C0_c = (double)accum_c x (double)scale, scale = the fp32 value 1 / (4 n) of the resolve (rounding C0 to fp32 gives what
//                     tonemap_gamma_kernel computes: the f64 product of two floats is exact);  V0_c = var_c / n / 16, var_c as in
//                     noise_channel_se before its sqrt.  demodulate: C_c / (A_c + eps), V_c / (A_c + eps)^2
//   denoise_level     one level with step s: the 5 x 5 taps q = p + s (i, j), i, j = -2 .. 2, rows first (j outer, i inner, ascending); a tap outside
//                     the image is skipped.  h = k[|i|] k[|j|], k = {3/8, 1/4, 1/16};  K(x) = max(0, 1 - x)^2
//                         x_n = |N_p - N_q|^2 / sigma_n^2              x_a = |A_p - A_q|^2 / sigma_a^2
//                         x_z = (Z_p - Z_q)^2 / (sigma_z^2 (Z_p^2 + Z_q^2) + tiny)        x_h = (H_p - H_q)^2
//                         x_c = |C_p - C_q|^2 / (sigma_c^2 (sumV_p + sumV_q) + tiny),  sumV = (V_r + V_g) + V_b
//                         w   = ((((h K(x_n)) K(x_a)) K(x_z)) K(x_h)) K(x_c)
//                         C'  = sum w C_q / sum w             V'_c = sum w^2 V_c,q / (sum w)^2
//                     The centre tap has every x = 0, so sum w >= 9/64.
//   denoise_final     D_c = (float)C_c, with demodulate (float)(C_c (A_c + eps))
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HR_DENOISE_HD __host__ __device__ __forceinline__
#else
#define HR_DENOISE_HD inline
#endif

namespace hr {

constexpr double DENOISE_EPS = 1e-3;     // demodulation: albedo + eps (a black or missed first hit divides by eps, and is multiplied back by it)
constexpr double DENOISE_TINY = 1e-30;   // keeps 0 / 0 out of x_z (two misses: Z = 0) and x_c (two pixels without variance)
constexpr uint32_t DENOISE_MAX_LEVELS = 5;

// the squares of the four sigmas, each one product
struct DenoiseSigmas { double c2, n2, a2, z2; };
HR_DENOISE_HD DenoiseSigmas denoise_sigmas(double sigma_color, double sigma_normal, double sigma_albedo, double sigma_depth) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    DenoiseSigmas s;
    s.c2 = sigma_color * sigma_color; s.n2 = sigma_normal * sigma_normal; s.a2 = sigma_albedo * sigma_albedo; s.z2 = sigma_depth * sigma_depth;
    return s;
}

// the fp32 scale of a pixel with n samplings: hr_resolve's 1.0f / (float)(n * 4u).  The device's fp32 division is not correctly rounded, so the
// quotient is taken in f64 and rounded once more: the same float for every n whose odd part is below 2^28 (tonemap_gamma_counted_kernel, post_kernels.h)
HR_DENOISE_HD float denoise_scale(uint32_t n) { return (float)(1.0 / (double)(float)(n * 4u)); }

// variance of the pixel's mean radiance in one channel: noise_channel_se's var / n, over 16 (the radiance is the per-sampling value over 4)
HR_DENOISE_HD double denoise_channel_var(double s1, double s2, double n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double m = s1 / n;
    const double p = s1 * m;
    const double d = s2 - p;
    const double v = d / (n - 1.0);
    const double var = v > 0.0 ? v : 0.0;   // (a NaN is clamped too)
    const double q = var / n;
    return q / 16.0;
}

// acc[3]: the pixel's accumulator; mom[6]: its moments; n >= 2: its samplings; g[8]: its guides
HR_DENOISE_HD void denoise_init(const float *acc, const double *mom, uint32_t n, const float *g, int demodulate, double *cv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double scale = (double)denoise_scale(n), nd = (double)n;
    for (int c = 0; c < 3; c++) {
        double C = (double)acc[c] * scale;
        double V = denoise_channel_var(mom[c], mom[3 + c], nd);
        if (demodulate) {
            const double a = (double)g[c] + DENOISE_EPS;
            const double a2 = a * a;
            C = C / a;
            V = V / a2;
        }
        cv[c] = C;
        cv[3 + c] = V;
    }
}

HR_DENOISE_HD double denoise_kernel_weight(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t = 1.0 - x;
    const double u = t > 0.0 ? t : 0.0;   // (a NaN is clamped too)
    return u * u;
}

// h of the tap (i, j), i, j = -2 .. 2: k[|i|] k[|j|], k = {3/8, 1/4, 1/16}
HR_DENOISE_HD double denoise_tap_h(int i, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double K[3] = {0.375, 0.25, 0.0625};
    return K[i < 0 ? -i : i] * K[j < 0 ? -j : j];
}

// The guide terms of a tap, from the guides gp[8] of the pixel and gq[8] of the tap (zp = (double)gp[6] and zp2 = zp zp come from the caller: a level
// takes them once for its 25 taps).  Every x is made of (a - b)^2 and Z_p^2 + Z_q^2: swapping the pixel and the tap gives the same bits.
struct DenoiseGuideX { double n, a, z, h; };
HR_DENOISE_HD DenoiseGuideX denoise_guide_x(const float *gp, const float *gq, double zp, double zp2, const DenoiseSigmas &sg) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    DenoiseGuideX r;
    const double n0 = (double)gp[3] - (double)gq[3], n1 = (double)gp[4] - (double)gq[4], n2 = (double)gp[5] - (double)gq[5];
    r.n = ((n0 * n0 + n1 * n1) + n2 * n2) / sg.n2;
    const double a0 = (double)gp[0] - (double)gq[0], a1 = (double)gp[1] - (double)gq[1], a2 = (double)gp[2] - (double)gq[2];
    r.a = ((a0 * a0 + a1 * a1) + a2 * a2) / sg.a2;
    const double zq = (double)gq[6], dz = zp - zq;
    r.z = (dz * dz) / (sg.z2 * (zp2 + zq * zq) + DENOISE_TINY);
    const double dh = (double)gp[7] - (double)gq[7];
    r.h = dh * dh;
    return r;
}
// the guide part of the tap's weight: (((h K(x_n)) K(x_a)) K(x_z)) K(x_h)
HR_DENOISE_HD double denoise_guide_product(double hw, const DenoiseGuideX &x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (((hw * denoise_kernel_weight(x.n)) * denoise_kernel_weight(x.a)) * denoise_kernel_weight(x.z)) * denoise_kernel_weight(x.h);
}
// both for one pair of pixels (restore_core.h: a spread without the colour term)
HR_DENOISE_HD double denoise_guide_weight(double hw, const float *gp, const float *gq, const DenoiseSigmas &sg) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double zp = (double)gp[6];
    return denoise_guide_product(hw, denoise_guide_x(gp, gq, zp, zp * zp, sg));
}

// One level for the pixel (x, y) of a w x h image: in[h][w][6] -> out[6]; guides[h][w][8].
HR_DENOISE_HD void denoise_level(const double *in, const float *guides, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t step, const DenoiseSigmas &sg, double *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t p = (size_t)y * w + x;
    const double *cp = in + p * 6;
    const float *gp = guides + p * 8;
    const double sv_p = (cp[3] + cp[4]) + cp[5];
    const double zp = (double)gp[6], zp2 = zp * zp;
    double sw = 0.0, sc[3] = {0.0, 0.0, 0.0}, sv[3] = {0.0, 0.0, 0.0};
    for (int j = -2; j <= 2; j++) {
        const int64_t qy = (int64_t)y + (int64_t)step * j;
        if (qy < 0 || qy >= (int64_t)h) continue;
        for (int i = -2; i <= 2; i++) {
            const int64_t qx = (int64_t)x + (int64_t)step * i;
            if (qx < 0 || qx >= (int64_t)w) continue;
            const size_t q = (size_t)qy * w + (size_t)qx;
            const double *cq = in + q * 6;
            const float *gq = guides + q * 8;
            const double hw = denoise_tap_h(i, j);
            const DenoiseGuideX gx = denoise_guide_x(gp, gq, zp, zp2, sg);
            const double c0 = cp[0] - cq[0], c1 = cp[1] - cq[1], c2 = cp[2] - cq[2];
            const double sv_q = (cq[3] + cq[4]) + cq[5];
            const double xc = ((c0 * c0 + c1 * c1) + c2 * c2) / (sg.c2 * (sv_p + sv_q) + DENOISE_TINY);
            const double wt = denoise_guide_product(hw, gx) * denoise_kernel_weight(xc);
            const double w2 = wt * wt;
            sw = sw + wt;
            for (int c = 0; c < 3; c++) {
                sc[c] = sc[c] + wt * cq[c];
                sv[c] = sv[c] + w2 * cq[3 + c];
            }
        }
    }
    const double sw2 = sw * sw;
    for (int c = 0; c < 3; c++) {
        out[c] = sc[c] / sw;
        out[3 + c] = sv[c] / sw2;
    }
}

HR_DENOISE_HD void denoise_final(const double *cv, const float *g, int demodulate, float *d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int c = 0; c < 3; c++) {
        double C = cv[c];
        if (demodulate) {
            const double a = (double)g[c] + DENOISE_EPS;
            C = C * a;
        }
        d[c] = (float)C;
    }
}

// the whole filter over a w x h image on one thread (the host side of the tests; the device runs one thread per pixel and one launch per
// level: atrous_kernel, post_kernels.h).  counts == nullptr: every pixel has n_all samplings.  work: 2 x w*h*6 doubles.
inline void denoise_image(const float *acc, const double *mom, const uint32_t *counts, uint32_t n_all, const float *guides, uint32_t w, uint32_t h, uint32_t levels,
                                 int demodulate, const DenoiseSigmas &sg, double *work, float *d) {
    const size_t pixels = (size_t)w * h;
    double *a = work, *b = work + pixels * 6;
    for (size_t p = 0; p < pixels; p++) denoise_init(acc + p * 3, mom + p * 6, counts ? counts[p] : n_all, guides + p * 8, demodulate, a + p * 6);
    for (uint32_t l = 0; l < levels; l++) {
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) denoise_level(a, guides, w, h, x, y, 1u << l, sg, b + ((size_t)y * w + x) * 6);
        double *t = a; a = b; b = t;
    }
    for (size_t p = 0; p < pixels; p++) denoise_final(a + p * 6, guides + p * 8, demodulate, d + p * 3);
}

}  // namespace hr
