// The denoiser that picks its level per pixel from held-out sample halves, all f64, host-compilable like denoise_core.h.
// THIS HEADER IS THE DEFINITION: every operation is a single IEEE f64 operation in the order written (+ - x /, comparisons and integer arithmetic
// only; no FMA — contraction is switched off below, a host compiler that contracts by default wants -ffp-contract=off), so the device, a host
// build and any restatement of these lines agree bit for bit.
//   inputs of a pixel   its K bucket sums B[K][3] (robust_core.h), its samplings n >= 2, its moments mom[6], its accumulator acc[3], its guides g[8]
//   halves              n_b = (n - b + K - 1) / K (integer: the samplings bucket b holds); half A: the buckets with even b, half B: the odd ones;
//                       n_A, n_B: the sums of their n_b (n >= 2: both at least 1)
//                       A0_c = ((B[0][c] + B[2][c]) + ..) / (double)n_A / 4.0      B0_c = ((B[1][c] + B[3][c]) + ..) / (double)n_B / 4.0
//                       (every sum starts with its first term and adds the others one at a time, ascending)
//   three states        W = denoise_init(acc, mom, n, g, demodulate), exactly
//                       A = {A0, V_W (double)n / (double)n_A}, V_W,c = denoise_channel_var(mom[c], mom[3 + c], (double)n): a product, then a quotient
//                       B = {B0, V_W (double)n / (double)n_B}
//                       demodulate: A and B divided as denoise_init divides — C / (A_c + eps), V / (A_c + eps)^2 — and A0, B0 ARE those divided values
//   levels              F_X,l: state X after l applications of denoise_level (steps 1, 2, 4, ..), l = 0 .. levels.  select_level3 advances the
//                       three states of a pixel by one level: a tap's guide terms (denoise_guide_x, denoise_guide_product) are computed once and
//                       serve the three colour weights; per state the operations are denoise_level's, in its order — the same bits
//   error               dA_c = F_A,l,c - B0_c    dB_c = F_B,l,c - A0_c     (each filtered half against the raw pixel of the other half)
//                       e_l = ((dA_r^2 + dB_r^2) + (dA_g^2 + dB_g^2)) + (dA_b^2 + dB_b^2)
//   smoothing           pass t = 0 .. smooth - 1 (smooth <= 3) with step 2^t: e'(p) = sum h e(q) / sum h over the 5 x 5 taps q = p + 2^t (i, j),
//                       rows first (j outer, i inner, ascending), h = denoise_tap_h(i, j); both sums start at 0.0; a tap outside the image is skipped
//   pick                l = 0: best = e_0, L = 0, S = denoise_final(F_W,0).  l = 1 .. levels: if e_l < best (strict: ties and NaN keep the lower
//                       level): best = e_l, L = l, S = denoise_final(F_W,l).  L is a uint8.
// Where L(p) = l, S(p) has the bits of denoise_image(levels = l) at p; with levels = 0, S is (float)C0 — the mean rounded once.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "denoise_core.h"
#include "robust_core.h"

namespace hr {

constexpr uint32_t SELECT_MAX_SMOOTH = 3;

// the halves' raw means A0[3], B0[3] of a pixel from its buckets; nA, nB: the samplings behind them.  K is a template parameter: every index is a constant
template <uint32_t K>
HR_ROBUST_HD void select_halves_k(const double *B, uint32_t n, double *A0, double *B0, uint32_t *nA, uint32_t *nB) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    static_assert(K >= 3 && K <= ROBUST_MAX_K && (K & 1u), "an odd number of buckets, 3 .. 15");
    const uint32_t nq = n / K, nr = n % K;                    // (n - b + K - 1) / K == n / K + (b < n % K)
    uint32_t na = 0, nb = 0;
    HR_ROBUST_UNROLL
    for (uint32_t b = 0; b < K; b++) {
        const uint32_t k = nq + (b < nr ? 1u : 0u);
        if (b & 1u) nb += k; else na += k;
    }
    const double nad = (double)na, nbd = (double)nb;
    HR_ROBUST_UNROLL
    for (int c = 0; c < 3; c++) {
        double sa = B[c], sb = B[3 + c];
        HR_ROBUST_UNROLL
        for (uint32_t b = 2; b < K; b++) {
            if (b & 1u) sb = sb + B[b * 3 + c]; else sa = sa + B[b * 3 + c];
        }
        const double qa = sa / nad, qb = sb / nbd;
        A0[c] = qa / 4.0;
        B0[c] = qb / 4.0;
    }
    *nA = na; *nB = nb;
}

// the three initial states of a pixel: sa[6], sb[6], sw[6] = {C, V} of the halves A, B and of the whole W
template <uint32_t K>
HR_ROBUST_HD void select_init_k(const double *B, uint32_t n, const float *acc, const double *mom, const float *g, int demodulate, double *sa, double *sb, double *sw) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    uint32_t nA, nB;
    select_halves_k<K>(B, n, sa, sb, &nA, &nB);
    denoise_init(acc, mom, n, g, demodulate, sw);
    const double nd = (double)n, nad = (double)nA, nbd = (double)nB;
    HR_ROBUST_UNROLL
    for (int c = 0; c < 3; c++) {
        const double V = denoise_channel_var(mom[c], mom[3 + c], nd);
        const double vn = V * nd;
        double va = vn / nad, vb = vn / nbd;
        if (demodulate) {
            const double a = (double)g[c] + DENOISE_EPS;
            const double a2 = a * a;
            sa[c] = sa[c] / a;
            sb[c] = sb[c] / a;
            va = va / a2;
            vb = vb / a2;
        }
        sa[3 + c] = va;
        sb[3 + c] = vb;
    }
}
// the same for a run-time K (robust_valid_k(K); anything else: all zero)
HR_ROBUST_HD void select_init(const double *B, uint32_t K, uint32_t n, const float *acc, const double *mom, const float *g, int demodulate, double *sa, double *sb, double *sw) {
    switch (K) {
    case 3: select_init_k<3>(B, n, acc, mom, g, demodulate, sa, sb, sw); break;
    case 5: select_init_k<5>(B, n, acc, mom, g, demodulate, sa, sb, sw); break;
    case 7: select_init_k<7>(B, n, acc, mom, g, demodulate, sa, sb, sw); break;
    case 9: select_init_k<9>(B, n, acc, mom, g, demodulate, sa, sb, sw); break;
    case 11: select_init_k<11>(B, n, acc, mom, g, demodulate, sa, sb, sw); break;
    case 13: select_init_k<13>(B, n, acc, mom, g, demodulate, sa, sb, sw); break;
    case 15: select_init_k<15>(B, n, acc, mom, g, demodulate, sa, sb, sw); break;
    default: for (int c = 0; c < 6; c++) sa[c] = sb[c] = sw[c] = 0.0; break;
    }
}

// one state's share of a tap and of a level's end: denoise_level's lines, with the guide part gw of the tap's weight handed in
struct SelectSums { double sw, sc[3], sv[3]; };
HR_DENOISE_HD void select_sums_zero(SelectSums &s) { s.sw = 0.0; s.sc[0] = s.sc[1] = s.sc[2] = 0.0; s.sv[0] = s.sv[1] = s.sv[2] = 0.0; }
HR_DENOISE_HD void select_tap(const double *cp, double sv_p, const double *cq, double gw, const DenoiseSigmas &sg, SelectSums &s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double c0 = cp[0] - cq[0], c1 = cp[1] - cq[1], c2 = cp[2] - cq[2];
    const double sv_q = (cq[3] + cq[4]) + cq[5];
    const double xc = ((c0 * c0 + c1 * c1) + c2 * c2) / (sg.c2 * (sv_p + sv_q) + DENOISE_TINY);
    const double wt = gw * denoise_kernel_weight(xc);
    const double w2 = wt * wt;
    s.sw = s.sw + wt;
    for (int c = 0; c < 3; c++) {
        s.sc[c] = s.sc[c] + wt * cq[c];
        s.sv[c] = s.sv[c] + w2 * cq[3 + c];
    }
}
HR_DENOISE_HD void select_sums_out(const SelectSums &s, double *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double sw2 = s.sw * s.sw;
    for (int c = 0; c < 3; c++) {
        out[c] = s.sc[c] / s.sw;
        out[3 + c] = s.sv[c] / sw2;
    }
}

// How the three states of an image lie in memory is the caller's: a level reads them through at(s, q, c) — component c (0 .. 5: C_r .. V_b) of
// state s (0: A, 1: B, 2: W) of pixel q.  SelectStatesAoS: three planes of 6 doubles per pixel, as denoise_level reads its one (the host side; the
// device keeps a plane per component, post_kernels.h).
struct SelectStatesAoS {
    const double *p[3];
    HR_DENOISE_HD double operator()(int s, size_t q, int c) const { return p[s][q * 6 + c]; }
};
// One level for the pixel (x, y) of a w x h image, the three states at once: at -> out[3][6]; guides[h][w][8].  The 25 taps are unrolled (under
// clang; the order of the operations is the loop's): on the device the loads of many taps are then in flight under the arithmetic of the others,
// which is what bounds the level (7.5 -> 5.1 ms at 1920x1080).
template <class At>
HR_DENOISE_HD void select_level3(const At &at, const float *guides, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t step, const DenoiseSigmas &sg, double (&out)[3][6]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t p = (size_t)y * w + x;
    double cp[3][6], sv_p[3];
    SelectSums sum[3];
    HR_ROBUST_UNROLL
    for (int s = 0; s < 3; s++) {
        HR_ROBUST_UNROLL
        for (int c = 0; c < 6; c++) cp[s][c] = at(s, p, c);
        sv_p[s] = (cp[s][3] + cp[s][4]) + cp[s][5];
        select_sums_zero(sum[s]);
    }
    const float *gp = guides + p * 8;
    const double zp = (double)gp[6], zp2 = zp * zp;
    HR_ROBUST_UNROLL
    for (int j = -2; j <= 2; j++) {
        const int64_t qy = (int64_t)y + (int64_t)step * j;
        if (qy < 0 || qy >= (int64_t)h) continue;
        HR_ROBUST_UNROLL
        for (int i = -2; i <= 2; i++) {
            const int64_t qx = (int64_t)x + (int64_t)step * i;
            if (qx < 0 || qx >= (int64_t)w) continue;
            const size_t q = (size_t)qy * w + (size_t)qx;
            const double gw = denoise_guide_product(denoise_tap_h(i, j), denoise_guide_x(gp, guides + q * 8, zp, zp2, sg));
            HR_ROBUST_UNROLL
            for (int s = 0; s < 3; s++) {
                double cq[6];
                HR_ROBUST_UNROLL
                for (int c = 0; c < 6; c++) cq[c] = at(s, q, c);
                select_tap(cp[s], sv_p[s], cq, gw, sg, sum[s]);
            }
        }
    }
    HR_ROBUST_UNROLL
    for (int s = 0; s < 3; s++) select_sums_out(sum[s], out[s]);
}

// e_l of a pixel: fa[6], fb[6] its filtered halves; a0[3], b0[3] the halves' level-0 radiance
HR_DENOISE_HD double select_error(const double *fa, const double *fb, const double *a0, const double *b0) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a_r = fa[0] - b0[0], a_g = fa[1] - b0[1], a_b = fa[2] - b0[2];
    const double b_r = fb[0] - a0[0], b_g = fb[1] - a0[1], b_b = fb[2] - a0[2];
    return ((a_r * a_r + b_r * b_r) + (a_g * a_g + b_g * b_g)) + (a_b * a_b + b_b * b_b);
}

// one smoothing pass for the pixel (x, y): e[h][w]
HR_DENOISE_HD double select_smooth(const double *e, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t step) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double se = 0.0, sh = 0.0;
    for (int j = -2; j <= 2; j++) {
        const int64_t qy = (int64_t)y + (int64_t)step * j;
        if (qy < 0 || qy >= (int64_t)h) continue;
        for (int i = -2; i <= 2; i++) {
            const int64_t qx = (int64_t)x + (int64_t)step * i;
            if (qx < 0 || qx >= (int64_t)w) continue;
            const double hw = denoise_tap_h(i, j);
            se = se + hw * e[(size_t)qy * w + (size_t)qx];
            sh = sh + hw;
        }
    }
    return se / sh;
}

// the pick at level l with the (smoothed) error e: best, L, S[3] are the pixel's; fw[6]: F_W,l
HR_DENOISE_HD void select_pick(double e, uint32_t l, const double *fw, const float *g, int demodulate, double *best, uint8_t *L, float *S) {
    if (l == 0u || e < *best) {
        *best = e;
        *L = (uint8_t)l;
        denoise_final(fw, g, demodulate, S);
    }
}

// The whole thing over a w x h image on one thread (the host side of the tests and of tools/select_quality.py; the device: select_init_kernel,
// atrous3_kernel, select_pick_kernel, select_smooth_kernel, post_kernels.h).  counts == nullptr: every pixel has n_all samplings; every n >= 2.
// demodulate: as the caller means it (it is dropped here with levels == 0, as hr_denoise does).  work: w*h*45 doubles.  states (or nullptr):
// w*h*18 doubles, the last level's {C, V} of A, B and W, plane after plane.
inline void select_image(const double *buckets, uint32_t K, const uint32_t *counts, uint32_t n_all, const float *acc, const double *mom, const float *guides, uint32_t w, uint32_t h,
                         uint32_t levels, int demodulate, const DenoiseSigmas &sg, uint32_t smooth, double *work, float *S, uint8_t *L, double *states) {
    const size_t pixels = (size_t)w * h;
    const int dem = demodulate && levels ? 1 : 0;
    double *st[2][3];
    for (int k = 0; k < 2; k++)
        for (int s = 0; s < 3; s++) st[k][s] = work + (size_t)(k * 3 + s) * pixels * 6;
    double *raw = work + pixels * 36, *e[2] = {work + pixels * 42, work + pixels * 43}, *best = work + pixels * 44;
    for (size_t p = 0; p < pixels; p++) {
        select_init(buckets + p * K * 3, K, counts ? counts[p] : n_all, acc + p * 3, mom + p * 6, guides + p * 8, dem, st[0][0] + p * 6, st[0][1] + p * 6, st[0][2] + p * 6);
        for (int c = 0; c < 3; c++) { raw[p * 6 + c] = st[0][0][p * 6 + c]; raw[p * 6 + 3 + c] = st[0][1][p * 6 + c]; }
    }
    for (uint32_t l = 0; l <= levels; l++) {
        double **cur = st[l & 1u], **nxt = st[(l + 1u) & 1u];
        for (size_t p = 0; p < pixels; p++) e[0][p] = select_error(cur[0] + p * 6, cur[1] + p * 6, raw + p * 6, raw + p * 6 + 3);
        for (uint32_t t = 0; t < smooth; t++) {
            for (uint32_t y = 0; y < h; y++)
                for (uint32_t x = 0; x < w; x++) e[1][(size_t)y * w + x] = select_smooth(e[0], w, h, x, y, 1u << t);
            double *sw = e[0]; e[0] = e[1]; e[1] = sw;
        }
        for (size_t p = 0; p < pixels; p++) select_pick(e[0][p], l, cur[2] + p * 6, guides + p * 8, dem, best + p, L + p, S + p * 3);
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
