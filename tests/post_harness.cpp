// The post-processing core headers behind a C interface for the CPU tier: one translation unit, every entry once.  tests/post_cores.py compiles it
// with g++ (-O2 -ffp-contract=off) and holds the argument types; the device kernels and tests/post_numpy.py are held against what it computes.
#include <vector>
#include "noise_core.h"
#include "adapt_core.h"
#include "denoise_core.h"
#include "robust_core.h"
#include "restore_core.h"
#include "select_core.h"
using namespace hr;

// ---- noise_core.h ----
extern "C" void noise_batch(const double *mom, const unsigned long long *n, const double *floor, int count, double *out) {
    for (int i = 0; i < count; i++) out[i] = hr::noise_pixel_error(mom + 6 * i, n[i], floor[i]);
}

// ---- adapt_core.h ----
static RenderParams params(const uint32_t *g, const uint32_t *list, uint32_t count) {
    RenderParams rp{};
    rp.width = g[0]; rp.height = g[1]; rp.org_x = g[2]; rp.org_y = g[3]; rp.reg_w = g[4]; rp.reg_h = g[5];
    rp.tiles_x = (g[4] + 3) / 4; rp.tiles_y = (g[5] + 3) / 4;
    rp.tile_list = list; rp.tile_count = count;
    return rp;
}
// frame pixel and sub-sample of lane j of every dense tile of a launch, with and without a list: out[dense][64][3]
extern "C" uint32_t lane_pixels(const uint32_t *g, const uint32_t *list, uint32_t count, uint32_t *out) {
    const RenderParams rp = params(g, list, count);
    const uint32_t n = list ? launch_tiles<true>(rp) : launch_tiles<false>(rp);
    for (uint32_t d = 0; d < n; d++)
        for (uint32_t j = 0; j < 64; j++) {
            uint32_t *o = out + ((size_t)d * 64 + j) * 3;
            tile_lane_frame_pixel(rp, list ? launch_tile<true>(rp, d) : launch_tile<false>(rp, d), j, o[0], o[1], o[2]);
        }
    return n;
}
extern "C" void tile_rule(const uint32_t *g, const double *moments, const uint32_t *counts, double floor, double threshold, unsigned char *out) {
    const RenderParams rp = params(g, nullptr, 0);
    for (uint32_t t = 0; t < rp.tiles_x * rp.tiles_y; t++) out[t] = adapt_tile_active(rp, t, moments, counts, floor, threshold) ? 1 : 0;
}
extern "C" void pixel_errors(const double *moments, const uint32_t *counts, double floor, int n, double *out) {
    for (int i = 0; i < n; i++) out[i] = noise_pixel_error(moments + 6 * (size_t)i, counts[i], floor);
}
extern "C" uint32_t default_params_mean_no_list() { RenderParams rp{}; return rp.tile_list == nullptr && rp.tile_count == 0u; }

// ---- denoise_core.h ----
// sig = {sigma_color, sigma_normal, sigma_albedo, sigma_depth}; counts may be null (every pixel: n_all); state (may be null): the last level's
// {C, V} of every pixel, w*h*6 doubles
extern "C" void denoise_run(const float *acc, const double *mom, const uint32_t *counts, uint32_t n_all, const float *guides, uint32_t w, uint32_t h, uint32_t levels,
                            int demodulate, const double *sig, float *d, double *state) {
    std::vector<double> work((size_t)w * h * 12);
    const int dem = demodulate && levels ? 1 : 0;
    denoise_image(acc, mom, counts, n_all, guides, w, h, levels, dem, denoise_sigmas(sig[0], sig[1], sig[2], sig[3]), work.data(), d);
    if (state) for (size_t i = 0; i < (size_t)w * h * 6; i++) state[i] = work[(levels & 1u ? (size_t)w * h * 6 : 0) + i];
}
// one level over an image of states
extern "C" void denoise_one_level(const double *in, const float *guides, uint32_t w, uint32_t h, uint32_t step, const double *sig, double *out) {
    const DenoiseSigmas sg = denoise_sigmas(sig[0], sig[1], sig[2], sig[3]);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) denoise_level(in, guides, w, h, x, y, step, sg, out + ((size_t)y * w + x) * 6);
}

// ---- robust_core.h ----  (buckets: pixels x K x 3; counts may be null (every pixel: n_all))
extern "C" void robust_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, uint64_t pixels, float *R, uint8_t *trim) {
    robust_image(buckets, counts, n_all, K, (size_t)pixels, R, trim);
}
extern "C" int robust_k_ok(double k) { return robust_valid_k(k) ? 1 : 0; }
template <uint32_t K>
static void robust_k_image(const double *buckets, const uint32_t *counts, uint64_t n_all, size_t pixels, float *R, uint8_t *trim) {
    for (size_t p = 0; p < pixels; p++) robust_pixel_k<K>(buckets + p * K * 3, counts ? (uint64_t)counts[p] : n_all, R + p * 3, trim + p);
}
extern "C" int robust_k_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, uint64_t pixels, float *R, uint8_t *trim) {
    switch (K) {
    case 3: robust_k_image<3>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 5: robust_k_image<5>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 7: robust_k_image<7>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 9: robust_k_image<9>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 11: robust_k_image<11>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 13: robust_k_image<13>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 15: robust_k_image<15>(buckets, counts, n_all, pixels, R, trim); return 0;
    }
    return 1;
}
extern "C" void robust_error_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, double floor, uint64_t pixels, double *e, uint8_t *trim) {
    robust_error_image(buckets, counts, n_all, K, floor, (size_t)pixels, e, trim);
}
extern "C" void robust_cv_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, uint64_t pixels, double *cv, uint8_t *trim) {
    for (size_t p = 0; p < pixels; p++) robust_pixel_cv(buckets + p * K * 3, K, counts ? (uint64_t)counts[p] : n_all, cv + p * 6, trim + p);
}
// sig = {sigma_color, sigma_normal, sigma_albedo, sigma_depth}; state (may be null): the last level's {C, V} of every pixel, w*h*6 doubles
extern "C" void robust_denoise_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, const float *guides, uint32_t w, uint32_t h, uint32_t levels,
                                   int demodulate, const double *sig, float *d, double *state) {
    std::vector<double> work((size_t)w * h * 12);
    const int dem = demodulate && levels ? 1 : 0;
    robust_denoise_image(buckets, counts, n_all, K, guides, w, h, levels, dem, denoise_sigmas(sig[0], sig[1], sig[2], sig[3]), work.data(), d);
    if (state) for (size_t i = 0; i < (size_t)w * h * 6; i++) state[i] = work[(levels & 1u ? (size_t)w * h * 6 : 0) + i];
}

// ---- restore_core.h ----
extern "C" void excess_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, uint64_t pixels, double *cx, uint8_t *trim) {
    for (size_t p = 0; p < pixels; p++) robust_pixel_excess(buckets + p * K * 3, K, counts ? (uint64_t)counts[p] : n_all, cx + p * 6, trim + p);
}
// sig = {sigma_n, sigma_a, sigma_z}; D (may be null): the base; x_out (may be null): X_L, w*h*3 doubles
extern "C" void restore_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, const float *guides, uint32_t w, uint32_t h, uint32_t levels,
                            const double *sig, const float *D, float *r, double *x_out) {
    std::vector<double> work((size_t)w * h * 15);
    restore_image(buckets, counts, n_all, K, guides, w, h, levels, denoise_sigmas(1.0, sig[0], sig[1], sig[2]), D, work.data(), r, x_out);
}
// the spread alone on a given excess X[h][w][3] -> out[h][w][3]
extern "C" void spread_run(const double *X, const float *guides, uint32_t w, uint32_t h, uint32_t levels, const double *sig, double *out) {
    const size_t pixels = (size_t)w * h;
    const DenoiseSigmas sg = denoise_sigmas(1.0, sig[0], sig[1], sig[2]);
    std::vector<double> a(X, X + pixels * 3), b(pixels * 3), S(pixels * 3);
    for (uint32_t l = 0; l < levels; l++) {
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) restore_norm(a.data(), 3, guides, w, h, x, y, 1u << l, sg, S.data() + ((size_t)y * w + x) * 3);
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) restore_gather(S.data(), guides, w, h, x, y, 1u << l, sg, b.data() + ((size_t)y * w + x) * 3);
        a.swap(b);
    }
    for (size_t i = 0; i < pixels * 3; i++) out[i] = a[i];
}

// ---- select_core.h ----
// sig as for denoise_run; states (may be null): w*h*18 doubles
extern "C" void select_run(const double *buckets, uint32_t K, const uint32_t *counts, uint32_t n_all, const float *acc, const double *mom, const float *guides, uint32_t w, uint32_t h,
                           uint32_t levels, int demodulate, const double *sig, uint32_t smooth, float *S, uint8_t *L, double *states) {
    std::vector<double> work((size_t)w * h * 45);
    select_image(buckets, K, counts, n_all, acc, mom, guides, w, h, levels, demodulate, denoise_sigmas(sig[0], sig[1], sig[2], sig[3]), smooth, work.data(), S, L, states);
}
