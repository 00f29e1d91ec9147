// The host build of csrc/select_noise_core.h behind tests/select_noise_cores.py: g++ -O2 -ffp-contract=off -shared, like tests/post_harness.cpp.
#include <vector>
#include "adapt_core.h"
#include "select_noise_core.h"
using namespace hr;

// select_noise_image over a whole image.  sig = {sigma_color, sigma_normal, sigma_albedo, sigma_depth}; counts may be null (every pixel: n_all)
extern "C" void select_noise_run(const double *buckets, uint32_t K, const uint32_t *counts, uint32_t n_all, const float *acc, const double *mom, const float *guides, uint32_t w,
                                 uint32_t h, uint32_t levels, int demodulate, const double *sig, uint32_t smooth, float *S, uint8_t *L, double *M) {
    std::vector<double> work((size_t)w * h * 53);
    select_noise_image(buckets, K, counts, n_all, acc, mom, guides, w, h, levels, demodulate, denoise_sigmas(sig[0], sig[1], sig[2], sig[3]), smooth, work.data(), S, L, nullptr, M);
}
// e_S of every pixel: select_noise_error
extern "C" void select_noise_errors(const double *M, const float *S, double floor, uint64_t pixels, double *out) {
    for (uint64_t i = 0; i < pixels; i++) out[i] = select_noise_error(M[i], S + i * 3, floor);
}
// the tile rule on an error image of a w x h region (adapt_pixel_above, what select_tiles_image_kernel asks per lane): out[tiles]
extern "C" void select_noise_tile_rule(const double *e_img, uint32_t w, uint32_t h, double threshold, unsigned char *out) {
    RenderParams rp{};
    rp.width = w; rp.height = h; rp.org_x = 0; rp.org_y = 0; rp.reg_w = w; rp.reg_h = h;
    rp.tiles_x = (w + 3) / 4; rp.tiles_y = (h + 3) / 4;
    for (uint32_t t = 0; t < rp.tiles_x * rp.tiles_y; t++) {
        bool any = false;
        for (uint32_t pix = 0; pix < 16u; pix++) any = adapt_pixel_above(rp, t, pix, e_img, threshold) || any;
        out[t] = any ? 1 : 0;
    }
}
