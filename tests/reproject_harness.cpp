// Host build of csrc/reproject_core.h — TEST INFRASTRUCTURE ONLY, built by tests/reproject_cores.py with g++ -ffp-contract=off as
// tests/post_harness.cpp is.  The very functions motion_kernel and reproject_kernel run, over arrays; nothing in the product loads this.
#include <cstdint>

#include "reproject_core.h"

using namespace hr;

static ReprojectCam cam_of(const double *c) {   // {eye, forward, phr, phu, focus}: 13 doubles
    ReprojectCam r;
    for (int k = 0; k < 3; k++) { r.eye[k] = c[k]; r.forward[k] = c[3 + k]; r.phr[k] = c[6 + k]; r.phu[k] = c[9 + k]; }
    r.focus = c[12];
    return r;
}

extern "C" {

// out[n][6] = {in front (1 | 0), v x, y, z, ncx, ncy}
void rp_project(const double *cam, const float *x, const uint8_t *at_infinity, uint64_t n, double *out) {
    const ReprojectCam from = cam_of(cam);
    for (uint64_t i = 0; i < n; i++) {
        double *o = out + i * 6;
        o[0] = reproject_project(from, x + i * 3, at_infinity[i] != 0, o + 1, o[4], o[5]) ? 1.0 : 0.0;
    }
}
// pix[n][3] = {px, py, sub}; out[n][3] = {inside (1 | 0), mx, my}
void rp_motion(const double *nc, uint32_t W, uint32_t H, const uint32_t *pix, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t sub = pix[i * 3 + 2];
        double *o = out + i * 3;
        o[0] = reproject_motion(nc[i * 2], nc[i * 2 + 1], W, H, pix[i * 3], pix[i * 3 + 1], (double)(sub & 1u) * 0.5 - 0.5, (double)(sub >> 1) * 0.5 - 0.5, o[1], o[2]) ? 1.0 : 0.0;
    }
}
// reproject_pixel over a w x h image; mom and out_mom may both be null
void rp_pixels(const float *motion, const float *acc, const uint32_t *counts, const double *mom, uint32_t w, uint32_t h, uint32_t max_history, float *out_acc, uint32_t *out_counts,
               double *out_mom) {
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            out_counts[i] = reproject_pixel(motion + i * 12, acc, counts, mom, w, h, x, y, max_history, out_acc + i * 3, mom ? out_mom + i * 6 : nullptr);
        }
}

}
