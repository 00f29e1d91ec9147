// Post chain kernels: renderer.rs:64-90 — included by hr_api.hip only (one translation unit: the kernels and the C ABI that launches them).
#pragma once
#include <hip/hip_runtime.h>

#include "denoise_core.h"
#include "device_scene.h"
#include "post_core.h"
#include "robust_core.h"

using namespace hr;

__global__ void tonemap_gamma_kernel(const float *__restrict__ acc, float *__restrict__ out, uint32_t n, float scale) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tonemap_gamma(acc[i * 3], acc[i * 3 + 1], acc[i * 3 + 2], scale, &out[i * 3]);
}
__global__ void bilateral_quantise_kernel(const float *__restrict__ img, uint8_t *__restrict__ out, uint32_t W, uint32_t H) {
    uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    bilateral_quantise(img, W, H, x, y, &out[((size_t)y * W + x) * 3]);
}

// The à-trous denoiser (denoise_core.h): one thread per pixel; an init kernel, one launch per level between two ping-pong planes
// of 6 doubles per pixel, and a final kernel.  The kernels carry no arithmetic of their own: every value is the core's.
// counts == nullptr: every pixel has n_all samplings (option "sample_counts" off).
__global__ __launch_bounds__(256) void denoise_init_kernel(const float *__restrict__ acc, const double *__restrict__ moments, const uint32_t *__restrict__ counts, uint32_t n_all,
                                                           const float *__restrict__ guides, double *__restrict__ cv, uint32_t pixels, int demodulate) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    denoise_init(acc + (size_t)i * 3, moments + (size_t)i * 6, counts ? counts[i] : n_all, guides + (size_t)i * 8, demodulate, cv + (size_t)i * 6);
}
__global__ __launch_bounds__(256) void atrous_kernel(const double *__restrict__ in, const float *__restrict__ guides, double *__restrict__ out, uint32_t W, uint32_t H, uint32_t step,
                                                     DenoiseSigmas sg) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    denoise_level(in, guides, W, H, x, y, step, sg, out + ((size_t)y * W + x) * 6);
}
__global__ __launch_bounds__(256) void denoise_final_kernel(const double *__restrict__ cv, const float *__restrict__ guides, float *__restrict__ d, uint32_t pixels, int demodulate) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    denoise_final(cv + (size_t)i * 6, guides + (size_t)i * 8, demodulate, d + (size_t)i * 3);
}

// The firefly-robust resolve (robust_core.h): one thread per pixel, R and the trim plane from the pixel's K buckets.  The kernel carries
// no arithmetic of its own.  counts == nullptr: every pixel has n_all samplings (option "sample_counts" off).
__global__ __launch_bounds__(256) void robust_kernel(const double *__restrict__ buckets, const uint32_t *__restrict__ counts, unsigned long long n_all, uint32_t K,
                                                     float *__restrict__ out, uint8_t *__restrict__ trim, uint32_t pixels) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    robust_pixel(buckets + (size_t)i * K * 3, K, counts ? (uint64_t)counts[i] : (uint64_t)n_all, out + (size_t)i * 3, trim + i);
}
