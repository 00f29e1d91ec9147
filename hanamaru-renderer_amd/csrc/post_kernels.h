// Post chain kernels: renderer.rs:64-90, and every kernel of the estimates, selections and denoisers of §4.7 to §4.17 — included by hr_api.hip only
// (one translation unit: the kernels and the C ABI that launches them).
#pragma once
#include <hip/hip_runtime.h>

#include "adapt_core.h"
#include "denoise_core.h"
#include "device_scene.h"
#include "noise_core.h"
#include "post_core.h"
#include "reproject_core.h"
#include "restore_core.h"
#include "robust_core.h"
#include "select_core.h"
#include "select_noise_core.h"
#include "trace_kernel.h"   // wave_ballot

using namespace hr;

__global__ void tonemap_gamma_kernel(const float *__restrict__ acc, float *__restrict__ out, uint32_t n, float scale) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tonemap_gamma(acc[i * 3], acc[i * 3 + 1], acc[i * 3 + 2], scale, &out[i * 3]);
}
// hr_resolve's first kernel with every pixel's own count: the scale is hr_resolve's expression 1.0f / (float)(count * 4u), which hr_resolve works
// out on the host, i.e. correctly rounded.  The device's fp32 division is not (the Makefile trades that for speed), so the quotient is taken in
// f64 and rounded to fp32: the same float as the host's for every count whose odd part is below 2^28 (a quotient 1 / n lies at least
// 1 / (odd(n) 2^25) of its value away from the midpoint of two floats, and rounding twice can only differ from rounding once within 2^-53).
// A pixel without samplings is radiance 0, whatever the accumulator holds.
__global__ void tonemap_gamma_counted_kernel(const float *__restrict__ acc, const uint32_t *__restrict__ counts, float *__restrict__ out, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = counts[i];
    if (k) tonemap_gamma(acc[i * 3], acc[i * 3 + 1], acc[i * 3 + 2], (float)(1.0 / (double)(float)(k * 4u)), &out[i * 3]);
    else tonemap_gamma(0.0f, 0.0f, 0.0f, 0.0f, &out[i * 3]);
}
__global__ void bilateral_quantise_kernel(const float *__restrict__ img, uint8_t *__restrict__ out, uint32_t W, uint32_t H) {
    uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    bilateral_quantise(img, W, H, x, y, &out[((size_t)y * W + x) * 3]);
}

// The summary of an estimate's image, {sum of e, max of e, pixels with e > threshold}, reduced in a FIXED ORDER, so that two calls return identical
// bits (the scheme of accumulator_sum_kernel, hr_api.hip): a grid of SUMMARY_BLOCKS workgroups of 256 threads, every thread its strided pixels in
// order (the kernel's own loop), then — here — the lanes of a wave down the __shfl_down ladder 32, 16, .. 1, the four waves' partial results in
// wave order ((w0 + w1) + w2) + w3 into out[block] = {sum, max, above}; the host adds the blocks in index order (BlockSummaries::summary, hr_api.hip).
// The tail of noise_kernel, robust_noise_kernel and select_noise_error_kernel; every thread of the workgroup calls it (the barrier).
constexpr unsigned SUMMARY_BLOCKS = 1024;
__device__ __forceinline__ void summary_block_reduce(double sum, double mx, double above, double *out) {
    __shared__ double part[4][3];
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off);
        const double o = __shfl_down(mx, off);
        mx = o > mx ? o : mx;
        above += __shfl_down(above, off);
    }
    if ((threadIdx.x & 63u) == 0u) { part[threadIdx.x >> 6][0] = sum; part[threadIdx.x >> 6][1] = mx; part[threadIdx.x >> 6][2] = above; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = out + (size_t)blockIdx.x * 3;
        o[0] = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
        o[1] = fmax(fmax(part[0][1], part[1][1]), fmax(part[2][1], part[3][1]));
        o[2] = ((part[0][2] + part[1][2]) + part[2][2]) + part[3][2];
    }
}

// The noise estimate of the moments (noise_core.h): e of every pixel into `img`, and its summary into out[block]
// (summary_block_reduce: reproducible run to run).
// CNTS (option "sample_counts" on): n is the PIXEL's own count (every one >= 2: noise_run has checked), not the samplings issued.
template <bool CNTS>
__global__ __launch_bounds__(256) void noise_kernel(const double *__restrict__ moments, size_t pixels, uint64_t samplings, double floor, double threshold,
                                                    double *__restrict__ img, double *__restrict__ out, const uint32_t *__restrict__ counts) {
    double sum = 0.0, mx = 0.0, above = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (size_t)gridDim.x * blockDim.x) {
        double m[6];
        for (int k = 0; k < 6; k++) m[k] = moments[i * 6 + k];
        const double e = hr::noise_pixel_error(m, CNTS ? (uint64_t)counts[i] : samplings, floor);
        img[i] = e;
        sum += e;
        mx = e > mx ? e : mx;
        above += e > threshold ? 1.0 : 0.0;
    }
    summary_block_reduce(sum, mx, above, out);
}
// hr_reproject's gather (reproject_pixel, reproject_core.h): one thread per pixel of the W x H region.  old_*: the call's copy of the
// planes as they were (a pixel's taps are other pixels' old values); acc, counts, mom (nullptr with old_mom: option "moments" off): the planes in
// place, every element one writer.  The kernel carries no arithmetic of its own; a tap's index is formed only after its f64 range check.
__global__ __launch_bounds__(256) void reproject_kernel(const float *__restrict__ motion, const float *__restrict__ old_acc, const uint32_t *__restrict__ old_counts,
                                                        const double *__restrict__ old_mom, uint32_t W, uint32_t H, uint32_t max_history, float *__restrict__ acc,
                                                        uint32_t *__restrict__ counts, double *__restrict__ mom) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    counts[i] = reproject_pixel(motion + i * 12, old_acc, old_counts, old_mom, W, H, x, y, max_history, acc + i * 3, old_mom ? mom + i * 6 : nullptr);
}
// the smallest and the largest count of a pixel of the region (option "sample_counts") into out[0], out[1]: an estimate needs 2 samplings behind
// EVERY pixel, and no pixel can have received more samplings than the moments have seen issued
__global__ __launch_bounds__(256) void counts_min_kernel(const uint32_t *__restrict__ counts, size_t pixels, uint32_t *__restrict__ out) {
    uint32_t mn = 0xffffffffu, mx = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t v = counts[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)mn, off), p = (uint32_t)__shfl_down((int)mx, off);
        mn = o < mn ? o : mn;
        mx = p > mx ? p : mx;
    }
    if ((threadIdx.x & 63u) == 0u) { atomicMin(out, mn); atomicMax(out + 1, mx); }
}

// The tile rule on the device (adapt_core.h): 16 lanes per tile (one per pixel), four tiles per wave; the ballot of a tile's lanes
// is its flag, ANDed with the flag it had (have_prev: a mask is in force — a tile that went inactive stays inactive).  The ascending compaction of
// the flags into the list is hipcub's DeviceSelect::Flagged over the tile indices (select_tiles_run, hr_api.hip): deterministic, two calls give
// identical lists.
__device__ __forceinline__ void tile_flag_from_lanes(bool hot, uint32_t tile, uint32_t tiles, uint32_t pix, int have_prev, uint32_t *__restrict__ flags) {
    const unsigned long long m = wave_ballot(hot);
    const bool any = ((m >> (((threadIdx.x & 63u) >> 4) * 16u)) & 0xffffull) != 0ull;
    if (pix == 0u && tile < tiles) flags[tile] = any && (!have_prev || flags[tile] != 0u) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void select_tiles_kernel(RenderParams rp, const double *__restrict__ moments, const uint32_t *__restrict__ counts, double floor, double threshold,
                                                           int have_prev, uint32_t *__restrict__ flags) {
    const uint32_t tile = blockIdx.x * 16u + (threadIdx.x >> 4), pix = threadIdx.x & 15u, tiles = rp.tiles_x * rp.tiles_y;
    const bool hot = tile < tiles && hr::adapt_pixel_active(rp, tile, pix, moments, counts, floor, threshold);
    tile_flag_from_lanes(hot, tile, tiles, pix, have_prev, flags);
}
// the same with the rule of hr_select_tiles_robust: e_R (the image a robust noise estimate has just left) in place of e
__global__ __launch_bounds__(256) void select_tiles_image_kernel(RenderParams rp, const double *__restrict__ e_img, double threshold, int have_prev, uint32_t *__restrict__ flags) {
    const uint32_t tile = blockIdx.x * 16u + (threadIdx.x >> 4), pix = threadIdx.x & 15u, tiles = rp.tiles_x * rp.tiles_y;
    const bool hot = tile < tiles && hr::adapt_pixel_above(rp, tile, pix, e_img, threshold);
    tile_flag_from_lanes(hot, tile, tiles, pix, have_prev, flags);
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

// A workgroup's 256 pixels through LDS, the staged form DESIGN.md §4.11 measured and kept (robust_noise_kernel below has it written out in its loop, and keeps
// it: with this call in the loop the compiler allocates and schedules all seven staged rows differently): the pixels of workgroup `base / 256` are one contiguous span of 256 x 24 K bytes; the lanes load it as consecutive doubles (a wave's load is 512
// contiguous bytes; past the last pixel of the image: zeros, nothing is read), park it in 256 x 24 K bytes of dynamic LDS, and every lane gets its own
// pixel's 3 K doubles back (stride 3 K doubles, 3 K odd: no bank conflict).  Every thread of the workgroup calls it (the barrier).
template <uint32_t K>
__device__ __forceinline__ const double *robust_stage_span(const double *__restrict__ buckets, size_t base, size_t pixels) {
    extern __shared__ double robust_stage[];
    constexpr uint32_t D = 3u * K;   // doubles per pixel
    const double *span = buckets + base * D;
    double v[D];
    if (base + 256u <= pixels) {
#pragma unroll
        for (uint32_t j = 0; j < D; j++) v[j] = span[j * 256u + threadIdx.x];
    } else {
        const size_t have = (pixels - base) * D;   // doubles of the span that exist
#pragma unroll
        for (uint32_t j = 0; j < D; j++) v[j] = j * 256u + threadIdx.x < have ? span[j * 256u + threadIdx.x] : 0.0;
    }
#pragma unroll
    for (uint32_t j = 0; j < D; j++) robust_stage[j * 256u + threadIdx.x] = v[j];
    __syncthreads();
    return robust_stage + threadIdx.x * D;
}

// The firefly-robust resolve (robust_pixel_k, robust_core.h): one thread per pixel, one workgroup per span of 256 pixels, R and the
// trim plane from the pixel's K buckets.  K is a template parameter: the bucket means live in registers, no array is indexed at run time, nothing
// goes to scratch.  The kernel carries no arithmetic of its own.  counts == nullptr: every pixel has n_all samplings (option "sample_counts" off).
template <uint32_t K>
__global__ __launch_bounds__(256) void robust_kernel(const double *__restrict__ buckets, const uint32_t *__restrict__ counts, unsigned long long n_all,
                                                     float *__restrict__ out, uint8_t *__restrict__ trim, size_t pixels) {
    const size_t base = (size_t)blockIdx.x * 256u, i = base + threadIdx.x;
    const double *B = robust_stage_span<K>(buckets, base, pixels);
    if (i >= pixels) return;
    robust_pixel_k<K>(B, counts ? (uint64_t)counts[i] : (uint64_t)n_all, out + i * 3, trim + i);
}

// The robust denoiser's init pass (robust_denoise_init_k, robust_core.h): the pixel's {C, V} from its K buckets into the
// call-scoped plane of 6 doubles per pixel that denoise_init_kernel fills for hr_denoise; the levels and the final pass are atrous_kernel and
// denoise_final_kernel above.  The same shape as robust_kernel; every pixel has n >= K samplings (hr_denoise_robust has checked).
template <uint32_t K>
__global__ __launch_bounds__(256) void robust_denoise_init_kernel(const double *__restrict__ buckets, const uint32_t *__restrict__ counts, unsigned long long n_all,
                                                                  const float *__restrict__ guides, double *__restrict__ cv, size_t pixels, int demodulate) {
    const size_t base = (size_t)blockIdx.x * 256u, i = base + threadIdx.x;
    const double *B = robust_stage_span<K>(buckets, base, pixels);
    if (i >= pixels) return;
    robust_denoise_init_k<K>(B, counts ? (uint64_t)counts[i] : (uint64_t)n_all, guides + i * 8, demodulate, cv + i * 6);
}

// The robust noise estimate (robust_pixel_error_k, robust_core.h): e_R of every pixel into `img`, the trim it took into `trim`
// (or nullptr), and the summary out[block] = {sum of e_R, max of e_R, pixels with e_R > threshold}, reduced in noise_kernel's fixed order
// (summary_block_reduce): two calls return identical bits.  The kernel carries no arithmetic of its own.
// K is a template parameter: the pixel's K keys live in registers, no array is indexed at run time, nothing goes to scratch.  counts == nullptr: every pixel has n_all samplings.
// STAGE: how the lanes come by their pixel's 3 K doubles — the arithmetic, and so every bit, is the same.
//   true   a workgroup's 256 pixels are one contiguous span of 256 x 24 K bytes: its lanes load it as consecutive doubles (a wave's load is 512
//          contiguous bytes), park it in 256 x 24 K bytes of dynamic LDS, and every lane reads its own pixel from there (stride 3 K doubles, 3 K odd:
//          no bank conflict)
//   false  every lane loads its own 24 K contiguous bytes from global memory: a wave's load touches 64 lines 24 K bytes apart
// The loop runs the same number of times for every thread of a workgroup (the barriers), a lane past the last pixel computes nothing.
template <uint32_t K, bool STAGE>
__global__ __launch_bounds__(256) void robust_noise_kernel(const double *__restrict__ buckets, const uint32_t *__restrict__ counts, unsigned long long n_all, size_t pixels,
                                                           double floor, double threshold, double *__restrict__ img, uint8_t *__restrict__ trim, double *__restrict__ out) {
    extern __shared__ double robust_noise_stage[];
    constexpr uint32_t D = 3u * K;   // doubles per pixel
    double sum = 0.0, mx = 0.0, above = 0.0;
    for (size_t base = (size_t)blockIdx.x * 256u; base < pixels; base += (size_t)gridDim.x * 256u) {
        const size_t i = base + threadIdx.x;
        const double *B = buckets + i * D;
        if (STAGE) {
            const double *span = buckets + base * D;
            double v[D];
            if (base + 256u <= pixels) {
#pragma unroll
                for (uint32_t j = 0; j < D; j++) v[j] = span[j * 256u + threadIdx.x];
            } else {
                const size_t have = (pixels - base) * D;   // doubles of the span that exist
#pragma unroll
                for (uint32_t j = 0; j < D; j++) v[j] = j * 256u + threadIdx.x < have ? span[j * 256u + threadIdx.x] : 0.0;
            }
#pragma unroll
            for (uint32_t j = 0; j < D; j++) robust_noise_stage[j * 256u + threadIdx.x] = v[j];
            __syncthreads();
            B = robust_noise_stage + threadIdx.x * D;
        }
        if (i < pixels) {
            double e;
            uint8_t t;
            robust_pixel_error_k<K>(B, counts ? (uint64_t)counts[i] : (uint64_t)n_all, floor, &e, &t);
            img[i] = e;
            if (trim) trim[i] = t;
            sum += e;
            mx = e > mx ? e : mx;
            above += e > threshold ? 1.0 : 0.0;
        }
        if (STAGE) __syncthreads();   // the next round overwrites the span
    }
    summary_block_reduce(sum, mx, above, out);
}

// The restored robust resolve R' (restore_core.h).  The kernels carry no arithmetic of their own: every value is the core's.
// restore_init_kernel<K>: the shape of robust_denoise_init_kernel — one workgroup per span of 256 pixels, the span through robust_stage_span's LDS —,
// {C, X} of the pixel into the call-scoped plane of 6 doubles per pixel.  counts == nullptr: every pixel has n_all samplings.
template <uint32_t K>
__global__ __launch_bounds__(256) void restore_init_kernel(const double *__restrict__ buckets, const uint32_t *__restrict__ counts, unsigned long long n_all,
                                                           double *__restrict__ cx, size_t pixels) {
    const size_t base = (size_t)blockIdx.x * 256u, i = base + threadIdx.x;
    const double *B = robust_stage_span<K>(buckets, base, pixels);
    if (i >= pixels) return;
    uint8_t t;
    robust_pixel_excess_k<K>(B, counts ? (uint64_t)counts[i] : (uint64_t)n_all, cx + i * 6, &t);
}
// One level of the spread, two launches, one thread per pixel, every element one writer, no atomics: S = X / N (X: xs doubles from one pixel to the
// next), then X' as the gather of S.  A pixel's guides are two 16-byte loads per tap (restore_guides).
__global__ __launch_bounds__(256) void spread_norm_kernel(const double *__restrict__ X, uint32_t xs, const float *__restrict__ guides, double *__restrict__ S, uint32_t W, uint32_t H,
                                                          uint32_t step, DenoiseSigmas sg) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    restore_norm(X, xs, guides, W, H, x, y, step, sg, S + ((size_t)y * W + x) * 3);
}
__global__ __launch_bounds__(256) void spread_gather_kernel(const double *__restrict__ S, const float *__restrict__ guides, double *__restrict__ out, uint32_t W, uint32_t H,
                                                            uint32_t step, DenoiseSigmas sg) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    restore_gather(S, guides, W, H, x, y, step, sg, out + ((size_t)y * W + x) * 3);
}
// R' = (float)(base + X_L): base C of the init plane, or D != nullptr: the denoised robust radiance
__global__ __launch_bounds__(256) void restore_final_kernel(const double *__restrict__ cx, const float *__restrict__ D, const double *__restrict__ X, uint32_t xs,
                                                            float *__restrict__ restored, uint32_t pixels) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    restore_final(cx + (size_t)i * 6, D ? D + (size_t)i * 3 : nullptr, X + (size_t)i * xs, restored + (size_t)i * 3);
}

// The denoiser that picks its level per pixel (select_core.h).  The kernels carry no arithmetic of their own: every value is the core's.
// The three states lie in call-scoped memory as 18 planes of one double per pixel — component c of state s (0: A, 1: B, 2: W) is plane 6 s + c —
// and the halves' level-0 radiance {A0, B0} as 6 more: a wave's load of one component is contiguous (a row of 32 lanes reads 256 bytes; with 6
// doubles per pixel side by side it would be spread over 1,536), and the pick reads the three C components it needs and no V.  select_plane_at is the
// one place that says so; the other layout — a pixel's N doubles side by side — is kept for the comparison of DESIGN.md §4.16: a library built with
// -DHR_SELECT_INTERLEAVED (`make EXPFLAGS=-DHR_SELECT_INTERLEAVED`) runs it instead — the same bits, another time.
template <uint32_t N>   // N: the planes of the block (18: the states, 6: {A0, B0})
__device__ __forceinline__ size_t select_plane_at(uint32_t plane, size_t q, size_t pixels) {
#if defined(HR_SELECT_INTERLEAVED)
    return q * N + plane;
#else
    return (size_t)plane * pixels + q;
#endif
}
struct SelectPlanes {
    const double *base;
    size_t pixels;
    __device__ __forceinline__ double operator()(int s, size_t q, int c) const { return base[select_plane_at<18>((uint32_t)(s * 6 + c), q, pixels)]; }
};
// select_init_kernel<K>: the shape of robust_denoise_init_kernel — one workgroup per span of 256 pixels, the span through robust_stage_span's LDS —,
// the initial {C, V} of A, B and W into `st` and {A0, B0} into `raw`.  K is a template parameter: no array is indexed at run time, nothing goes to
// scratch.  Every pixel has n >= 2 samplings (hr_denoise_select has checked).  counts == nullptr: every pixel has n_all samplings.
template <uint32_t K>
__global__ __launch_bounds__(256) void select_init_kernel(const double *__restrict__ buckets, const uint32_t *__restrict__ counts, uint32_t n_all, const float *__restrict__ acc,
                                                          const double *__restrict__ moments, const float *__restrict__ guides, double *__restrict__ st, double *__restrict__ raw,
                                                          size_t pixels, int demodulate) {
    const size_t base = (size_t)blockIdx.x * 256u, i = base + threadIdx.x;
    const double *B = robust_stage_span<K>(buckets, base, pixels);
    if (i >= pixels) return;
    double a[6], b[6], w[6];
    select_init_k<K>(B, counts ? counts[i] : n_all, acc + i * 3, moments + i * 6, guides + i * 8, demodulate, a, b, w);
#pragma unroll
    for (uint32_t c = 0; c < 6; c++) { st[select_plane_at<18>(c, i, pixels)] = a[c]; st[select_plane_at<18>(6 + c, i, pixels)] = b[c]; st[select_plane_at<18>(12 + c, i, pixels)] = w[c]; }
#pragma unroll
    for (uint32_t c = 0; c < 3; c++) { raw[select_plane_at<6>(c, i, pixels)] = a[c]; raw[select_plane_at<6>(3 + c, i, pixels)] = b[c]; }
}
// One level of the three states in one launch (select_level3): a tap's guides are read once and its guide weight is computed once for the three
// colour weights — three atrous_kernel launches read them and compute it three times.  One thread per pixel, straight from global memory like
// atrous_kernel: at steps >= 4 an LDS tile with its halo would be mostly holes, and the 25 taps of neighbouring pixels meet in the caches.
// select_level3 unrolls its 25 taps: what bounds a level is the latency of a tap's chain of loads, divisions and sums, and unrolled the loads of
// many taps are in flight under the arithmetic of the others (DESIGN.md §4.16 has the three measurements).
__global__ __launch_bounds__(256) void atrous3_kernel(const double *__restrict__ in, const float *__restrict__ guides, double *__restrict__ out, uint32_t W, uint32_t H, uint32_t step,
                                                      DenoiseSigmas sg) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t pixels = (size_t)W * H, p = (size_t)y * W + x;
    double o[3][6];
    select_level3(SelectPlanes{in, pixels}, guides, W, H, x, y, step, sg, o);
#pragma unroll
    for (int s = 0; s < 3; s++) {
#pragma unroll
        for (int c = 0; c < 6; c++) out[select_plane_at<18>((uint32_t)(s * 6 + c), p, pixels)] = o[s][c];
    }
}
// The error of level l and the pick.  e_out != nullptr: e_l of every pixel into that plane, nothing else (the smoothing passes come next).
// Otherwise the pick, with the error taken from e_in (the smoothed plane) or, e_in == nullptr, computed here (smooth = 0: one launch per level).
__global__ __launch_bounds__(256) void select_pick_kernel(const double *__restrict__ st, const double *__restrict__ raw, const float *__restrict__ guides,
                                                          const double *__restrict__ e_in, double *__restrict__ e_out, uint32_t l, double *__restrict__ best,
                                                          uint8_t *__restrict__ L, float *__restrict__ S, uint32_t pixels, int demodulate) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    const SelectPlanes at{st, pixels};
    const size_t p = i;
    double e;
    if (e_in) e = e_in[p];
    else {
        const double fa[3] = {at(0, p, 0), at(0, p, 1), at(0, p, 2)}, fb[3] = {at(1, p, 0), at(1, p, 1), at(1, p, 2)};
        const double a0[3] = {raw[select_plane_at<6>(0, p, pixels)], raw[select_plane_at<6>(1, p, pixels)], raw[select_plane_at<6>(2, p, pixels)]};
        const double b0[3] = {raw[select_plane_at<6>(3, p, pixels)], raw[select_plane_at<6>(4, p, pixels)], raw[select_plane_at<6>(5, p, pixels)]};
        e = select_error(fa, fb, a0, b0);
    }
    if (e_out) { e_out[p] = e; return; }
    const double fw[3] = {at(2, p, 0), at(2, p, 1), at(2, p, 2)};   // (denoise_final reads C alone)
    select_pick(e, l, fw, guides + p * 8, demodulate, best + p, L + p, S + p * 3);
}
__global__ __launch_bounds__(256) void select_smooth_kernel(const double *__restrict__ e, double *__restrict__ out, uint32_t W, uint32_t H, uint32_t step) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= W || y >= H) return;
    out[(size_t)y * W + x] = select_smooth(e, W, H, x, y, step);
}

// The error estimate of S (select_noise_core.h).  The kernels carry no arithmetic of their own: every value is the core's.  The run is
// hr_denoise_select's with select_noise_kernel in select_pick_kernel's place: select_init_kernel, atrous3_kernel and select_smooth_kernel (over the e
// plane and over the m plane) are launched as they are.  var0: six more planes of a double per pixel, {va0, vb0} — the V of F_A,0 and F_B,0, which the
// ping-pong of the states overwrites at level 2; the launch of level 0 that computes m writes them, every later one reads them.
// select_noise_kernel has select_pick_kernel's three forms.  e_out != nullptr: e_l and m_l of every pixel into e_out and m_out, nothing else (the
// smoothing passes come next).  Otherwise the pick with M beside it, the error and m taken from e_in and m_in (the smoothed planes) or, e_in == nullptr,
// computed here (smooth = 0: one launch per level).
__global__ __launch_bounds__(256) void select_noise_kernel(const double *__restrict__ st, const double *__restrict__ raw, double *__restrict__ var0, const float *__restrict__ guides,
                                                           const double *__restrict__ e_in, const double *__restrict__ m_in, double *__restrict__ e_out, double *__restrict__ m_out,
                                                           uint32_t l, double *__restrict__ best, uint8_t *__restrict__ L, float *__restrict__ S, double *__restrict__ M,
                                                           uint32_t pixels, int demodulate) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    const SelectPlanes at{st, pixels};
    const size_t p = i;
    const float *g = guides + p * 8;
    double e, m;
    if (e_in) { e = e_in[p]; m = m_in[p]; }
    else {
        double fa[6], fb[6], a0[3], b0[3], va0[3], vb0[3];
#pragma unroll
        for (int c = 0; c < 6; c++) { fa[c] = at(0, p, c); fb[c] = at(1, p, c); }
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            a0[c] = raw[select_plane_at<6>(c, p, pixels)];
            b0[c] = raw[select_plane_at<6>(3 + c, p, pixels)];
            if (l == 0u) {
                va0[c] = fa[3 + c]; vb0[c] = fb[3 + c];
                var0[select_plane_at<6>(c, p, pixels)] = va0[c];
                var0[select_plane_at<6>(3 + c, p, pixels)] = vb0[c];
            } else {
                va0[c] = var0[select_plane_at<6>(c, p, pixels)];
                vb0[c] = var0[select_plane_at<6>(3 + c, p, pixels)];
            }
        }
        e = select_error(fa, fb, a0, b0);
        m = select_noise_m(fa, fb, a0, b0, va0, vb0, g, demodulate);
    }
    if (e_out) { e_out[p] = e; m_out[p] = m; return; }
    const double va[3] = {at(0, p, 3), at(0, p, 4), at(0, p, 5)}, vb[3] = {at(1, p, 3), at(1, p, 4), at(1, p, 5)};
    const double fw[6] = {at(2, p, 0), at(2, p, 1), at(2, p, 2), at(2, p, 3), at(2, p, 4), at(2, p, 5)};
    const double mse = select_noise_mse(m, va, vb, fw + 3, g, demodulate);
    select_noise_pick(e, mse, l, fw, g, demodulate, best + p, L + p, S + p * 3, M + p);
}
// e_S of every pixel from M and the run's S into `img`, and the summary out[block] = {sum of e_S, max of e_S, pixels with e_S > threshold}, reduced in
// robust_noise_kernel's fixed order (summary_block_reduce): two calls return identical bits.
__global__ __launch_bounds__(256) void select_noise_error_kernel(const double *__restrict__ M, const float *__restrict__ S, size_t pixels, double floor, double threshold,
                                                                 double *__restrict__ img, double *__restrict__ out) {
    double sum = 0.0, mx = 0.0, above = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < pixels; i += (size_t)gridDim.x * 256u) {
        const double e = select_noise_error(M[i], S + i * 3, floor);
        img[i] = e;
        sum += e;
        mx = e > mx ? e : mx;
        above += e > threshold ? 1.0 : 0.0;
    }
    summary_block_reduce(sum, mx, above, out);
}
