// hr_api.hip — the device context and the C ABI of include/hanamaru_hip.h (+ the test / measurement entry points of hanamaru_hip_debug.h) (gfx950).  One translation unit with its kernels:
//   seed_kernels.h   seed_seg_kernel (default: the ISAAC-64 init sweep as three runs computed side by side from states the producer
//                    waves work out ahead in registers, consumer waves run the LDS-bound round), seed_pc_kernel (the same roles with
//                    a ring of generator words), seed_isaac64_kernel (fused form), seed_debug_kernel
//   trace_kernel.h   trace_kernel — the path-tracing megakernel: persistent waves pull 4x4-pixel tiles from a global
//                    counter, one lane per path, stackless threaded-BVH traversal in box / leaf phases, finished lanes are
//                    refilled with ballot / mbcnt prefix ranks; no LDS, so it co-resides with the seed kernel of the NEXT
//                    batch (own stream) — plus trace_debug_kernel (the same traversal, for hr_debug_trace), intersect_debug_kernel
//                    and debug_render_kernel (renderer.rs:101-146)
//   wf_kernels.h     the split pipeline (option trace_mode 1): wf_start_kernel, wf_traverse_kernel (the same traversal at <= 64 VGPRs),
//                    wf_shade_kernel — the megakernel cut at scene.intersect, the path parked in HBM between the two
//   post_kernels.h   tonemap_gamma_kernel, tonemap_gamma_counted_kernel, bilateral_quantise_kernel; summary_block_reduce — the estimates' one fixed-order
//                    reduction — with noise_kernel (noise_core.h) and counts_min_kernel; select_tiles_kernel and select_tiles_image_kernel (adapt_core.h);
//                    the denoiser: denoise_init_kernel, atrous_kernel, denoise_final_kernel (denoise_core.h);
//                    robust_kernel, robust_denoise_init_kernel and robust_noise_kernel (robust_core.h); restore_init_kernel, spread_norm_kernel,
//                    spread_gather_kernel and restore_final_kernel (restore_core.h); select_init_kernel, atrous3_kernel, select_pick_kernel and
//                    select_smooth_kernel (select_core.h); select_noise_kernel and select_noise_error_kernel (select_noise_core.h)
//   gpu_bvh.h        the device BVH builders' kernels (option bvh_builder = 1 LBVH, 2 PLOC)
//   here             governor_kernel, add_accumulator_kernel, fold_plane_kernel (hr_fold_statistics), accumulator_sum_kernel
// The exported functions are declared extern "C" by the two headers; their definitions here follow those declarations and so have C linkage.
// Which instantiation of these kernels a launch runs is decided in kernel_variants.h: one table and one select_*() per family; the launch sites
// here call the selector, create_resources walks the tables (the seed kernels' LDS attribute, the trace side's "no LDS" guard).
// The buffers that have the render region's shape (accumulator, resolve buffers, all-reduced total, moments, noise image, counts, guides, denoised image, sample buckets, robust image and its trim plane, robust noise image and its trim plane, restored robust image, selected image and its level plane) are rows of one
// table, PLANES, with one set of routines for their bytes, life cycle, zeroing and host copies; scratch a call needs lives in a CallScratch.
// The images made of them and kept for later reads (guides, D, R, R', S) are rows of a second table, IMAGES: what each goes stale with, and one check for its reads.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "bvh_build.h"
#include "device_scene.h"
#include "flatten.h"
#include "gpu_bvh.h"
#include "hanamaru_hip.h"
#include "hanamaru_hip_debug.h"
#include "hr_comm.h"
#include "isaac_core.h"
#include "post_core.h"
#include "pt_core.h"

using namespace hr;

// ------------------------------------------------------------------------------------------ helpers

static thread_local std::string g_err;
static int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fail(HR_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
// the same for the entry points whose callers have always been told "<entry point>: <HIP's text>"
#define HIP_TRY_AS(who, expr)                                                                                 \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fail(HR_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e_));               \
    } while (0)
template <class T>
static int free_device(T *&p) {
    if (p) { HIP_TRY(hipFree(p)); p = nullptr; }
    return HR_OK;
}
// Device memory for the duration of one call: every block is freed when the holder goes out of scope, on every path out of the call.
struct CallScratch {
    std::vector<void *> blocks;
    CallScratch() = default;
    CallScratch(const CallScratch &) = delete;
    CallScratch &operator=(const CallScratch &) = delete;
    ~CallScratch() { for (void *q : blocks) (void)hipFree(q); }
    hipError_t alloc(void **out, size_t bytes) {
        const hipError_t e = hipMalloc(out, bytes);
        if (e == hipSuccess) blocks.push_back(*out);
        return e;
    }
};

#include "seed_kernels.h"
#include "trace_kernel.h"
#include "wf_kernels.h"
#include "post_kernels.h"
#include "kernel_variants.h"

// ------------------------------------------------------------------------------------------ context

struct EventPair { hipEvent_t a, b; };

// What a derived image (IMAGES, behind the planes) can be made of: a call that changes one of these says so to changed().
enum : uint32_t { SRC_ACCUM = 1, SRC_MOMENTS = 2, SRC_COUNTS = 4, SRC_BUCKETS = 8, SRC_GUIDES = 16, SRC_SCENE = 32, SRC_TARGET = 64, SRC_NEW_D = 128 };
enum ImageId { GUIDE_IMAGE, D_IMAGE, R_IMAGE, RESTORED_IMAGE, SELECTED_IMAGE, MOTION_IMAGE, N_IMAGES };

struct hr_ctx {
    int device = 0;
    int num_cus = 256;
    // streams: trace + post on `stream` (own or the caller's), the seed kernel of the NEXT batch on `seed_stream`,
    hipStream_t stream = nullptr, own_stream = nullptr, seed_stream = nullptr;
    // scene
    std::vector<void *> scene_allocs;
    Scene dsc{};
    bool have_scene = false;
    hr_camera camera{};           // the f64 camera in place, as hr_upload_scene or hr_set_camera took it (hr_get_camera)
    uint64_t st_nodes = 0, st_tris = 0, st_spheres = 0, st_cuboids = 0;
    uint32_t num_images = 0;   // of the scene in place: what hr_debug_texture checks its image indices against
    // target
    uint32_t W = 0, H = 0;
    // the region (hr_set_region): the window [RX, RX + RW) x [RY, RY + RH) of the W x H frame that is rendered; the accumulator and
    // everything shaped like it is RW x RH.  hr_set_resolution makes it the whole frame.
    uint32_t RX = 0, RY = 0, RW = 0, RH = 0;
    float *accum_own = nullptr, *accum = nullptr;
    float *post_tmp = nullptr;
    uint8_t *d_rgb8 = nullptr;
    // option "moments": per pixel {S1r, S1g, S1b, S2r, S2g, S2b} of the per-sampling values (accumulate_kernel<true>), the samplings behind
    // them, and the noise image of the last estimate (allocated when one is first asked for)
    bool moments_on = false;
    double *moments = nullptr, *noise_img = nullptr;
    uint64_t moments_n = 0;
    // option "sample_counts" (DESIGN.md §4.8): the samplings every pixel of the region has received (accumulate_kernel<.., true>), region-local
    bool counts_on = false;
    uint32_t *counts = nullptr;
    // the denoiser: the guide planes {albedo rgb, normal xyz, depth, coverage} of the region — rendered by hr_render_guides or written
    // by the host — and the denoised radiance D of the last hr_denoise or hr_denoise_robust
    float *guides = nullptr, *denoised = nullptr;
    // temporal reuse: the motion plane {mx, my, code} of every sub-sample, written by the host, that hr_reproject gathers along
    float *motion = nullptr;
    // the derived images' validity (IMAGES): the sources the image in place goes stale with, as it was made; 0: there is none
    uint32_t made_of[N_IMAGES] = {};
    uint32_t guide_bounces = 0;   // option "guide_bounces": mirrors and glass the guide rays follow to the first non-delta hit (0: the first hit's planes)
    // option "robust_buckets" = K: per pixel K x 3 sums of the per-sampling values, sampling j of a pixel in bucket j mod K
    // (bucket_kernel), the samplings behind them, and the robust radiance R with its trim plane of the last hr_robust
    bool robust_on = false;
    uint32_t robust_k = 0;
    bool bucket_by_sampling = false;   // option "bucket_by_sampling" (DESIGN.md §4.13): sampling s in bucket (s - 1) mod K, so that shards add up (hr_fold_statistics)
    double *buckets = nullptr;
    uint64_t buckets_n = 0;
    float *robust = nullptr;
    uint8_t *robust_trim = nullptr;
    // the restored robust radiance R' of the last hr_robust_restore
    float *restored = nullptr;
    // the selected radiance S of the last hr_denoise_select and the level each pixel took
    float *selected = nullptr;
    uint8_t *selected_levels = nullptr;
    // the robust noise estimate: e_R of every pixel and the trim behind it, as the last estimate or selection left them (allocated
    // when one is first asked for; every call that reads them has just written them)
    double *robust_noise_img = nullptr;
    uint8_t *robust_noise_trim = nullptr;
    // the tile mask (hr_set_tile_mask / hr_select_tiles): which 4x4 tiles of the region hr_render covers.  On the device the compacted list of the
    // active tiles' indices, ascending (RenderParams::tile_list), and the flags it was compacted from; on the host the same flags as bytes.
    bool mask_on = false;
    std::vector<uint8_t> mask;               // [tiles_y * tiles_x] 0 / 1
    uint32_t mask_active = 0;                // entries of the list
    uint64_t mask_pixels = 0;                // in-region pixels of the active tiles (hr_stats.paths)
    uint32_t *d_tile_list = nullptr, *d_tile_flags = nullptr;   // [tiles] each
    uint32_t *d_select_out = nullptr;        // [3]: hipcub's count of selected tiles, the smallest and the largest count of a pixel (counts_min_kernel)
    void *select_tmp = nullptr;              // hipcub's scratch for the compaction
    size_t select_tmp_bytes = 0;
    // multi-GPU: RCCL communicator of this rank, and the all-reduced accumulator (valid until the next render / clear / write)
    hrcomm::Comm comm = nullptr;
    int comm_world = 0, comm_rank = 0;
    int comm_path = HR_COMM_NONE;              // how the group was formed (hr_comm_info)
    uint64_t comm_group = 0;                   // hr_comm_init_local over distinct devices: the same number on every context of ONE call (hr_fold_statistics_group asks that its contexts are one group's), else 0
    uint64_t allreduces = 0;                   // collectives this context has enqueued since its communicator was made
    std::vector<hr_ctx *> same_device_peers;   // hr_comm_init_local over contexts that share ONE device: summed by a kernel, not by RCCL
    float *accum_total = nullptr;
    bool total_valid = false;
    // seed -> trace hand-off, double buffered (slot = batch & 1)
    float *recs[2] = {nullptr, nullptr};     // 128-byte record per path (device_scene.h)
    uint32_t *ovf = nullptr;                 // per consumer wave: list of the paths it re-derives at the end of a launch (seed_fixup_wave)
    uint32_t ovf_cap = 0;                    // entries per consumer wave the list is allocated for (ensure_ovf)
    u64 *ovf_win = nullptr;                  // per consumer wave: raw-output window of that fix-up
    size_t draws_cap = 0;                    // items (tile x sampling) per buffer
    uint64_t rec_lo_off = 0;                 // floats from a record buffer's start to its twin (the draws' residuals, precise shading); 0: the buffers have none
    int draw_residuals = 1;                  // debug option: precise shading's records carry the draws' residuals (0: the fp32 draws alone, the A/B)
    u64 *ring = nullptr;                     // seed kernels' hand-off ring (three-run kernel: 120 KiB per CU of 16-register states; ring kernel: <= 680 KiB per CU)
    int seed_split = 16;                      // option seed_split: init blocks done by the producer waves (8, 12, 16, 20, 24, 28)
    uint32_t init_prio = 1;                  // s_setprio of the producer waves
    hipEvent_t seed_done[2] = {nullptr, nullptr}, trace_done[2] = {nullptr, nullptr};
    bool seed_pending[2] = {false, false}, trace_pending[2] = {false, false};
    uint64_t batch_counter = 0;
    Counters *d_counters = nullptr;
    uint32_t *d_tile_counter = nullptr;      // [2]: next tile of the trace launch in each slot
    // options (hr_set_option)
    bool counters = false;
    uint32_t batch = 0;                      // samplings per launch; 0 = automatic: about 33 M paths per launch (4 at 1080p, more for small images)
    uint32_t adv_den = 2, leaf_den = 2;      // trace-kernel phase thresholds
    int min_waves = 5;                       // occupancy variant of the trace kernel
    uint32_t trace_wgs = 6;                  // trace-kernel workgroups per CU in the grid (persistent waves)
    uint32_t tail_div = 16;                  // debug: the last 1 / tail_div of a launch's tiles go out one sampling at a time (0 = off)
    uint32_t trace_grid = 0, trace_budget = 0;   // debug: absolute grid size (0 = trace_wgs per CU) / workgroups that stay (0 = all)
    uint32_t node_unroll = 2;                // box phase: node visits per pass of the loop
    uint32_t kchunk = 0;                     // samplings per work unit of the trace kernel (0 = 4)
    int trace_boost = -1;                    // which kernel's waves come first: -1 = governed on the device from the kernels' own time stamps (default), 0 .. 4 = fixed level
    GovDev *gov = nullptr;                   // the governor's state (device memory; device_scene.h)
    bool quant_nodes = true;                 // trace kernel walks the 16-byte quantised nodes (host-built trees; next upload)
    int max_leaf = 4;                        // BVH leaf size (next upload)
    double split_ratio = -1.0;               // early split clipping: -1 = automatic (kept when it cuts the SAH cost by more than 7 %), 0 = off, > 0 = ratio
    int bvh_builder = -1;                    // -1 = by scene size (default: host SAH below AUTO_BUILDER_PRIMS primitives, device PLOC from there on), 0 = host binned SAH (bvh_build.cpp), 1 = device LBVH, 2 = device PLOC (gpu_bvh.h); next upload
    int builder_in_use = 0;                  // what the last hr_upload_scene built with (0 | 1 | 2)
    double bvh_build_ms = 0;                 // device builder: key + sort + hierarchy + fit + emit + gather kernels
    uint64_t max_tail_bytes = 20ull << 30;   // cap of each hand-off buffer
    int seed_mode = 2;                       // 2 = three-run seed kernel (default), 1 = producer / consumer kernel with the state ring, 0 = fused seed kernel
    int seed_prof = 0;                       // phase timing build of the seed kernel (three-run kernel: 1 = consumer waves, 2 = producer waves; ring kernel: splits 16 and 20)
    int seed_prerun = 1;                     // three-run seed kernel: 1 = the pre-run form of its window (seed_kernels.h), 0 = three equal runs
    uint32_t seed_prio = 3;                  // s_setprio of the seed / round kernel's waves
    uint32_t nee_cull = 7;                   // debug option nee_cull: mask of nee_setup's shortcuts in force (1 far side | 2 GGX below the horizon; bit 2 reserved); 0 = trace every NEE shadow ray (bit-identical image, more rays)
    uint32_t rr_start = 0;                   // Russian roulette from this path iteration on (0 = off: the reference has none; NOT image-preserving)
    uint32_t ploc_top = hr::lbvh::PLOC_TOP_CLUSTERS;   // builder 2: clusters the bottom-up merges leave for the top-down build (1 = merge to the root)
    // the split pipeline (wf_kernels.h): queues of the launch being traced, sized for the largest launch so far
    int trace_mode = 0;                      // IN FORCE (resolve_modes): 0 = megakernel (trace_kernel), 1 = split: traversal kernel + shading kernel per path iteration
    int trace_mode_opt = -1;                 // debug option trace_mode: -1 = automatic (the split pipeline for precise shading of scenes with many triangles), 0 / 1 = pinned
    int precise_opt = -1;                    // option precise_shading: -1 = automatic (on for scenes without triangle meshes), 0 = off, 1 = on
    bool precise = false;                    // IN FORCE (resolve_modes) — option precise_shading: the bounce geometry in f64 (prec_core.h) — in the megakernel (path_advance<.., PREC>), or in the split pipeline's shading kernel with trace_mode 1
    bool wf_has_prec = false;                // the queues hold the residual quads
    WfQueues wf{};
    void *wf_block = nullptr;                // one allocation behind every pointer of wf
    uint32_t wf_adv_den = 2, wf_trav_wgs = 8, wf_shade_wgs = 8;   // debug: traversal kernel leaves its walk when 1/wf_adv_den of the lanes are done; workgroups per CU
    int debug_skip = 0;                      // timing experiments only (garbage image): 2 = skip the seed kernel, 4 = no ring stores, 8 = no ring fills, 16 = skip the trace kernel
    // timing (HIP events around every launch, summed when the streams are drained)
    std::vector<EventPair> seed_events, trace_events, post_events, debug_events;
    double seed_ms = 0, trace_ms = 0, post_ms = 0, debug_ms = 0;
    uint64_t seed_launches = 0, trace_launches = 0, debug_launches = 0;
    uint64_t paths_rendered = 0;
    // hr_mark / hr_wait: markers on the main stream, oldest first
    std::vector<std::pair<uint64_t, hipEvent_t>> markers;
    uint64_t next_ticket = 1;
};

// caller-owned accumulators (hr_bind_accumulator): one context per buffer.  accumulate_kernel adds a launch's radiance with plain loads and
// stores (no atomics since round 3), so two contexts accumulating into one buffer would race silently: a second binding is refused.
static std::mutex g_bound_mu;
static std::map<const void *, std::pair<const hr_ctx *, size_t>> g_bound;   // buffer -> (context, bytes)
static void unbind_accumulator(hr_ctx *c) {
    std::lock_guard<std::mutex> lk(g_bound_mu);
    for (auto it = g_bound.begin(); it != g_bound.end();) it = it->second.first == c ? g_bound.erase(it) : std::next(it);
}
static void free_scene(hr_ctx *c) {
    for (void *p : c->scene_allocs) (void)hipFree(p);
    c->scene_allocs.clear();
    c->have_scene = false;
}
template <class T>
static int upload(hr_ctx *c, const std::vector<T> &v, const T **out) {
    void *d = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIP_TRY(hipMalloc(&d, bytes));
    c->scene_allocs.push_back(d);
    if (!v.empty()) HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<const T *>(d);
    return HR_OK;
}
// Priority governor.  All waves run at priority 0 except the seed kernel's consumer waves (3); which of the REST comes first decides which
// of the two kernels is the slower one.  Five levels, from "the seed kernel's producer waves first" to "the trace kernel first":
//   0  producers at init_prio (1), trace kernel at 0          3  producers at 0, the trace kernel's box phases at 1
//   1  producers alternate between init_prio and 0 per group   4  ... box and leaf phases at 1
//   2  producers at 0, trace kernel at 0
// The decision is taken ON THE DEVICE: a launch is enqueued many launches before it runs (hr_render never blocks), so a level put into
// its arguments by the host would be decided from measurements that are tens of launches old — or, inside one long hr_render call,
// never.  Both kernels stamp their first start and last end into GovDev (s_memrealtime), this one-thread kernel runs behind every trace
// kernel (in the gap in which the trace stream waits for the next seed kernel anyway), and kernels read GovDev::level when they start.
// A launch counts if its seed kernel ran beside the trace kernel of the launch before and its trace kernel beside the seed kernel of
// the launch after (the first and last launches of a burst do not).  An untried neighbouring level is tried when the balance asks for
// it (one kernel more than 1.5 % behind the other), otherwise the level with the best smoothed max(seed, trace) wins.
static const int GOV_LEVELS = 5;
__global__ void governor_kernel(GovDev *g, uint32_t slot) {
    typedef unsigned long long u64t;
    const uint32_t other = slot ^ 1u;
    const u64t none = ~0ull;
    const u64t s0 = g->t0[0][slot], s1 = g->t1[0][slot], r0 = g->t0[1][slot], r1 = g->t1[1][slot];
    const bool have = s0 != none && s1 > s0 && r0 != none && r1 > r0;
    if (have && g->fixed < 0) {
        const u64t p0 = g->prev_t0, p1 = g->prev_t1;
        // the next launch's seed kernel: running (its waves are updating these stamps with atomicMin / atomicMax right now; n1 not final) or done
        const u64t n0 = __hip_atomic_load(&g->t0[0][other], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), n1 = __hip_atomic_load(&g->t1[0][other], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        float ov_seed = 0.0f, ov_trace = 0.0f;
        if (p1 > p0) {
            const u64t lo = p0 > s0 ? p0 : s0, hi = p1 < s1 ? p1 : s1;
            if (hi > lo) ov_seed = (float)(hi - lo) / (float)(s1 - s0);
        }
        if (n0 != none && n0 < r1) {
            const u64t lo = n0 > r0 ? n0 : r0, hi = (n1 > n0 && n1 < r1) ? n1 : r1;
            if (hi > lo) ov_trace = (float)(hi - lo) / (float)(r1 - r0);
        }
        const int L = (int)g->lvl[0][slot];
        const float seed_t = (float)(s1 - s0), trace_t = (float)(r1 - r0), m = seed_t > trace_t ? seed_t : trace_t;
        // (a trace kernel that takes much longer than a seed kernel can never have one beside it for 70 % of its time — rtcamp6_v2 / _v1: 48 and
        // 38 ms against 26 — and is the slower kernel beyond doubt: such launches count too.  Until round 4 they did not, and the governor sat
        // at level 0, the wrong end, on exactly the scenes where the trace kernel needs the slots: +2.5 % there.)
        const bool beside = ov_trace > 0.7f || trace_t > 1.25f * seed_t;
        // The wave budget comes first.  While the trace kernel is the faster kernel of the pair at level 0, workgroups it can do without are
        // taken away (one step per judged launch, down to budget_lo), and given back step by step as soon as it comes within 3 % of the
        // seed kernel; the priority levels only come into play with every workgroup in place.  Measured on the headline (1080p,
        // 256 CUs; trace / seed ms per launch): all 1,536 workgroups 19.4 / 25.3, 896 20.6 / 24.7, 768 22.0 / 24.4, 704 23.3 / 24.3,
        // 640 24.5 / 24.3 — the seed kernel gains what the trace kernel's waves no longer take, +3.5 % on the pair at 704 - 768.
        const uint32_t B = g->bud[slot] ? g->bud[slot] - 1u : ~0u;   // what every workgroup of the judged launch obeyed (stored + 1; unset: no trace kernel stamped it)
        // (a trace kernel far shorter than the seed kernel — the sphere scenes: 6 ms against 24 — never covers 70 % of a seed kernel, but that it
        // has workgroups to spare is beyond doubt: it is judged for the budget when it ran beside the next launch's seed kernel itself)
        const bool spare = trace_t < 0.7f * seed_t && ov_trace > 0.7f;
        if ((ov_seed > 0.7f || spare) && beside && L == (int)g->lvl[1][slot] && L >= 0 && L < GOV_LEVELS) {
            g->decisions++;
            bool budget_moved = false;
            if (L == 0 && g->level == 0 && B == g->budget && g->budget_step) {
                const uint32_t nb = gov_budget_next(B, trace_t / seed_t, g->budget_lo, g->budget_hi, g->budget_step, g->thr_down, g->thr_up);
                if (nb != B) {
                    budget_moved = true;
                    g->budget_moves++;
                    __hip_atomic_store(&g->budget, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (int k = 0; k < GOV_LEVELS; k++) g->known[k] = 0;   // another balance: what the levels were worth is to be learnt again
                }
            }
            if (!budget_moved && B == 0 && g->budget == 0) {
                g->known[L] = g->known[L] > 0 ? 0.5f * (g->known[L] + m) : m;
                if (L == g->level) {   // (a launch that started before the last change of level: noted, nothing decided from it)
                    int next = L;
                    if (trace_t > 1.015f * seed_t && L < GOV_LEVELS - 1 && g->known[L + 1] == 0) next = L + 1;
                    else if (seed_t > 1.015f * trace_t && L > 0 && g->known[L - 1] == 0) next = L - 1;
                    else
                        for (int k = 0; k < GOV_LEVELS; k++)
                            if (g->known[k] > 0 && g->known[k] < 0.995f * g->known[next]) next = k;
                    if (next != L) { g->moves++; __hip_atomic_store(&g->level, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                }
            }
        }
    }
    if (r0 != none && r1 > r0) { g->prev_t0 = r0; g->prev_t1 = r1; }
    for (int k = 0; k < 2; k++) { g->t0[k][slot] = none; g->t1[k][slot] = 0; }
    g->bud[slot] = 0;   // unset: the next launch in this slot fixes its own
    if (g->fixed >= 0) __hip_atomic_store(&g->level, g->fixed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// What options precise_shading / trace_mode mean for the scene in place.  Precise shading has two homes that render the same bits
// (path_advance<.., PREC> in the megakernel at 128 VGPRs; the split pipeline's shading kernel), so which one runs is a question of speed only:
// the megakernel form costs 1.9 - 3.7 % on scenes without meshes (the trace side stays hidden behind the seed kernel), on every mesh scene the
// split form is the faster one (7 - 30 % below fp32 shading; profiles/r06_precise_pipelines.txt).  AUTOMATIC precise shading: on for scenes
// without triangle meshes — small spheres are what multiplies an fp32 ray's error, and there it costs little —, off where it costs.
static void resolve_modes(hr_ctx *c) {
    const bool has_scene = c->have_scene;
    const uint32_t tris = has_scene ? c->dsc.num_tris : 0u;
    c->precise = c->precise_opt == 1 || (c->precise_opt < 0 && has_scene && tris == 0u && !c->rr_start);
    c->trace_mode = c->trace_mode_opt >= 0 ? c->trace_mode_opt : (c->precise && tris > 0u ? 1 : 0);
}
// a new scene, resolution or option: the balance of the two kernels is another one.  The governor starts at level 0 — next to a trace
// kernel that needs 16 ms per 33 M paths on the reference's scenes the seed kernel (24 ms) is the slower one almost everywhere.
// (Callers have synchronised the context: no kernel is stamping.)
static int govern_reset(hr_ctx *c) {
    resolve_modes(c);
    if (!c->gov) return HR_OK;
    GovDev h;
    memset(&h, 0, sizeof h);
    for (int k = 0; k < 2; k++)
        for (int sl = 0; sl < 2; sl++) h.t0[k][sl] = ~0ull;
    h.fixed = c->trace_boost;
    h.level = c->trace_boost >= 0 ? c->trace_boost : 0;
    // the wave budget is governed with the level (a fixed level pins it at "all"): 2.5 .. 3.5 workgroups per CU in steps of a quarter
    if (c->trace_boost < 0) { h.budget_step = (uint32_t)c->num_cus / 4u; h.budget_lo = (uint32_t)c->num_cus * 5u / 2u; h.budget_hi = (uint32_t)c->num_cus * 7u / 2u; }
    h.thr_down = 0.88f; h.thr_up = 0.97f;
    if (c->trace_mode == 1 && !c->rr_start && c->trace_boost < 0) {   // (the roulette estimator lives in the megakernel: plan_launch)
        // the split pipeline's traversal kernel: 3 .. 7 workgroups of four 64-VGPR waves per CU in steps of a half, "all" = 8 (device_scene.h gov_budget_next)
        h.budget_step = (uint32_t)c->num_cus / 2u; h.budget_lo = (uint32_t)c->num_cus * 3u; h.budget_hi = (uint32_t)c->num_cus * 7u;
        h.thr_down = 0.96f; h.thr_up = 1.02f;
    }
    HIP_TRY(hipMemcpy(c->gov, &h, sizeof h, hipMemcpyHostToDevice));
    return HR_OK;
}
// `sources` of `c` are about to change: every derived image made of one of them is stale, and with the accumulator the totals
// that include it — its own and, in a same-device group, its peers'
static void changed(hr_ctx *c, uint32_t sources) {
    if (sources & SRC_ACCUM) {
        c->total_valid = false;
        for (hr_ctx *p : c->same_device_peers) p->total_valid = false;
    }
    for (uint32_t &made_of : c->made_of) if (made_of & sources) made_of = 0;
}
static int drain_events(hr_ctx *c) {
    auto sum = [](std::vector<EventPair> &ev, double &acc) -> hipError_t {
        // a pair whose query fails is dropped with the rest (left in the list it would fail every later drain, i.e. every later API call)
        hipError_t first = hipSuccess;
        for (auto &e : ev) {
            float ms = 0;
            hipError_t r = hipEventElapsedTime(&ms, e.a, e.b);
            if (r == hipSuccess) acc += ms;
            else if (first == hipSuccess) first = r;
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
        ev.clear();
        return first;
    };
    HIP_TRY(sum(c->seed_events, c->seed_ms));
    HIP_TRY(sum(c->trace_events, c->trace_ms));
    HIP_TRY(sum(c->post_events, c->post_ms));
    HIP_TRY(sum(c->debug_events, c->debug_ms));
    return HR_OK;
}
// Long renders: retire the event pairs of launches that have finished (both kernels), oldest first, without waiting for anything —
// the lists stay a few launches long however many samplings one hr_render call covers, and no drain ever has to stop the pipeline.
static void retire_finished_launches(hr_ctx *c) {
    size_t n = 0;
    const size_t limit = std::min(c->seed_events.size(), c->trace_events.size());
    while (n < limit && hipEventQuery(c->seed_events[n].b) == hipSuccess && hipEventQuery(c->trace_events[n].b) == hipSuccess) n++;
    if (n > 2) n -= 2; else return;
    for (size_t i = 0; i < n; i++) {
        float sm = 0, tm = 0;
        if (hipEventElapsedTime(&sm, c->seed_events[i].a, c->seed_events[i].b) == hipSuccess) c->seed_ms += sm;
        if (hipEventElapsedTime(&tm, c->trace_events[i].a, c->trace_events[i].b) == hipSuccess) c->trace_ms += tm;
        (void)hipEventDestroy(c->seed_events[i].a); (void)hipEventDestroy(c->seed_events[i].b);
        (void)hipEventDestroy(c->trace_events[i].a); (void)hipEventDestroy(c->trace_events[i].b);
    }
    c->seed_events.erase(c->seed_events.begin(), c->seed_events.begin() + (long)n);
    c->trace_events.erase(c->trace_events.begin(), c->trace_events.begin() + (long)n);
}
static int sync_all(hr_ctx *c) {
    HIP_TRY(hipStreamSynchronize(c->seed_stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->trace_pending[0] = c->trace_pending[1] = false;
    c->seed_pending[0] = c->seed_pending[1] = false;
    for (auto &m : c->markers) (void)hipEventDestroy(m.second);
    c->markers.clear();
    return drain_events(c);
}
// A timed launch: timed_begin / timed_end bracket what a caller enqueues on `st` with an event pair that the drains above sum into the
// context's times.  A pair goes into its list (and its launch is counted) only when both events were really recorded; anything less is
// destroyed on the spot, so no drain ever queries an event that was not recorded.  timed_end is handed what the launch itself returned
// and passes the first error on.
static void drop_pair(EventPair &ev) {
    if (ev.a) (void)hipEventDestroy(ev.a);
    if (ev.b) (void)hipEventDestroy(ev.b);
    ev = EventPair{nullptr, nullptr};
}
static hipError_t timed_begin(EventPair &ev, hipStream_t st) {
    ev = EventPair{nullptr, nullptr};
    hipError_t e = hipEventCreate(&ev.a);
    if (e == hipSuccess) e = hipEventCreate(&ev.b);
    if (e == hipSuccess) e = hipEventRecord(ev.a, st);
    if (e != hipSuccess) drop_pair(ev);
    return e;
}
static hipError_t timed_end(hipError_t launched, EventPair &ev, hipStream_t st, std::vector<EventPair> &list, uint64_t *launches = nullptr) {
    hipError_t e = launched;
    if (e == hipSuccess && ev.a) e = hipEventRecord(ev.b, st);
    if (e != hipSuccess || !ev.a) { drop_pair(ev); return e; }
    list.push_back(ev);
    if (launches) ++*launches;
    return hipSuccess;
}
// an event pair for the duration of one call (the device BVH build's)
struct CallEvents : EventPair {
    CallEvents() : EventPair{nullptr, nullptr} {}
    CallEvents(const CallEvents &) = delete;
    CallEvents &operator=(const CallEvents &) = delete;
    ~CallEvents() { drop_pair(*this); }
};

// `c` leaves its same-device group (hr_comm_init_local over one device): the group is over for its peers too
static void reset_same_device_peers(hr_ctx *c) {
    for (hr_ctx *p : c->same_device_peers) if (p != c) { p->same_device_peers.clear(); p->comm_world = 0; p->total_valid = false; p->comm_path = HR_COMM_NONE; p->allreduces = 0; }
}
// The tile mask's device buffers and what the selection and the counts' check work in.  All four are allocated by whoever needs them first
// (mask_buffers, select_out_buffer, hr_select_tiles) and released here, by remove_mask and hr_destroy.
static int free_mask_buffers(hr_ctx *c) {
    c->select_tmp_bytes = 0;
    for (uint32_t **p : {&c->d_tile_list, &c->d_tile_flags, &c->d_select_out}) { int rc = free_device(*p); if (rc) return rc; }
    return free_device(c->select_tmp);
}

// ------------------------------------------------------------------------------------------ region planes
// A plane is a device buffer of RW x RH x comps elements of one type: the accumulator and everything that has its shape.  This table is the one
// place that says what each plane holds; the routines below are the one place that turns it into bytes, and set_target / hr_clear / hr_destroy
// walk it.  Life cycles:
//   WITH_TARGET   allocated by set_target for every target
//   WITH_OPTION   allocated while the option `on` is on: when it is switched on, and by set_target while it is on; gone when it is switched off
//   ON_FIRST_USE  allocated by the first call that needs it (accum_total: the first all-reduce; noise_img: the first estimate; guides: the first
//                 hr_render_guides / hr_write_guides; denoised: the first hr_denoise; robust, robust_trim: the first hr_robust; robust_noise_img,
//                 robust_noise_trim: the first robust noise estimate; restored: the first hr_robust_restore; selected, selected_levels: the first
//                 hr_denoise_select; motion: the first hr_write_motion), freed by set_target —
//                 noise_img also with the moments it is made of, guides also by hr_upload_scene (they show the scene), robust, robust_trim
//                 and the robust noise planes also with the buckets they are made of
// at_alloc: zeroed when allocated.  at_clear: zeroed by hr_clear.  n: the count that belongs to the plane's contents and is zeroed with them.
// per: a plane whose components are `comps` times a number the context holds (the sample buckets: 3 per bucket, K buckets).
enum PlaneLife { WITH_TARGET, WITH_OPTION, ON_FIRST_USE };
struct Plane {
    void **(*slot)(hr_ctx *);
    size_t elem;
    uint32_t comps;
    PlaneLife life;
    bool at_alloc, at_clear;
    const char *option = nullptr;       // WITH_OPTION: the key of hr_set_option
    bool hr_ctx::*on = nullptr;
    uint64_t hr_ctx::*n = nullptr;
    uint32_t hr_ctx::*per = nullptr;
};
#define PLANE_SLOT(member) [](hr_ctx *c) -> void ** { return (void **)&c->member; }
static const Plane ACCUM_OWN{PLANE_SLOT(accum_own), sizeof(float), 3, WITH_TARGET, true, true};   // hr_clear zeroes c->accum: this plane, or the caller's bound buffer of its size
static const Plane POST_TMP{PLANE_SLOT(post_tmp), sizeof(float), 3, WITH_TARGET, false, false};
static const Plane RGB8{PLANE_SLOT(d_rgb8), sizeof(uint8_t), 3, WITH_TARGET, false, false};
static const Plane ACCUM_TOTAL{PLANE_SLOT(accum_total), sizeof(float), 3, ON_FIRST_USE, false, false};
static const Plane MOMENTS{PLANE_SLOT(moments), sizeof(double), 6, WITH_OPTION, true, true, "moments", &hr_ctx::moments_on, &hr_ctx::moments_n};
static const Plane NOISE_IMG{PLANE_SLOT(noise_img), sizeof(double), 1, ON_FIRST_USE, false, false};
static const Plane COUNTS{PLANE_SLOT(counts), sizeof(uint32_t), 1, WITH_OPTION, true, true, "sample_counts", &hr_ctx::counts_on};
static const Plane GUIDES{PLANE_SLOT(guides), sizeof(float), 8, ON_FIRST_USE, false, false};
static const Plane DENOISED{PLANE_SLOT(denoised), sizeof(float), 3, ON_FIRST_USE, false, false};
static const Plane BUCKETS{PLANE_SLOT(buckets), sizeof(double), 3, WITH_OPTION, true, true, "robust_buckets", &hr_ctx::robust_on, &hr_ctx::buckets_n, &hr_ctx::robust_k};
static const Plane ROBUST{PLANE_SLOT(robust), sizeof(float), 3, ON_FIRST_USE, false, false};
static const Plane ROBUST_TRIM{PLANE_SLOT(robust_trim), sizeof(uint8_t), 1, ON_FIRST_USE, false, false};
static const Plane ROBUST_NOISE_IMG{PLANE_SLOT(robust_noise_img), sizeof(double), 1, ON_FIRST_USE, false, false};
static const Plane ROBUST_NOISE_TRIM{PLANE_SLOT(robust_noise_trim), sizeof(uint8_t), 1, ON_FIRST_USE, false, false};
static const Plane RESTORED{PLANE_SLOT(restored), sizeof(float), 3, ON_FIRST_USE, false, false};
static const Plane SELECTED{PLANE_SLOT(selected), sizeof(float), 3, ON_FIRST_USE, false, false};
static const Plane SELECTED_LEVELS{PLANE_SLOT(selected_levels), sizeof(uint8_t), 1, ON_FIRST_USE, false, false};
static const Plane MOTION{PLANE_SLOT(motion), sizeof(float), 12, ON_FIRST_USE, false, false};
#undef PLANE_SLOT
static const Plane *const PLANES[] = {&ACCUM_OWN, &POST_TMP, &RGB8, &ACCUM_TOTAL, &MOMENTS, &NOISE_IMG, &COUNTS, &GUIDES, &DENOISED, &BUCKETS, &ROBUST, &ROBUST_TRIM, &ROBUST_NOISE_IMG, &ROBUST_NOISE_TRIM, &RESTORED, &SELECTED, &SELECTED_LEVELS, &MOTION};

static size_t region_pixels(const hr_ctx *c) { return (size_t)c->RW * c->RH; }
static size_t plane_elems(const hr_ctx *c, const Plane &p) { return region_pixels(c) * p.comps * (p.per ? c->*p.per : 1u); }
static size_t plane_bytes(const hr_ctx *c, const Plane &p) { return plane_elems(c, p) * p.elem; }
static int plane_free(hr_ctx *c, const Plane &p) {
    if (p.n) c->*p.n = 0;
    return free_device(*p.slot(c));
}
// The plane's contents start over: `dev` (a buffer of the plane's size; default: the plane's own, if there is one) is zeroed on `st`, the count
// that belongs to them with it.  Outside a render that is the null stream, which is waited for: the render streams do not wait for it.
static int plane_zero(hr_ctx *c, const Plane &p, hipStream_t st = nullptr, void *dev = nullptr) {
    if (!dev && !(dev = *p.slot(c))) return HR_OK;
    HIP_TRY(hipMemsetAsync(dev, 0, plane_bytes(c, p), st));
    if (!st) HIP_TRY(hipStreamSynchronize(nullptr));
    if (p.n) c->*p.n = 0;
    return HR_OK;
}
// (re)allocate the plane for the region in force
static int plane_alloc(hr_ctx *c, const Plane &p) {
    int rc = plane_free(c, p);
    if (rc) return rc;
    HIP_TRY(hipMalloc(p.slot(c), plane_bytes(c, p)));
    return p.at_alloc ? plane_zero(c, p) : HR_OK;
}
// Host copies of a buffer of the plane's size.  A read goes through hr_synchronize (which can return the RNG-window error); a write through
// sync_all, and one into the accumulator makes the totals that include it stale.
static int plane_read(hr_ctx *c, const Plane &p, const void *dev, void *host) {
    int rc = hr_synchronize(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(host, dev, plane_bytes(c, p), hipMemcpyDeviceToHost));
    return HR_OK;
}
static int plane_write(hr_ctx *c, const Plane &p, void *dev, const void *host) {
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    // (conservative, kept: a write of one statistics plane counts as a write of all three)
    changed(c, dev == c->guides ? SRC_GUIDES : dev == c->motion ? 0u : (dev == c->accum ? SRC_ACCUM : 0u) | SRC_MOMENTS | SRC_COUNTS | SRC_BUCKETS);   // (nothing is kept that is made of the motion plane)
    HIP_TRY(hipMemcpy(dev, host, plane_bytes(c, p), hipMemcpyHostToDevice));
    return HR_OK;
}
// the plane of an option: refused while the option is off (`who`: the entry point); its host copies ask that first, then for the host's pointer
static int plane_ready(hr_ctx *c, const Plane &p, const char *who) {
    if (!c) return fail(HR_ERR_INVALID, "%s: null ctx", who);
    if (!(c->*p.on) || !*p.slot(c)) return fail(HR_ERR_INVALID, "%s: option %s is off", who, p.option);
    return HR_OK;
}
static int option_plane_read(hr_ctx *c, const Plane &p, const char *who, void *host) {
    int rc = plane_ready(c, p, who);
    if (!rc && !host) rc = fail(HR_ERR_INVALID, "%s: null argument", who);
    return rc ? rc : plane_read(c, p, *p.slot(c), host);
}
static int option_plane_write(hr_ctx *c, const Plane &p, const char *who, const void *host) {
    int rc = plane_ready(c, p, who);
    if (!rc && !host) rc = fail(HR_ERR_INVALID, "%s: null argument", who);
    return rc ? rc : plane_write(c, p, *p.slot(c), host);
}

// ------------------------------------------------------------------------------------------ derived images
// What is made of the planes and kept until one of its sources changes: its plane(s), the sources it goes stale with whoever made
// it — the maker adds what was decided when it was made (hr_ctx::made_of) —, the option its reads ask for first, and what they say when there is
// none.  Every call that changes a source says so to changed(); nothing else clears made_of.  "kept": more than the data flow needs, as it always was.
struct Image {
    const Plane *plane, *second;   // (second: R's trim plane, S's level plane)
    uint32_t stale_with;
    const Plane *option;
    const char *none;
};
static const Image IMAGES[N_IMAGES] = {
    {&GUIDES, nullptr, SRC_GUIDES | SRC_SCENE | SRC_TARGET, nullptr, "no guide planes (hr_render_guides or hr_write_guides first)"},
    // D: + SRC_MOMENTS made by hr_denoise, + SRC_BUCKETS made by hr_denoise_robust (for that one the accumulator is kept)
    {&DENOISED, nullptr, SRC_ACCUM | SRC_COUNTS | SRC_GUIDES | SRC_SCENE | SRC_TARGET | SRC_NEW_D, nullptr, "no denoised image (hr_denoise first; anything that changes its inputs invalidates it)"},
    {&ROBUST, &ROBUST_TRIM, SRC_COUNTS | SRC_BUCKETS | SRC_TARGET, &BUCKETS, "no robust image (hr_robust first; anything that changes its inputs invalidates it)"},
    // R': + SRC_NEW_D made on D (base 1); the accumulator is kept
    {&RESTORED, nullptr, SRC_ACCUM | SRC_COUNTS | SRC_BUCKETS | SRC_GUIDES | SRC_SCENE | SRC_TARGET, nullptr, "no restored image (hr_robust_restore first; anything that changes its inputs invalidates it)"},
    // S and its level plane: neither says nor listens to "a new D"
    {&SELECTED, &SELECTED_LEVELS, SRC_ACCUM | SRC_MOMENTS | SRC_COUNTS | SRC_BUCKETS | SRC_GUIDES | SRC_SCENE | SRC_TARGET, &BUCKETS,
     "no selected image (hr_denoise_select first; anything that changes its inputs invalidates it)"},
    // the motion plane: it relates the view in place to an earlier one
    {&MOTION, nullptr, SRC_SCENE | SRC_TARGET, nullptr, "no motion plane (hr_write_motion first; a new camera, scene or target makes it stale)"},
};
static bool image_valid(const hr_ctx *c, ImageId id) { return c->made_of[id] != 0; }
static void image_made(hr_ctx *c, ImageId id, uint32_t decided = 0) { c->made_of[id] = IMAGES[id].stale_with | decided; }
// the image of an entry point that reads it (`who`): the option first where it has one, then the arguments, then the image itself
static int image_ready(hr_ctx *c, ImageId id, const char *who, const void *host) {
    const Image &im = IMAGES[id];
    int rc;
    if (im.option && (rc = plane_ready(c, *im.option, who))) return rc;
    if (!c || !host) return fail(HR_ERR_INVALID, "%s: null argument", who);
    if (!*im.plane->slot(c) || (im.second && !*im.second->slot(c)) || !image_valid(c, id)) return fail(HR_ERR_INVALID, "%s: %s", who, im.none);
    return HR_OK;
}
// the host copy of the image's plane (second: of its second plane) behind hr_read_*; image_resolve (behind resolve_region) is hr_resolve_*'s
static int image_read(hr_ctx *c, ImageId id, const char *who, void *host, bool second = false) {
    const Plane &p = second ? *IMAGES[id].second : *IMAGES[id].plane;
    int rc = image_ready(c, id, who, host);
    return rc ? rc : plane_read(c, p, *p.slot(c), host);
}
// the guide planes of a call that filters along them: the valid ones, or the ones it renders now
static int guides_or_render(hr_ctx *c) { return image_valid(c, GUIDE_IMAGE) ? HR_OK : hr_render_guides(c); }
// a bucket count K without a row in `kernel`'s table (`who`: the entry point)
static int no_instantiation(const char *who, const char *kernel, uint32_t K) {
    return fail(HR_ERR_UNSUPPORTED, "%s: no %s instantiation for %u buckets (kernel_variants.h)", who, kernel, K);
}

// ------------------------------------------------------------------------------------------ C ABI

static int create_resources(hr_ctx *c);

const char *hr_last_error(void) { return g_err.c_str(); }
int hr_abi_version(void) { return HR_ABI_VERSION; }

int hr_create(int device_id, hr_ctx **out) {
    if (!out) return fail(HR_ERR_INVALID, "hr_create: out is null");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) return fail(HR_ERR_INVALID, "hr_create: device %d not in [0,%d)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    hr_ctx *c = new hr_ctx;
    c->device = device_id;
    int rc = create_resources(c);
    if (rc) { (void)hr_destroy(c); return rc; }
    *out = c;
    return HR_OK;
}

static int create_resources(hr_ctx *c) {
    const int device_id = c->device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c->seed_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    for (int i = 0; i < 2; i++) {
        HIP_TRY(hipEventCreateWithFlags(&c->seed_done[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->trace_done[i], hipEventDisableTiming));
    }
    HIP_TRY(hipMalloc((void **)&c->d_counters, sizeof(Counters)));
    HIP_TRY(hipMemset(c->d_counters, 0, sizeof(Counters)));
    HIP_TRY(hipMalloc((void **)&c->d_tile_counter, 2 * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&c->gov, sizeof(GovDev)));
    { int grc = govern_reset(c); if (grc) return grc; }
    for (const SeedVariant &v : SEED_VARIANTS) HIP_TRY(hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEED_LDS_BYTES));
    for (const RobustNoiseVariant &v : ROBUST_NOISE_VARIANTS) if (v.lds()) HIP_TRY(hipFuncSetAttribute((const void *)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds()));
    for (const RobustVariant &v : ROBUST_VARIANTS) HIP_TRY(hipFuncSetAttribute((const void *)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds()));
    for (const RobustDenoiseInitVariant &v : ROBUST_DENOISE_INIT_VARIANTS) HIP_TRY(hipFuncSetAttribute((const void *)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds()));
    for (const RestoreInitVariant &v : RESTORE_INIT_VARIANTS) HIP_TRY(hipFuncSetAttribute((const void *)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds()));
    for (const SelectInitVariant &v : SELECT_INIT_VARIANTS) HIP_TRY(hipFuncSetAttribute((const void *)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds()));
    HIP_TRY(hipFuncSetAttribute((const void *)seed_debug_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * 64 * 8));
    // The seed kernel owns all 160 KiB of a CU's LDS and runs next to the trace side of the previous batch: a trace-side kernel that
    // uses ANY LDS (the compiler promotes small private arrays to LDS unless told not to, see the Makefile) could not share a CU
    // with it — the two would silently run one after the other, 40 % slower.  Refuse to start in that state.  Every instantiation a
    // launch can select is a row of these tables (kernel_variants.h).
    {
        std::vector<const void *> beside_seed;
        for (const TraceVariant &v : TRACE_VARIANTS) beside_seed.push_back((const void *)v.fn);
        for (const WfStartVariant &v : WF_START_VARIANTS) beside_seed.push_back((const void *)v.fn);
        for (const WfTraverseVariant &v : WF_TRAVERSE_VARIANTS) beside_seed.push_back((const void *)v.fn);
        for (const WfShadeVariant &v : WF_SHADE_VARIANTS) beside_seed.push_back((const void *)v.fn);
        for (const MotionVariant &v : MOTION_VARIANTS) beside_seed.push_back((const void *)v.fn);   // (a frame's motion pass may be enqueued behind the frame before's render)
        for (const void *f : beside_seed) {
            hipFuncAttributes fa;
            HIP_TRY(hipFuncGetAttributes(&fa, f));
            if (fa.sharedSizeBytes != 0) return fail(HR_ERR_DEVICE, "build error: a trace kernel variant uses %zu bytes of LDS (it must use none to run beside the seed kernel)", (size_t)fa.sharedSizeBytes);
        }
    }
    HIP_TRY(hipMalloc((void **)&c->ovf_win, (size_t)c->num_cus * 2 * SEED_WIN_WORDS * sizeof(u64)));
    return HR_OK;
}

int hr_destroy(hr_ctx *c) {
    if (!c) return HR_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    unbind_accumulator(c);
    free_scene(c);
    for (auto *ev : {&c->seed_events, &c->trace_events, &c->post_events, &c->debug_events})
        for (auto &e : *ev) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &m : c->markers) (void)hipEventDestroy(m.second);
    for (const Plane *p : PLANES) (void)plane_free(c, *p);
    (void)free_mask_buffers(c);
    for (int i = 0; i < 2; i++) {
        if (c->seed_done[i]) (void)hipEventDestroy(c->seed_done[i]);
        if (c->trace_done[i]) (void)hipEventDestroy(c->trace_done[i]);
    }
    for (void *p : {(void *)c->recs[0], (void *)c->recs[1], (void *)c->ring, c->wf_block, (void *)c->ovf, (void *)c->ovf_win, (void *)c->d_counters, (void *)c->d_tile_counter, (void *)c->gov})
        if (p) (void)hipFree(p);
    if (c->comm && hrcomm::api().CommDestroy) (void)hrcomm::api().CommDestroy(c->comm);
    reset_same_device_peers(c);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->seed_stream) (void)hipStreamDestroy(c->seed_stream);
    delete c;
    return HR_OK;
}

// Device builders (option bvh_builder = 1 LBVH, 2 PLOC; gpu_bvh.h): the primitive arrays were uploaded in input order; split long
// thin triangles into references (early split clipping), build the tree over them, emit it in both record formats (16-byte quantised
// records in per-octant near-first preorder — what the trace kernel walks — and the 32-byte fp32 records), re-store the primitives
// in leaf order and point the scene at the results.  The scratch and the event pair live for the call (CallScratch, CallEvents).
static int build_bvh_on_device(hr_ctx *c, const HostScene &hs, const Tri *tris_in) {
    using namespace lbvh;
    Scene &d = c->dsc;
    Prims p{};
    p.tris = tris_in; p.num_tris = d.num_tris; p.spheres = d.spheres; p.num_spheres = d.num_spheres; p.cuboids = d.cuboids; p.num_cuboids = d.num_cuboids;
    p.ref_tri = nullptr; p.ref_box = nullptr;
    double scene_sa = 0.0;
    for (int a = 0; a < 3; a++) {
        double ext = hs.scene_max[a] - hs.scene_min[a];
        p.smin[a] = (float)hs.scene_min[a];
        p.sinv[a] = ext > 0 ? (float)(1.0 / ext) : 0.0f;
    }
    {
        const double e0 = hs.scene_max[0] - hs.scene_min[0], e1 = hs.scene_max[1] - hs.scene_min[1], e2 = hs.scene_max[2] - hs.scene_min[2];
        if (e0 >= 0 && e1 >= 0 && e2 >= 0) scene_sa = 2.0 * (e0 * e1 + e1 * e2 + e2 * e0);
    }
    CallScratch scratch;
    CallEvents ev;   // around everything the build puts on the stream
    auto alloc = [&](size_t bytes, bool keep) -> void * {
        void *q = nullptr;
        if (keep) { if (hipMalloc(&q, std::max<size_t>(bytes, 16)) == hipSuccess) c->scene_allocs.push_back(q); }
        else (void)scratch.alloc(&q, std::max<size_t>(bytes, 16));
        return q;
    };
#define LBVH_ALLOC(var, type, count, keep)                                                                        \
    type *var = (type *)alloc(sizeof(type) * (size_t)(count), keep);                                                \
    if (!var) return fail(HR_ERR_DEVICE, "hr_upload_scene: out of device memory in the BVH build");
    (void)timed_begin(ev, c->stream);   // (best effort: without the pair the build goes on and reports 0 ms)
    // Early split clipping on the device (option split_ratio: -1 = on with the host builder's automatic ratio of 2, 0 = off, > 0 = that
    // ratio; the host builder's automatic mode also builds the unsplit tree and keeps the better one, the device always keeps the split):
    // pieces per triangle, a scan, then the pieces' boxes and owners.  The builders below then see one primitive per piece.
    if (c->split_ratio != 0.0 && d.num_tris > 0) {
        SplitParams sp{c->split_ratio < 0 ? 2.0 : c->split_ratio, 1e-4 * scene_sa, SPLIT_MAX_DEPTH};
        const uint32_t nt = d.num_tris;
        LBVH_ALLOC(split_counts, uint32_t, nt, false)
        LBVH_ALLOC(split_offsets, uint32_t, nt, false)
        size_t sbytes = 0;
        HIP_TRY_AS("device split clipping", hipcub::DeviceScan::ExclusiveSum(nullptr, sbytes, split_counts, split_offsets, (int)nt, c->stream));
        LBVH_ALLOC(split_tmp, unsigned char, sbytes, false)
        split_count_kernel<<<(nt + 127) / 128, 128, 0, c->stream>>>(tris_in, nt, sp, split_counts);
        HIP_TRY_AS("device split clipping", hipcub::DeviceScan::ExclusiveSum(split_tmp, sbytes, split_counts, split_offsets, (int)nt, c->stream));
        uint32_t last[2] = {0, 0};
        HIP_TRY_AS("device split clipping", hipMemcpyAsync(&last[0], split_offsets + (nt - 1), 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY_AS("device split clipping", hipMemcpyAsync(&last[1], split_counts + (nt - 1), 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY_AS("device split clipping", hipStreamSynchronize(c->stream));
        const uint64_t refs = (uint64_t)last[0] + last[1];
        // (bounded together with the spheres and cuboids: the builder's n = refs + spheres + cuboids indexes its sort keys and INFO_COUNT with
        // 24 bits; beyond that the split references are dropped and the triangles go in as they are)
        if (refs > nt && refs + p.num_spheres + p.num_cuboids < MAX_PRIMS_PER_TYPE) {
            LBVH_ALLOC(ref_tri, uint32_t, refs, false)
            LBVH_ALLOC(ref_box, float, 6 * refs, false)
            split_emit_kernel<<<(nt + 127) / 128, 128, 0, c->stream>>>(tris_in, nt, sp, split_offsets, ref_tri, ref_box);
            p.ref_tri = ref_tri; p.ref_box = ref_box; p.num_tris = (uint32_t)refs;
        }
    }
    const int n = (int)(p.num_tris + p.num_spheres + p.num_cuboids);
    p.index_bits = key_index_bits_for((uint64_t)n);
    if (n <= 0 || (uint64_t)n >= (1ull << p.index_bits)) return fail(HR_ERR_UNSUPPORTED, "device BVH build: %d primitives do not fit the %d index bits of the sort keys", n, p.index_bits);
    const int N = 2 * n - 1;
    LBVH_ALLOC(keys_in, mkey_t, n, false)
    LBVH_ALLOC(keys, mkey_t, n, false)
    Work w{};
    LBVH_ALLOC(parent, uint32_t, N, false) LBVH_ALLOC(left, uint32_t, n, false) LBVH_ALLOC(right, uint32_t, n, false)
    LBVH_ALLOC(flags, uint32_t, n, false)
    LBVH_ALLOC(bmin, float, 3 * (size_t)N, false) LBVH_ALLOC(bmax, float, 3 * (size_t)N, false)
    LBVH_ALLOC(info, uint32_t, N, false) LBVH_ALLOC(tc, u64t, N, false) LBVH_ALLOC(size, uint32_t, N, false)
    LBVH_ALLOC(word, uint32_t, N, false) LBVH_ALLOC(axis_low, uint32_t, n, false)
    LBVH_ALLOC(prim_pos, uint32_t, n, false) LBVH_ALLOC(cl_a, uint32_t, n, false) LBVH_ALLOC(cl_b, uint32_t, n, false) LBVH_ALLOC(nn, uint32_t, n, false)
    LBVH_ALLOC(frame, float, 8, false)
    w.parent = parent; w.left = left; w.right = right; w.flags = flags;
    w.bmin = bmin; w.bmax = bmax; w.info = info; w.tc = tc; w.size = size; w.axis_low = axis_low; w.word = word;
    // the emitted tree has size[root] <= 2n-1 records per octant (collapsed subtrees are one record): sized for the worst case
    LBVH_ALLOC(nodes, Node, 8 * (size_t)N + 1, true)
    LBVH_ALLOC(qnodes, QNode, 8 * ((size_t)N + 1), true)
    LBVH_ALLOC(tris, TriT, p.num_tris, true)
    LBVH_ALLOC(tri_shade, TriS, p.num_tris, true)
    LBVH_ALLOC(tri_face, uint32_t, p.num_tris, true)
    LBVH_ALLOC(spheres, f4, d.num_spheres, true)
    LBVH_ALLOC(sphere_elem, int32_t, d.num_spheres, true)
    LBVH_ALLOC(sphere_lo, f4, d.num_spheres, true)
    LBVH_ALLOC(cuboids, f4, 2 * (size_t)d.num_cuboids, true)
    size_t sort_bytes = 0;
    HIP_TRY_AS("hipcub sort (size query)", hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, keys_in, keys, n, 0, 64, c->stream));
    LBVH_ALLOC(sort_tmp, unsigned char, sort_bytes, false)
    // multi-workgroup PLOC: packed role counters, their scan, the two-slot iteration state
    const bool ploc_multi = c->builder_in_use == 2 && n > 1;
    size_t scan_bytes = 0;
    if (ploc_multi) HIP_TRY_AS("hipcub scan (size query)", hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (u64t *)nullptr, (u64t *)nullptr, n, c->stream));
    LBVH_ALLOC(ploc_flags, u64t, ploc_multi ? n : 1, false)
    LBVH_ALLOC(ploc_pos, u64t, ploc_multi ? n : 1, false)
    LBVH_ALLOC(scan_tmp, unsigned char, scan_bytes, false)
    LBVH_ALLOC(ploc_state, PlocState, 2, false)
    const int T = 256;
    hipStream_t st = c->stream;
    static const char *const who = "device BVH build";
    HIP_TRY_AS(who, hipMemsetAsync(flags, 0, sizeof(uint32_t) * (size_t)n, st));
    HIP_TRY_AS(who, hipMemsetAsync(parent, 0xff, sizeof(uint32_t) * (size_t)N, st));   // n == 1: the lone leaf is the root
    key_kernel<<<(n + T - 1) / T, T, 0, st>>>(p, n, keys_in);
    HIP_TRY_AS(who, hipcub::DeviceRadixSort::SortKeys(sort_tmp, sort_bytes, keys_in, keys, n, 0, 64, st));
    leaf_kernel<<<(n + T - 1) / T, T, 0, st>>>(p, keys, n, w);
    if (n > 1 && c->builder_in_use == 1) hierarchy_kernel<<<(n - 1 + T - 1) / T, T, 0, st>>>(keys, n, w);
    if (ploc_multi) {
        ploc_init_kernel<<<(n + T - 1) / T, T, 0, st>>>(n, cl_a, ploc_state);
        uint32_t *cur = cl_a, *nxt = cl_b;
        // (the loop's control — the read-back cadence, the end, the stall rule — is lbvh_core.h's PlocLoop, shared with the emulation)
        PlocLoop loop = ploc_loop_begin((uint32_t)n, c->ploc_top);
        while (ploc_loop_more(loop)) {
            const uint32_t g = (loop.m_known + T - 1) / T, it = loop.its;
            const PlocState *sin = ploc_state + (it & 1);
            ploc_nn_kernel<<<g, T, 0, st>>>(w, cur, nn, sin);
            ploc_role_kernel<<<g, T, 0, st>>>(nn, ploc_flags, loop.m_known, sin);
            HIP_TRY_AS(who, hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, ploc_flags, ploc_pos, (int)loop.m_known, st));
            ploc_merge_kernel<<<g, T, 0, st>>>(w, cur, nxt, nn, ploc_flags, ploc_pos, sin, ploc_state + ((it + 1) & 1));
            std::swap(cur, nxt);
            if (ploc_loop_launched(loop)) {   // how many are left?
                PlocState hs{};
                HIP_TRY_AS(who, hipMemcpyAsync(&hs, ploc_state + ((it + 1) & 1), sizeof hs, hipMemcpyDeviceToHost, st));
                HIP_TRY_AS(who, hipStreamSynchronize(st));
                if (hs.m == 0u || hs.m > loop.m_known) return fail(HR_ERR_DEVICE, "device BVH build: implausible cluster count %u after %u of %d", hs.m, loop.m_known, n);
                ploc_loop_read(loop, hs.m);
            }
        }
        const uint32_t m_known = loop.m_known;   // exact: the loop ends on a read-back
        // the top of the tree: binned SAH over the clusters that are left, on the host (a few thousand boxes)
        if (m_known > 1u) {
            const uint32_t m = m_known;
            std::vector<float> hb(6 * (size_t)m);
            std::vector<uint32_t> hc(m);
            // (sized here, by what is left: <= ploc_top clusters as a rule, up to n of them when the merges stalled)
            LBVH_ALLOC(top_boxes, float, 6 * (size_t)m, false)
            LBVH_ALLOC(top_counts, uint32_t, m, false)
            LBVH_ALLOC(top_left, int32_t, m, false)
            LBVH_ALLOC(top_right, int32_t, m, false)
            ploc_top_gather_kernel<<<(m + T - 1) / T, T, 0, st>>>(w, cur, m, top_boxes, top_counts);
            HIP_TRY_AS(who, hipMemcpyAsync(hb.data(), top_boxes, hb.size() * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_TRY_AS(who, hipMemcpyAsync(hc.data(), top_counts, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY_AS(who, hipStreamSynchronize(st));
            std::vector<int32_t> tl, tr;
            build_top_tree(hb.data(), hc.data(), m, tl, tr);
            if (tl.size() != (size_t)m - 1) return fail(HR_ERR_DEVICE, "device BVH build: the top-down build made %zu inner nodes over %u clusters", tl.size(), m);
            HIP_TRY_AS(who, hipMemcpyAsync(top_left, tl.data(), tl.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_TRY_AS(who, hipMemcpyAsync(top_right, tr.data(), tr.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
            ploc_top_apply_kernel<<<(m - 1 + T - 1) / T, T, 0, st>>>(w, m - 1, top_left, top_right, cur);
            HIP_TRY_AS(who, hipStreamSynchronize(st));   // tl / tr are host vectors about to go out of scope
        }
    }
#undef LBVH_ALLOC
    fit_kernel<<<(n + T - 1) / T, T, 0, st>>>(n, (uint32_t)c->max_leaf, w);
    finish_kernel<<<(N + T - 1) / T, T, 0, st>>>(p, n, w, prim_pos);
    frame_kernel<<<1, 64, 0, st>>>(w, frame);
    emit_kernel<<<(8 * N + T - 1) / T, T, 0, st>>>(n, w, frame, nodes, qnodes);
    gather_kernel<<<(n + T - 1) / T, T, 0, st>>>(p, keys, prim_pos, n, tris, tri_shade, tri_face, spheres, sphere_elem, d.sphere_elem, sphere_lo, d.sphere_lo, cuboids);
    HIP_TRY_AS(who, hipGetLastError());
    if (ev.b) (void)hipEventRecord(ev.b, st);
    float hframe[8] = {0, 0, 0, 1, 1, 1, 0, 0};
    HIP_TRY_AS(who, hipMemcpyAsync(hframe, frame, sizeof hframe, hipMemcpyDeviceToHost, st));
    HIP_TRY_AS(who, hipStreamSynchronize(st));
    float ms = 0;
    if (ev.b) (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    uint32_t total = 0;
    memcpy(&total, &hframe[6], sizeof total);
    if (total == 0 || total > (uint32_t)N) return fail(HR_ERR_DEVICE, "device BVH build: implausible record count %u for %d primitives", total, n);
    if (c->quant_nodes && (uint64_t)(total + 1u) * 8u * sizeof(QNode) >= (1ull << 31)) return fail(HR_ERR_UNSUPPORTED, "device BVH build: %u records per octant exceed the 2^31-byte offset range of the quantised records (set quant_nodes = 0)", total);
    c->bvh_build_ms = ms;
    d.nodes = nodes; d.num_nodes = total;
    d.qnodes = c->quant_nodes ? qnodes : nullptr;
    for (int a = 0; a < 3; a++) { d.qmin[a] = hframe[a]; d.qstep[a] = hframe[3 + a]; }

    d.tris = tris; d.tri_shade = tri_shade; d.tri_face = tri_face; d.spheres = spheres; d.sphere_elem = sphere_elem; d.sphere_lo = sphere_lo; d.cuboids = cuboids;   // the input-order copies stay in scene_allocs until the next upload
    d.num_tris = p.num_tris;   // leaf-ordered records: one per reference (a split triangle appears once per piece)
    return HR_OK;
}

int hr_upload_scene(hr_ctx *c, const hr_scene_desc *sd) {
    if (!c || !sd) return fail(HR_ERR_INVALID, "hr_upload_scene: null argument");
    if (!sd->elements || sd->num_elements == 0) return fail(HR_ERR_INVALID, "hr_upload_scene: scene has no elements");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;

    HostScene hs;
    std::string ferr;
    // Which builder: the host's binned-SAH build with split clipping gives the best tree (1 - 3 % fewer node tests than the device PLOC
    // build) but is one thread — 12 k triangles take 20 ms, 10^6 six seconds, 4 x 10^6 twenty-five — while the device builds 4 x 10^6 in
    // 38 ms.  By default the scene's size decides: below AUTO_BUILDER_PRIMS primitives (host build < 1 s) the host tree, above it PLOC.
    static const uint64_t AUTO_BUILDER_PRIMS = 200000;
    int builder = c->bvh_builder;
    if (builder < 0) {
        uint64_t prims = 0;
        for (uint32_t e = 0; e < sd->num_elements; e++) prims += sd->elements[e].kind == HR_MESH ? sd->elements[e].num_faces : 1;
        builder = prims >= AUTO_BUILDER_PRIMS ? 2 : 0;
    }
    c->builder_in_use = builder;
    const bool gpu_build = builder != 0;
    rc = flatten_scene(sd, hs, ferr, c->max_leaf, gpu_build ? 0.0 : c->split_ratio, !gpu_build);
    if (rc) return fail(rc, "hr_upload_scene: %s", ferr.c_str());   // a description that is refused leaves the scene in place
    free_scene(c);
    changed(c, SRC_SCENE);   // the guide planes show the scene that goes
    if ((rc = plane_free(c, GUIDES))) return rc;
    Scene &d = c->dsc;
    d = hs.view();
    int r;
    const Tri *tris_in = nullptr;   // the geometry records: input of the device builders, or (host-built tree, leaf order) of the derivation below
    if ((r = upload(c, hs.tris, &tris_in))) return r;
    if ((r = upload(c, hs.spheres, &d.spheres))) return r;
    if ((r = upload(c, hs.sphere_elem, &d.sphere_elem))) return r;
    if ((r = upload(c, hs.sphere_lo, &d.sphere_lo))) return r;
    if ((r = upload(c, hs.cuboids, &d.cuboids))) return r;
    if ((r = upload(c, hs.cuboid_lo, &d.cuboid_lo))) return r;
    if ((r = upload(c, hs.tri_exact, &d.tri_exact))) return r;
    if ((r = upload(c, hs.materials, &d.materials))) return r;
    if ((r = upload(c, hs.images, &d.images))) return r;
    if ((r = upload(c, hs.emitters, &d.emitters))) return r;
    if ((r = upload(c, hs.texels, &d.texels))) return r;
    if ((r = upload(c, std::vector<CameraD>(1, hs.camd), &d.camd))) return r;
    if (!hs.sky_quads.empty()) { if ((r = upload(c, hs.sky_quads, &d.sky_quads))) return r; }
    else d.sky_quads = nullptr;
    c->bvh_build_ms = 0;
    if (gpu_build) { if ((r = build_bvh_on_device(c, hs, tris_in))) return r; }
    else {
        // the records the kernels read for a triangle, derived on the device (as the device builders' gather does)
        TriT *tt = nullptr; TriS *tsh = nullptr;
        const size_t nt = hs.tris.size();
        HIP_TRY(hipMalloc((void **)&tt, std::max<size_t>(nt * sizeof(TriT), 16)));
        c->scene_allocs.push_back(tt);
        HIP_TRY(hipMalloc((void **)&tsh, std::max<size_t>(nt * sizeof(TriS), 16)));
        c->scene_allocs.push_back(tsh);
        uint32_t *tfc = nullptr;
        HIP_TRY(hipMalloc((void **)&tfc, std::max<size_t>(nt * sizeof(uint32_t), 16)));
        c->scene_allocs.push_back(tfc);
        if (nt) {
            lbvh::tri_derive_kernel<<<(unsigned)((nt + 255) / 256), 256, 0, c->stream>>>(tris_in, (uint32_t)nt, tt, tsh, tfc);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        d.tris = tt; d.tri_shade = tsh; d.tri_face = tfc;
        if ((r = upload(c, hs.nodes, &d.nodes))) return r;
        d.qnodes = nullptr;
        if (c->quant_nodes && hs.qnodes.size() * sizeof(QNode) >= (1ull << 31)) return fail(HR_ERR_UNSUPPORTED, "hr_upload_scene: the quantised BVH records exceed their 2^31-byte offset range (set quant_nodes = 0)");
        if (c->quant_nodes && !hs.qnodes.empty() && (r = upload(c, hs.qnodes, &d.qnodes))) return r;
    }
    c->st_nodes = d.num_nodes; c->st_tris = hs.num_input_tris; c->st_spheres = d.num_spheres; c->st_cuboids = d.num_cuboids;
    c->num_images = (uint32_t)hs.images.size();
    c->camera = sd->camera;
    c->have_scene = true;
    if ((r = govern_reset(c))) return r;   // another scene: the balance of the two kernels is another one
    return HR_OK;
}

// The camera of the scene in place, replaced where it lives: Scene::cam, which every launch takes by value, and the one CameraD on the device — with
// flatten_scene's conversions (flatten_camera).  What shows the old view goes, as with hr_upload_scene; what is accumulated stays, and so does the tree.
int hr_set_camera(hr_ctx *c, const hr_camera *cam) {
    if (!c || !cam) return fail(HR_ERR_INVALID, "hr_set_camera: null argument");
    if (!c->have_scene) return fail(HR_ERR_NO_SCENE, "hr_set_camera: no scene uploaded");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    CameraF camf;
    CameraD camd;
    std::string ferr;
    if ((rc = flatten_camera(*cam, camf, camd, ferr))) return fail(rc, "hr_set_camera: %s", ferr.c_str());   // the camera in place stays
    HIP_TRY(hipMemcpy(const_cast<CameraD *>(c->dsc.camd), &camd, sizeof camd, hipMemcpyHostToDevice));
    c->dsc.cam = camf;
    c->camera = *cam;
    changed(c, SRC_SCENE);
    return plane_free(c, GUIDES);
}
int hr_get_camera(hr_ctx *c, hr_camera *out) {
    if (!c || !out) return fail(HR_ERR_INVALID, "hr_get_camera: null argument");
    if (!c->have_scene) return fail(HR_ERR_NO_SCENE, "hr_get_camera: no scene uploaded");
    *out = c->camera;
    return HR_OK;
}

// No tile mask: hr_render covers every tile of the region again.  The mask's buffers are sized by the region's tiles and go with it.
// (Callers have synchronised the context: no kernel is reading the list.)
static int remove_mask(hr_ctx *c) {
    c->mask_on = false;
    c->mask.clear();
    c->mask_active = 0; c->mask_pixels = 0;
    return free_mask_buffers(c);
}

// The target: the W x H frame and the window of it that is rendered (the whole frame, or hr_set_region's).  Every plane is freed, and those that
// live with the target, or with an option that is on, are allocated again for the window (zeroed where the table says so).
static int set_target(hr_ctx *c, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    // no target while the buffers are being replaced (a failed allocation leaves the context without one, not with dangling
    // pointers); a caller-bound accumulator was sized for the old target: it is unbound, the caller rebinds
    c->accum = nullptr; c->W = c->H = 0; c->RX = c->RY = c->RW = c->RH = 0; c->total_valid = false;
    changed(c, SRC_TARGET);
    unbind_accumulator(c);
    for (const Plane *p : PLANES) if ((rc = plane_free(c, *p))) return rc;
    if ((rc = remove_mask(c))) return rc;   // the mask is over the old region's tiles
    c->RW = w; c->RH = h;   // what sizes a plane; W stays 0 — no target — until every plane is there
    for (const Plane *p : PLANES)
        if ((p->life == WITH_TARGET || (p->life == WITH_OPTION && c->*p->on)) && (rc = plane_alloc(c, *p))) { c->RW = c->RH = 0; return rc; }
    c->W = W; c->H = H;
    c->RX = x0; c->RY = y0;
    c->accum = c->accum_own;
    return govern_reset(c);
}
static bool has_region(const hr_ctx *c) { return c->RW != c->W || c->RH != c->H; }
// What the debug entry points refuse, after their own argument check, in this order: a region, a tile mask, no target, no scene.  `needs` says
// which of the four an entry point asks for.
enum { NO_REGION = 1, NO_MASK = 2, A_TARGET = 4, A_SCENE = 8 };
static int debug_refusal(const hr_ctx *c, const char *who, int needs) {
    if ((needs & NO_REGION) && has_region(c)) return fail(HR_ERR_UNSUPPORTED, "%s: not while a region is set (hr_set_region)", who);
    if ((needs & NO_MASK) && c->mask_on) return fail(HR_ERR_UNSUPPORTED, "%s: not while a tile mask is set (hr_set_tile_mask)", who);
    if ((needs & A_TARGET) && (!c->accum || !c->W)) return fail(HR_ERR_NO_TARGET, "%s: hr_set_resolution not called", who);
    if ((needs & A_SCENE) && !c->have_scene) return fail(HR_ERR_NO_SCENE, "%s: no scene uploaded", who);
    return HR_OK;
}

int hr_set_resolution(hr_ctx *c, uint32_t w, uint32_t h) {
    if (!c || !w || !h) return fail(HR_ERR_INVALID, "hr_set_resolution: bad argument");
    if ((uint64_t)w * h > (1ull << 27)) return fail(HR_ERR_UNSUPPORTED, "resolution too large");
    return set_target(c, w, h, 0, 0, w, h);
}

int hr_set_region(hr_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    if (!c) return fail(HR_ERR_INVALID, "hr_set_region: null ctx");
    if (!c->W) return fail(HR_ERR_NO_TARGET, "hr_set_region: hr_set_resolution not called");
    if (!w || !h || x0 > c->W || w > c->W - x0 || y0 > c->H || h > c->H - y0)
        return fail(HR_ERR_INVALID, "hr_set_region: the window %u,%u %ux%u does not fit in the %ux%u frame", x0, y0, w, h, c->W, c->H);
    return set_target(c, c->W, c->H, x0, y0, w, h);
}

int hr_get_region(hr_ctx *c, uint32_t out_xywh[4]) {
    if (!c || !out_xywh) return fail(HR_ERR_INVALID, "hr_get_region: null argument");
    if (!c->W) return fail(HR_ERR_NO_TARGET, "hr_get_region: hr_set_resolution not called");
    out_xywh[0] = c->RX; out_xywh[1] = c->RY; out_xywh[2] = c->RW; out_xywh[3] = c->RH;
    return HR_OK;
}

int hr_bind_accumulator(hr_ctx *c, float *device_rgb) {
    if (!c) return fail(HR_ERR_INVALID, "hr_bind_accumulator: null ctx");
    if (!c->W) return fail(HR_ERR_NO_TARGET, "hr_bind_accumulator: hr_set_resolution not called");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = plane_bytes(c, ACCUM_OWN);
    if (device_rgb) {
        // what can be checked of a caller's pointer is checked: device memory, of this context's device, float-aligned, and w x h x 3 floats
        // (the region's) inside the allocation it points into (a tensor of another shape or dtype would otherwise be overrun by plain stores, silently)
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, device_rgb) != hipSuccess || at.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            return fail(HR_ERR_INVALID, "hr_bind_accumulator: %p is not device memory", (void *)device_rgb);
        }
        if (at.device != c->device) return fail(HR_ERR_INVALID, "hr_bind_accumulator: the buffer lives on device %d, the context on device %d", at.device, c->device);
        if ((uintptr_t)device_rgb % sizeof(float)) return fail(HR_ERR_INVALID, "hr_bind_accumulator: the buffer is not aligned for floats");
        void *base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)device_rgb) == hipSuccess) {
            if ((const char *)device_rgb + bytes > (const char *)base + size)
                return fail(HR_ERR_INVALID, "hr_bind_accumulator: the buffer is too small (%zu bytes from this address to the end of its allocation, %u x %u x 3 floats = %zu needed)",
                            (size_t)((const char *)base + size - (const char *)device_rgb), c->RW, c->RH, bytes);
        } else (void)hipGetLastError();
    }
    int rc = sync_all(c);
    if (rc) return rc;
    {
        // look-up, release of this context's old binding and the new entry under ONE lock: two threads binding one buffer to two contexts
        // cannot both pass.  The registry holds byte ranges: a buffer that overlaps another context's is refused like an equal one.
        // (The caller binds NULL before it frees a bound buffer: an entry left behind would refuse whoever is handed the address next.)
        std::lock_guard<std::mutex> lk(g_bound_mu);
        if (device_rgb)
            for (const auto &kv : g_bound) {
                const char *a = (const char *)kv.first, *b = (const char *)device_rgb;
                if (kv.second.first != c && a < b + bytes && b < a + kv.second.second)
                    return fail(HR_ERR_INVALID, "hr_bind_accumulator: this buffer is already bound to another context (one context per accumulator: the launch's radiance is added with plain loads and stores)");
            }
        for (auto it = g_bound.begin(); it != g_bound.end();) it = it->second.first == c ? g_bound.erase(it) : std::next(it);
        if (device_rgb) g_bound[device_rgb] = std::make_pair((const hr_ctx *)c, bytes);
    }
    c->accum = device_rgb ? device_rgb : c->accum_own;
    changed(c, SRC_ACCUM | SRC_MOMENTS | SRC_COUNTS | SRC_BUCKETS);   // (conservative, kept: another accumulator counts as other statistics)
    return HR_OK;
}
void *hr_accumulator_device_ptr(hr_ctx *c) { return c ? c->accum : nullptr; }

int hr_set_stream(hr_ctx *c, void *s) {
    if (!c) return fail(HR_ERR_INVALID, "hr_set_stream: null ctx");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return HR_OK;
}

int hr_clear(hr_ctx *c) {
    if (!c) return fail(HR_ERR_INVALID, "hr_clear: null ctx");
    if (!c->accum) return fail(HR_ERR_NO_TARGET, "hr_clear: no accumulator (call hr_set_resolution)");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    changed(c, SRC_ACCUM | SRC_MOMENTS | SRC_COUNTS | SRC_BUCKETS);
    // the planes the table marks, the accumulator through c->accum (it may be the caller's bound buffer); the tile mask stays: a setting, like the region
    for (const Plane *p : PLANES)
        if (p->at_clear && (rc = plane_zero(c, *p, c->stream, p == &ACCUM_OWN ? c->accum : nullptr))) return rc;
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(Counters), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->seed_ms = c->trace_ms = c->post_ms = c->debug_ms = 0;
    c->seed_launches = c->trace_launches = c->debug_launches = 0;
    c->paths_rendered = 0;
    return HR_OK;
}

// Precise shading computes with the reference's f64 draws: the seed kernel (the default one, seed_mode 2) writes what rounding a draw to fp32
// took away into the records' twin behind the records (device_scene.h RenderParams::rec_lo_off).
static bool draws_twin(const hr_ctx *c) { return c->precise && c->seed_mode == 2 && c->draw_residuals; }
static uint64_t rec_lo_off(const hr_ctx *c) { return draws_twin(c) ? c->rec_lo_off : 0; }
static int ensure_draws(hr_ctx *c, size_t items) {
    const bool twin = draws_twin(c);
    if (items <= c->draws_cap && (!twin || c->rec_lo_off)) return HR_OK;
    int rc = sync_all(c);   // kernels of an earlier hr_render may still be reading the buffers that are about to be replaced
    if (rc) return rc;
    items = std::max(items, c->draws_cap);
    c->draws_cap = 0;       // stays 0 if an allocation below fails: the next call starts over
    c->rec_lo_off = 0;
    const size_t floats = (items + SEED_SPARE_ITEMS) * REC_ITEM_FLOATS;   // + spare items for the padding lanes of the last group
    for (int i = 0; i < 2; i++) {
        if (c->recs[i]) { HIP_TRY(hipFree(c->recs[i])); c->recs[i] = nullptr; }
        HIP_TRY(hipMalloc((void **)&c->recs[i], floats * (twin ? 2 : 1) * sizeof(float)));
    }
    c->draws_cap = items;
    c->rec_lo_off = twin ? floats : 0;
    return HR_OK;
}

// Fix-up lists of the seed kernel's consumer waves: a path whose lens rejection loop rejects its first LENS_FAST attempts (round
// lens: (1 - pi/4)^5 = 4.6e-4 of the paths) is queued by the wave that seeded it.  The paths per wave grow with the launch and
// shrink with the CU count, so the lists are sized per launch: 8 x the expected count (the count is Poisson: 8 x is > 30 sigma away
// for any launch that matters), never below SEED_OVF_MIN.
static int ensure_ovf(hr_ctx *c, uint64_t paths_per_launch) {
    const uint64_t groups = (paths_per_launch + SEED_COLS - 1) / SEED_COLS;
    const uint64_t waves = 2 * std::min<uint64_t>(std::max<uint64_t>(groups, 1), (uint64_t)c->num_cus);
    const double expected = 4.7e-4 * (double)paths_per_launch / (double)waves;
    const uint64_t want = std::max<uint64_t>(SEED_OVF_MIN, ((uint64_t)(8.0 * expected) + 64 + 255) / 256 * 256);
    if (want <= c->ovf_cap) return HR_OK;
    int rc = sync_all(c);   // a seed kernel in flight may still be writing its lists
    if (rc) return rc;
    if (c->ovf) { HIP_TRY(hipFree(c->ovf)); c->ovf = nullptr; }
    c->ovf_cap = 0;
    HIP_TRY(hipMalloc((void **)&c->ovf, (size_t)c->num_cus * 2 * want * sizeof(uint32_t)));
    c->ovf_cap = (uint32_t)want;
    return HR_OK;
}

// Queues of the split pipeline for launches of up to `paths` paths: a step's rays are at most one main ray and one shadow ray per emitter
// for every path (renderer.rs:274), both parities of the ray queue, one hit per ray, both parities of the live-path state.
static int ensure_wf(hr_ctx *c, uint64_t paths) {
    // per sub-queue: the items (tile x sampling) it owns x 64 paths, and per path a main ray + one shadow ray per emitter
    const uint64_t sub_paths = ((paths / 64u + WF_SUBQ - 1u) / WF_SUBQ) * 64u, sub_rays = sub_paths * (1ull + c->dsc.num_emitters);
    if (sub_paths <= c->wf.cap_paths && sub_rays <= c->wf.cap_rays && c->wf_block && (c->wf_has_prec || !c->precise)) return HR_OK;
    if (sub_rays * WF_SUBQ >= 0xffffffffull) return fail(HR_ERR_UNSUPPORTED, "split pipeline: %llu ray slots per launch exceed the 32-bit queue index (reduce option batch)", (unsigned long long)(sub_rays * WF_SUBQ));
    int rc = sync_all(c);
    if (rc) return rc;
    if (c->wf_block) { HIP_TRY(hipFree(c->wf_block)); c->wf_block = nullptr; }
    c->wf.cap_paths = c->wf.cap_rays = 0;
    const uint64_t rays = sub_rays * WF_SUBQ, pths = sub_paths * WF_SUBQ;
    const size_t ray_q = (size_t)rays * sizeof(f4), st_q = (size_t)pths * sizeof(f4), cnt = (WF_STEPS + 2) * WF_SUBQ * sizeof(WfCounts);
    const size_t total = cnt + 4 * ray_q + (size_t)rays * sizeof(WfHitRec) + (c->precise ? 10 : 6) * st_q;
    hipError_t e = hipMalloc(&c->wf_block, total);
    if (e != hipSuccess) { c->wf_block = nullptr; return fail(HR_ERR_DEVICE, "split pipeline: %.1f GiB of queues: %s", (double)total / (1ull << 30), hipGetErrorString(e)); }
    char *b = (char *)c->wf_block;
    c->wf.counts = (WfCounts *)b; b += cnt;
    for (int i = 0; i < 2; i++) { c->wf.ray_a[i] = (f4 *)b; b += ray_q; c->wf.ray_b[i] = (f4 *)b; b += ray_q; }
    c->wf.hits = (WfHitRec *)b; b += (size_t)rays * sizeof(WfHitRec);
    for (int i = 0; i < 2; i++) { c->wf.st_a[i] = (f4 *)b; b += st_q; c->wf.st_b[i] = (f4 *)b; b += st_q; c->wf.st_c[i] = (f4 *)b; b += st_q; }
    for (int i = 0; i < 2; i++) { c->wf.st_d[i] = c->wf.st_e[i] = c->wf.st_f[i] = nullptr; c->wf.tag[i] = nullptr; }
    if (c->precise) for (int i = 0; i < 2; i++) { c->wf.st_d[i] = (f4 *)b; b += st_q; c->wf.st_e[i] = (f4 *)b; b += st_q; }
    c->wf_has_prec = c->precise;
    c->wf.cap_paths = (uint32_t)sub_paths; c->wf.cap_rays = (uint32_t)sub_rays;
    return HR_OK;
}
// One launch through the split pipeline, on the main stream: camera rays, then per path iteration the traversal kernel over the step's rays
// and the shading kernel over its live paths.  Empty steps (every path has ended) are two kernels that read one counter and leave.
static int launch_split(hr_ctx *c, const RenderParams &rp, int slot, std::vector<hipEvent_t> *marks = nullptr, uint32_t *plog = nullptr, const WfQueues *queues = nullptr) {
    const WfQueues wq = queues ? *queues : c->wf;
    hipStream_t st = c->stream;
    auto mark = [&]() -> hipError_t { if (!marks) return hipSuccess; hipEvent_t e; hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; marks->push_back(e); return hipEventRecord(e, st); };
    const bool log = plog != nullptr;
    const WfStartFn start = select_wf_start_kernel(c->precise, rp.tile_list != nullptr);
    const WfTraverseFn traverse = select_wf_traverse_kernel(c->counters, c->dsc.qnodes != nullptr, log);
    const WfShadeFn shade = select_wf_shade_kernel(c->counters, c->precise, log);
    if (!start || !traverse || !shade) return fail(HR_ERR_UNSUPPORTED, "split pipeline: no kernel instantiation for these options (kernel_variants.h)");
    HIP_TRY(hipMemsetAsync(wq.counts, 0, (WF_STEPS + 2) * WF_SUBQ * sizeof(WfCounts), st));
    HIP_TRY(mark());
    // grids: whole multiples of WF_SUBQ waves (16 workgroups of 4), so that every sub-queue has the same number of waves
    auto grid_of = [&](uint32_t wgs_per_cu) { return dim3(std::max<uint32_t>(16u, (uint32_t)c->num_cus * wgs_per_cu / 16u * 16u)); };
    hipLaunchKernelGGL(start, grid_of(8u), dim3(256), 0, st, c->dsc, rp, c->recs[slot], wq);
    HIP_TRY(mark());
    RenderParams rt = rp;
    rt.adv_den = c->wf_adv_den;
    const dim3 gt = grid_of(c->wf_trav_wgs), gs = grid_of(c->wf_shade_wgs), b(256);
    for (uint32_t step = 1; step <= WF_STEPS; step++) {
        hipLaunchKernelGGL(traverse, gt, b, 0, st, c->dsc, rt, wq, step, c->d_counters);
        HIP_TRY(mark());
        hipLaunchKernelGGL(shade, gs, b, 0, st, c->dsc, rp, c->recs[slot], wq, step, c->d_counters, plog);
        HIP_TRY(mark());
    }
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

static int launch_seed(hr_ctx *c, const RenderParams &rp, int slot, hipStream_t st) {
    const bool list = rp.tile_list != nullptr;
    uint64_t paths = (uint64_t)(list ? rp.tile_count : rp.tiles_x * rp.tiles_y) * rp.num_k * 64u;
    uint32_t grid = (uint32_t)std::min<uint64_t>((paths + SEED_COLS - 1) / SEED_COLS, (uint64_t)c->num_cus);
    const SeedVariant *v = select_seed_kernel(c->seed_mode, c->seed_split, c->seed_prof, rp.rec_lo_off != 0, list, c->seed_prerun != 0);
    if (!v) return fail(HR_ERR_UNSUPPORTED, "no seed kernel instantiation for seed_mode %d, seed_split %d, seed_prof %d%s (kernel_variants.h)", c->seed_mode, c->seed_split, c->seed_prof, list ? " under a tile mask" : "");
    const bool skip = (c->debug_skip & 2) != 0;
    if (!skip && v->ring && !c->ring) HIP_TRY(hipMalloc((void **)&c->ring, (size_t)c->num_cus * SEED_RING_WORDS_MAX * sizeof(u64)));
    EventPair ev;
    HIP_TRY(timed_begin(ev, st));
    hipError_t e = hipSuccess;
    if (!skip) {
        RenderParams krp = rp;
        int lens_shape = c->dsc.cam.lens_shape;
        void *args[7] = {&krp, &lens_shape, &c->ring, &c->recs[slot], &c->ovf, &c->ovf_win, &c->d_counters};
        if (!v->ring) std::copy(args + 3, args + 7, args + 2);   // the fused kernel has no ring argument
        e = hipLaunchKernel(v->fn, dim3(grid), dim3(v->threads), args, SEED_LDS_BYTES, st);
    }
    HIP_TRY(timed_end(e, ev, st, c->seed_events, &c->seed_launches));
    return HR_OK;
}

// ---- the launch plan ----
// the launch geometry: the frame, the region and the region's tiles
static void target_params(const hr_ctx *c, RenderParams &rp) {
    rp.width = c->W; rp.height = c->H;
    rp.org_x = c->RX; rp.org_y = c->RY; rp.reg_w = c->RW; rp.reg_h = c->RH;
    rp.tiles_x = (c->RW + 3) / 4; rp.tiles_y = (c->RH + 3) / 4;
}
// the trace side's knobs (debug options adv_den, leaf_den, node_unroll, kchunk, nee_cull)
static void knob_params(const hr_ctx *c, RenderParams &rp) {
    rp.adv_den = c->adv_den; rp.leaf_den = c->leaf_den;
    rp.node_unroll = c->node_unroll; rp.kchunk = c->kchunk;
    rp.nee_cull_off = ~c->nee_cull & 7u;
}
// Samplings per launch of hr_render: option batch, or automatically launches of the size the kernels are tuned on (4 samplings of
// 1920x1080), at most 64 samplings — under the caps of the launch's buffers.
static uint32_t render_batch(const hr_ctx *c, uint32_t tiles, bool split) {
    uint64_t batch = c->batch;
    if (!batch) {
        const uint64_t per_sampling_paths = (uint64_t)tiles * 64u;
        batch = std::min<uint64_t>(64, std::max<uint64_t>(4, (33177600ull + per_sampling_paths - 1) / per_sampling_paths));
    }
    // the hand-off costs 8 KiB per (tile, sampling): keep each of the two buffers under max_tail_bytes
    const uint64_t per_sampling = (uint64_t)tiles * REC_ITEM_FLOATS * sizeof(float) * (draws_twin(c) ? 2 : 1);
    batch = std::min(batch, std::max<uint64_t>(1, c->max_tail_bytes / std::max<uint64_t>(1, per_sampling)));
    if (split) {
        // the split pipeline's queues are sized for the worst case (a main ray + a shadow ray per emitter for every path, both parities): keep
        // them under the same cap as a hand-off buffer — a 3840x2160 launch then holds one sampling (33 M paths) instead of four
        const uint64_t per_path = (1ull + c->dsc.num_emitters) * (4 * sizeof(f4) + sizeof(WfHitRec)) + (c->precise ? 10 : 6) * sizeof(f4);
        batch = std::min(batch, std::max<uint64_t>(1, c->max_tail_bytes / std::max<uint64_t>(1, (uint64_t)tiles * 64u * per_path)));
    }
    return (uint32_t)batch;
}
// What traces a planned launch: nothing (the seed kernel alone), whatever is in force, or the split pipeline whatever is in force.
enum TraceSide { TRACE_NONE, TRACE_IN_FORCE, TRACE_SPLIT };
// The launch plan: the RenderParams for samplings begin, begin + stride, .. of the current target, `batch` of them per launch (0: hr_render's
// own batch), and the hand-off buffers made ready for a launch of that size — the records with their residual twin, the fix-up lists and,
// when the split pipeline traces, its queues.  What belongs to ONE launch stays with the caller: sampling_begin and num_k of the launches
// after the first, and the governor's fields (left at none: the queries launch with the chip to themselves).
struct LaunchPlan {
    RenderParams rp;
    uint32_t tiles;   // 4x4-pixel tiles the launch covers: the region's, or under a tile mask the active ones
    uint32_t batch;   // samplings per launch
    bool split;       // the split pipeline traces (the roulette estimator lives in the megakernel only)
};
static int plan_launch(hr_ctx *c, uint32_t begin, uint32_t stride, uint32_t batch, TraceSide side, LaunchPlan &p) {
    p = LaunchPlan{};
    RenderParams &rp = p.rp;
    target_params(c, rp);
    knob_params(c, rp);
    rp.sampling_begin = begin; rp.stride = stride; rp.num_k = batch;
    rp.pad[0] = c->seed_prio;
    p.tiles = rp.tiles_x * rp.tiles_y;
    if (c->mask_on) { rp.tile_list = c->d_tile_list; rp.tile_count = c->mask_active; p.tiles = c->mask_active; }   // (never with 0 active tiles: hr_render returns before it plans)
    p.split = side == TRACE_SPLIT || (side == TRACE_IN_FORCE && c->trace_mode == 1 && !c->rr_start);
    p.batch = batch ? batch : render_batch(c, p.tiles, p.split);
    int rc = ensure_draws(c, (size_t)p.tiles * p.batch);
    if (rc) return rc;
    rp.rec_lo_off = rec_lo_off(c);
    if ((rc = ensure_ovf(c, (uint64_t)p.tiles * 64u * p.batch))) return rc;
    if (p.split && (rc = ensure_wf(c, (uint64_t)p.tiles * 64u * p.batch))) return rc;
    rp.ovf_cap = c->ovf_cap;
    return HR_OK;
}
// the grid of a trace_kernel launch: persistent waves, enough workgroups to fill every CU (6 per CU covers every occupancy variant), never
// more waves than work units
static uint32_t trace_grid_size(const hr_ctx *c, uint32_t tiles, uint32_t nk, uint32_t fixed_grid) {
    const uint32_t kch = c->kchunk ? c->kchunk : TRACE_KCHUNK;
    const uint64_t units = (uint64_t)tiles * ((nk + kch - 1) / kch);   // work units of the trace kernel
    return (uint32_t)std::min<uint64_t>(fixed_grid ? fixed_grid : (uint64_t)c->num_cus * c->trace_wgs, (units + TRACE_WAVES - 1) / TRACE_WAVES);
}

int hr_render(hr_ctx *c, uint32_t s_begin, uint32_t s_end, uint32_t stride) {
    if (!c || !stride) return fail(HR_ERR_INVALID, "hr_render: bad argument");
    if (!c->have_scene) return fail(HR_ERR_NO_SCENE, "hr_render: no scene uploaded");
    if (!c->accum || !c->W) return fail(HR_ERR_NO_TARGET, "hr_render: hr_set_resolution not called");
    if (s_end <= s_begin) return HR_OK;
    HIP_TRY(hipSetDevice(c->device));
    changed(c, SRC_ACCUM | SRC_MOMENTS | SRC_COUNTS | SRC_BUCKETS);
    if (c->precise_opt == 1 && c->rr_start) return fail(HR_ERR_UNSUPPORTED, "hr_render: russian_roulette and precise_shading exclude each other (the roulette estimator has no f64 instantiation)");
    const uint32_t total_k = (s_end - s_begin + stride - 1) / stride;
    const bool list = c->mask_on;
    if (list) {
        // the list forms are rows of their own (kernel_variants.h) and exist for what a product host runs: anything else is refused, as a missing row is
        const char *what = c->counters ? "option counters" : c->rr_start ? "option russian_roulette" : c->min_waves != 5 ? "debug option min_waves" :
                           c->seed_mode != 2 ? "a seed_mode other than 2" : c->seed_prof ? "debug option seed_prof" : nullptr;
        if (what) return fail(HR_ERR_UNSUPPORTED, "hr_render: %s has no kernel form for a tile mask (hr_set_tile_mask(NULL) removes the mask)", what);
        if (!c->mask_active) {   // nothing is active: nothing to enqueue; the samplings count as issued (hr_noise.samplings), like those of any masked launch
            if (c->moments) c->moments_n += total_k;
            if (c->buckets) c->buckets_n += total_k;
            return HR_OK;
        }
    }
    LaunchPlan plan;
    int rc = plan_launch(c, s_begin, stride, 0, TRACE_IN_FORCE, plan);
    if (rc) return rc;
    RenderParams &rp = plan.rp;
    const uint32_t tiles = plan.tiles, batch = plan.batch;
    // hr_render alone: the roulette estimator, the finer tail, the timing experiments, the debug wave budget
    rp.rr_start = c->rr_start;
    rp.tail_div = c->tail_div;
    rp.pad[2] = (uint32_t)c->debug_skip;
    rp.wg_budget = c->trace_budget;
    const TraceFn trace = select_trace_kernel(c->counters, c->dsc.qnodes != nullptr, c->rr_start != 0, c->precise, c->min_waves, false, list);
    if (!trace) return fail(HR_ERR_UNSUPPORTED, "hr_render: no trace kernel instantiation for these options%s (kernel_variants.h)", list ? " under a tile mask" : "");
    const AccumulateFn accumulate = select_accumulate_kernel(c->moments != nullptr, c->counts != nullptr, list);
    if (!accumulate) return fail(HR_ERR_UNSUPPORTED, "hr_render: no accumulate kernel instantiation for these options (kernel_variants.h)");
    const BucketFn bucket = c->buckets ? select_bucket_kernel(c->counts != nullptr, list, c->bucket_by_sampling) : nullptr;   // option robust_buckets off: nothing more is launched
    if (c->buckets && !bucket) return fail(HR_ERR_UNSUPPORTED, "hr_render: no bucket kernel instantiation for these options (kernel_variants.h)");
    for (uint32_t done = 0; done < total_k; done += batch) {
        uint32_t nk = std::min(batch, total_k - done);
        rp.sampling_begin = s_begin + done * stride;
        rp.num_k = nk;
        int slot = (int)(c->batch_counter & 1);
        c->batch_counter++;
        // the priority governor lives on the device (governor_kernel above): the kernels read its level when they start
        rp.gov = c->gov; rp.gov_slot = (uint32_t)slot;
        rp.trace_boost = 0;
        rp.pad[1] = c->init_prio;   // the producer waves' priority at level 0
        hipStream_t sstream = c->seed_stream;  // (alternating two seed streams to overlap kernel tails was measured: no gain)
        // seed of this batch may only overwrite draws[slot] once the trace that read it has finished
        if (c->trace_pending[slot]) HIP_TRY(hipStreamWaitEvent(sstream, c->trace_done[slot], 0));
        if ((rc = launch_seed(c, rp, slot, sstream))) return rc;
        HIP_TRY(hipEventRecord(c->seed_done[slot], sstream));
        c->seed_pending[slot] = true;
        HIP_TRY(hipStreamWaitEvent(c->stream, c->seed_done[slot], 0));
        EventPair ev;
        HIP_TRY(timed_begin(ev, c->stream));
        HIP_TRY(hipMemsetAsync(c->d_tile_counter + slot, 0, sizeof(uint32_t), c->stream));
        if (c->debug_skip & 16) {
        } else if (plan.split) {
            if ((rc = launch_split(c, rp, slot))) return rc;
        } else
            hipLaunchKernelGGL(trace, dim3(trace_grid_size(c, tiles, nk, c->trace_grid)), dim3(64 * TRACE_WAVES), 0, c->stream, c->dsc, rp, c->recs[slot], c->d_counters,
                               c->d_tile_counter + slot, (uint32_t *)nullptr);
        HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->trace_events, &c->trace_launches));
        // the launch's radiance into the accumulator (the trace kernel left every path's in its record), in the gap in which this
        // stream waits for the next seed kernel anyway
        if (!(c->debug_skip & 16)) {
            if (bucket) {   // in front of accumulate_kernel: a pixel's ordinal under sample_counts is its count BEFORE this launch
                // by sampling: the launch's first bucket, (sampling_begin - 1) mod K, instead of the samplings behind the buckets
                const unsigned long long start = c->bucket_by_sampling ? ((unsigned long long)rp.sampling_begin + c->robust_k - 1u) % c->robust_k : (unsigned long long)c->buckets_n;
                hipLaunchKernelGGL(bucket, dim3((tiles + 3) / 4), dim3(256), 0, c->stream, rp, c->recs[slot], c->buckets, c->counts, c->robust_k, start);
                HIP_TRY(hipGetLastError());
                c->buckets_n += nk;
            }
            hipLaunchKernelGGL(accumulate, dim3((tiles + 3) / 4), dim3(256), 0, c->stream, rp, c->recs[slot], c->accum, c->moments, c->counts);
            HIP_TRY(hipGetLastError());
            if (c->moments) c->moments_n += nk;
        }
        // the governor judges the launch that has just finished and frees its stamps; the seed kernel that reuses the slot waits for
        // trace_done, recorded behind it
        hipLaunchKernelGGL(governor_kernel, dim3(1), dim3(1), 0, c->stream, c->gov, (uint32_t)slot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->trace_done[slot], c->stream));
        c->trace_pending[slot] = true;
        c->paths_rendered += (list ? c->mask_pixels : (uint64_t)region_pixels(c)) * 4 * nk;
        if (c->trace_events.size() >= 64 && c->seed_events.size() == c->trace_events.size()) retire_finished_launches(c);
        if (c->trace_events.size() > 4096) {  // (never reached while launches finish: the host would have to be 4,096 launches ahead)
            if ((rc = sync_all(c))) return rc;
        }
    }
    return HR_OK;
}

// One pass of a single-ray tile kernel (trace_kernel.h: the debug renderer, the guide kernels) over the region: one wave per 4x4-pixel tile, the
// trace side's knobs (the kernels read leaf_den and node_unroll of them), timed into debug_kernel_ms / debug_launches.  `args`: what the kernel
// takes behind (Scene, RenderParams).
template <class Fn, class... Args>
static int launch_tile_pass(hr_ctx *c, Fn fn, Args... args) {
    RenderParams rp{};
    target_params(c, rp);
    knob_params(c, rp);
    const uint32_t tiles = rp.tiles_x * rp.tiles_y;
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    hipLaunchKernelGGL(fn, dim3((tiles + TRACE_WAVES - 1) / TRACE_WAVES), dim3(64 * TRACE_WAVES), 0, c->stream, c->dsc, rp, args...);
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->debug_events, &c->debug_launches));
    return HR_OK;
}

int hr_render_debug(hr_ctx *c, int mode) {
    if (!c || mode < 0 || mode > 3) return fail(HR_ERR_INVALID, "hr_render_debug: mode must be 0..3");
    // (this entry point has always asked in an order of its own — scene, target, moments, mask, counts — and renders a region: one need at a time)
    int rc;
    if ((rc = debug_refusal(c, "hr_render_debug", A_SCENE)) || (rc = debug_refusal(c, "hr_render_debug", A_TARGET))) return rc;
    if (c->moments_on) return fail(HR_ERR_UNSUPPORTED, "hr_render_debug: not with option moments on (a debug sampling goes into the accumulator without per-sampling values)");
    if ((rc = debug_refusal(c, "hr_render_debug", NO_MASK))) return rc;
    if (c->counts_on) return fail(HR_ERR_UNSUPPORTED, "hr_render_debug: not with option sample_counts on (a debug sampling goes into the accumulator without being counted)");
    if (c->robust_on) return fail(HR_ERR_UNSUPPORTED, "hr_render_debug: not with option robust_buckets on (a debug sampling goes into the accumulator without per-sampling values)");
    HIP_TRY(hipSetDevice(c->device));
    changed(c, SRC_ACCUM);   // (the accumulator alone: the three options are off)
    const DebugRenderFn fn = select_debug_render_kernel(c->counters, c->dsc.qnodes != nullptr);
    if (!fn) return fail(HR_ERR_UNSUPPORTED, "hr_render_debug: no kernel instantiation for these options (kernel_variants.h)");
    return launch_tile_pass(c, fn, mode, c->accum, c->d_counters);
}

int hr_synchronize(hr_ctx *c) {
    if (!c) return fail(HR_ERR_INVALID, "hr_synchronize: null ctx");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    Counters h;
    HIP_TRY(hipMemcpy(&h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    if (h.rng_overflow) return fail(HR_ERR_RNG_WINDOW, "%llu paths needed more than %d ISAAC-64 outputs for the lens rejection loop (or the fix-up queue overflowed)", h.rng_overflow, ISAAC_TAIL);
    return HR_OK;
}

int hr_mark(hr_ctx *c, uint64_t *ticket) {
    if (!c || !ticket) return fail(HR_ERR_INVALID, "hr_mark: null argument");
    HIP_TRY(hipSetDevice(c->device));
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, c->stream);
    if (e != hipSuccess) { (void)hipEventDestroy(ev); return fail(HR_ERR_DEVICE, "hr_mark: %s", hipGetErrorString(e)); }
    *ticket = c->next_ticket++;
    c->markers.emplace_back(*ticket, ev);
    return HR_OK;
}
int hr_wait(hr_ctx *c, uint64_t ticket) {
    if (!c) return fail(HR_ERR_INVALID, "hr_wait: null ctx");
    HIP_TRY(hipSetDevice(c->device));
    size_t n = 0;
    while (n < c->markers.size() && c->markers[n].first <= ticket) n++;
    if (!n) return HR_OK;   // already waited for (or swept by hr_synchronize)
    hipError_t e = hipEventSynchronize(c->markers[n - 1].second);
    for (size_t i = 0; i < n; i++) (void)hipEventDestroy(c->markers[i].second);
    c->markers.erase(c->markers.begin(), c->markers.begin() + (long)n);
    if (e != hipSuccess) return fail(HR_ERR_DEVICE, "hr_wait: %s", hipGetErrorString(e));
    return HR_OK;
}

int hr_read_accumulator(hr_ctx *c, float *host) {
    if (!c || !host) return fail(HR_ERR_INVALID, "hr_read_accumulator: null argument");
    if (!c->accum) return fail(HR_ERR_NO_TARGET, "hr_read_accumulator: no accumulator");
    return plane_read(c, ACCUM_OWN, c->total_valid ? c->accum_total : c->accum, host);
}
int hr_write_accumulator(hr_ctx *c, const float *host) {
    if (!c || !host) return fail(HR_ERR_INVALID, "hr_write_accumulator: null argument");
    if (!c->accum) return fail(HR_ERR_NO_TARGET, "hr_write_accumulator: no accumulator");
    return plane_write(c, ACCUM_OWN, c->accum, host);
}

// ---- multi-GPU: one all-reduce of the accumulators over RCCL (hr_comm.h) ------------------------------------------------------
#define NCCL_TRY(expr)                                                                                                    \
    do {                                                                                                                  \
        int r_ = (expr);                                                                                                  \
        if (r_ != 0) return fail(HR_ERR_DEVICE, "%s failed: %s", #expr, hrcomm::api().GetErrorString ? hrcomm::api().GetErrorString(r_) : "?"); \
    } while (0)

int hr_comm_get_unique_id(void *id_out) {
    if (!id_out) return fail(HR_ERR_INVALID, "hr_comm_get_unique_id: null argument");
    if (!hrcomm::load()) return fail(HR_ERR_UNSUPPORTED, "%s", hrcomm::api().error.c_str());
    hrcomm::UniqueId id;
    NCCL_TRY(hrcomm::api().GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return HR_OK;
}
__global__ void add_accumulator_kernel(float *__restrict__ total, const float *__restrict__ part, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) total[i] += part[i];
}
static int comm_release(hr_ctx *c) {
    if (c->comm) { NCCL_TRY(hrcomm::api().CommDestroy(c->comm)); c->comm = nullptr; }
    reset_same_device_peers(c);
    c->same_device_peers.clear();
    c->comm_world = 0; c->comm_rank = 0; c->total_valid = false;
    c->comm_path = HR_COMM_NONE; c->allreduces = 0; c->comm_group = 0;
    return HR_OK;
}
int hr_comm_init_rank(hr_ctx *c, const void *id, int world_size, int rank) {
    if (!c || !id || world_size < 1 || rank < 0 || rank >= world_size) return fail(HR_ERR_INVALID, "hr_comm_init_rank: bad argument");
    if (!hrcomm::load()) return fail(HR_ERR_UNSUPPORTED, "%s", hrcomm::api().error.c_str());
    HIP_TRY(hipSetDevice(c->device));
    int rc = comm_release(c);
    if (rc) return rc;
    hrcomm::UniqueId uid;
    memcpy(&uid, id, sizeof uid);
    NCCL_TRY(hrcomm::api().CommInitRank(&c->comm, world_size, uid, rank));
    c->comm_world = world_size; c->comm_rank = rank; c->comm_path = HR_COMM_RCCL_RANK;
    return HR_OK;
}
int hr_comm_init_local(hr_ctx **ctxs, int n) {
    if (!ctxs || n < 1) return fail(HR_ERR_INVALID, "hr_comm_init_local: bad argument");
    for (int i = 0; i < n; i++) if (!ctxs[i]) return fail(HR_ERR_INVALID, "hr_comm_init_local: null context");
    {
        // all contexts on ONE device (RCCL wants one rank per device): the "collective" is a sum kernel on that device
        bool same = n > 1;
        for (int i = 1; i < n; i++) same = same && ctxs[i]->device == ctxs[0]->device;
        if (same) {
            for (int i = 0; i < n; i++) { int rc = comm_release(ctxs[i]); if (rc) return rc; }
            for (int i = 0; i < n; i++) { ctxs[i]->same_device_peers.assign(ctxs, ctxs + n); ctxs[i]->comm_world = n; ctxs[i]->comm_rank = i; ctxs[i]->comm_path = HR_COMM_SAME_DEVICE_SUM; }
            return HR_OK;
        }
    }
    if (!hrcomm::load()) return fail(HR_ERR_UNSUPPORTED, "%s", hrcomm::api().error.c_str());
    std::vector<int> devs(n);
    std::vector<hrcomm::Comm> comms(n, nullptr);
    for (int i = 0; i < n; i++) {
        int rc = comm_release(ctxs[i]);
        if (rc) return rc;
        devs[i] = ctxs[i]->device;
        for (int j = 0; j < i; j++) if (devs[j] == devs[i]) return fail(HR_ERR_INVALID, "hr_comm_init_local: device %d appears twice (RCCL needs one rank per device)", devs[i]);
    }
    NCCL_TRY(hrcomm::api().CommInitAll(comms.data(), n, devs.data()));
    static std::atomic<uint64_t> groups{0};
    const uint64_t group = ++groups;
    for (int i = 0; i < n; i++) { ctxs[i]->comm = comms[i]; ctxs[i]->comm_world = n; ctxs[i]->comm_rank = i; ctxs[i]->comm_path = HR_COMM_RCCL_GROUP; ctxs[i]->comm_group = group; }
    return HR_OK;
}
int hr_comm_destroy(hr_ctx *c) {
    if (!c) return fail(HR_ERR_INVALID, "hr_comm_destroy: null ctx");
    if (!c->comm && c->same_device_peers.empty()) return HR_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    return comm_release(c);
}
// enqueue this rank's part of the collective behind its render work (caller: inside a group when it drives several ranks)
static int allreduce_enqueue(hr_ctx *c) {
    if (!c->comm && c->same_device_peers.empty()) return fail(HR_ERR_INVALID, "hr_allreduce_accumulator: no communicator (hr_comm_init_rank / hr_comm_init_local)");
    if (!c->accum || !c->W) return fail(HR_ERR_NO_TARGET, "hr_allreduce_accumulator: no accumulator");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = plane_elems(c, ACCUM_OWN);
    if (!c->accum_total) { int rc = plane_alloc(c, ACCUM_TOTAL); if (rc) return rc; }
    if (!c->same_device_peers.empty()) {
        for (hr_ctx *p : c->same_device_peers) {
            if (p->W != c->W || p->H != c->H || p->RX != c->RX || p->RY != c->RY || p->RW != c->RW || p->RH != c->RH || !p->accum)
                return fail(HR_ERR_INVALID, "hr_allreduce_accumulator: the contexts of the group differ in resolution or region");
            if (p != c) { int rc = sync_all(p); if (rc) return rc; }   // the peers' render work (their own streams)
        }
        // rank order, so that every context of the group gets bit-identical totals (as an all-reduce delivers them)
        int rc = sync_all(c);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->accum_total, c->same_device_peers[0]->accum, plane_bytes(c, ACCUM_OWN), hipMemcpyDeviceToDevice, c->stream));
        for (size_t k = 1; k < c->same_device_peers.size(); k++)
            hipLaunchKernelGGL(add_accumulator_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->accum_total, c->same_device_peers[k]->accum, n);
        HIP_TRY(hipGetLastError());
        // the adds read the PEERS' accumulators from this context's stream: they are finished before the call returns, so that a
        // peer's next hr_render / hr_clear / hr_write_accumulator cannot race with them
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->total_valid = true;
        c->allreduces++;
        return HR_OK;
    }
    NCCL_TRY(hrcomm::api().AllReduce(c->accum, c->accum_total, n, hrcomm::kFloat, hrcomm::kSum, c->comm, c->stream));
    c->allreduces++;
    return HR_OK;   // total_valid is set by the callers once the collective is known to be enqueued (group end)
}
int hr_allreduce_accumulator(hr_ctx *c) {
    if (!c) return fail(HR_ERR_INVALID, "hr_allreduce_accumulator: null ctx");
    int rc = allreduce_enqueue(c);
    if (rc == HR_OK) c->total_valid = true;
    return rc;
}
int hr_allreduce_accumulators(hr_ctx **ctxs, int n) {
    if (!ctxs || n < 1) return fail(HR_ERR_INVALID, "hr_allreduce_accumulators: bad argument");
    for (int i = 0; i < n; i++)
        if (!ctxs[i] || (!ctxs[i]->comm && ctxs[i]->same_device_peers.empty())) return fail(HR_ERR_INVALID, "hr_allreduce_accumulators: context %d has no communicator", i);
    if (!ctxs[0]->same_device_peers.empty()) {
        for (int i = 0; i < n; i++) { int rc = allreduce_enqueue(ctxs[i]); if (rc) return rc; }
        return HR_OK;
    }
    NCCL_TRY(hrcomm::api().GroupStart());
    int rc = HR_OK;
    for (int i = 0; i < n && rc == HR_OK; i++) rc = allreduce_enqueue(ctxs[i]);
    int r_ = hrcomm::api().GroupEnd();
    if (rc) return rc;
    if (r_ != 0) return fail(HR_ERR_DEVICE, "ncclGroupEnd failed: %s", hrcomm::api().GetErrorString(r_));
    for (int i = 0; i < n; i++) ctxs[i]->total_valid = true;
    return HR_OK;
}
void *hr_total_device_ptr(hr_ctx *c) { return c && c->total_valid ? c->accum_total : nullptr; }

// ---- hr_fold_statistics: every additive plane moves to rank 0 ------------------------------------------------
// The planes a fold moves — the accumulator, and each option's plane while the option is on — in the order they are folded, with the RCCL type
// of their elements.  FOLD_PLANES is the one list of them: the same-device kernel launches, the reduces and the non-roots' memsets walk it.
struct FoldPlane { const Plane *plane; int dtype; };
static const FoldPlane FOLD_PLANES[] = {{&ACCUM_OWN, hrcomm::kFloat}, {&MOMENTS, hrcomm::kDouble}, {&COUNTS, hrcomm::kUint32}, {&BUCKETS, hrcomm::kDouble}};
static void *fold_plane_ptr(hr_ctx *c, const Plane &p) { return &p == &ACCUM_OWN ? (void *)c->accum : (p.on && !(c->*p.on)) ? nullptr : *p.slot(c); }

__device__ __forceinline__ void fold_add(double2 &a, const double2 &b) { a.x += b.x; a.y += b.y; }
__device__ __forceinline__ void fold_add(float4 &a, const float4 &b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ void fold_add(uint4 &a, const uint4 &b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
template <class T> struct FoldVec;
template <> struct FoldVec<double> { typedef double2 type; };
template <> struct FoldVec<float> { typedef float4 type; };
template <> struct FoldVec<uint32_t> { typedef uint4 type; };
// root[i] += peer[i]; peer[i] = 0 over n elements: a stream of 16-byte loads and stores over the first `nvec` vectors (the host hands over
// n / width, or 0 when one of the two buffers is not 16-byte aligned — a caller's bound accumulator may not be), a grid-stride loop under the
// capped grid, then the elements behind the vectors one by one.  Every element is read and written by exactly one thread: no atomics.
template <class T>
__global__ __launch_bounds__(256) void fold_plane_kernel(T *__restrict__ root, T *__restrict__ peer, size_t n, size_t nvec) {
    typedef typename FoldVec<T>::type V;
    const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    V *rv = reinterpret_cast<V *>(root), *pv = reinterpret_cast<V *>(peer);
    for (size_t i = first; i < nvec; i += step) {
        V a = rv[i];
        const V b = pv[i];
        fold_add(a, b);
        rv[i] = a;
        pv[i] = V{};
    }
    for (size_t i = nvec * (sizeof(V) / sizeof(T)) + first; i < n; i += step) {
        root[i] += peer[i];
        peer[i] = T(0);
    }
}
template <class T>
static hipError_t fold_plane_launch(void *root, void *peer, size_t n, hipStream_t st) {
    const size_t width = 16 / sizeof(T);
    const size_t nvec = ((uintptr_t)root | (uintptr_t)peer) % 16 ? 0 : n / width;
    const size_t threads = nvec ? nvec + (n - nvec * width) : n;   // (a thread per vector; the tail is shorter than one vector)
    const unsigned grid = (unsigned)std::min<size_t>(2048, std::max<size_t>(1, (threads + 255) / 256));
    hipLaunchKernelGGL(fold_plane_kernel<T>, dim3(grid), dim3(256), 0, st, (T *)root, (T *)peer, n, nvec);
    return hipGetLastError();
}

// What a fold asks of one context, before anything is touched (`who`: the entry point).
static int fold_refusal(hr_ctx *c, const char *who) {
    if (!c) return fail(HR_ERR_INVALID, "%s: null ctx", who);
    if (!c->comm && c->same_device_peers.empty()) return fail(HR_ERR_INVALID, "%s: no communicator (hr_comm_init_rank / hr_comm_init_local)", who);
    if (!c->accum || !c->W) return fail(HR_ERR_NO_TARGET, "%s: no accumulator (hr_set_resolution not called)", who);
    if (c->robust_on && !c->bucket_by_sampling)
        return fail(HR_ERR_INVALID, "%s: robust_buckets is on with bucket_by_sampling 0 — buckets indexed by each pixel's ordinal do not add up across contexts "
                    "(rank r's j-th sampling is not the j-th overall); set option bucket_by_sampling 1 on every context before it renders", who);
    return HR_OK;
}
// ... and of the contexts of one group among each other: `ctxs` are the group's, all of them, in rank order
static int fold_group_refusal(hr_ctx **ctxs, int n, const char *who) {
    if (!ctxs || n < 1) return fail(HR_ERR_INVALID, "%s: bad argument", who);
    for (int i = 0; i < n; i++) { int rc = fold_refusal(ctxs[i], who); if (rc) return rc; }
    const hr_ctx *a = ctxs[0];
    if (n != a->comm_world) return fail(HR_ERR_INVALID, "%s: %d contexts were given, the group has %d", who, n, a->comm_world);
    for (int i = 0; i < n; i++) {
        const hr_ctx *p = ctxs[i];
        if (p->comm_world != n || p->comm_rank != i || p->comm_path != a->comm_path || p->comm_group != a->comm_group || (!a->same_device_peers.empty() && a->same_device_peers[i] != p))
            return fail(HR_ERR_INVALID, "%s: context %d is not rank %d of the group of context 0 (the group's contexts, in the order hr_comm_init_local took them)", who, i, i);
        if (p->W != a->W || p->H != a->H || p->RX != a->RX || p->RY != a->RY || p->RW != a->RW || p->RH != a->RH)
            return fail(HR_ERR_INVALID, "%s: the contexts of the group differ in resolution or region", who);
        if (p->moments_on != a->moments_on || p->counts_on != a->counts_on || p->robust_on != a->robust_on || p->robust_k != a->robust_k)
            return fail(HR_ERR_INVALID, "%s: the contexts of the group differ in the options moments, sample_counts or robust_buckets (context %d: %d / %d / %u, context 0: %d / %d / %u)", who, i,
                        (int)p->moments_on, (int)p->counts_on, p->robust_k, (int)a->moments_on, (int)a->counts_on, a->robust_k);
    }
    return HR_OK;
}
// what holds on every rank after a fold: the planes changed hands, so nothing made of them stands
static void fold_invalidate(hr_ctx *c) { changed(c, SRC_ACCUM | SRC_MOMENTS | SRC_COUNTS | SRC_BUCKETS); }
// One device: for k = 1 .. n-1 in rank order root += peer_k, peer_k = 0, plane by plane — ((r0 + r1) + r2) .. to the bit.  Ordered as
// allreduce_enqueue orders its sum: every context's render work is waited for, the kernels run on rank 0's stream, and they are finished
// before the call returns (they write the PEERS' planes: a peer's next hr_render must not race with them).
static int fold_same_device(hr_ctx **ctxs, int n) {
    hr_ctx *root = ctxs[0];
    HIP_TRY(hipSetDevice(root->device));
    for (int i = n - 1; i >= 0; i--) { int rc = sync_all(ctxs[i]); if (rc) return rc; }
    EventPair ev;
    HIP_TRY(timed_begin(ev, root->stream));
    hipError_t e = hipSuccess;
    for (int k = 1; k < n && e == hipSuccess; k++)
        for (const FoldPlane &f : FOLD_PLANES) {
            void *to = fold_plane_ptr(root, *f.plane), *from = fold_plane_ptr(ctxs[k], *f.plane);
            if (!to || !from || e != hipSuccess) continue;
            const size_t elems = plane_elems(root, *f.plane);
            e = f.dtype == hrcomm::kFloat ? fold_plane_launch<float>(to, from, elems, root->stream) :
                f.dtype == hrcomm::kDouble ? fold_plane_launch<double>(to, from, elems, root->stream) : fold_plane_launch<uint32_t>(to, from, elems, root->stream);
        }
    HIP_TRY(timed_end(e, ev, root->stream, root->post_events));
    HIP_TRY(hipStreamSynchronize(root->stream));
    for (int k = 1; k < n; k++) {
        root->moments_n += ctxs[k]->moments_n; ctxs[k]->moments_n = 0;
        root->buckets_n += ctxs[k]->buckets_n; ctxs[k]->buckets_n = 0;
    }
    for (int i = 0; i < n; i++) fold_invalidate(ctxs[i]);
    return drain_events(root);
}
// RCCL: per plane one ncclReduce in place to root 0 behind the render work on each context's stream, the two counts as a 2-word u64 buffer through
// the same reduce, then the non-roots' planes are zeroed on their streams.  `group`: one thread drives several ranks — their calls sit between
// ncclGroupStart and ncclGroupEnd.  The summation order is RCCL's.
static int fold_rccl(hr_ctx **ctxs, int n, bool group) {
    const hrcomm::Api &api = hrcomm::api();
    CallScratch scratch;
    std::vector<uint64_t *> d_n(n, nullptr);
    std::vector<uint64_t> h_n((size_t)n * 2);
    for (int i = 0; i < n; i++) {
        hr_ctx *c = ctxs[i];
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(scratch.alloc((void **)&d_n[i], 2 * sizeof(uint64_t)));
        h_n[i * 2] = c->moments_n; h_n[i * 2 + 1] = c->buckets_n;
        HIP_TRY(hipMemcpyAsync(d_n[i], &h_n[i * 2], 2 * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    }
    if (group) NCCL_TRY(api.GroupStart());
    int r_ = 0;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && !r_ && e == hipSuccess; i++) {
        hr_ctx *c = ctxs[i];
        if ((e = hipSetDevice(c->device)) != hipSuccess) break;
        for (const FoldPlane &f : FOLD_PLANES) {
            void *p = fold_plane_ptr(c, *f.plane);
            if (p && !r_) r_ = api.Reduce(p, p, plane_elems(c, *f.plane), f.dtype, hrcomm::kSum, 0, c->comm, c->stream);
        }
        if (!r_) r_ = api.Reduce(d_n[i], d_n[i], 2, hrcomm::kUint64, hrcomm::kSum, 0, c->comm, c->stream);
    }
    const int g_ = group ? api.GroupEnd() : 0;
    if (e != hipSuccess) return fail(HR_ERR_DEVICE, "hr_fold_statistics: %s", hipGetErrorString(e));
    if (r_ || g_) return fail(HR_ERR_DEVICE, "hr_fold_statistics: %s failed: %s", r_ ? "ncclReduce" : "ncclGroupEnd", api.GetErrorString(r_ ? r_ : g_));
    for (int i = 0; i < n; i++) {
        hr_ctx *c = ctxs[i];
        HIP_TRY(hipSetDevice(c->device));
        if (c->comm_rank != 0) {
            for (const FoldPlane &f : FOLD_PLANES)
                if (void *p = fold_plane_ptr(c, *f.plane)) HIP_TRY(hipMemsetAsync(p, 0, plane_bytes(c, *f.plane), c->stream));
        } else
            HIP_TRY(hipMemcpyAsync(&h_n[i * 2], d_n[i], 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    for (int i = 0; i < n; i++) {
        hr_ctx *c = ctxs[i];
        HIP_TRY(hipSetDevice(c->device));
        int rc = sync_all(c);
        if (rc) return rc;
        c->moments_n = c->comm_rank == 0 ? h_n[i * 2] : 0;
        c->buckets_n = c->comm_rank == 0 ? h_n[i * 2 + 1] : 0;
        fold_invalidate(c);
    }
    return HR_OK;
}
int hr_fold_statistics_group(hr_ctx **ctxs, int n) {
    static const char *const who = "hr_fold_statistics_group";
    int rc = fold_group_refusal(ctxs, n, who);
    if (rc) return rc;
    const bool same_device = !ctxs[0]->same_device_peers.empty();
    if (!same_device && !hrcomm::load()) return fail(HR_ERR_UNSUPPORTED, "%s", hrcomm::api().error.c_str());
    rc = same_device ? fold_same_device(ctxs, n) : fold_rccl(ctxs, n, true);
    // a fold that fails on the way (HR_ERR_DEVICE) may have moved some planes and not others, and the counts not at all: nothing made of them
    // stands on any rank, and the group's statistics are the host's to start over (hr_clear)
    if (rc) for (int i = 0; i < n; i++) fold_invalidate(ctxs[i]);
    return rc;
}
int hr_fold_statistics(hr_ctx *c) {
    static const char *const who = "hr_fold_statistics";
    int rc = fold_refusal(c, who);
    if (rc) return rc;
    // a context of a same-device group knows its peers: the fold is the group's, whichever of them asks
    if (!c->same_device_peers.empty()) return hr_fold_statistics_group(c->same_device_peers.data(), (int)c->same_device_peers.size());
    if (c->comm_path == HR_COMM_RCCL_GROUP && c->comm_world > 1)
        return fail(HR_ERR_INVALID, "%s: this context is one of %d that one process drives (hr_comm_init_local): hr_fold_statistics_group folds them in one RCCL group", who, c->comm_world);
    if (!hrcomm::load()) return fail(HR_ERR_UNSUPPORTED, "%s", hrcomm::api().error.c_str());
    if ((rc = fold_rccl(&c, 1, false))) fold_invalidate(c);   // (as in the group form: a fold that failed on the way leaves nothing to trust)
    return rc;
}

// What the communicator says about itself — asked of RCCL, not remembered from the init call: the evidence a bench line needs that
// its all-reduce ran over N ranks (ncclCommCount / ncclCommUserRank / ncclCommCuDevice / ncclGetVersion).
int hr_comm_info(hr_ctx *c, hr_comm_info_t *out) {
    if (!c || !out) return fail(HR_ERR_INVALID, "hr_comm_info: null argument");
    memset(out, 0, sizeof *out);
    out->path = c->comm_path; out->device = c->device; out->allreduces = c->allreduces;
    if (c->comm) {
        int v = 0;
        NCCL_TRY(hrcomm::api().CommCount(c->comm, &v)); out->nranks = v;
        NCCL_TRY(hrcomm::api().CommUserRank(c->comm, &v)); out->rank = v;
        NCCL_TRY(hrcomm::api().CommCuDevice(c->comm, &v)); out->device = v;
        NCCL_TRY(hrcomm::api().GetVersion(&v)); out->rccl_version = v;
    } else if (!c->same_device_peers.empty()) {
        out->nranks = (int32_t)c->same_device_peers.size(); out->rank = c->comm_rank;
    }
    return HR_OK;
}

int hr_comm_library(char *path_out, size_t cap, int *reused_out) {
    if (!path_out || !cap) return fail(HR_ERR_INVALID, "hr_comm_library: null argument");
    if (!hrcomm::load()) return fail(HR_ERR_UNSUPPORTED, "%s", hrcomm::api().error.c_str());
    snprintf(path_out, cap, "%s", hrcomm::api().path.c_str());
    if (reused_out) *reused_out = hrcomm::api().reused ? 1 : 0;
    return HR_OK;
}

// Sum of an accumulator in f64, per channel, on the device: sum_of(rank's own accumulators) == sum(all-reduced total) is the checksum of
// the exchange (bench.py multi_gpu.checksum).  Deterministic: a fixed grid, every workgroup leaves its partial sums (waves in order), the
// host adds the 1,024 partial sums in order — two contexts that hold the same total report the same sum to the last bit.
static const unsigned ACC_SUM_BLOCKS = 1024;
__global__ __launch_bounds__(256) void accumulator_sum_kernel(const float *__restrict__ a, size_t pixels, double *__restrict__ out) {
    double s[3] = {0.0, 0.0, 0.0};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (size_t)gridDim.x * blockDim.x) {
        s[0] += (double)a[i * 3]; s[1] += (double)a[i * 3 + 1]; s[2] += (double)a[i * 3 + 2];
    }
    __shared__ double part[4][3];
    for (int k = 0; k < 3; k++) {
        double x = s[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) out[blockIdx.x * 3 + threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}
int hr_accumulator_sum(hr_ctx *c, int which, double out_rgb[3]) {
    if (!c || !out_rgb || which < 0 || which > 1) return fail(HR_ERR_INVALID, "hr_accumulator_sum: bad argument (which: 0 = this context's own accumulator, 1 = the all-reduced total)");
    if (!c->accum || !c->W) return fail(HR_ERR_NO_TARGET, "hr_accumulator_sum: no accumulator");
    if (which == 1 && !c->total_valid) return fail(HR_ERR_INVALID, "hr_accumulator_sum: no all-reduced total (hr_allreduce_accumulator first)");
    int rc = hr_synchronize(c);
    if (rc) return rc;
    CallScratch scratch;
    double *d = nullptr;
    std::vector<double> h(ACC_SUM_BLOCKS * 3);
    HIP_TRY(scratch.alloc((void **)&d, h.size() * sizeof(double)));
    hipLaunchKernelGGL(accumulator_sum_kernel, dim3(ACC_SUM_BLOCKS), dim3(256), 0, c->stream, which ? c->accum_total : c->accum, region_pixels(c), d);
    HIP_TRY_AS("hr_accumulator_sum", hipGetLastError());
    HIP_TRY_AS("hr_accumulator_sum", hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY_AS("hr_accumulator_sum", hipStreamSynchronize(c->stream));
    out_rgb[0] = out_rgb[1] = out_rgb[2] = 0.0;
    for (unsigned b = 0; b < ACC_SUM_BLOCKS; b++) for (int k = 0; k < 3; k++) out_rgb[k] += h[b * 3 + k];
    return HR_OK;
}

// ---- option "moments": the moments, and the noise estimate made of them (noise_core.h) ----
int hr_read_moments(hr_ctx *c, double *host, uint64_t *samplings) {
    int rc = option_plane_read(c, MOMENTS, "hr_read_moments", host);
    if (rc) return rc;
    if (samplings) *samplings = c->moments_n;
    return HR_OK;
}
int hr_write_moments(hr_ctx *c, const double *host, uint64_t samplings) {
    int rc = option_plane_write(c, MOMENTS, "hr_write_moments", host);
    if (rc) return rc;
    c->moments_n = samplings;
    return HR_OK;
}

static int select_out_buffer(hr_ctx *c) {
    if (!c->d_select_out) HIP_TRY(hipMalloc((void **)&c->d_select_out, 3 * sizeof(uint32_t)));
    return HR_OK;
}
// mm[0], mm[1]: the smallest and the largest count of the region
static int counts_range(hr_ctx *c, uint32_t mm[2]) {
    const size_t pixels = region_pixels(c);
    int rc = select_out_buffer(c);
    if (rc) return rc;
    mm[0] = 0xffffffffu; mm[1] = 0u;
    HIP_TRY(hipMemcpyAsync(c->d_select_out + 1, mm, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (mm is the caller's: on a stack)
    hipLaunchKernelGGL(counts_min_kernel, dim3((unsigned)std::min<size_t>((pixels + 255) / 256, 1024)), dim3(256), 0, c->stream, c->counts, pixels, c->d_select_out + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mm, c->d_select_out + 1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HR_OK;
}
static int counts_cover_an_estimate(hr_ctx *c, const char *who) {
    uint32_t mm[2];
    int rc = counts_range(c, mm);
    if (rc) return rc;
    if (mm[0] < 2) return fail(HR_ERR_INVALID, "%s: a pixel of the region has received %u samplings (option sample_counts), a variance needs 2", who, mm[0]);
    // counts and moments that do not cover the same samplings (written apart, or one of them replaced by the host): n would be wrong, silently
    if ((uint64_t)mm[1] > c->moments_n)
        return fail(HR_ERR_INVALID, "%s: a pixel has received %u samplings but the moments cover %llu (the counts and the moments must cover the same samplings)", who, mm[1], (unsigned long long)c->moments_n);
    return HR_OK;
}
// the floor and the threshold of an estimate or a selection (`who`)
static int floor_and_threshold_ok(const char *who, double floor, double threshold) {
    if (!(floor > 0.0) || !(floor < INFINITY)) return fail(HR_ERR_INVALID, "%s: floor must be a positive finite radiance", who);
    if (!(threshold >= 0.0)) return fail(HR_ERR_INVALID, "%s: threshold must not be negative", who);
    return HR_OK;
}
// the samplings behind the moments cover a variance (`who`); needs_resolve_scale: and fit the scale the resolve of a denoised image works with
static int moments_cover_an_estimate(const hr_ctx *c, const char *who, bool needs_resolve_scale) {
    if (!c->counts && c->moments_n < 2) return fail(HR_ERR_INVALID, "%s: %llu samplings behind the moments, a variance needs 2", who, (unsigned long long)c->moments_n);
    if (needs_resolve_scale && c->moments_n >= (1ull << 30)) return fail(HR_ERR_INVALID, "%s: %llu samplings do not fit the resolve's 32-bit scale", who, (unsigned long long)c->moments_n);
    return HR_OK;
}
// The host side of an estimate's summary (summary_block_reduce, post_kernels.h) for one call: the kernel's out[SUMMARY_BLOCKS] = {sum, max, above}
// in the call's scratch, their copy to the host on c->stream and, once that stream is synchronised, the summary: the blocks added in index order.
struct BlockSummaries {
    double *dev = nullptr;
    std::vector<double> host = std::vector<double>(SUMMARY_BLOCKS * 3);
    hipError_t alloc(CallScratch &scratch) { return scratch.alloc((void **)&dev, host.size() * sizeof(double)); }
    hipError_t fetch(const hr_ctx *c) { return hipMemcpyAsync(host.data(), dev, host.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream); }
    void summary(uint64_t samplings, size_t pixels, hr_noise *est) const {
        double sum = 0.0, mx = 0.0, above = 0.0;
        for (size_t b = 0; b < SUMMARY_BLOCKS; b++) { sum += host[b * 3]; mx = host[b * 3 + 1] > mx ? host[b * 3 + 1] : mx; above += host[b * 3 + 2]; }
        est->samplings = samplings;
        est->pixels = (uint64_t)pixels;
        est->pixels_above = (uint64_t)above;
        est->mean_error = sum / (double)pixels;
        est->max_error = mx;
    }
};
// host_img: the image as well (or NULL); est: the summary (or NULL)
static int noise_run(hr_ctx *c, const char *who, double floor, double threshold, double *host_img, hr_noise *est) {
    int rc = plane_ready(c, MOMENTS, who);
    if (rc) return rc;
    if ((rc = floor_and_threshold_ok(who, floor, threshold))) return rc;
    if ((rc = moments_cover_an_estimate(c, who, false))) return rc;
    if ((rc = hr_synchronize(c))) return rc;
    if (c->counts && (rc = counts_cover_an_estimate(c, who))) return rc;
    const size_t pixels = region_pixels(c);
    if (!c->noise_img && (rc = plane_alloc(c, NOISE_IMG))) return rc;
    CallScratch scratch;
    BlockSummaries blocks;
    HIP_TRY(blocks.alloc(scratch));
    if (c->counts) hipLaunchKernelGGL(noise_kernel<true>, dim3(SUMMARY_BLOCKS), dim3(256), 0, c->stream, c->moments, pixels, c->moments_n, floor, threshold, c->noise_img, blocks.dev, c->counts);
    else hipLaunchKernelGGL(noise_kernel<false>, dim3(SUMMARY_BLOCKS), dim3(256), 0, c->stream, c->moments, pixels, c->moments_n, floor, threshold, c->noise_img, blocks.dev, (const uint32_t *)nullptr);
    HIP_TRY_AS(who, hipGetLastError());
    HIP_TRY_AS(who, blocks.fetch(c));
    if (host_img) HIP_TRY_AS(who, hipMemcpyAsync(host_img, c->noise_img, plane_bytes(c, NOISE_IMG), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY_AS(who, hipStreamSynchronize(c->stream));
    if (est) blocks.summary(c->moments_n, pixels, est);
    return HR_OK;
}
int hr_noise_estimate(hr_ctx *c, double floor, double threshold, hr_noise *out) {
    if (c && !out) return fail(HR_ERR_INVALID, "hr_noise_estimate: null argument");
    return noise_run(c, "hr_noise_estimate", floor, threshold, nullptr, out);
}
int hr_read_noise_image(hr_ctx *c, double floor, double *host) {
    if (c && !host) return fail(HR_ERR_INVALID, "hr_read_noise_image: null argument");
    return noise_run(c, "hr_read_noise_image", floor, 0.0, host, nullptr);
}

// ---- option "sample_counts", the tile mask and the selection of tiles (adapt_core.h) ----
int hr_read_sample_counts(hr_ctx *c, uint32_t *host) { return option_plane_read(c, COUNTS, "hr_read_sample_counts", host); }
int hr_write_sample_counts(hr_ctx *c, const uint32_t *host) { return option_plane_write(c, COUNTS, "hr_write_sample_counts", host); }

// The resolve behind hr_resolve (every pixel scaled by 1 / (4 samplings)) and hr_resolve_counted (samplings == 0: by its own count): the first
// kernel differs, the rest is one.  The region's accumulator is resolved as an image of its own: the bilateral filter's clamp and wrap act at
// the region's edges.
// `radiance` (hr_resolve_denoised): that image instead of an accumulator, with the scale 1.0f.
static int resolve_region(hr_ctx *c, uint32_t samplings, uint8_t *host_rgb8, const float *radiance = nullptr) {
    int rc = hr_synchronize(c);
    if (rc) return rc;
    const uint32_t n = (uint32_t)region_pixels(c);
    const float *acc = c->total_valid ? c->accum_total : c->accum;
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    if (radiance) hipLaunchKernelGGL(tonemap_gamma_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, radiance, c->post_tmp, n, 1.0f);
    else if (samplings) hipLaunchKernelGGL(tonemap_gamma_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, acc, c->post_tmp, n, 1.0f / (float)(samplings * 4u));
    else hipLaunchKernelGGL(tonemap_gamma_counted_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, acc, c->counts, c->post_tmp, n);
    hipLaunchKernelGGL(bilateral_quantise_kernel, dim3((c->RW + 31) / 32, (c->RH + 7) / 8), dim3(32, 8), 0, c->stream, c->post_tmp, c->d_rgb8, c->RW, c->RH);
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->post_events));
    HIP_TRY(hipMemcpyAsync(host_rgb8, c->d_rgb8, plane_bytes(c, RGB8), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return drain_events(c);
}
int hr_resolve(hr_ctx *c, uint32_t samplings, uint8_t *host_rgb8) {
    if (!c || !host_rgb8 || !samplings) return fail(HR_ERR_INVALID, "hr_resolve: bad argument");
    if (!c->accum) return fail(HR_ERR_NO_TARGET, "hr_resolve: no accumulator");
    return resolve_region(c, samplings, host_rgb8);
}
int hr_resolve_counted(hr_ctx *c, uint8_t *host_rgb8) {
    int rc = plane_ready(c, COUNTS, "hr_resolve_counted");
    if (rc) return rc;
    if (!host_rgb8) return fail(HR_ERR_INVALID, "hr_resolve_counted: null argument");
    if (!c->accum) return fail(HR_ERR_NO_TARGET, "hr_resolve_counted: no accumulator");
    return resolve_region(c, 0, host_rgb8);
}
// the resolve of a derived image's (float) radiance plane behind hr_resolve_* (`who`)
static int image_resolve(hr_ctx *c, ImageId id, const char *who, uint8_t *host_rgb8) {
    int rc = image_ready(c, id, who, host_rgb8);
    return rc ? rc : resolve_region(c, 0, host_rgb8, (const float *)*IMAGES[id].plane->slot(c));
}

// ---- the denoiser: guide planes, the à-trous filter and its resolve (denoise_core.h) ----
int hr_denoise_default_params(hr_denoise_params *out) {
    if (!out) return fail(HR_ERR_INVALID, "hr_denoise_default_params: null argument");
    memset(out, 0, sizeof *out);
    out->levels = 4; out->demodulate = 1;
    out->sigma_color = 3.0; out->sigma_normal = 0.5; out->sigma_albedo = 0.25; out->sigma_depth = 0.1;
    return HR_OK;
}
// One pinhole pass over the whole region, whatever tile mask is set, into the guide planes (stored, not added).  Nothing else is touched: not the
// accumulator, the moments, the counts or hr_stats.paths; its time goes to debug_kernel_ms / debug_launches.  Option "guide_bounces" = K > 0:
// guide_chain_kernel follows mirrors and glass for up to K bounces; 0 is guide_render_kernel, the first hit's planes.
int hr_render_guides(hr_ctx *c) {
    if (!c) return fail(HR_ERR_INVALID, "hr_render_guides: null ctx");
    int rc;
    if ((rc = debug_refusal(c, "hr_render_guides", A_SCENE)) || (rc = debug_refusal(c, "hr_render_guides", A_TARGET))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    changed(c, SRC_GUIDES);
    if (!c->guides && (rc = plane_alloc(c, GUIDES))) return rc;
    const GuideRenderFn fn = select_guide_render_kernel(c->dsc.qnodes != nullptr);
    const GuideChainFn chain = select_guide_chain_kernel(c->dsc.qnodes != nullptr);
    if (c->guide_bounces ? !chain : !fn) return fail(HR_ERR_UNSUPPORTED, "hr_render_guides: no kernel instantiation for this node format (kernel_variants.h)");
    if ((rc = c->guide_bounces ? launch_tile_pass(c, chain, c->guide_bounces, c->guides) : launch_tile_pass(c, fn, c->guides))) return rc;
    image_made(c, GUIDE_IMAGE);
    return HR_OK;
}
// hr_render_guides with the planes averaged over `lens_points` (4 or 16) points of the thin lens per sub-sample: guide_lens_kernel, one launch, the
// same contract and accounting.  A camera without an aperture has one lens point: the call is hr_render_guides then, to the bit.  What is refused is
// refused before anything is touched: the planes and what was filtered with them stay.
int hr_render_guides_lens(hr_ctx *c, uint32_t lens_points) {
    if (!c) return fail(HR_ERR_INVALID, "hr_render_guides_lens: null ctx");
    if (!guide_lens_count_ok(lens_points)) return fail(HR_ERR_INVALID, "hr_render_guides_lens: lens_points must be 4 or 16");
    int rc;
    if ((rc = debug_refusal(c, "hr_render_guides_lens", A_SCENE)) || (rc = debug_refusal(c, "hr_render_guides_lens", A_TARGET))) return rc;
    if (c->dsc.cam.lens_radius == 0.0f) return hr_render_guides(c);
    HIP_TRY(hipSetDevice(c->device));
    const GuideLensFn fn = select_guide_lens_kernel(c->dsc.qnodes != nullptr);
    if (!fn) return fail(HR_ERR_UNSUPPORTED, "hr_render_guides_lens: no kernel instantiation for this node format (kernel_variants.h)");
    changed(c, SRC_GUIDES);
    if (!c->guides && (rc = plane_alloc(c, GUIDES))) return rc;
    if ((rc = launch_tile_pass(c, fn, c->guide_bounces, lens_points, c->guides))) return rc;
    image_made(c, GUIDE_IMAGE);
    return HR_OK;
}
// the table of guide_lens_point (pt_core.h): uv = {u0, v0, u1, v1, ..}; needs no device
int hr_guide_lens_points(int lens_shape, uint32_t lens_points, float *uv) {
    if (!uv) return fail(HR_ERR_INVALID, "hr_guide_lens_points: null argument");
    if (lens_shape != 0 && lens_shape != 1) return fail(HR_ERR_INVALID, "hr_guide_lens_points: lens_shape must be 0 (square) or 1 (circle)");
    if (!guide_lens_count_ok(lens_points)) return fail(HR_ERR_INVALID, "hr_guide_lens_points: lens_points must be 4 or 16");
    for (uint32_t i = 0; i < lens_points; i++) guide_lens_point(lens_shape, lens_points, i, uv[2 * i], uv[2 * i + 1]);
    return HR_OK;
}
int hr_read_guides(hr_ctx *c, float *host) { return image_read(c, GUIDE_IMAGE, "hr_read_guides", host); }
int hr_write_guides(hr_ctx *c, const float *host) {
    if (!c || !host) return fail(HR_ERR_INVALID, "hr_write_guides: null argument");
    if (!c->accum || !c->W) return fail(HR_ERR_NO_TARGET, "hr_write_guides: hr_set_resolution not called");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if (!c->guides && (rc = plane_alloc(c, GUIDES))) return rc;
    if ((rc = plane_write(c, GUIDES, c->guides, host))) return rc;   // (it says changed(SRC_GUIDES): the planes of before go with what was made of them)
    image_made(c, GUIDE_IMAGE);
    return HR_OK;
}
// the parameters of a denoiser (`who`), or the defaults, checked into `p`
static int denoise_params(const char *who, const hr_denoise_params *params, hr_denoise_params &p) {
    if (params) p = *params;
    else (void)hr_denoise_default_params(&p);
    if (p.levels > DENOISE_MAX_LEVELS) return fail(HR_ERR_INVALID, "%s: levels must be in [0,%u]", who, DENOISE_MAX_LEVELS);
    if (p.demodulate > 1u) return fail(HR_ERR_INVALID, "%s: demodulate must be 0 or 1", who);
    for (double s : {p.sigma_color, p.sigma_normal, p.sigma_albedo, p.sigma_depth})
        if (!(s > 0.0) || !(s < INFINITY)) return fail(HR_ERR_INVALID, "%s: every sigma must be positive and finite", who);
    return HR_OK;
}
// The à-trous run of both denoisers (`who`), whose checks are done and whose guide planes are there: D from the {C, V} plane that `init(grid, cv,
// demodulate)` — the caller's own launch on c->stream — fills, through p.levels levels and the final pass.  `made_of`: the source D is made of
// besides what every D is (IMAGES).  The scratch planes go with the call.
template <class Init>
static int atrous_run(hr_ctx *c, const char *who, const hr_denoise_params &p, uint32_t made_of, Init init) {
    int rc;
    const size_t pixels = region_pixels(c);
    if (!c->denoised && (rc = plane_alloc(c, DENOISED))) return rc;
    CallScratch scratch;
    double *cv[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++) HIP_TRY_AS(who, scratch.alloc((void **)&cv[k], pixels * 6 * sizeof(double)));
    changed(c, SRC_NEW_D);
    const DenoiseSigmas sg = denoise_sigmas(p.sigma_color, p.sigma_normal, p.sigma_albedo, p.sigma_depth);
    const int demodulate = p.demodulate && p.levels ? 1 : 0;   // without a level there is nothing to filter: D = (float)C, as the header says
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    const dim3 flat((unsigned)((pixels + 255) / 256)), tiles2d((c->RW + 31) / 32, (c->RH + 7) / 8);
    init(flat, cv[0], demodulate);
    for (uint32_t l = 0; l < p.levels; l++)
        hipLaunchKernelGGL(atrous_kernel, tiles2d, dim3(32, 8), 0, c->stream, cv[l & 1u], c->guides, cv[(l + 1u) & 1u], c->RW, c->RH, 1u << l, sg);
    hipLaunchKernelGGL(denoise_final_kernel, flat, dim3(256), 0, c->stream, cv[p.levels & 1u], c->guides, c->denoised, (uint32_t)pixels, demodulate);
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->post_events));
    HIP_TRY_AS(who, hipStreamSynchronize(c->stream));   // the scratch planes go with the call
    image_made(c, D_IMAGE, made_of);
    return drain_events(c);
}
int hr_denoise(hr_ctx *c, const hr_denoise_params *params) {
    static const char *const who = "hr_denoise";
    int rc = plane_ready(c, MOMENTS, who);
    if (rc) return rc;
    hr_denoise_params p;
    // what is refused is refused before anything is touched: the denoised image of an earlier call stays
    if ((rc = denoise_params(who, params, p))) return rc;
    if ((rc = moments_cover_an_estimate(c, who, true))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = hr_synchronize(c))) return rc;
    if (c->counts && (rc = counts_cover_an_estimate(c, who))) return rc;
    if ((rc = guides_or_render(c))) return rc;
    const uint32_t pixels = (uint32_t)region_pixels(c);
    return atrous_run(c, who, p, SRC_MOMENTS, [&](dim3 flat, double *cv, int demodulate) {
        hipLaunchKernelGGL(denoise_init_kernel, flat, dim3(256), 0, c->stream, c->accum, c->moments, c->counts, (uint32_t)c->moments_n, c->guides, cv, pixels, demodulate);
    });
}
int hr_read_denoised(hr_ctx *c, float *host) { return image_read(c, D_IMAGE, "hr_read_denoised", host); }
int hr_resolve_denoised(hr_ctx *c, uint8_t *host_rgb8) { return image_resolve(c, D_IMAGE, "hr_resolve_denoised", host_rgb8); }

// ---- temporal reuse: the motion plane and the gather of a frame's history along it (reproject_core.h) ----
int hr_reproject_default_params(hr_reproject_params *out) {
    if (!out) return fail(HR_ERR_INVALID, "hr_reproject_default_params: null argument");
    memset(out, 0, sizeof *out);
    out->max_history = 32; out->min_roughness = 0.3; out->depth_tolerance = 1e-3;
    return HR_OK;
}
// the parameters of hr_render_motion / hr_reproject (`who`), or the defaults, checked into `p`
static int reproject_params(const char *who, const hr_reproject_params *params, hr_reproject_params &p) {
    if (params) p = *params;
    else (void)hr_reproject_default_params(&p);
    if (!p.max_history) return fail(HR_ERR_INVALID, "%s: max_history must be positive", who);
    for (double v : {p.min_roughness, p.depth_tolerance})
        if (!(v >= 0.0) || !(v < INFINITY)) return fail(HR_ERR_INVALID, "%s: min_roughness and depth_tolerance must be finite and not negative", who);
    return HR_OK;
}
// One pass over the whole region, whatever tile mask is set, into the motion plane (stored): motion_kernel, one launch, hr_render_guides' contract and
// accounting.  `from`: the camera of the frame whose history is to be reused, as Camera::new builds it.
int hr_render_motion(hr_ctx *c, const hr_camera *from, const hr_reproject_params *params) {
    static const char *const who = "hr_render_motion";
    if (!c || !from) return fail(HR_ERR_INVALID, "%s: null argument", who);
    int rc;
    hr_reproject_params p;
    if ((rc = reproject_params(who, params, p))) return rc;
    if ((rc = debug_refusal(c, who, A_SCENE)) || (rc = debug_refusal(c, who, A_TARGET))) return rc;
    CameraF camf;
    CameraD camd;
    std::string ferr;
    if ((rc = flatten_camera(*from, camf, camd, ferr))) return fail(rc, "%s: %s", who, ferr.c_str());
    ReprojectCam rc0;
    for (int k = 0; k < 3; k++) { rc0.eye[k] = camd.eye[k]; rc0.forward[k] = camd.forward[k]; rc0.phr[k] = camd.phr[k]; rc0.phu[k] = camd.phu[k]; }
    rc0.focus = camd.focus_distance;
    HIP_TRY(hipSetDevice(c->device));
    const MotionFn fn = select_motion_kernel(c->dsc.qnodes != nullptr);
    if (!fn) return fail(HR_ERR_UNSUPPORTED, "%s: no kernel instantiation for this node format (kernel_variants.h)", who);
    c->made_of[MOTION_IMAGE] = 0;
    if (!c->motion && (rc = plane_alloc(c, MOTION))) return rc;
    if ((rc = launch_tile_pass(c, fn, rc0, (float)p.min_roughness, (float)p.depth_tolerance, c->motion))) return rc;
    image_made(c, MOTION_IMAGE);
    return HR_OK;
}
int hr_read_motion(hr_ctx *c, float *host) { return image_read(c, MOTION_IMAGE, "hr_read_motion", host); }
int hr_write_motion(hr_ctx *c, const float *host) {
    if (!c || !host) return fail(HR_ERR_INVALID, "hr_write_motion: null argument");
    if (!c->accum || !c->W) return fail(HR_ERR_NO_TARGET, "hr_write_motion: hr_set_resolution not called");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if (!c->motion && (rc = plane_alloc(c, MOTION))) return rc;
    if ((rc = plane_write(c, MOTION, c->motion, host))) return rc;
    image_made(c, MOTION_IMAGE);
    return HR_OK;
}
// The region's accumulator, counts and moments replaced by their history along the motion plane: reproject_kernel reads the call's copy of the three
// as they were and writes the planes in place.  What is refused is refused before anything is touched.
int hr_reproject(hr_ctx *c, const hr_reproject_params *params) {
    static const char *const who = "hr_reproject";
    int rc = plane_ready(c, COUNTS, who);
    if (rc) return rc;
    hr_reproject_params p;
    if ((rc = reproject_params(who, params, p))) return rc;
    if (c->robust_on) return fail(HR_ERR_UNSUPPORTED, "%s: not with option robust_buckets on (buckets are not carried along the motion plane)", who);
    if (c->mask_on) return fail(HR_ERR_INVALID, "%s: not while a tile mask is set (the history replaces every pixel of the region)", who);
    if (!c->motion || !image_valid(c, MOTION_IMAGE)) return fail(HR_ERR_INVALID, "%s: %s", who, IMAGES[MOTION_IMAGE].none);
    if (!c->accum) return fail(HR_ERR_NO_TARGET, "%s: no accumulator", who);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = hr_synchronize(c))) return rc;
    const bool with_moments = c->moments_on && c->moments;
    CallScratch scratch;
    float *old_acc = nullptr;
    uint32_t *old_counts = nullptr;
    double *old_mom = nullptr;
    HIP_TRY_AS(who, scratch.alloc((void **)&old_acc, plane_bytes(c, ACCUM_OWN)));
    HIP_TRY_AS(who, scratch.alloc((void **)&old_counts, plane_bytes(c, COUNTS)));
    if (with_moments) HIP_TRY_AS(who, scratch.alloc((void **)&old_mom, plane_bytes(c, MOMENTS)));
    HIP_TRY_AS(who, hipMemcpyAsync(old_acc, c->accum, plane_bytes(c, ACCUM_OWN), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY_AS(who, hipMemcpyAsync(old_counts, c->counts, plane_bytes(c, COUNTS), hipMemcpyDeviceToDevice, c->stream));
    if (with_moments) HIP_TRY_AS(who, hipMemcpyAsync(old_mom, c->moments, plane_bytes(c, MOMENTS), hipMemcpyDeviceToDevice, c->stream));
    changed(c, SRC_ACCUM | SRC_MOMENTS | SRC_COUNTS);
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    hipLaunchKernelGGL(reproject_kernel, dim3((c->RW + 31) / 32, (c->RH + 7) / 8), dim3(32, 8), 0, c->stream, c->motion, old_acc, old_counts, old_mom, c->RW, c->RH, p.max_history,
                       c->accum, c->counts, c->moments);
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->post_events));
    HIP_TRY_AS(who, hipStreamSynchronize(c->stream));   // the copies go with the call
    if (with_moments) {   // no count exceeds the samplings behind the moments: they become the largest count written
        uint32_t mm[2];
        if ((rc = counts_range(c, mm))) return rc;
        c->moments_n = mm[1];
    }
    return drain_events(c);
}

// ---- option "robust_buckets": the sample buckets and the firefly-robust resolve made of them (robust_core.h) ----
int hr_read_buckets(hr_ctx *c, double *host, uint64_t *samplings) {
    int rc = option_plane_read(c, BUCKETS, "hr_read_buckets", host);
    if (rc) return rc;
    if (samplings) *samplings = c->buckets_n;
    return HR_OK;
}
int hr_write_buckets(hr_ctx *c, const double *host, uint64_t samplings) {
    int rc = option_plane_write(c, BUCKETS, "hr_write_buckets", host);
    if (rc) return rc;
    c->buckets_n = samplings;
    return HR_OK;
}
int hr_robust(hr_ctx *c) {
    static const char *const who = "hr_robust";
    int rc = plane_ready(c, BUCKETS, who);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = hr_synchronize(c))) return rc;
    const RobustVariant *v = select_robust_kernel(c->robust_k);
    if (!v) return no_instantiation(who, "robust_kernel", c->robust_k);
    if (!c->robust && (rc = plane_alloc(c, ROBUST))) return rc;
    if (!c->robust_trim && (rc = plane_alloc(c, ROBUST_TRIM))) return rc;
    c->made_of[R_IMAGE] = 0;   // (R alone: R' is not made of R)
    const size_t pixels = region_pixels(c);
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    hipLaunchKernelGGL(v->fn, dim3((unsigned)((pixels + 255) / 256)), dim3(256), v->lds(), c->stream, c->buckets, c->counts, (unsigned long long)c->buckets_n, c->robust, c->robust_trim, pixels);
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->post_events));
    HIP_TRY_AS(who, hipStreamSynchronize(c->stream));
    image_made(c, R_IMAGE);
    return drain_events(c);
}
int hr_read_robust(hr_ctx *c, float *host) { return image_read(c, R_IMAGE, "hr_read_robust", host); }
int hr_read_robust_trim(hr_ctx *c, uint8_t *host) { return image_read(c, R_IMAGE, "hr_read_robust_trim", host, true); }
int hr_resolve_robust(hr_ctx *c, uint8_t *host_rgb8) { return image_resolve(c, R_IMAGE, "hr_resolve_robust", host_rgb8); }

// the mask's host side from its flags: the count of active tiles and of their in-region pixels
static void mask_totals(hr_ctx *c) {
    const uint32_t tx = (c->RW + 3) / 4, ty = (c->RH + 3) / 4;
    c->mask_active = 0; c->mask_pixels = 0;
    for (uint32_t y = 0; y < ty; y++)
        for (uint32_t x = 0; x < tx; x++)
            if (c->mask[(size_t)y * tx + x]) {
                c->mask_active++;
                c->mask_pixels += (uint64_t)std::min(4u, c->RW - 4u * x) * std::min(4u, c->RH - 4u * y);
            }
}
static int mask_buffers(hr_ctx *c, uint32_t tiles) {
    if (!c->d_tile_list) HIP_TRY(hipMalloc((void **)&c->d_tile_list, (size_t)tiles * sizeof(uint32_t)));
    if (!c->d_tile_flags) HIP_TRY(hipMalloc((void **)&c->d_tile_flags, (size_t)tiles * sizeof(uint32_t)));
    return select_out_buffer(c);
}
int hr_set_tile_mask(hr_ctx *c, const uint8_t *mask) {
    if (!c) return fail(HR_ERR_INVALID, "hr_set_tile_mask: null ctx");
    if (!c->W) return fail(HR_ERR_NO_TARGET, "hr_set_tile_mask: hr_set_resolution not called");
    if (!c->counts_on) return fail(HR_ERR_INVALID, "hr_set_tile_mask: option sample_counts is off (an image whose pixels have unequal counts cannot be resolved without them)");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);   // kernels of an earlier hr_render may still be reading the list
    if (rc) return rc;
    if (!mask) return remove_mask(c);
    const uint32_t tiles = ((c->RW + 3) / 4) * ((c->RH + 3) / 4);
    if ((rc = mask_buffers(c, tiles))) return rc;
    std::vector<uint32_t> flags(tiles), list;
    c->mask.assign(tiles, 0);
    for (uint32_t t = 0; t < tiles; t++)
        if (mask[t]) { c->mask[t] = 1; flags[t] = 1u; list.push_back(t); }   // ascending
    mask_totals(c);
    HIP_TRY(hipMemcpy(c->d_tile_flags, flags.data(), (size_t)tiles * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!list.empty()) HIP_TRY(hipMemcpy(c->d_tile_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->mask_on = true;
    return HR_OK;
}
int hr_get_tile_mask(hr_ctx *c, uint8_t *mask, uint32_t *active) {
    if (!c) return fail(HR_ERR_INVALID, "hr_get_tile_mask: null ctx");
    if (!c->W) return fail(HR_ERR_NO_TARGET, "hr_get_tile_mask: hr_set_resolution not called");
    const uint32_t tiles = ((c->RW + 3) / 4) * ((c->RH + 3) / 4);
    if (mask) { if (c->mask_on) memcpy(mask, c->mask.data(), tiles); else memset(mask, 1, tiles); }
    if (active) *active = c->mask_on ? c->mask_active : tiles;
    return HR_OK;
}

// The selection behind hr_select_tiles and hr_select_tiles_robust (`who`), whose checks are done: the flags by the rule (e_img == nullptr: the
// moments', else that image's), the compaction, the host's mask.
static int select_tiles_run(hr_ctx *c, const char *who, const double *e_img, double floor, double threshold, uint32_t *active) {
    int rc;
    RenderParams rp{};
    target_params(c, rp);
    const uint32_t tiles = rp.tiles_x * rp.tiles_y;
    if ((rc = mask_buffers(c, tiles))) return rc;
    const hipcub::CountingInputIterator<uint32_t> indices(0u);
    size_t need = 0;
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, need, indices, c->d_tile_flags, c->d_tile_list, c->d_select_out, (int)tiles, c->stream));
    if (need > c->select_tmp_bytes) {
        if ((rc = free_device(c->select_tmp))) return rc;
        c->select_tmp_bytes = 0;
        HIP_TRY(hipMalloc(&c->select_tmp, std::max<size_t>(need, 16)));
        c->select_tmp_bytes = std::max<size_t>(need, 16);
    }
    if (e_img) hipLaunchKernelGGL(select_tiles_image_kernel, dim3((tiles + 15) / 16), dim3(256), 0, c->stream, rp, e_img, threshold, c->mask_on ? 1 : 0, c->d_tile_flags);
    else hipLaunchKernelGGL(select_tiles_kernel, dim3((tiles + 15) / 16), dim3(256), 0, c->stream, rp, c->moments, c->counts, floor, threshold, c->mask_on ? 1 : 0, c->d_tile_flags);
    HIP_TRY(hipGetLastError());
    size_t bytes = c->select_tmp_bytes;
    HIP_TRY(hipcub::DeviceSelect::Flagged(c->select_tmp, bytes, indices, c->d_tile_flags, c->d_tile_list, c->d_select_out, (int)tiles, c->stream));
    std::vector<uint32_t> flags(tiles);
    uint32_t selected = 0;
    HIP_TRY(hipMemcpyAsync(flags.data(), c->d_tile_flags, (size_t)tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&selected, c->d_select_out, sizeof selected, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mask.assign(tiles, 0);
    for (uint32_t t = 0; t < tiles; t++) c->mask[t] = flags[t] ? 1 : 0;
    mask_totals(c);
    c->mask_on = true;
    if (selected != c->mask_active) return fail(HR_ERR_DEVICE, "%s: the compaction kept %u tiles, the flags say %u", who, selected, c->mask_active);
    if (active) *active = c->mask_active;
    return HR_OK;
}
int hr_select_tiles(hr_ctx *c, double floor, double threshold, uint32_t *active) {
    int rc = plane_ready(c, MOMENTS, "hr_select_tiles");
    if (rc) return rc;
    if ((rc = plane_ready(c, COUNTS, "hr_select_tiles"))) return rc;
    if ((rc = floor_and_threshold_ok("hr_select_tiles", floor, threshold))) return rc;
    if ((rc = hr_synchronize(c))) return rc;   // (also: no kernel is reading the list that is about to be rewritten)
    if ((rc = counts_cover_an_estimate(c, "hr_select_tiles"))) return rc;
    return select_tiles_run(c, "hr_select_tiles", nullptr, floor, threshold, active);
}

// What every call that takes the K bucket means of a pixel asks of the buckets (`who`), after its own checks: a sampling in each bucket of every
// pixel — without the counts K samplings behind the buckets; with them, read on the device behind the context's work (the call is synchronised on
// the way, as its callers always were at this point), K for every pixel and none beyond the samplings the buckets cover.
static int buckets_cover_every_pixel(hr_ctx *c, const char *who) {
    const uint32_t K = c->robust_k;
    if (!c->counts && c->buckets_n < K) return fail(HR_ERR_INVALID, "%s: %llu samplings behind the %u buckets, the bucket means need one in each", who, (unsigned long long)c->buckets_n, K);
    HIP_TRY(hipSetDevice(c->device));
    int rc = hr_synchronize(c);
    if (rc || !c->counts) return rc;
    uint32_t mm[2];
    if ((rc = counts_range(c, mm))) return rc;
    if (mm[0] < K) return fail(HR_ERR_INVALID, "%s: a pixel of the region has received %u samplings (option sample_counts), %u bucket means need one in each", who, mm[0], K);
    if ((uint64_t)mm[1] > c->buckets_n)
        return fail(HR_ERR_INVALID, "%s: a pixel has received %u samplings but the buckets cover %llu (the counts and the buckets must cover the same samplings)", who, mm[1], (unsigned long long)c->buckets_n);
    return HR_OK;
}

// ---- the robust noise estimate of the sample buckets, and the selection of tiles by it (robust_core.h) ----
// e_R of every pixel of the region into the context's robust noise planes, and its summary.  Everything that is refused is refused before anything
// is touched; nothing but those two planes is written.  need_counts: hr_select_tiles_robust (it also needs option sample_counts).
static int robust_noise_run(hr_ctx *c, const char *who, bool need_counts, double floor, double threshold, hr_noise *est) {
    int rc = plane_ready(c, BUCKETS, who);
    if (rc) return rc;
    if (need_counts && (rc = plane_ready(c, COUNTS, who))) return rc;
    if ((rc = floor_and_threshold_ok(who, floor, threshold))) return rc;
    const uint32_t K = c->robust_k;
    if ((rc = buckets_cover_every_pixel(c, who))) return rc;   // (synchronised — for the selection also: no kernel is reading the list that is about to be rewritten)
    const RobustNoiseVariant *v = select_robust_noise_kernel(K, ROBUST_NOISE_STAGED);
    if (!v) return no_instantiation(who, "robust_noise_kernel", K);
    const size_t pixels = region_pixels(c);
    if (!c->robust_noise_img && (rc = plane_alloc(c, ROBUST_NOISE_IMG))) return rc;
    if (!c->robust_noise_trim && (rc = plane_alloc(c, ROBUST_NOISE_TRIM))) return rc;
    CallScratch scratch;
    BlockSummaries blocks;
    HIP_TRY(blocks.alloc(scratch));
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    hipLaunchKernelGGL(v->fn, dim3(SUMMARY_BLOCKS), dim3(256), v->lds(), c->stream, c->buckets, c->counts, (unsigned long long)c->buckets_n, pixels, floor, threshold,
                       c->robust_noise_img, c->robust_noise_trim, blocks.dev);
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->post_events));
    HIP_TRY_AS(who, blocks.fetch(c));
    HIP_TRY_AS(who, hipStreamSynchronize(c->stream));
    if (est) blocks.summary(c->buckets_n, pixels, est);
    return drain_events(c);
}
int hr_robust_noise_estimate(hr_ctx *c, double floor, double threshold, hr_noise *out) {
    if (c && !out) return fail(HR_ERR_INVALID, "hr_robust_noise_estimate: null argument");
    return robust_noise_run(c, "hr_robust_noise_estimate", false, floor, threshold, out);
}
int hr_read_robust_noise_image(hr_ctx *c, double floor, double *host) {
    if (c && !host) return fail(HR_ERR_INVALID, "hr_read_robust_noise_image: null argument");
    int rc = robust_noise_run(c, "hr_read_robust_noise_image", false, floor, 0.0, nullptr);
    return rc ? rc : plane_read(c, ROBUST_NOISE_IMG, c->robust_noise_img, host);
}
int hr_read_robust_noise_trim(hr_ctx *c, double floor, uint8_t *host) {
    if (c && !host) return fail(HR_ERR_INVALID, "hr_read_robust_noise_trim: null argument");
    int rc = robust_noise_run(c, "hr_read_robust_noise_trim", false, floor, 0.0, nullptr);
    return rc ? rc : plane_read(c, ROBUST_NOISE_TRIM, c->robust_noise_trim, host);
}
int hr_select_tiles_robust(hr_ctx *c, double floor, double threshold, uint32_t *active) {
    int rc = robust_noise_run(c, "hr_select_tiles_robust", true, floor, threshold, nullptr);
    return rc ? rc : select_tiles_run(c, "hr_select_tiles_robust", c->robust_noise_img, floor, threshold, active);
}

// ---- the robust denoiser (robust_core.h, denoise_core.h): hr_denoise's levels on {C, V} of the sample buckets ----
// Everything that is refused is refused before anything is touched: D of an earlier call stays.  Nothing but D (and, without guide planes, the
// guides) is written: R, the buckets, the accumulator, the moments and the counts are read only or not at all.
int hr_denoise_robust(hr_ctx *c, const hr_denoise_params *params) {
    static const char *const who = "hr_denoise_robust";
    int rc = plane_ready(c, BUCKETS, who);
    if (rc) return rc;
    hr_denoise_params p;
    if ((rc = denoise_params(who, params, p))) return rc;
    const uint32_t K = c->robust_k;
    if ((rc = buckets_cover_every_pixel(c, who))) return rc;
    const RobustDenoiseInitVariant *v = select_robust_denoise_init_kernel(K);
    if (!v) return no_instantiation(who, "robust_denoise_init_kernel", K);
    if ((rc = guides_or_render(c))) return rc;
    const size_t pixels = region_pixels(c);
    return atrous_run(c, who, p, SRC_BUCKETS, [&](dim3 flat, double *cv, int demodulate) {   // (without a level: D = (float)C = R)
        hipLaunchKernelGGL(v->fn, flat, dim3(256), v->lds(), c->stream, c->buckets, c->counts, (unsigned long long)c->buckets_n, c->guides, cv, pixels, demodulate);
    });
}

// ---- the restored robust resolve (restore_core.h): R' = base + the trimmed buckets' excess, spread along the guide planes ----
// Everything that is refused is refused before anything is touched: R' of an earlier call stays.  Nothing but R' (and, without guide planes, the
// guides) is written: R, D, the buckets, the accumulator, the moments and the counts are read only or not at all.
int hr_restore_default_params(hr_restore_params *out) {
    if (!out) return fail(HR_ERR_INVALID, "hr_restore_default_params: null argument");
    memset(out, 0, sizeof *out);
    out->levels = 4; out->base = 0;
    out->sigma_n = 0.5; out->sigma_a = 0.25; out->sigma_z = 0.1;
    return HR_OK;
}
int hr_robust_restore(hr_ctx *c, const hr_restore_params *params) {
    static const char *const who = "hr_robust_restore";
    int rc = plane_ready(c, BUCKETS, who);
    if (rc) return rc;
    hr_restore_params p;
    if (params) p = *params;
    else (void)hr_restore_default_params(&p);
    if (p.levels > RESTORE_MAX_LEVELS) return fail(HR_ERR_INVALID, "%s: levels must be in [0,%u]", who, RESTORE_MAX_LEVELS);
    if (p.base > 1u) return fail(HR_ERR_INVALID, "%s: base must be 0 (the robust radiance) or 1 (the denoised robust radiance)", who);
    for (double s : {p.sigma_n, p.sigma_a, p.sigma_z})
        if (!(s > 0.0) || !(s < INFINITY)) return fail(HR_ERR_INVALID, "%s: every sigma must be positive and finite", who);
    if (p.base == 1u && !(c->denoised && (c->made_of[D_IMAGE] & SRC_BUCKETS)))
        return fail(HR_ERR_INVALID, "%s: base 1 needs a valid denoised image made by hr_denoise_robust", who);
    const uint32_t K = c->robust_k;
    if ((rc = buckets_cover_every_pixel(c, who))) return rc;
    const RestoreInitVariant *v = select_restore_init_kernel(K);
    if (!v) return no_instantiation(who, "restore_init_kernel", K);
    if ((rc = guides_or_render(c))) return rc;   // (base 1 never comes here: a valid D has valid guides)
    const size_t pixels = region_pixels(c);
    if (!c->restored && (rc = plane_alloc(c, RESTORED))) return rc;
    CallScratch scratch;
    double *cx = nullptr, *S = nullptr, *xp[2] = {nullptr, nullptr};
    HIP_TRY_AS(who, scratch.alloc((void **)&cx, pixels * 6 * sizeof(double)));
    if (p.levels) {
        HIP_TRY_AS(who, scratch.alloc((void **)&S, pixels * 3 * sizeof(double)));
        for (uint32_t k = 0; k < (p.levels > 1u ? 2u : 1u); k++) HIP_TRY_AS(who, scratch.alloc((void **)&xp[k], pixels * 3 * sizeof(double)));
    }
    c->made_of[RESTORED_IMAGE] = 0;
    const DenoiseSigmas sg = denoise_sigmas(1.0, p.sigma_n, p.sigma_a, p.sigma_z);
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    const dim3 flat((unsigned)((pixels + 255) / 256)), tiles2d((c->RW + 31) / 32, (c->RH + 7) / 8);
    hipLaunchKernelGGL(v->fn, flat, dim3(256), v->lds(), c->stream, c->buckets, c->counts, (unsigned long long)c->buckets_n, cx, pixels);
    const double *X = cx + 3;
    uint32_t xs = 6;
    for (uint32_t l = 0; l < p.levels; l++) {
        hipLaunchKernelGGL(spread_norm_kernel, tiles2d, dim3(32, 8), 0, c->stream, X, xs, c->guides, S, c->RW, c->RH, 1u << l, sg);
        hipLaunchKernelGGL(spread_gather_kernel, tiles2d, dim3(32, 8), 0, c->stream, S, c->guides, xp[l & 1u], c->RW, c->RH, 1u << l, sg);
        X = xp[l & 1u]; xs = 3;
    }
    hipLaunchKernelGGL(restore_final_kernel, flat, dim3(256), 0, c->stream, cx, p.base ? c->denoised : (const float *)nullptr, X, xs, c->restored, (uint32_t)pixels);
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->post_events));
    HIP_TRY_AS(who, hipStreamSynchronize(c->stream));   // the scratch planes go with the call
    image_made(c, RESTORED_IMAGE, p.base == 1u ? SRC_NEW_D : 0u);
    return drain_events(c);
}
int hr_read_restored(hr_ctx *c, float *host) { return image_read(c, RESTORED_IMAGE, "hr_read_restored", host); }
int hr_resolve_restored(hr_ctx *c, uint8_t *host_rgb8) { return image_resolve(c, RESTORED_IMAGE, "hr_resolve_restored", host_rgb8); }

// ---- the denoiser that picks its level per pixel (select_core.h): S and its level plane L ----
// Everything that is refused is refused before anything is touched: S of an earlier call stays.  Nothing but S, L (and, without guide planes, the
// guides) is written: D, R, R', the buckets, the accumulator, the moments and the counts are read only or not at all.
int hr_select_default_params(hr_select_params *out) {
    if (!out) return fail(HR_ERR_INVALID, "hr_select_default_params: null argument");
    memset(out, 0, sizeof *out);
    out->smooth = 2;   // the lowest worst case of tools/select_quality.py's table
    return HR_OK;
}
// What hr_denoise_select and the error estimate of its image (selected_noise_run) ask before they touch anything, in one order: the options, the
// parameters (p, s: the caller's or the defaults), the samplings behind the planes, then ft — {floor, threshold} of an estimate, or nullptr: none
// to check —, then the device's part: the counts, the init kernel's row (v), the guide planes (rendered when there are none).
// need_counts: hr_select_tiles_selected (it also needs option sample_counts).
static int select_ready(hr_ctx *c, const char *who, const hr_denoise_params *params, const hr_select_params *select, bool need_counts, const double *ft,
                        hr_denoise_params &p, hr_select_params &s, const SelectInitVariant *&v) {
    int rc = plane_ready(c, BUCKETS, who);
    if (rc || (rc = plane_ready(c, MOMENTS, who))) return rc;
    if (need_counts && (rc = plane_ready(c, COUNTS, who))) return rc;
    if ((rc = denoise_params(who, params, p))) return rc;
    if (select) s = *select;
    else (void)hr_select_default_params(&s);
    if (s.smooth > SELECT_MAX_SMOOTH) return fail(HR_ERR_INVALID, "%s: smooth must be in [0,%u]", who, SELECT_MAX_SMOOTH);
    if (s.reserved != 0u) return fail(HR_ERR_INVALID, "%s: reserved must be 0", who);
    if ((rc = moments_cover_an_estimate(c, who, true))) return rc;
    if (c->moments_n != c->buckets_n)
        return fail(HR_ERR_INVALID, "%s: the moments cover %llu samplings, the buckets %llu (they must cover the same samplings)", who, (unsigned long long)c->moments_n, (unsigned long long)c->buckets_n);
    if (ft && (rc = floor_and_threshold_ok(who, ft[0], ft[1]))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = hr_synchronize(c))) return rc;
    if (c->counts && (rc = counts_cover_an_estimate(c, who))) return rc;   // (every n >= 2 and none beyond the moments' — which are the buckets')
    const uint32_t K = c->robust_k;
    v = select_select_init_kernel(K);
    if (!v) return no_instantiation(who, "select_init_kernel", K);
    return guides_or_render(c);
}
// The pipeline hr_denoise_select and the estimate of its error (selected_noise_run) share, whose checks are done (select_ready: p, s, v), in two
// steps: a caller allocates its own planes between them and brackets the launches with its event pair.
//   planes()   the common call scratch: the states twice (once without a level), {A0, B0}, with smoothing e twice, best
//   launch()   select_init_kernel, then for l = 0 .. levels: [with smoothing: pass(e_in = nullptr, e_out = e[0]), then s.smooth times
//              select_smooth_kernel over e and, behind it, over the plane pair `more` (or nullptr),] pass(e_in = the smoothed e or nullptr,
//              e_out = nullptr), and atrous3_kernel to the next level
// `pass(flat, cur, e_in, e_out, l, demodulate)`: the caller's own launch on c->stream, in the idiom of atrous_run's init — select_pick_kernel or
// select_noise_kernel, which have these forms (post_kernels.h).
struct SelectRun {
    CallScratch scratch;
    double *st[2] = {nullptr, nullptr}, *raw = nullptr, *e[2] = {nullptr, nullptr}, *best = nullptr;   // (st: 18 planes of a double per pixel each, raw: 6; post_kernels.h)
    int planes(hr_ctx *c, const char *who, const hr_denoise_params &p, const hr_select_params &s) {
        const size_t pixels = region_pixels(c);
        for (int k = 0; k < (p.levels ? 2 : 1); k++) HIP_TRY_AS(who, scratch.alloc((void **)&st[k], pixels * 18 * sizeof(double)));
        HIP_TRY_AS(who, scratch.alloc((void **)&raw, pixels * 6 * sizeof(double)));
        for (int k = 0; k < (s.smooth ? 2 : 0); k++) HIP_TRY_AS(who, scratch.alloc((void **)&e[k], pixels * sizeof(double)));
        HIP_TRY_AS(who, scratch.alloc((void **)&best, pixels * sizeof(double)));
        return HR_OK;
    }
    template <class Pass>
    void launch(hr_ctx *c, const hr_denoise_params &p, const hr_select_params &s, const SelectInitVariant *v, double *const *more, Pass pass) {
        const size_t pixels = region_pixels(c);
        const DenoiseSigmas sg = denoise_sigmas(p.sigma_color, p.sigma_normal, p.sigma_albedo, p.sigma_depth);
        const int demodulate = p.demodulate && p.levels ? 1 : 0;   // as hr_denoise: without a level there is nothing to filter
        const dim3 flat((unsigned)((pixels + 255) / 256)), tiles2d((c->RW + 31) / 32, (c->RH + 7) / 8);
        hipLaunchKernelGGL(v->fn, flat, dim3(256), v->lds(), c->stream, c->buckets, c->counts, (uint32_t)c->moments_n, c->accum, c->moments, c->guides, st[0], raw, pixels, demodulate);
        for (uint32_t l = 0; l <= p.levels; l++) {
            double *cur = st[l & 1u], *nxt = st[(l + 1u) & 1u];
            if (s.smooth) {
                pass(flat, cur, nullptr, e[0], l, demodulate);
                for (uint32_t t = 0; t < s.smooth; t++) {
                    hipLaunchKernelGGL(select_smooth_kernel, tiles2d, dim3(32, 8), 0, c->stream, e[t & 1u], e[(t + 1u) & 1u], c->RW, c->RH, 1u << t);
                    if (more) hipLaunchKernelGGL(select_smooth_kernel, tiles2d, dim3(32, 8), 0, c->stream, more[t & 1u], more[(t + 1u) & 1u], c->RW, c->RH, 1u << t);
                }
            }
            pass(flat, cur, s.smooth ? e[s.smooth & 1u] : nullptr, nullptr, l, demodulate);
            if (l < p.levels) hipLaunchKernelGGL(atrous3_kernel, tiles2d, dim3(32, 8), 0, c->stream, cur, c->guides, nxt, c->RW, c->RH, 1u << l, sg);
        }
    }
};
int hr_denoise_select(hr_ctx *c, const hr_denoise_params *params, const hr_select_params *select) {
    static const char *const who = "hr_denoise_select";
    hr_denoise_params p;
    hr_select_params s;
    const SelectInitVariant *v = nullptr;
    int rc = select_ready(c, who, params, select, false, nullptr, p, s, v);
    if (rc) return rc;
    const uint32_t pixels = (uint32_t)region_pixels(c);
    SelectRun run;
    if ((rc = run.planes(c, who, p, s))) return rc;   // the call's planes first: a device without room leaves S as it was
    if (!c->selected && (rc = plane_alloc(c, SELECTED))) return rc;
    if (!c->selected_levels && (rc = plane_alloc(c, SELECTED_LEVELS))) return rc;
    c->made_of[SELECTED_IMAGE] = 0;
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    run.launch(c, p, s, v, nullptr, [&](dim3 flat, const double *cur, const double *e_in, double *e_out, uint32_t l, int demodulate) {
        hipLaunchKernelGGL(select_pick_kernel, flat, dim3(256), 0, c->stream, cur, run.raw, c->guides, e_in, e_out, l, run.best, c->selected_levels, c->selected, pixels, demodulate);
    });
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->post_events));
    HIP_TRY_AS(who, hipStreamSynchronize(c->stream));   // the scratch planes go with the call
    image_made(c, SELECTED_IMAGE);
    return drain_events(c);
}
int hr_read_selected(hr_ctx *c, float *host) { return image_read(c, SELECTED_IMAGE, "hr_read_selected", host); }
int hr_read_selected_levels(hr_ctx *c, uint8_t *host) { return image_read(c, SELECTED_IMAGE, "hr_read_selected_levels", host, true); }
int hr_resolve_selected(hr_ctx *c, uint8_t *host_rgb8) { return image_resolve(c, SELECTED_IMAGE, "hr_resolve_selected", host_rgb8); }

// ---- the error estimate of S, its stop rule and its tile selection (select_noise_core.h) ----
// One run behind the four entry points (`who`): hr_denoise_select's pipeline with select_noise_kernel in the pick's place, everything in call
// scratch — the run's own S and L too — so no kept image and no validity word is touched (the guide planes are rendered when there are none, as
// hr_denoise_select does).  Everything that is refused is refused before anything is touched.  What is asked for: est (the summary of e_S),
// host_img (e_S), host_mse (M), tiles (the selection by e_S; `active` may be null).  floor and threshold are checked unless host_mse alone is asked.
// The call holds 453 bytes per pixel with levels and smooth: the states twice (288), {A0, B0} (48), {va0, vb0} (48), e and m twice (32), best (8),
// M (8), e_S (8), S (12), L (1).
static int selected_noise_run(hr_ctx *c, const char *who, const hr_denoise_params *params, const hr_select_params *select, double floor, double threshold, hr_noise *est,
                              double *host_img, double *host_mse, bool tiles, uint32_t *active) {
    hr_denoise_params p;
    hr_select_params s;
    const SelectInitVariant *v = nullptr;
    const bool want_error = est || host_img || tiles;
    const double ft[2] = {floor, threshold};
    int rc = select_ready(c, who, params, select, tiles, want_error ? ft : nullptr, p, s, v);
    if (rc) return rc;
    const size_t pixels = region_pixels(c);
    SelectRun run;
    if ((rc = run.planes(c, who, p, s))) return rc;
    CallScratch &scratch = run.scratch;
    double *var0 = nullptr, *m[2] = {nullptr, nullptr}, *M = nullptr, *img = nullptr;
    float *S = nullptr;
    uint8_t *L = nullptr;
    HIP_TRY_AS(who, scratch.alloc((void **)&var0, pixels * 6 * sizeof(double)));
    for (int k = 0; k < (s.smooth ? 2 : 0); k++) HIP_TRY_AS(who, scratch.alloc((void **)&m[k], pixels * sizeof(double)));
    HIP_TRY_AS(who, scratch.alloc((void **)&M, pixels * sizeof(double)));
    HIP_TRY_AS(who, scratch.alloc((void **)&S, pixels * 3 * sizeof(float)));
    HIP_TRY_AS(who, scratch.alloc((void **)&L, pixels));
    BlockSummaries blocks;
    if (want_error) {
        HIP_TRY_AS(who, scratch.alloc((void **)&img, pixels * sizeof(double)));
        HIP_TRY_AS(who, blocks.alloc(scratch));
    }
    EventPair ev;
    HIP_TRY(timed_begin(ev, c->stream));
    run.launch(c, p, s, v, s.smooth ? m : nullptr, [&](dim3 flat, const double *cur, const double *e_in, double *e_out, uint32_t l, int demodulate) {
        hipLaunchKernelGGL(select_noise_kernel, flat, dim3(256), 0, c->stream, cur, run.raw, var0, c->guides, e_in, e_in ? m[s.smooth & 1u] : nullptr, e_out, e_out ? m[0] : nullptr, l, run.best,
                           L, S, M, (uint32_t)pixels, demodulate);
    });
    if (want_error) hipLaunchKernelGGL(select_noise_error_kernel, dim3(SUMMARY_BLOCKS), dim3(256), 0, c->stream, M, S, pixels, floor, threshold, img, blocks.dev);
    HIP_TRY(timed_end(hipGetLastError(), ev, c->stream, c->post_events));
    if (est) HIP_TRY_AS(who, blocks.fetch(c));
    if (host_img) HIP_TRY_AS(who, hipMemcpyAsync(host_img, img, pixels * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (host_mse) HIP_TRY_AS(who, hipMemcpyAsync(host_mse, M, pixels * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY_AS(who, hipStreamSynchronize(c->stream));   // the scratch planes go with the call
    if (est) blocks.summary(c->moments_n, pixels, est);
    if (tiles && (rc = select_tiles_run(c, who, img, floor, threshold, active))) return rc;
    return drain_events(c);
}
int hr_selected_noise_estimate(hr_ctx *c, const hr_denoise_params *params, const hr_select_params *select, double floor, double threshold, hr_noise *out) {
    if (c && !out) return fail(HR_ERR_INVALID, "hr_selected_noise_estimate: null argument");
    return selected_noise_run(c, "hr_selected_noise_estimate", params, select, floor, threshold, out, nullptr, nullptr, false, nullptr);
}
int hr_read_selected_noise_image(hr_ctx *c, const hr_denoise_params *params, const hr_select_params *select, double floor, double *host) {
    if (c && !host) return fail(HR_ERR_INVALID, "hr_read_selected_noise_image: null argument");
    return selected_noise_run(c, "hr_read_selected_noise_image", params, select, floor, 0.0, nullptr, host, nullptr, false, nullptr);
}
int hr_read_selected_mse(hr_ctx *c, const hr_denoise_params *params, const hr_select_params *select, double *host) {
    if (c && !host) return fail(HR_ERR_INVALID, "hr_read_selected_mse: null argument");
    return selected_noise_run(c, "hr_read_selected_mse", params, select, 0.0, 0.0, nullptr, nullptr, host, false, nullptr);
}
int hr_select_tiles_selected(hr_ctx *c, const hr_denoise_params *params, const hr_select_params *select, double floor, double threshold, uint32_t *active) {
    return selected_noise_run(c, "hr_select_tiles_selected", params, select, floor, threshold, nullptr, nullptr, nullptr, true, active);
}

int hr_get_stats(hr_ctx *c, hr_stats *out) {
    if (!c || !out) return fail(HR_ERR_INVALID, "hr_get_stats: null argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    Counters h;
    HIP_TRY(hipMemcpyAsync(&h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof *out);
    out->paths = c->counters ? h.paths : c->paths_rendered;
    out->rays = h.rays; out->node_tests = h.node_tests; out->tri_tests = h.tri_tests;
    out->sphere_tests = h.sphere_tests; out->cuboid_tests = h.cuboid_tests; out->rng_overflow = h.rng_overflow; out->shadow_culled = h.shadow_culled;
    out->seed_kernel_ms = c->seed_ms; out->trace_kernel_ms = c->trace_ms; out->post_kernel_ms = c->post_ms;
    out->seed_launches = c->seed_launches; out->trace_launches = c->trace_launches;
    out->bvh_build_ms = c->bvh_build_ms; out->bvh_builder_used = (uint64_t)c->builder_in_use;
    out->shading_in_force = c->precise ? (c->trace_mode == 1 ? 2u : 1u) : (c->trace_mode == 1 ? 3u : 0u);
    out->debug_kernel_ms = c->debug_ms; out->debug_launches = c->debug_launches;
    {
        GovDev g;
        HIP_TRY(hipMemcpyAsync(&g, c->gov, sizeof g, hipMemcpyDeviceToHost, c->stream));   // on the context's own stream: a null-stream copy could serialise against other contexts' launches
        HIP_TRY(hipStreamSynchronize(c->stream));
        out->governor_level = (uint64_t)(g.level < 0 ? 0 : g.level); out->governor_decisions = g.decisions; out->governor_moves = g.moves;
        out->governor_budget = g.budget; out->governor_budget_moves = g.budget_moves;
    }
    out->shade_calls = h.shade_calls; out->shade_lanes = h.shade_lanes; out->box_passes = h.box_passes; out->box_lanes = h.box_lanes;
    out->leaf_calls = h.leaf_calls; out->leaf_lanes = h.leaf_lanes; out->outer_iters = h.outer_iters;
    for (int i = 0; i < 4; i++) out->phase_cycles[i] = h.phase_cycles[i];
    for (int i = 0; i < 8; i++) out->seed_phase_cycles[i] = h.seed_phase[i];
    out->bvh_nodes = c->st_nodes; out->triangles = c->st_tris; out->spheres = c->st_spheres; out->cuboids = c->st_cuboids;
    return HR_OK;
}

// ---- options ----
// A plain knob is a row: the key, the member it is stored into, what is accepted, what is said otherwise, and whether the context is
// synchronised first / the governor starts over afterwards.  Accepted: any value with lo > hi; else lo <= value <= hi — every value in
// between with step 0 (the fraction is dropped when it is stored), only lo, lo + step, .. with a step.  Keys with logic of their own are
// explicit code in hr_set_option / hr_set_debug_option, behind the table.
struct OptionField {
    bool hr_ctx::*b = nullptr;
    uint32_t hr_ctx::*u = nullptr;
    int hr_ctx::*i = nullptr;
    constexpr OptionField(bool hr_ctx::*p) : b(p) {}
    constexpr OptionField(uint32_t hr_ctx::*p) : u(p) {}
    constexpr OptionField(int hr_ctx::*p) : i(p) {}
};
enum { OPT_SYNC = 1, OPT_GOVERN = 2 };
struct OptionRow {
    const char *key;
    OptionField field;
    double lo, hi, step;
    const char *error;
    int flags;
};
static const OptionRow PRODUCT_OPTIONS[] = {
    {"counters", &hr_ctx::counters, 1, 0, 0, "", 0},
    {"batch", &hr_ctx::batch, 0, 64, 0, "batch must be in [1,64], or 0 for automatic", OPT_SYNC},
    {"trace_boost", &hr_ctx::trace_boost, -1, 4, 1, "trace_boost must be -1 (governed by the measured kernel times) or a level 0 .. 4", OPT_SYNC | OPT_GOVERN},
    // the bounce geometry in f64: closer to the reference's f64 arithmetic, a few per cent slower
    {"precise_shading", &hr_ctx::precise_opt, -1, 1, 1, "precise_shading must be -1 (automatic), 0 or 1", OPT_SYNC | OPT_GOVERN},
    {"quant_nodes", &hr_ctx::quant_nodes, 1, 0, 0, "", 0},   // next hr_upload_scene
    {"bvh_builder", &hr_ctx::bvh_builder, -1, 2, 1, "bvh_builder must be -1 (by scene size), 0 (host SAH), 1 (device LBVH) or 2 (device PLOC)", 0},   // next hr_upload_scene
    {"max_leaf", &hr_ctx::max_leaf, 1, 15, 0, "max_leaf must be in [1,15]", 0},   // next hr_upload_scene
};
static const OptionRow DEBUG_OPTIONS[] = {
    {"adv_den", &hr_ctx::adv_den, 1, 64, 0, "adv_den must be in [1,64]", 0},
    {"leaf_den", &hr_ctx::leaf_den, 1, 64, 0, "leaf_den must be in [1,64]", 0},
    {"min_waves", &hr_ctx::min_waves, 4, 6, 0, "min_waves must be in [4,6]", 0},
    {"kchunk", &hr_ctx::kchunk, 0, 64, 0, "kchunk must be in [1,64], or 0 for the default", 0},
    {"node_unroll", &hr_ctx::node_unroll, 1, 2, 1, "node_unroll must be 1 or 2", 0},
    // (the three go into uint32_t fields, and the budget is handed on as budget + 1: nothing negative, not a number or beyond 2^31)
    {"tail_div", &hr_ctx::tail_div, 0, 2147483648.0, 0, "tail_div must be in [0,2^31] (0 = no finer tail)", 0},
    {"trace_grid", &hr_ctx::trace_grid, 0, 2147483648.0, 0, "trace_grid must be in [0,2^31] (0 = trace_wgs per CU)", 0},
    {"trace_budget", &hr_ctx::trace_budget, 0, 2147483648.0, 0, "trace_budget must be in [0,2^31] (0 = every workgroup stays)", 0},
    {"trace_wgs", &hr_ctx::trace_wgs, 1, 8, 0, "trace_wgs must be in [1,8]", 0},
    {"seed_prio", &hr_ctx::seed_prio, 0, 3, 0, "seed_prio must be in [0,3]", 0},
    {"init_prio", &hr_ctx::init_prio, 0, 3, 0, "init_prio must be in [0,3]", 0},
    {"seed_split", &hr_ctx::seed_split, 8, 28, 4, "seed_split must be 8, 12, 16, 20, 24 or 28", 0},
    {"seed_prof", &hr_ctx::seed_prof, 1, 0, 0, "", 0},
    {"seed_prerun", &hr_ctx::seed_prerun, 0, 1, 1, "seed_prerun must be 1 (pre-run window of the three-run seed kernel) or 0 (its three equal runs)", OPT_SYNC},
    {"ploc_top", &hr_ctx::ploc_top, 1, 1 << 16, 0, "ploc_top must be in [1,65536]", 0},
    {"trace_mode", &hr_ctx::trace_mode_opt, -1, 1, 1, "trace_mode must be -1 (automatic), 0 (megakernel) or 1 (split: traversal kernel + shading kernel)", OPT_SYNC | OPT_GOVERN},
    {"draw_residuals", &hr_ctx::draw_residuals, 0, 1, 1, "draw_residuals must be 0 or 1", 0},
    {"wf_adv_den", &hr_ctx::wf_adv_den, 0, 64, 0, "wf_adv_den must be in [0,64]", 0},
    {"wf_trav_wgs", &hr_ctx::wf_trav_wgs, 1, 16, 0, "wf_trav_wgs must be in [1,16]", 0},
    {"wf_shade_wgs", &hr_ctx::wf_shade_wgs, 1, 16, 0, "wf_shade_wgs must be in [1,16]", 0},
    {"debug_skip", &hr_ctx::debug_skip, 1, 0, 0, "", 0},
};
static int apply_option(hr_ctx *c, const OptionRow &r, double value) {
    if (r.lo <= r.hi) {
        bool ok = value >= r.lo && value <= r.hi;   // (false for a NaN)
        if (ok && r.step > 0) ok = std::fmod(value - r.lo, r.step) == 0.0;
        if (!ok) return fail(HR_ERR_INVALID, "%s", r.error);
    }
    if (r.flags & OPT_SYNC) { int rc = sync_all(c); if (rc) return rc; }
    if (r.field.b) c->*r.field.b = value != 0.0;
    else if (r.field.u) c->*r.field.u = (uint32_t)value;
    else c->*r.field.i = (int)value;
    return r.flags & OPT_GOVERN ? govern_reset(c) : HR_OK;
}

// An option that owns a plane (`p.option`, `p.on`).  Off: `off_first`, then the plane goes.  On: the plane is allocated, zeroed — a failed
// allocation leaves the option off —, and `other`, when it is already running, starts over with it: the counts are the moments' n, the two
// must cover the same samplings (the accumulator stays).  Set on while on: what has been gathered stays.
static int set_plane_option(hr_ctx *c, double value, const Plane &p, const Plane &other, int (*off_first)(hr_ctx *)) {
    if (value != 0 && value != 1) return fail(HR_ERR_INVALID, "%s must be 0 or 1", p.option);
    if (value == 1 && !c->W) return fail(HR_ERR_NO_TARGET, "%s: hr_set_resolution not called", p.option);
    int rc = sync_all(c);
    if (rc) return rc;
    if (value == 0 || !(c->*p.on)) changed(c, SRC_MOMENTS | SRC_COUNTS);   // the moments or the counts go, or start over (conservative, kept: whichever of the two it is)
    if (value == 0) {
        c->*p.on = false;
        if ((rc = off_first(c))) return rc;
        return plane_free(c, p);
    }
    if (c->*p.on) return HR_OK;
    if ((rc = plane_alloc(c, p))) { (void)plane_free(c, p); return rc; }
    c->*p.on = true;
    return plane_zero(c, other);
}

// Option "robust_buckets" = K.  0: the buckets go, and R with them.  K in {3, 5, .., 15}: K buckets per pixel, zeroed — set again
// with the value it has: what has been gathered stays; with another K they start over.  Buckets that start (over) while option "sample_counts"
// runs start the counts over too: a pixel's count is the ordinal of its next sampling.  The counts are the moments' n, so the moments go with them.
static int set_robust_buckets(hr_ctx *c, double value) {
    if (value != 0 && !robust_valid_k(value)) return fail(HR_ERR_INVALID, "robust_buckets must be 0 (off) or an odd number of buckets in [3,15]");
    if (value != 0 && !c->W) return fail(HR_ERR_NO_TARGET, "robust_buckets: hr_set_resolution not called");
    if (c->robust_on && (uint32_t)value == c->robust_k) return HR_OK;
    changed(c, SRC_BUCKETS);
    int rc = sync_all(c);
    if (rc) return rc;
    c->robust_on = false;
    c->robust_k = 0;
    if ((rc = plane_free(c, BUCKETS)) || (rc = plane_free(c, ROBUST)) || (rc = plane_free(c, ROBUST_TRIM)) || (rc = plane_free(c, ROBUST_NOISE_IMG)) || (rc = plane_free(c, ROBUST_NOISE_TRIM)) || (rc = plane_free(c, RESTORED))) return rc;
    if (value == 0) return HR_OK;
    c->robust_k = (uint32_t)value;
    if ((rc = plane_alloc(c, BUCKETS))) { (void)plane_free(c, BUCKETS); c->robust_k = 0; return rc; }
    c->robust_on = true;
    if (c->counts_on) { changed(c, SRC_COUNTS | SRC_MOMENTS); if ((rc = plane_zero(c, COUNTS)) || (rc = plane_zero(c, MOMENTS))) return rc; }
    return HR_OK;
}

// The options of the sharded statistics, asked before hr_set_option's own keys: true when `key` is one of them, `rc` is then the call's.
// "bucket_by_sampling": which bucket a sampling goes into — 0: the pixel's ordinal mod K, 1: (the sampling's index - 1) mod K.  Buckets filled under
// one rule mean nothing under the other: switched while robust_buckets is on they start over as they do with another K — the counts and the moments
// with them while sample_counts runs, R and a D made of R are gone.  With robust_buckets off the value is only recorded; any value but 0 and 1 is
// refused and changes nothing.
static bool set_sharding_option(hr_ctx *c, const std::string &key, double value, int &rc) {
    if (key != "bucket_by_sampling") return false;
    rc = HR_OK;
    if (value != 0 && value != 1) { rc = fail(HR_ERR_INVALID, "bucket_by_sampling must be 0 (a pixel's j-th sampling in bucket j mod K) or 1 (sampling s in bucket (s - 1) mod K)"); return true; }
    if ((value == 1) == c->bucket_by_sampling) return true;
    if ((rc = sync_all(c))) return true;
    c->bucket_by_sampling = value == 1;
    if (!c->robust_on) return true;
    changed(c, SRC_BUCKETS);
    if ((rc = plane_zero(c, BUCKETS))) return true;
    if (c->counts_on) { changed(c, SRC_COUNTS | SRC_MOMENTS); if ((rc = plane_zero(c, COUNTS))) return true; rc = plane_zero(c, MOMENTS); }
    return true;
}

static const char *const RR_EXCLUDES_PRECISE = "russian_roulette and precise_shading 1 exclude each other (the roulette estimator has no f64 instantiation)";
int hr_set_option(hr_ctx *c, const char *key, double value) {
    if (!c || !key) return fail(HR_ERR_INVALID, "hr_set_option: null argument");
    HIP_TRY(hipSetDevice(c->device));
    std::string k = key;
    // the pair is refused where it is asked for, whichever comes second, and what was in force stays (hr_render keeps its own check)
    if (k == "precise_shading" && value == 1 && c->rr_start) return fail(HR_ERR_UNSUPPORTED, "%s", RR_EXCLUDES_PRECISE);
    { int rc; if (set_sharding_option(c, k, value, rc)) return rc; }
    if (const OptionRow *row = find_row(PRODUCT_OPTIONS, [&](const OptionRow &r) { return k == r.key; })) return apply_option(c, *row, value);
    // per-pixel first and second moments of the per-sampling values, for the noise estimate, and how many samplings every pixel
    // has received: what a tile mask (hr_set_tile_mask) needs — the mask goes when the counts go
    if (k == "moments") {   // (moments that start zero the counts, and the counts are the buckets' ordinals: the buckets start over with them)
        const bool was_on = c->moments_on;
        const int rc = set_plane_option(c, value, MOMENTS, COUNTS, [](hr_ctx *x) { return plane_free(x, NOISE_IMG); });
        return !rc && value == 1 && !was_on && c->counts_on ? plane_zero(c, BUCKETS) : rc;
    }
    if (k == "sample_counts") {   // (the counts are the buckets' ordinals as well as the moments' n: both start over with them)
        const bool was_on = c->counts_on;
        const int rc = set_plane_option(c, value, COUNTS, MOMENTS, remove_mask);
        return !rc && value == 1 && !was_on ? plane_zero(c, BUCKETS) : rc;
    }
    if (k == "robust_buckets") return set_robust_buckets(c, value);
    if (k == "guide_bounces") {  // next hr_render_guides; a new value drops the planes it would no longer describe, and the image filtered with them
        if (!(value >= 0 && value <= 8) || value != std::floor(value)) return fail(HR_ERR_INVALID, "guide_bounces must be a whole number in [0,8]");
        if ((uint32_t)value == c->guide_bounces) return HR_OK;
        c->guide_bounces = (uint32_t)value;
        changed(c, SRC_GUIDES);
        return HR_OK;
    }
    if (k == "max_tail_gib") {
        if (value < 1 || value > 128) return fail(HR_ERR_INVALID, "max_tail_gib must be in [1,128]");
        c->max_tail_bytes = (uint64_t)value << 30;
        return HR_OK;
    }
    if (k == "split_ratio") {  // early split clipping of triangle references (-1 = automatic, 0 = off), next hr_upload_scene
        if ((value < 0 && value != -1) || value > 1000) return fail(HR_ERR_INVALID, "split_ratio must be -1 (automatic), 0 (off) or in (0,1000]");
        c->split_ratio = value;
        return HR_OK;
    }
    if (k == "rng_window") {
        if ((int)value != ISAAC_TAIL) return fail(HR_ERR_UNSUPPORTED, "rng_window is fixed at %d in this build", ISAAC_TAIL);
        return HR_OK;
    }
    if (k == "russian_roulette") {  // NOT image-preserving (see the header): 0 = off, else the first path iteration that plays
        if (value != 0 && (value < 2 || value > 9)) return fail(HR_ERR_INVALID, "russian_roulette must be 0 (off) or the first iteration that plays, in [2,9]");
        if (value != 0 && c->precise_opt == 1) return fail(HR_ERR_UNSUPPORTED, "%s", RR_EXCLUDES_PRECISE);
        int rc = sync_all(c);
        if (rc) return rc;
        c->rr_start = (uint32_t)value;
        // automatic precise shading stands back (the roulette estimator has no f64 instantiation), so shading and pipeline in force may change
        // here as they do under precise_shading and trace_mode: the governor starts over with the thresholds and the budget range of what runs
        return govern_reset(c);
    }
    return fail(HR_ERR_INVALID, "unknown option '%s' (measurement knobs live behind hr_set_debug_option)", key);
}

// Measurement / experiment knobs.  Kept apart from hr_set_option on purpose (two tables, each looked up by its own entry point only): a host
// that only uses hr_set_option cannot change the kernels' schedule, and cannot reach "debug_skip", which produces a garbage image.
int hr_set_debug_option(hr_ctx *c, const char *key, double value) {
    if (!c || !key) return fail(HR_ERR_INVALID, "hr_set_debug_option: null argument");
    HIP_TRY(hipSetDevice(c->device));
    std::string k = key;
    if (const OptionRow *row = find_row(DEBUG_OPTIONS, [&](const OptionRow &r) { return k == r.key; })) return apply_option(c, *row, value);
    if (k == "seed_mode") {
        if (value != 0 && value != 1 && value != 2 && value != 3 && value != 4) return fail(HR_ERR_INVALID, "seed_mode must be 4 (five-wave four-run kernel), 3 (phase-shifted four-run kernel), 2 (three-run kernel), 1 (producer / consumer kernel with a state ring) or 0 (fused kernel)");
#if !defined(HR_EXPERIMENTS)
        if (value >= 3) return fail(HR_ERR_UNSUPPORTED, "seed_mode %d is a measured experiment (slower than the default): build with `make EXPERIMENTS=1` to have it", (int)value);
#endif
        int rc = sync_all(c);
        if (rc) return rc;
        c->seed_mode = (int)value;
        return HR_OK;
    }
    if (k == "nee_cull") { c->nee_cull = (uint32_t)value & 7u; return HR_OK; }
    return fail(HR_ERR_INVALID, "unknown debug option '%s'", key);
}

int hr_debug_draws(hr_ctx *c, uint32_t sampling, uint32_t first_path, uint32_t num_paths, uint32_t window, uint64_t *host_out) {
    if (!c || !host_out || !num_paths) return fail(HR_ERR_INVALID, "hr_debug_draws: bad argument");
    int rc = debug_refusal(c, "hr_debug_draws", NO_REGION | NO_MASK | A_TARGET);
    if (rc) return rc;
    if (window == 0 || window > (uint32_t)ISAAC_TAIL) return fail(HR_ERR_INVALID, "window must be in [1,%d]", ISAAC_TAIL);
    if ((uint64_t)first_path + num_paths > (uint64_t)c->W * c->H * 4) return fail(HR_ERR_INVALID, "path range outside the image");
    HIP_TRY(hipSetDevice(c->device));
    CallScratch scratch;
    u64 *d = nullptr;
    HIP_TRY(scratch.alloc((void **)&d, (size_t)num_paths * window * 8));
    hipLaunchKernelGGL(seed_debug_kernel, dim3((num_paths + 63) / 64), dim3(64), 256 * 64 * 8, c->stream, c->W, c->H, sampling, first_path, num_paths,
                       (int)window, d);
    HIP_TRY_AS("hr_debug_draws", hipGetLastError());
    HIP_TRY_AS("hr_debug_draws", hipStreamSynchronize(c->stream));
    HIP_TRY_AS("hr_debug_draws", hipMemcpy(host_out, d, (size_t)num_paths * window * 8, hipMemcpyDeviceToHost));
    return HR_OK;
}

static int path_draws_out(hr_ctx *c, uint32_t sampling, float *host_out, bool residuals, const char *who) {
    // the 20 fp32 draws per path exactly as the production seed kernel hands them to the trace kernel (residuals: the same slots of the
    // records' twin), re-ordered to pixel-major paths: out[((y*W + x)*4 + sub) * 20 + d]
    if (!c || !host_out) return fail(HR_ERR_INVALID, "%s: bad argument", who);
    int rc = debug_refusal(c, who, NO_REGION | NO_MASK | A_TARGET);
    if (rc) return rc;
    if (!c->have_scene) return fail(HR_ERR_NO_SCENE, "%s: no scene (lens shape needed)", who);   // (a text of its own)
    if (residuals && !draws_twin(c)) return fail(HR_ERR_UNSUPPORTED, "%s: no residuals are written (needs precise shading in force, seed_mode 2, draw_residuals 1)", who);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = sync_all(c))) return rc;
    LaunchPlan plan;
    if ((rc = plan_launch(c, sampling, 1, 1, TRACE_NONE, plan))) return rc;   // (no region: refused above)
    RenderParams &rp = plan.rp;
    const uint32_t tiles = plan.tiles;
    if (!residuals) rp.rec_lo_off = 0;   // the fp32 draws are asked for: the seed kernel's form without the twin
    rp.pad[0] = 0;                       // the seed kernel alone on the chip: its consumer waves stay at the priority they start with
    if ((rc = launch_seed(c, rp, 0, c->stream))) return rc;   // on the main stream, slot 0: nothing else is in flight
    std::vector<float> h((size_t)tiles * REC_ITEM_FLOATS), lo;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(h.data(), c->recs[0], h.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (residuals) {
        lo.resize(h.size());
        HIP_TRY(hipMemcpy(lo.data(), c->recs[0] + rp.rec_lo_off, lo.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (uint32_t t = 0; t < tiles; t++)
        for (uint32_t j = 0; j < 64; j++) {
            uint32_t tx = t % rp.tiles_x, ty = t / rp.tiles_x, pix = j >> 2, sub = j & 3;
            uint32_t px = tx * 4 + (pix & 3), py = ty * 4 + (pix >> 2);
            if (px >= c->W || py >= c->H) continue;
            const float *rec = &h[(size_t)t * REC_ITEM_FLOATS];
            const uint32_t lb = j * 4u;
            uint32_t a = float_as_uint(rec[rec_slot(lb, REC_HEAD)]);
            float *o = &host_out[(((size_t)py * c->W + px) * 4 + sub) * DRAWS_PER_PATH];
            if (residuals) {
                const float *rl = &lo[(size_t)t * REC_ITEM_FLOATS];
                for (uint32_t d = 0; d < (uint32_t)DRAWS_PER_PATH; d++) o[d] = rl[rec_slot(lb, 2 * a + d)];
                continue;
            }
            o[0] = rec[rec_slot(lb, REC_HEAD + 1)];
            o[1] = rec[rec_slot(lb, REC_HEAD + 2)];
            for (uint32_t d = 2; d < (uint32_t)DRAWS_PER_PATH; d++) o[d] = rec[rec_slot(lb, 2 * a + d)];
        }
    return drain_events(c);
}
int hr_debug_path_draws(hr_ctx *c, uint32_t sampling, float *host_out) { return path_draws_out(c, sampling, host_out, false, "hr_debug_path_draws"); }
int hr_debug_path_draw_residuals(hr_ctx *c, uint32_t sampling, float *host_out) { return path_draws_out(c, sampling, host_out, true, "hr_debug_path_draw_residuals"); }

int hr_debug_path_log(hr_ctx *c, uint32_t sampling, uint32_t *host_out) {
    // one sampling through the production pipeline — the seed kernel, then the LOG instantiation of trace_kernel (same traversal, same
    // path_advance) — with every path's radiance, ray count and event log written out instead of being accumulated
    if (!c || !host_out) return fail(HR_ERR_INVALID, "hr_debug_path_log: bad argument");
    int rc = debug_refusal(c, "hr_debug_path_log", NO_REGION | NO_MASK | A_TARGET | A_SCENE);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = sync_all(c))) return rc;
    LaunchPlan plan;
    if ((rc = plan_launch(c, sampling, 1, 1, TRACE_IN_FORCE, plan))) return rc;   // (no region: refused above)
    const RenderParams &rp = plan.rp;
    const bool split = plan.split;
    const TraceFn trace = select_trace_kernel(c->counters, c->dsc.qnodes != nullptr, c->rr_start != 0, c->precise, c->min_waves, true);
    if (!split && !trace) return fail(HR_ERR_UNSUPPORTED, "hr_debug_path_log: no trace kernel instantiation for these options (kernel_variants.h)");
    if ((rc = launch_seed(c, rp, 0, c->stream))) return rc;   // on the main stream, slot 0: nothing else is in flight
    const size_t words = (size_t)c->W * c->H * 4u * 8u;
    CallScratch scratch;
    uint32_t *d_log = nullptr;
    HIP_TRY(scratch.alloc((void **)&d_log, words * sizeof(uint32_t)));
    HIP_TRY_AS("hr_debug_path_log", hipMemsetAsync(d_log, 0, words * sizeof(uint32_t), c->stream));
    if (split) {
        // the split pipeline's LOG instantiation: the event log rides in two more state quads and a tag per ray slot, allocated for this call only
        WfQueues wq = c->wf;
        const size_t st_q = (size_t)wq.cap_paths * WF_SUBQ * sizeof(f4), tg_q = (size_t)wq.cap_rays * WF_SUBQ * sizeof(uint32_t);
        char *b = nullptr;
        HIP_TRY_AS("hr_debug_path_log", scratch.alloc((void **)&b, 2 * st_q + 2 * tg_q));
        for (int i = 0; i < 2; i++) { wq.st_f[i] = (f4 *)b; b += st_q; }
        for (int i = 0; i < 2; i++) { wq.tag[i] = (uint32_t *)b; b += tg_q; }
        if ((rc = launch_split(c, rp, 0, nullptr, d_log, &wq))) return rc;
    } else {
        HIP_TRY_AS("hr_debug_path_log", hipMemsetAsync(c->d_tile_counter, 0, sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(trace, dim3(trace_grid_size(c, plan.tiles, 1, 0)), dim3(64 * TRACE_WAVES), 0, c->stream, c->dsc, rp, c->recs[0], c->d_counters, c->d_tile_counter, d_log);
        HIP_TRY_AS("hr_debug_path_log", hipGetLastError());
    }
    HIP_TRY_AS("hr_debug_path_log", hipStreamSynchronize(c->stream));
    HIP_TRY_AS("hr_debug_path_log", hipMemcpy(host_out, d_log, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return drain_events(c);
}

int hr_debug_wf_profile(hr_ctx *c, uint32_t sampling, uint32_t num_k, double *ms_out, uint32_t *counts_out) {
    // one launch of the split pipeline with the chip to itself, an event between every two kernels: ms_out[0] = wf_start_kernel,
    // ms_out[2 s - 1] / ms_out[2 s] = traversal / shading kernel of step s = 1 .. WF_STEPS; counts_out[2 s] / [2 s + 1] = rays / live paths of step s
    if (!c || !ms_out || !counts_out || !num_k) return fail(HR_ERR_INVALID, "hr_debug_wf_profile: bad argument");
    int rc = debug_refusal(c, "hr_debug_wf_profile", NO_REGION | NO_MASK | A_TARGET | A_SCENE);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = sync_all(c))) return rc;
    LaunchPlan plan;
    if ((rc = plan_launch(c, sampling, 1, num_k, TRACE_SPLIT, plan))) return rc;   // (no region: refused above); the split pipeline whatever is in force
    RenderParams &rp = plan.rp;
    rp.kchunk = 0;   // not passed: the split pipeline has no work units of samplings
    if ((rc = launch_seed(c, rp, 0, c->stream))) return rc;   // on the main stream, slot 0: nothing else is in flight
    std::vector<hipEvent_t> marks;
    rc = launch_split(c, rp, 0, &marks);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (!rc && e == hipSuccess && marks.size() == 2u + 2u * WF_STEPS) {
        for (size_t i = 0; i + 1 < marks.size(); i++) { float ms = 0; (void)hipEventElapsedTime(&ms, marks[i], marks[i + 1]); ms_out[i] = ms; }
        std::vector<WfCounts> h((WF_STEPS + 2) * WF_SUBQ);
        e = hipMemcpy(h.data(), c->wf.counts, h.size() * sizeof(WfCounts), hipMemcpyDeviceToHost);
        for (uint32_t s = 0; s <= WF_STEPS; s++) {
            counts_out[2 * s] = counts_out[2 * s + 1] = 0;
            for (uint32_t k = 0; k < WF_SUBQ; k++) { counts_out[2 * s] += wf_rays(h[s * WF_SUBQ + k]); counts_out[2 * s + 1] += wf_paths(h[s * WF_SUBQ + k]); }
        }
    }
    for (hipEvent_t ev : marks) (void)hipEventDestroy(ev);
    if (rc) return rc;
    if (e != hipSuccess) return fail(HR_ERR_DEVICE, "hr_debug_wf_profile: %s", hipGetErrorString(e));
    return drain_events(c);
}

int hr_debug_intersect(hr_ctx *c, uint32_t n, const float *rays, float *out, int32_t *out_element) {
    if (!c || !rays || !out || !out_element || !n) return fail(HR_ERR_INVALID, "hr_debug_intersect: bad argument");
    int rc = debug_refusal(c, "hr_debug_intersect", NO_REGION | NO_MASK | A_SCENE);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    CallScratch scratch;
    float *d_rays = nullptr, *d_out = nullptr;
    int32_t *d_el = nullptr;
    HIP_TRY_AS("hr_debug_intersect", scratch.alloc((void **)&d_rays, (size_t)n * 6 * 4));
    HIP_TRY_AS("hr_debug_intersect", scratch.alloc((void **)&d_out, (size_t)n * 8 * 4));
    HIP_TRY_AS("hr_debug_intersect", scratch.alloc((void **)&d_el, (size_t)n * 4));
    HIP_TRY_AS("hr_debug_intersect", hipMemcpy(d_rays, rays, (size_t)n * 6 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(intersect_debug_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->dsc, n, d_rays, d_out, d_el);
    HIP_TRY_AS("hr_debug_intersect", hipGetLastError());
    HIP_TRY_AS("hr_debug_intersect", hipStreamSynchronize(c->stream));
    HIP_TRY_AS("hr_debug_intersect", hipMemcpy(out, d_out, (size_t)n * 8 * 4, hipMemcpyDeviceToHost));
    HIP_TRY_AS("hr_debug_intersect", hipMemcpy(out_element, d_el, (size_t)n * 4, hipMemcpyDeviceToHost));
    return HR_OK;
}

int hr_debug_trace(hr_ctx *c, uint32_t n, const float *rays, const float *shadow_len, float *out, int32_t *out_element) {
    if (!c || !rays || !out || !out_element || !n) return fail(HR_ERR_INVALID, "hr_debug_trace: bad argument");
    int rc = debug_refusal(c, "hr_debug_trace", NO_REGION | NO_MASK | A_SCENE);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const TraceDebugFn fn = select_trace_debug_kernel(c->counters, c->dsc.qnodes != nullptr);
    if (!fn) return fail(HR_ERR_UNSUPPORTED, "hr_debug_trace: no kernel instantiation for these options (kernel_variants.h)");
    CallScratch scratch;
    float *d_rays = nullptr, *d_out = nullptr, *d_sl = nullptr;
    int32_t *d_el = nullptr;
    HIP_TRY_AS("hr_debug_trace", scratch.alloc((void **)&d_rays, (size_t)n * 6 * 4));
    HIP_TRY_AS("hr_debug_trace", scratch.alloc((void **)&d_out, (size_t)n * 8 * 4));
    HIP_TRY_AS("hr_debug_trace", scratch.alloc((void **)&d_el, (size_t)n * 4));
    if (shadow_len) HIP_TRY_AS("hr_debug_trace", scratch.alloc((void **)&d_sl, (size_t)n * 4));
    HIP_TRY_AS("hr_debug_trace", hipMemcpy(d_rays, rays, (size_t)n * 6 * 4, hipMemcpyHostToDevice));
    if (shadow_len) HIP_TRY_AS("hr_debug_trace", hipMemcpy(d_sl, shadow_len, (size_t)n * 4, hipMemcpyHostToDevice));
    RenderParams rp{};
    knob_params(c, rp);   // (no geometry: the rays are the caller's)
    // the record format hr_render walks on this scene; timed with HIP events (hr_stats.debug_kernel_ms), counted with option "counters".
    // The timing is best effort: the launch goes out without it if an event cannot be made, and only a pair that was really recorded
    // is ever queried (timed_end)
    EventPair ev;
    (void)timed_begin(ev, c->stream);
    hipLaunchKernelGGL(fn, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->dsc, rp, n, d_rays, d_sl, d_out, d_el, c->counters ? c->d_counters : (Counters *)nullptr);
    const hipError_t launched = hipGetLastError();
    (void)timed_end(launched, ev, c->stream, c->debug_events, &c->debug_launches);
    HIP_TRY_AS("hr_debug_trace", launched);
    HIP_TRY_AS("hr_debug_trace", hipStreamSynchronize(c->stream));
    HIP_TRY_AS("hr_debug_trace", hipMemcpy(out, d_out, (size_t)n * 8 * 4, hipMemcpyDeviceToHost));
    HIP_TRY_AS("hr_debug_trace", hipMemcpy(out_element, d_el, (size_t)n * 4, hipMemcpyDeviceToHost));
    return drain_events(c);
}

// The point queries (query_core.h): hr_debug_intersect's pattern — scratch for the call, one launch of 64-thread groups, a point per thread.
int hr_debug_surface(hr_ctx *c, uint32_t n, const float *rays, const float *fix, const double *draws, int precise, float *out, double *out64, int32_t *out_element) {
    if (!c || !rays || !out || !out_element || !n) return fail(HR_ERR_INVALID, "hr_debug_surface: bad argument");
    int rc = debug_refusal(c, "hr_debug_surface", NO_REGION | NO_MASK | A_SCENE);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    CallScratch scratch;
    float *d_rays = nullptr, *d_fix = nullptr, *d_out = nullptr;
    double *d_draws = nullptr, *d_out64 = nullptr;
    int32_t *d_el = nullptr;
    HIP_TRY_AS("hr_debug_surface", scratch.alloc((void **)&d_rays, (size_t)n * 6 * 4));
    if (fix) HIP_TRY_AS("hr_debug_surface", scratch.alloc((void **)&d_fix, (size_t)n * 6 * 4));
    if (draws) HIP_TRY_AS("hr_debug_surface", scratch.alloc((void **)&d_draws, (size_t)n * 2 * 8));
    HIP_TRY_AS("hr_debug_surface", scratch.alloc((void **)&d_out, (size_t)n * QUERY_SURFACE_FLOATS * 4));
    if (out64) HIP_TRY_AS("hr_debug_surface", scratch.alloc((void **)&d_out64, (size_t)n * 6 * 8));
    HIP_TRY_AS("hr_debug_surface", scratch.alloc((void **)&d_el, (size_t)n * 4));
    HIP_TRY_AS("hr_debug_surface", hipMemcpy(d_rays, rays, (size_t)n * 6 * 4, hipMemcpyHostToDevice));
    if (fix) HIP_TRY_AS("hr_debug_surface", hipMemcpy(d_fix, fix, (size_t)n * 6 * 4, hipMemcpyHostToDevice));
    if (draws) HIP_TRY_AS("hr_debug_surface", hipMemcpy(d_draws, draws, (size_t)n * 2 * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(surface_debug_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->dsc, n, d_rays, d_fix, d_draws, precise, d_out, d_out64, d_el);
    HIP_TRY_AS("hr_debug_surface", hipGetLastError());
    HIP_TRY_AS("hr_debug_surface", hipStreamSynchronize(c->stream));
    HIP_TRY_AS("hr_debug_surface", hipMemcpy(out, d_out, (size_t)n * QUERY_SURFACE_FLOATS * 4, hipMemcpyDeviceToHost));
    if (out64) HIP_TRY_AS("hr_debug_surface", hipMemcpy(out64, d_out64, (size_t)n * 6 * 8, hipMemcpyDeviceToHost));
    HIP_TRY_AS("hr_debug_surface", hipMemcpy(out_element, d_el, (size_t)n * 4, hipMemcpyDeviceToHost));
    return HR_OK;
}

int hr_debug_sky(hr_ctx *c, uint32_t n, const float *dirs, float *rgb, uint32_t *where) {
    if (!c || !dirs || !rgb || !where || !n) return fail(HR_ERR_INVALID, "hr_debug_sky: bad argument");
    int rc = debug_refusal(c, "hr_debug_sky", NO_REGION | NO_MASK | A_SCENE);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    CallScratch scratch;
    float *d_dirs = nullptr, *d_rgb = nullptr;
    uint32_t *d_where = nullptr;
    HIP_TRY_AS("hr_debug_sky", scratch.alloc((void **)&d_dirs, (size_t)n * 3 * 4));
    HIP_TRY_AS("hr_debug_sky", scratch.alloc((void **)&d_rgb, (size_t)n * 3 * 4));
    HIP_TRY_AS("hr_debug_sky", scratch.alloc((void **)&d_where, (size_t)n * 3 * 4));
    HIP_TRY_AS("hr_debug_sky", hipMemcpy(d_dirs, dirs, (size_t)n * 3 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sky_debug_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->dsc, n, d_dirs, d_rgb, d_where);
    HIP_TRY_AS("hr_debug_sky", hipGetLastError());
    HIP_TRY_AS("hr_debug_sky", hipStreamSynchronize(c->stream));
    HIP_TRY_AS("hr_debug_sky", hipMemcpy(rgb, d_rgb, (size_t)n * 3 * 4, hipMemcpyDeviceToHost));
    HIP_TRY_AS("hr_debug_sky", hipMemcpy(where, d_where, (size_t)n * 3 * 4, hipMemcpyDeviceToHost));
    return HR_OK;
}

int hr_debug_texture(hr_ctx *c, uint32_t n, const int32_t *image, const double *uv, float *rgb, float *rough64, uint32_t *quad) {
    if (!c || !image || !uv || !rgb || !rough64 || !quad || !n) return fail(HR_ERR_INVALID, "hr_debug_texture: bad argument");
    int rc = debug_refusal(c, "hr_debug_texture", NO_REGION | NO_MASK | A_SCENE);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++)   // the kernel indexes the scene's image table with it
        if (image[i] < 0 || (uint32_t)image[i] >= c->num_images) return fail(HR_ERR_INVALID, "hr_debug_texture: point %u names image %d, the scene has %u", i, image[i], c->num_images);
    HIP_TRY(hipSetDevice(c->device));
    CallScratch scratch;
    int32_t *d_image = nullptr;
    double *d_uv = nullptr;
    float *d_rgb = nullptr, *d_rough = nullptr;
    uint32_t *d_quad = nullptr;
    HIP_TRY_AS("hr_debug_texture", scratch.alloc((void **)&d_image, (size_t)n * 4));
    HIP_TRY_AS("hr_debug_texture", scratch.alloc((void **)&d_uv, (size_t)n * 2 * 8));
    HIP_TRY_AS("hr_debug_texture", scratch.alloc((void **)&d_rgb, (size_t)n * 3 * 4));
    HIP_TRY_AS("hr_debug_texture", scratch.alloc((void **)&d_rough, (size_t)n * 4));
    HIP_TRY_AS("hr_debug_texture", scratch.alloc((void **)&d_quad, (size_t)n * 4 * 4));
    HIP_TRY_AS("hr_debug_texture", hipMemcpy(d_image, image, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY_AS("hr_debug_texture", hipMemcpy(d_uv, uv, (size_t)n * 2 * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(texture_debug_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->dsc, n, d_image, d_uv, d_rgb, d_rough, d_quad);
    HIP_TRY_AS("hr_debug_texture", hipGetLastError());
    HIP_TRY_AS("hr_debug_texture", hipStreamSynchronize(c->stream));
    HIP_TRY_AS("hr_debug_texture", hipMemcpy(rgb, d_rgb, (size_t)n * 3 * 4, hipMemcpyDeviceToHost));
    HIP_TRY_AS("hr_debug_texture", hipMemcpy(rough64, d_rough, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY_AS("hr_debug_texture", hipMemcpy(quad, d_quad, (size_t)n * 4 * 4, hipMemcpyDeviceToHost));
    return HR_OK;
}
