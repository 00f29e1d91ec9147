/*
 * hanamaru_hip.h — C ABI of the MI355X back end for hanamaru-renderer's render loop.
 *
 * What this replaces in the reference (all citations into /root/reference/src):
 *   - `Renderer::render`  (renderer.rs:25-46): the per-sampling, per-pixel, 2x2 sub-sample loop that
 *     accumulates `calc_pixel` into `accumulation_buf`          -> hr_render()
 *   - `PathTracingRenderer::calc_pixel` + `next_event_estimation` (renderer.rs:163-203, 269-296)
 *     incl. everything below it (scene.rs / bvh.rs / material.rs / texture.rs / camera.rs:66-96)
 *                                                               -> the HIP kernels behind hr_render()
 *   - `Renderer::update_imgbuf` (renderer.rs:64-90): scale, tonemap.rs Reinhard, gamma, filter.rs
 *     bilateral, color.rs quantise                              -> hr_resolve()
 *
 * The reference has no FFI; the seam is the `Renderer` trait (renderer.rs:20-25).  A Rust host keeps
 * its Scene/Camera/Material builders, loader and PNG writer, fills an `hr_scene_desc` with pointers
 * into its own `Vec<Vector3>` (Vector3 is #[repr(C)] {x,y,z: f64}, vector.rs:6-12) and calls these
 * entry points from `Renderer::render`.  See INTEGRATION.md for the Rust `extern "C"` block.
 *
 * Conventions: every function returns 0 (HR_OK) or a negative hr_status; hr_last_error() gives text.
 * No exceptions cross the boundary.  A context is bound to ONE GPU and is not thread-safe; different contexts may be driven by
 * different host threads at the same time (hr_last_error is per thread).  Multi-GPU is one context per GPU — one process each, or one
 * process driving them all —, sharded by sampling index (hr_render's `stride`).
 * Host buffers passed in are copied — the caller keeps ownership.  No torch / STL types in signatures.
 */
#ifndef HANAMARU_HIP_H
#define HANAMARU_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HR_ABI_VERSION 7

typedef enum hr_status {
    HR_OK = 0,
    HR_ERR_INVALID = -1,      /* bad argument / call order */
    HR_ERR_DEVICE = -2,       /* HIP runtime error (text in hr_last_error) */
    HR_ERR_NO_SCENE = -3,
    HR_ERR_NO_TARGET = -4,    /* hr_set_resolution not called */
    HR_ERR_RNG_WINDOW = -5,   /* a path consumed more ISAAC-64 outputs than the stored window */
    HR_ERR_UNSUPPORTED = -6
} hr_status;

/* vector.rs:6-12 — #[repr(C)] f64 triple */
typedef struct hr_vec3 { double x, y, z; } hr_vec3;

/* material.rs:9-15 SurfaceType.  `param` = f0 (GGX) or refractive_index (Refraction / GGXRefraction). */
enum { HR_DIFFUSE = 0, HR_SPECULAR = 1, HR_REFRACTION = 2, HR_GGX = 3, HR_GGX_REFRACTION = 4 };

/* texture.rs:72-75 Texture { image_texture: Option<ImageTexture>, color } */
typedef struct hr_texture {
    hr_vec3 color;            /* tint, multiplied with the bilinear sample (texture.rs:108-114) */
    int32_t image;            /* index into hr_scene_desc.images, or -1 = constant colour */
    int32_t _pad;
} hr_texture;

/* material.rs:17-23 Material */
typedef struct hr_material {
    int32_t surface;          /* HR_DIFFUSE ... */
    int32_t _pad;
    double param;
    hr_texture albedo, emission, roughness;
} hr_material;

/* decoded image, RGBA8, row 0 = top row (image crate order, texture.rs:59-63 flips y itself) */
typedef struct hr_image {
    const uint8_t *rgba;
    uint32_t width, height;
} hr_image;

/* scene.rs Intersectable implementors used by live scenes: Sphere :51, Cuboid :146, BvhMesh :236 */
enum { HR_SPHERE = 0, HR_CUBOID = 1, HR_MESH = 2 };

typedef struct hr_element {
    int32_t kind;
    int32_t _pad;
    hr_material material;
    hr_vec3 center; double radius;          /* HR_SPHERE  (scene.rs:51-55) */
    hr_vec3 aabb_min, aabb_max;             /* HR_CUBOID  (scene.rs:146-149, bvh.rs:8-11) */
    const hr_vec3 *vertexes;                /* HR_MESH: world-space (loader.rs:31) */
    uint64_t num_vertexes;
    const uint64_t *faces;                  /* 3 vertex indices per face (scene.rs:196-200, usize) */
    uint64_t num_faces;
} hr_element;

/* camera.rs:7-29 Camera (already built by Camera::new, camera.rs:45-64) */
typedef struct hr_camera {
    hr_vec3 eye, right, up, forward, plane_half_right, plane_half_up;
    double lens_radius, focus_distance;
    int32_t lens_shape;                     /* 0 = Square, 1 = Circle (camera.rs:31-36) */
    int32_t _pad;
} hr_camera;

/* scene.rs:268-276 Skybox: px, nx, py, ny, pz, nz */
typedef struct hr_skybox {
    int32_t face_image[6];
    hr_vec3 intensity;
} hr_skybox;

typedef struct hr_scene_desc {
    const hr_element *elements; uint32_t num_elements;   /* order = Scene.elements order (scene.rs:327-330) */
    const hr_image *images;     uint32_t num_images;
    hr_skybox skybox;
    hr_camera camera;
} hr_scene_desc;

/* Work / timing counters.  Counter fields are only filled when option "counters" = 1. */
typedef struct hr_stats {
    uint64_t paths;            /* calc_pixel-equivalents rendered since hr_clear */
    uint64_t rays;             /* scene.intersect-equivalents (primary + bounce + shadow) */
    uint64_t node_tests;       /* AABB tests performed by the traversal kernel */
    uint64_t tri_tests, sphere_tests, cuboid_tests;
    uint64_t rng_overflow;     /* paths that ran past the stored ISAAC window */
    double seed_kernel_ms;     /* sum of HIP-event durations of the seed kernel launches */
    double trace_kernel_ms;    /* ... of the path-trace megakernel launches */
    double post_kernel_ms;
    uint64_t seed_launches, trace_launches;
    uint64_t bvh_nodes, triangles, spheres, cuboids;   /* triangles: of the scene (early split clipping may store one as several references) */
    /* counters build only: wave-level phase statistics of the trace kernel (invocations, lanes served) */
    uint64_t shade_calls, shade_lanes, box_passes, box_lanes, leaf_calls, leaf_lanes, outer_iters;
    uint64_t phase_cycles[4];  /* counters build: wave-cycles in A shade, B refill, C box phase, C leaf phase */
    double bvh_build_ms;       /* device BVH build of the last hr_upload_scene (option bvh_builder = 1 | 2), else 0 */
    uint64_t seed_phase_cycles[8]; /* debug option seed_prof: consumer-wave cycles per phase of the seed kernel, [7] = groups */
    double debug_kernel_ms;    /* sum of HIP-event durations of the hr_render_debug launches (the traversal-only workload) */
    uint64_t debug_launches;
    /* the priority governor (option trace_boost): the level kernels start at now (0 = the seed kernel's producer waves first .. 4 = the
     * trace kernel's box and leaf phases first), launches it has judged since the last scene / resolution / option change, level changes */
    uint64_t governor_level, governor_decisions, governor_moves;
    /* counters build: NEE shadow rays the reference traces and discards, which the kernel knows to add nothing before it traces them
     * (sample on the emitter's far side; GGX with the emitter below the horizon) — not in `rays` */
    uint64_t shadow_culled;
    /* the governor's wave budget: how many of the trace kernel's persistent workgroups stay (0 = all of them) — fewer where the trace
     * kernel is the faster kernel of the pair and its surplus waves only slow the seed kernel beside it —, and how often it changed */
    uint64_t governor_budget, governor_budget_moves;
    uint64_t bvh_builder_used;  /* the builder the last hr_upload_scene used (0 host SAH, 1 device LBVH, 2 device PLOC): what option bvh_builder = -1 chose */
    uint64_t shading_in_force;  /* what option precise_shading means for the scene in place: 0 = fp32 shading (megakernel), 1 = precise shading in the
                                 * megakernel, 2 = precise shading in the split pipeline (same bits as 1), 3 = fp32 shading in the split pipeline (debug) */
} hr_stats;

typedef struct hr_ctx hr_ctx;

const char *hr_last_error(void);
int hr_abi_version(void);

int hr_create(int device_id, hr_ctx **out);
int hr_destroy(hr_ctx *ctx);

/* Scene: copies + converts to fp32 SoA, builds the device BVH, uploads.  HR_ERR_INVALID for a description the reference could not render
 * either (no elements, a mesh without data, an image index out of range, non-finite geometry or camera — the reference panics in its BVH
 * build on a NaN): the scene uploaded before stays in place. */
int hr_upload_scene(hr_ctx *ctx, const hr_scene_desc *scene);

/* Output target (ImageBuffer dims, renderer.rs:26-28).  Allocates + zeroes the fp32 RGB accumulator. */
int hr_set_resolution(hr_ctx *ctx, uint32_t width, uint32_t height);
/* Optional: accumulate into caller-owned DEVICE memory (W*H*3 floats), e.g. a torch tensor that
 * torch.distributed all-reduces over RCCL.  Pass NULL to return to the internal buffer.
 * EXCLUSIVE: one context per buffer, and the caller must not touch the buffer on another stream between hr_render and the next
 * hr_synchronize / read — a launch's radiance is added with plain loads and stores (no atomics), in a fixed order (bit-reproducible
 * renders).  Binding a buffer another context of this process holds returns HR_ERR_INVALID, and so does a pointer that is not device memory of
 * this context's device, is not float-aligned, or has fewer than W*H*3 floats between it and the end of its allocation.  hr_set_resolution unbinds. */
int hr_bind_accumulator(hr_ctx *ctx, float *device_rgb);
/* Region rendering (border / crop render): render only the window [x0, x0+w) x [y0, y0+h) of the W x H frame set by hr_set_resolution.
 *   - Needs hr_set_resolution first (else HR_ERR_NO_TARGET).  w == 0, h == 0 or a window that does not fit in the frame (x0 > W || w > W - x0,
 *     the same for y) is HR_ERR_INVALID, and the previous region, accumulator and binding stay in place.
 *   - On success the accumulator is reallocated to w*h*3 floats and zeroed, as hr_set_resolution does, and a bound accumulator is unbound.
 *     (0, 0, W, H) is the whole frame, as without a region; hr_set_resolution resets the region to the whole frame.
 *   - Every accumulator-shaped entry point then works on the region's w*h*3 floats, row-major, top row first: hr_render, hr_render_debug,
 *     hr_read_accumulator / hr_write_accumulator, hr_bind_accumulator (its size check), hr_accumulator_sum, hr_allreduce_accumulator(s),
 *     hr_total_device_ptr.  hr_stats.paths counts w*h*4 per sampling.
 *   - The contract: a path's seed and camera ray come from its pixel's FRAME coordinates (renderer.rs:48-60, 164-168), so pixel (i, j) of a
 *     region accumulator is bit-identical to pixel (x0+i, y0+j) of a full-frame render with the same hr_render calls and options — both
 *     shading modes, both trace pipelines, and hr_render_debug's four modes.
 *   - hr_resolve writes w*h*3 bytes: renderer.rs:64-90 applied to the region's accumulator as an image of its own.  The bilateral filter's
 *     clamp and wrap (filter.rs) act at the region's edges, so every pixel at least one pixel inside them equals the full-frame image's byte and
 *     the border ring does not.  Exact 8-bit tiles of a frame come from stitching the tiles' ACCUMULATORS (hr_write_accumulator into a
 *     full-frame context, then one hr_resolve), not from stitching their images.
 *   - The unit-level hr_debug_* entry points (hanamaru_hip_debug.h) return HR_ERR_UNSUPPORTED while a region is set.
 * hr_get_region: the window in force as x0, y0, w, h ((0, 0, W, H) without a region). */
int hr_set_region(hr_ctx *ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h);
int hr_get_region(hr_ctx *ctx, uint32_t out_xywh[4]);
void *hr_accumulator_device_ptr(hr_ctx *ctx);
/* Optional: run on a caller-owned hipStream_t (opaque).  NULL = the context's own stream. */
int hr_set_stream(hr_ctx *ctx, void *hip_stream);

int hr_clear(hr_ctx *ctx);                 /* zero accumulator + stats */

/* Accumulate samplings s = begin, begin+stride, ... (s < end) — 1-origin like renderer.rs:31-32.
 * Each sampling adds the 2x2 sub-sample sum of calc_pixel to every pixel (renderer.rs:33-38,48-60).
 * Asynchronous with respect to the host; hr_synchronize() or any read waits. */
int hr_render(hr_ctx *ctx, uint32_t sampling_begin, uint32_t sampling_end, uint32_t stride);
int hr_synchronize(hr_ctx *ctx);
/* hr_render only enqueues.  hr_mark records a marker behind everything enqueued so far; hr_wait blocks until that marker is
 * reached while later work keeps running (a host loop can keep one chunk of samplings in flight while it reports on the
 * previous one — the reference's report_progress cadence, renderer.rs:205-251, without draining the GPU).  hr_synchronize
 * waits for everything and reports kernel-side errors. */
int hr_mark(hr_ctx *ctx, uint64_t *ticket);
int hr_wait(hr_ctx *ctx, uint64_t ticket);

/* DebugRenderer (renderer.rs:101-146, max_sampling = 1): adds ONE sampling of the chosen visualiser to the
 * accumulator — pinhole rays, no RNG.  mode: 0 Shading, 1 Normal, 2 Depth, 3 FocalPlane (renderer.rs:102-107;
 * the reference's -d flag selects FocalPlane, main.rs:1280).  Resolve with samplings_done = 1.
 * The rays go through the render kernel's traversal (same records, same box / leaf phases): Depth mode doubles as the
 * traversal-only workload of bench.py (hr_stats.debug_kernel_ms; with option "counters" the node / primitive test counts). */
int hr_render_debug(hr_ctx *ctx, int mode);

int hr_read_accumulator(hr_ctx *ctx, float *host_rgb);        /* W*H*3, row-major, top row first */
int hr_write_accumulator(hr_ctx *ctx, const float *host_rgb); /* resume / post-chain tests */

/* renderer.rs:64-90: scale by 1/(samplings*4) -> Reinhard -> gamma -> bilateral 3x3 -> u8 RGB. */
int hr_resolve(hr_ctx *ctx, uint32_t samplings_done, uint8_t *host_rgb8);

/* ---- multi-GPU (one node, RCCL over xGMI) --------------------------------------------------------------------------
 * The loop being sharded is renderer.rs:32-43: samplings are independent and seeded by index, so rank r of N renders
 * s = begin + r, begin + r + N, ... (hr_render's stride) into its own accumulator.  Before the resolve of renderer.rs:64-90
 * the accumulators are summed with ONE ncclAllReduce (fp32, W*H*3 values: 24.9 MB at 1080p).  The sum goes to a separate
 * buffer: the rank's own accumulator is untouched, so rendering can continue after a progress image.  After the call
 * hr_resolve / hr_read_accumulator return the TOTAL, until the next hr_render / hr_render_debug / hr_clear /
 * hr_write_accumulator on that context.  The collective is enqueued on the context's stream behind its render work.
 *   one process per GPU:   rank 0: hr_comm_get_unique_id -> share the HR_COMM_ID_BYTES with the other ranks (any transport)
 *                          every rank: hr_comm_init_rank, ..., hr_allreduce_accumulator
 *   one process, N GPUs:   hr_comm_init_local(ctxs, N), ..., hr_allreduce_accumulators(ctxs, N)   (one RCCL group call)
 * RCCL is loaded on first use; without it these return HR_ERR_UNSUPPORTED (the library has no host-side sum; a host that must run
 * on such a box sums hr_read_accumulator results itself, as the hanamaru-hip CLI does).  RCCL wants one
 * rank per device: hr_comm_init_local over contexts that all share ONE device (a single-GPU box) sums them with a kernel on
 * that device instead; a mix of shared and distinct devices is rejected. */
#define HR_COMM_ID_BYTES 128
int hr_comm_get_unique_id(void *id_out);
int hr_comm_init_rank(hr_ctx *ctx, const void *id, int world_size, int rank);
int hr_comm_init_local(hr_ctx **ctxs, int n);
int hr_comm_destroy(hr_ctx *ctx);
int hr_allreduce_accumulator(hr_ctx *ctx);
int hr_allreduce_accumulators(hr_ctx **ctxs, int n);
void *hr_total_device_ptr(hr_ctx *ctx);   /* device pointer of the all-reduced accumulator, NULL when not valid */

/* What the context's communicator says about ITSELF (asked of RCCL at the time of the call: ncclCommCount, ncclCommUserRank,
 * ncclCommCuDevice, ncclGetVersion) — so that a host can print evidence that its all-reduce really ran over N ranks:
 *   path  HR_COMM_NONE            no communicator
 *         HR_COMM_RCCL_RANK       hr_comm_init_rank: this process is one rank of an RCCL communicator
 *         HR_COMM_RCCL_GROUP      hr_comm_init_local over distinct devices: one process, one RCCL communicator per device
 *         HR_COMM_SAME_DEVICE_SUM hr_comm_init_local over contexts that share one device: NOT RCCL, a sum kernel on that device
 *   nranks / rank / device: RCCL's answers (same-device sum: the group's size, this context's index, the shared device)
 *   rccl_version: ncclGetVersion's code (0 without RCCL);  allreduces: collectives this context has enqueued on that communicator */
enum { HR_COMM_NONE = 0, HR_COMM_RCCL_RANK = 1, HR_COMM_RCCL_GROUP = 2, HR_COMM_SAME_DEVICE_SUM = 3 };
typedef struct hr_comm_info_t {
    int32_t path, nranks, rank, device;
    int32_t rccl_version, _pad;
    uint64_t allreduces;
} hr_comm_info_t;
int hr_comm_info(hr_ctx *ctx, hr_comm_info_t *out);
/* Which RCCL the library runs its collective on: the path of the shared object ncclAllReduce was resolved from (NUL-terminated into
 * path_out, truncated to cap), *reused_out = 1 when an RCCL already mapped into the process was taken instead of loading another one —
 * the library never puts a second RCCL build beside the host's (PyTorch maps its own torch/lib/librccl.so).  Loads RCCL if nothing has
 * yet; HR_ERR_UNSUPPORTED (and the loader's message) when there is none. */
int hr_comm_library(char *path_out, size_t cap, int *reused_out);
/* Per-channel sum of an accumulator, in f64 on the device: which = 0 this context's own accumulator, 1 = the all-reduced total.
 * The checksum of the exchange: the ranks' own sums add up to the total's sum (to fp32 rounding of the all-reduce: ~1e-7 relative). */
int hr_accumulator_sum(hr_ctx *ctx, int which, double out_rgb[3]);

/* ---- per-pixel sample moments and the noise estimate (option "moments", off by default) ------------------------------
 * "How converged is this image?"  With option "moments" = 1 the context keeps, per pixel and channel, the first and second moments of the
 * per-sampling pixel values x_s (the 2x2 sub-sample sum of calc_pixel, renderer.rs:33-38,48-60: what a sampling adds to the accumulator),
 *     S1 = sum x_s,  S2 = sum x_s^2   (f64; x_s is the fp32 value hr_clear + hr_render(s, s+1, 1) + hr_read_accumulator returns for the pixel)
 * added one sampling at a time in the order the samplings are rendered — so, unlike the fp32 accumulator, they do not depend on how
 * hr_render cuts samplings into launches ("batch", "max_tail_gib", calls in pieces).  Layout: h x w x 6 doubles {S1r, S1g, S1b, S2r, S2g, S2b},
 * row-major, top row first (100 MB at 1920x1080), plus the count n of samplings behind them.  The accumulator is bit-identical with the
 * option on or off; with it off nothing changes (same kernels).  Cost with it on: not yet measured on the device — from the code about
 * 200 MB of extra traffic per 24-ms launch at 1080p (expected well under 1 %).
 *   - hr_set_option "moments" 1 needs hr_set_resolution first (HR_ERR_NO_TARGET), allocates and zeroes the buffer and the count (set again
 *     while on: nothing happens); 0 frees it.  The moments cover the samplings rendered since the latest of: switching on, hr_clear,
 *     hr_set_resolution, hr_set_region (all zero them; the last two reallocate to the new size), hr_write_moments.  hr_write_accumulator
 *     does not touch them (a host that resumes writes both).  hr_render_debug returns HR_ERR_UNSUPPORTED while the option is on.
 *   - With the option off the four functions below return HR_ERR_INVALID.  With a region they work on its w x h pixels.
 *   - The estimate, per pixel (n >= 2, else HR_ERR_INVALID; all f64):
 *         m_c = S1_c / n      var_c = max(0, (S2_c - S1_c m_c) / (n - 1))      se_c = sqrt(var_c / n) / 4      mu_c = m_c / 4
 *         e   = (se_r + se_g + se_b) / (mu_r + mu_g + mu_b + 3 floor)
 *     se is the standard error of the pixel's radiance under independent samplings (the per-path seeding guarantees that).  `floor`
 *     (radiance units, > 0) keeps black pixels from dividing by zero: below it error is judged absolutely instead of relatively.  It says
 *     nothing about bias, nor about fireflies that have not happened yet.
 *     hr_noise_estimate: mean and maximum of e over the pixels and how many have e > threshold (threshold >= 0), reduced on the device in a
 *     fixed order (two calls return identical bits).  hr_read_noise_image: e of every pixel, w*h doubles.
 *   - Multi-GPU: each context counts and accumulates its own shard (hr_render's stride).  Moments are additive: a host adds the ranks'
 *     hr_read_moments results and counts in rank order and may hr_write_moments the total into one context to ask for the estimate.
 *     hr_fold_statistics (below) does that on the device: it moves every rank's moments and count to rank 0, which then answers.
 *   - All of them synchronise (they read results back), like hr_accumulator_sum. */
typedef struct hr_noise {
    uint64_t samplings, pixels, pixels_above;
    double mean_error, max_error;
} hr_noise;
int hr_read_moments(hr_ctx *ctx, double *host /* w*h*6 */, uint64_t *samplings /* may be NULL */);
int hr_write_moments(hr_ctx *ctx, const double *host, uint64_t samplings);   /* resume, tile stitching */
int hr_noise_estimate(hr_ctx *ctx, double floor, double threshold, hr_noise *out);
int hr_read_noise_image(hr_ctx *ctx, double floor, double *host /* w*h */);

/* ---- adaptive sampling: per-pixel sample counts and the active-tile mask (option "sample_counts", off by default) ----------
 * "Stop rendering what is done."  A frame converges unevenly; with a tile mask in force hr_render covers only the ACTIVE 4x4-pixel tiles of the
 * region, and with option "sample_counts" = 1 every pixel knows how many samplings it has received.
 *   - The contract: a path's seed and camera ray depend only on its frame pixel, its sub-sample and its sampling index.  Under a mask
 *     hr_render(b, e, stride) adds to every pixel of an active tile exactly the per-sampling values x_s a render without the mask adds, and
 *     nothing to any other pixel.  A pixel that has received samplings 1 .. n holds the accumulator contributions and the moments of a uniform
 *     render of samplings 1 .. n (the moments bit for bit; the fp32 accumulator as far as the launches are cut alike, see option "batch").
 *   - hr_set_option "sample_counts" 1 needs hr_set_resolution first (HR_ERR_NO_TARGET), allocates and zeroes counts[h][w] (uint32, region-local
 *     like the accumulator; set again while on: nothing happens); 0 frees it and removes the mask.  Every hr_render launch adds its samplings to
 *     the count of each pixel it adds radiance to.  The counts are zeroed by hr_clear, reallocated and zeroed by hr_set_resolution and
 *     hr_set_region, replaced by hr_write_sample_counts, and not touched by hr_write_accumulator / hr_write_moments (a host that resumes writes
 *     all three).  The accumulator and the moments are bit-identical with the option on or off.  hr_render_debug returns HR_ERR_UNSUPPORTED
 *     while it is on.  With the option off the functions below return HR_ERR_INVALID (hr_get_tile_mask excepted).
 *   - hr_read_sample_counts / hr_write_sample_counts: w*h uint32, row-major, top row first — resume, tile stitching, shards.  Counts are
 *     additive like moments: a host adds the ranks' counts, or hr_fold_statistics (below) moves them to rank 0.
 *   - With "sample_counts" and "moments" both on, hr_noise_estimate and hr_read_noise_image take the PIXEL's count as n, and return
 *     HR_ERR_INVALID if any pixel of the region has a count below 2.  hr_noise.samplings keeps its meaning (samplings issued since the
 *     moments were zeroed).  With "sample_counts" off nothing about the two changes.  The counts are the moments' n, so the two cover the
 *     same samplings: switching either option on while the other is on zeroes the other as well (the accumulator stays), and the estimate
 *     and hr_select_tiles return HR_ERR_INVALID when a pixel's count exceeds the samplings behind the moments (a host that writes one of
 *     them writes both).
 *   - hr_resolve_counted: hr_resolve with the scale 1.0f / (float)(counts[p] * 4u) per pixel — equal counts S give the bytes of
 *     hr_resolve(ctx, S, ..).  A count of 0 resolves as radiance 0.  Like hr_resolve it reads the all-reduced total while that is valid: the
 *     caller must then have written the summed counts.
 *   - hr_set_tile_mask: mask = tiles_y * tiles_x bytes over the region's 4x4 tiles, row-major, top row first, tiles_x = (w + 3) / 4,
 *     tiles_y = (h + 3) / 4, nonzero = render the tile; NULL removes the mask.  Needs "sample_counts" on (HR_ERR_INVALID: an image whose pixels
 *     have unequal counts cannot be resolved without them).  The mask is a setting, like the region: hr_clear keeps it; hr_set_resolution,
 *     hr_set_region and switching "sample_counts" off remove it.  With no tile active hr_render enqueues nothing and returns HR_OK.
 *     hr_stats.paths counts 4 x (in-region pixels of the active tiles) per sampling.  A sparse mask gets more samplings per launch (up to 64),
 *     as a small region does.
 *   - hr_get_tile_mask: the mask in force into `mask` (may be NULL) and the number of active tiles into `active` (may be NULL); without a mask
 *     every byte is 1 and *active is the region's tile count.
 *   - hr_select_tiles (needs "moments" and "sample_counts"; every count >= 2, else HR_ERR_INVALID): a tile is active iff e > threshold for at
 *     least one of its in-region pixels, e being exactly the value hr_read_noise_image(floor) returns for the pixel.  The result is ANDed
 *     with the mask in force and becomes the mask: a tile that went inactive stays inactive until hr_set_tile_mask(NULL) starts over, so a
 *     pixel's samplings are always a prefix 1 .. n of those issued.  Decided and compacted on the device, deterministically: two calls give
 *     the same mask.  *active (may be NULL): tiles left.
 *   - While a mask is set: hr_render_debug and the unit-level hr_debug_* entry points return HR_ERR_UNSUPPORTED, and so does hr_render with
 *     "counters", "russian_roulette", or the debug options min_waves, seed_mode (other than 2) or seed_prof changed — the kernels over a tile
 *     list exist for fp32 and precise shading, both trace pipelines and both node formats.
 *   - What it is not: selecting tiles by the same samples that form the estimate biases the image slightly (a pixel that looks converged by
 *     luck stops early).  A uniform first phase keeps that small; the library does not dilate the mask and has no held-out estimate. */
int hr_read_sample_counts(hr_ctx *ctx, uint32_t *host /* w*h */);
int hr_write_sample_counts(hr_ctx *ctx, const uint32_t *host);
int hr_resolve_counted(hr_ctx *ctx, uint8_t *host_rgb8);
int hr_set_tile_mask(hr_ctx *ctx, const uint8_t *mask /* tiles_y*tiles_x, NULL = none */);
int hr_get_tile_mask(hr_ctx *ctx, uint8_t *mask /* may be NULL */, uint32_t *active /* may be NULL */);
int hr_select_tiles(hr_ctx *ctx, double floor, double threshold, uint32_t *active /* may be NULL */);

/* ---- guide planes and the variance-guided denoiser ---------------------------------------------------------------------------
 * "Do something about the noise that is left."  An edge-avoiding a-trous filter over the mean radiance, steered by the per-pixel variance the
 * moments give and by first-hit guide planes.  hr_resolve's 3x3 bilateral filter is part of the reference's look and stays what it is.
 *   - The guide planes: h x w x 8 floats per pixel {albedo r, g, b (texture x tint), normal x, y, z, depth (hit distance along the pinhole ray),
 *     coverage}, row-major, top row first: the mean over the pixel's 2x2 sub-samples of the primary PINHOLE ray's hit (no lens, no RNG: the
 *     rays of hr_render_debug); a sub-sample that misses contributes eight zeros, so coverage is the fraction that hit.  hr_render_guides is one
 *     pass of the production traversal over the whole region — whatever tile mask is set — that STORES the planes.  A guide pixel depends on its
 *     frame pixel only: a region's guides are bit-identical to that window of a full-frame pass.  The pass touches neither the accumulator nor the
 *     moments, the counts or hr_stats.paths; its time goes to hr_stats.debug_kernel_ms / debug_launches.  hr_read_guides returns the planes as
 *     outputs in their own right (AOVs; HR_ERR_INVALID while there are none); hr_write_guides replaces them (resume, stitching, synthetic inputs).
 *     The buffer is allocated on first use, dropped by hr_set_resolution, hr_set_region and hr_upload_scene, and kept by hr_clear.
 *   - Option "guide_bounces" = K, 1 .. 8 (default 0: the planes above): the guide ray follows mirrors and glass — the Specular and Refraction
 *     surface types, whose bounce is deterministic — for up to K bounces, and the planes hold the first hit that is neither.  A mirror is
 *     followed along its mirror direction; glass along the branch the sampler takes for the draw r0 = 1: transmission, or the reflection on total
 *     internal reflection.  GGX, GGXRefraction and Diffuse end the chain; a chain that leaves the scene after a bounce ends at its last hit (a
 *     mirror that shows sky is guided like the mirror); a primary miss is eight zeros as before.  Albedo is then the PRODUCT of the albedos along
 *     the chain, the normal the terminal hit's world normal, depth the path length summed over the segments; coverage, the 2x2 mean, the layout,
 *     the region contract, the ignored tile mask and the accounting are as above.  The definition is guide_chain_link in csrc/pt_core.h; with
 *     K = 0 it is the first hit's values bit for bit.  Setting a new value drops the guide planes (rendered or written) and invalidates D.
 *   - hr_render_guides_lens(ctx, L), L = 4 or 16: the image is rendered through the thin lens (camera.rs:83-96) and the pinhole planes are sharper
 *     than it where it is out of focus.  This call is hr_render_guides with each sub-sample's values averaged over L fixed points of the lens: the
 *     ray of lens point (u, v) starts at eye + lens_radius (u right + v up) and passes through the sub-sample's point of the focus plane, in fp32
 *     (guide_lens_ray in csrc/pt_core.h); the chain of "guide_bounces" runs along it; per sub-sample the eight values are added in fp32 over
 *     l = 0 .. L - 1, the four sub-samples as before, and the sum x 0.25 / L is stored.  A ray that misses adds eight zeros: coverage is the
 *     fraction of the 4 L rays that hit.  The points are a fixed table (guide_lens_point; no RNG): multiples of 1/64 in the reference's [-1, 1]^2
 *     lens coordinates, symmetric under (u, v) -> (-u, -v), centroid exactly 0, all strictly inside the lens.  hr_guide_lens_points(lens_shape
 *     0 Square | 1 Circle, L, uv) returns them as {u0, v0, u1, v1, ..} in the order they are summed; it needs no device.  Everything else is
 *     hr_render_guides' contract: the whole region whatever the tile mask, a region's planes are the frame's window bit for bit, nothing but the
 *     guide planes is touched, the time goes to debug_kernel_ms / debug_launches (one launch), the planes count as rendered planes (they replace
 *     the old ones and invalidate D; a new "guide_bounces" value drops them; a later hr_render_guides replaces them with pinhole planes).  L other
 *     than 4 or 16 is HR_ERR_INVALID and leaves the planes and D as they were.  A camera with lens_radius == 0 has one lens point: the call then
 *     IS hr_render_guides (the same kernels, the same bits).  The cost is about L pinhole passes.
 *   - hr_denoise computes D, w x h x 3 floats of radiance (what accumulator x 1 / (4 n) is), from this context's OWN accumulator — never the
 *     all-reduced total: a sharded host writes the summed accumulator, moments and counts into one context, as it does for the estimate —,
 *     the moments and the guides.  The definition is csrc/denoise_core.h, to the bit (f64, + - x / max only, one IEEE operation per step, no FMA):
 *         C0_c = accumulator_c x fp32(1 / (4 n))      V0_c = var_c / n / 16   (var_c as in the noise estimate: the variance of the mean)
 *         demodulate = 1 and levels > 0: C / (A + eps) and V / (A + eps)^2 are filtered and the result is multiplied by (A + eps), eps = 1e-3
 *         level l = 0 .. levels - 1, step s = 2^l, taps q = p + s (i, j), i, j in -2 .. 2 (a tap outside the region is skipped, not clamped),
 *         h = k[|i|] k[|j|], k = {3/8, 1/4, 1/16},  K(x) = max(0, 1 - x)^2,  tiny = 1e-30
 *             x_n = |N_p - N_q|^2 / sigma_normal^2        x_a = |A_p - A_q|^2 / sigma_albedo^2        x_h = (H_p - H_q)^2
 *             x_z = (Z_p - Z_q)^2 / (sigma_depth^2 (Z_p^2 + Z_q^2) + tiny)
 *             x_c = |C_p - C_q|^2 / (sigma_color^2 (sumV_p + sumV_q) + tiny)          (C, V of the level's input)
 *             w = h K(x_n) K(x_a) K(x_z) K(x_h) K(x_c)      C'(p) = sum w C(q) / sum w      V'_c(p) = sum w^2 V_c(q) / (sum w)^2
 *         D = (float)C of the last level; levels = 0: D = (float)C0, the radiance the resolve tone-maps.
 *     n is the samplings behind the moments, or with option "sample_counts" on the pixel's own count.
 *   - hr_denoise returns HR_ERR_INVALID with option "moments" off; when a pixel has n < 2 (like the noise estimate); with "sample_counts" on when
 *     a count exceeds the samplings behind the moments (like hr_select_tiles); for levels > 5, demodulate > 1 or a sigma that is not finite and
 *     > 0.  In all of these D stays as it was.  params = NULL: hr_denoise_default_params' (levels 4, demodulate 1, sigma_color 3, sigma_normal 0.5,
 *     sigma_albedo 0.25, sigma_depth 0.1; it needs no device).  Without guide planes (none rendered or written since they were last dropped)
 *     hr_denoise runs hr_render_guides itself.
 *   - D is valid until anything it was made of changes: hr_render, hr_render_debug, hr_clear, hr_write_accumulator / _moments / _sample_counts /
 *     _guides, hr_render_guides, hr_upload_scene, hr_bind_accumulator, switching "moments" or "sample_counts", hr_set_resolution, hr_set_region.
 *     hr_read_denoised and hr_resolve_denoised return HR_ERR_INVALID without a valid D.  hr_resolve_denoised is renderer.rs:64-90 on D with
 *     the scale 1.0f: with levels = 0 the bytes of hr_resolve(ctx, n, ..) — of hr_resolve_counted with "sample_counts" on.
 *   - Nothing changes for a caller that never calls these functions (same kernels), and none of them writes the accumulator, moments or counts.
 *   - With a region the taps stop at the region's edge: the last level reaches 2 x 2^(levels - 1) pixels, and through the levels before it a
 *     pixel depends on inputs up to 2 x (2^levels - 1) pixels away, so pixels within that distance of the edge differ from the full-frame
 *     result and those further inside equal it.  As with the bilateral filter, exact tiles of a frame come from stitching the tiles'
 *     accumulators, moments, counts and guides into one full-frame context.
 *   - What it is not: the filter itself has no temporal part — history comes in before it, as counts and moments (hr_reproject below).  By default the guides are the FIRST hit's — what is seen through or in glass and mirrors is
 *     guided by the glass surface; "guide_bounces" follows mirrors and glass to the first rough hit, but not low-roughness GGX, only one branch
 *     at glass (no separate reflect / transmit planes), and the normal is not reflected into a mirror's virtual space.  The sigmas are design
 *     parameters: the defaults are the best row of a small host-side sweep (DESIGN.md 4.9 has the tables).  With first-hit guides that sweep
 *     shows the filter RAISING the error of a 64-sampling rtcamp6_v3_1 render (ratio 1.50); with "guide_bounces" 2 the same figure is 0.60.
 *   - Cost at 1920x1080: not yet measured on the device (hr_stats.post_kernel_ms of one hr_denoise, debug_kernel_ms of one hr_render_guides);
 *     hr_denoise holds 2 x w x h x 6 doubles of scratch for the call (199 MB).  All of these synchronise except hr_render_guides. */
typedef struct hr_denoise_params {
    uint32_t levels;       /* 0..5 */
    uint32_t demodulate;   /* 0 | 1 */
    double sigma_color, sigma_normal, sigma_albedo, sigma_depth;
} hr_denoise_params;
int hr_denoise_default_params(hr_denoise_params *out);
int hr_render_guides(hr_ctx *ctx);                         /* one pinhole pass into the guide buffer ("guide_bounces": through mirrors and glass) */
int hr_render_guides_lens(hr_ctx *ctx, uint32_t lens_points /* 4 | 16 */);   /* the same, averaged over fixed points of the thin lens */
int hr_guide_lens_points(int lens_shape, uint32_t lens_points, float *uv /* 2*lens_points */);   /* the lens points' table; needs no device */
int hr_read_guides(hr_ctx *ctx, float *host /* w*h*8 */);  /* the planes as outputs in their own right (AOVs) */
int hr_write_guides(hr_ctx *ctx, const float *host);       /* resume, stitching, synthetic inputs */
int hr_denoise(hr_ctx *ctx, const hr_denoise_params *p /* NULL = defaults */);
int hr_read_denoised(hr_ctx *ctx, float *host /* w*h*3 radiance */);
int hr_resolve_denoised(hr_ctx *ctx, uint8_t *host_rgb8);  /* renderer.rs:64-90 on D with scale 1.0f */

/* ---- sample buckets and the firefly-robust resolve (option "robust_buckets", off by default) -------------------------------------
 * The estimator has next-event estimation to small emitters and no MIS: a short render is dominated by a few paths that carry hundreds of times
 * their pixel's mean, and the plain mean of the samplings shows them as fireflies.  With option "robust_buckets" = K (K odd, 3 .. 15) the context
 * keeps, per pixel, K x 3 f64 sums of the per-sampling values x_s of "moments" above: the j-th sampling a pixel receives (j = 0, 1, .. per pixel,
 * in the order rendered) adds (double)x_s per channel to bucket j mod K, one sampling at a time from the value in the buffer.  hr_robust turns
 * them into R, an adaptive median of the bucket means (after Buisine et al. 2021): no extra path is traced.
 *   - buckets[h][w][K][3] f64, region-local.  Memory: 3 K doubles per pixel — 448 MB at 1920x1080 with K = 9, 747 MB with K = 15.
 *   - With "sample_counts" on, j starts at the pixel's own count; without it at the samplings behind the buckets (the count hr_read_buckets
 *     returns).  The buckets therefore do not depend on how samplings are cut into launches, and under a tile mask a pixel that has received
 *     samplings 1 .. n holds the buckets of a uniform render of samplings 1 .. n.
 *   - hr_set_option "robust_buckets" K needs hr_set_resolution first (HR_ERR_NO_TARGET), allocates and zeroes the buckets and their count; the
 *     value it already has changes nothing; another K starts them over; 0 frees them; any other value is HR_ERR_INVALID and changes nothing.
 *     hr_clear, hr_set_resolution and hr_set_region zero them (the last two at the new size).  Buckets that start (over) while "sample_counts"
 *     is on zero the counts — a pixel's count is the ordinal of its next sampling — and with the counts the moments whose n they are; switching
 *     "sample_counts" on (or "moments" on while the counts run, which zeroes the counts) zeroes the buckets.  hr_write_accumulator / _moments /
 *     _sample_counts do not touch them: a host that resumes writes all of them.  hr_render_debug returns HR_ERR_UNSUPPORTED while the option is
 *     on.  The option does not need "moments".  The accumulator, the moments and the counts are bit-identical with the option on or off, and
 *     with it off nothing more is launched.
 *   - hr_read_buckets / hr_write_buckets: w*h*K*3 doubles and the samplings behind them — resume, tile stitching.  Buckets of several ranks can
 *     be added only when every rank rendered a multiple of K samplings (bucket b of every rank then holds the same share) — or, whatever
 *     they rendered, when they were filled with option "bucket_by_sampling" 1 (see hr_fold_statistics below, which then adds them on the device).
 *   - hr_robust computes R (w x h x 3 floats of radiance) and the trim plane (w x h bytes) — both allocated on first use; its time goes to
 *     hr_stats.post_kernel_ms.  The definition is csrc/robust_core.h, to the bit (f64; + - x /, comparisons and one truncation; one IEEE
 *     operation per step, no FMA).  For a pixel with n samplings (its own count with "sample_counts" on, else the count behind the buckets) and
 *     bucket sums B[b][c]:
 *         n == 0   R = 0;      n < K   R_c = ((B[0][c] + B[1][c]) + .. + B[K-1][c]) / n / 4 (the plain mean), trim = 0;       otherwise
 *         n_b = (n - b + K - 1) / K (integer);   m_b,c = B[b][c] / n_b / 4;   y_b = (m_b,r + m_b,g) + m_b,b;   buckets ascending by (y_b, b);
 *         T = sum_i y_(i);   Gn = sum_i (2 i - K - 1) y_(i), i = 1 .. K;   trim = 0 if T <= 0, else G = Gn / (K T) (the Gini coefficient of the
 *         bucket means), trim = G > 0 ? min((K - 1) / 2, (int)(G K / 2)) : 0;   R_c = (sum_{i = trim + 1 .. K - trim} m_(i),c) / (K - 2 trim).
 *     Equal buckets give trim 0 (the mean of the bucket means), one bucket holding everything gives (K - 1) / 2 (the median bucket).  R is biased
 *     dark where it trims; the bias shrinks as the bucket means converge (DESIGN.md 4.10 has the measured figures).
 *   - R is valid until anything it was made of changes: hr_render, hr_clear, hr_write_accumulator / _moments / _sample_counts / _buckets,
 *     hr_bind_accumulator, switching "robust_buckets", "moments" or "sample_counts", hr_set_resolution, hr_set_region.  hr_read_robust,
 *     hr_read_robust_trim and hr_resolve_robust return HR_ERR_INVALID without a valid R; all six functions return HR_ERR_INVALID with the option
 *     off; in both cases R stays as it was.  hr_resolve_robust is renderer.rs:64-90 on R with the scale 1.0f, as hr_resolve_denoised is on D.
 *   - hr_noise_estimate, hr_select_tiles and hr_denoise still read the raw moments; the robust noise estimate and hr_denoise_robust below read
 *     the buckets.  All of these synchronise. */
int hr_read_buckets(hr_ctx *ctx, double *host /* w*h*K*3 */, uint64_t *samplings /* may be NULL */);
int hr_write_buckets(hr_ctx *ctx, const double *host, uint64_t samplings);   /* resume, tile stitching */
int hr_robust(hr_ctx *ctx);
int hr_read_robust(hr_ctx *ctx, float *host /* w*h*3 radiance */);
int hr_read_robust_trim(hr_ctx *ctx, uint8_t *host /* w*h: buckets dropped at either end */);
int hr_resolve_robust(hr_ctx *ctx, uint8_t *host_rgb8);  /* renderer.rs:64-90 on R with scale 1.0f */
/* The robust noise estimate: how converged R is, from the spread of the pixel's own bucket means — not from the raw moments, which
 * the few paths that R leaves out dominate.  e_R of a pixel is the Tukey-McLaughlin (winsorized) standard error of the trim-trimmed mean of its K
 * bucket means, taken on the channel sum y, over that mean plus 3 floor.  The definition is robust_pixel_error in csrc/robust_core.h, to the bit but
 * for the device's f64 sqrt (within 4 ulp; bit-identical where the spread is 0): with n_b, y_b, their ascending order and trim exactly as above,
 *         kept = K - 2 trim;   Ry = (y_(trim+1) + .. + y_(K-trim)) / kept;   w_i = y_(i) clamped to [y_(trim+1), y_(K-trim)] by RANK, i = 1 .. K;
 *         wbar = (sum_i w_i) / K;   ss = sum_i (w_i - wbar)^2;   se = sqrt(ss / (K - 1) / K) K / kept;   den = Ry + 3 floor;
 *         e_R = den > 0 ? se / den : 0.
 *   - It is an error of the channel SUM, not hr_noise_estimate's se_r + se_g + se_b; with trim = (K - 1) / 2 (the median bucket) se is 0 by
 *     construction; and it is blind to R's dark bias, which is no noise.
 *   - All of them need "robust_buckets" on ("moments" is not needed) and return HR_ERR_INVALID with it off, for floor <= 0 or not finite, for
 *     threshold < 0, while any pixel of the region has fewer than K samplings (its own count with "sample_counts" on, else the count behind the
 *     buckets), and with "sample_counts" on when a pixel's count exceeds the samplings behind the buckets.  What is refused touches nothing.
 *   - hr_robust_noise_estimate: hr_noise of e_R (samplings: the count behind the buckets), reduced on the device in a fixed order — two calls
 *     return identical bits.  hr_read_robust_noise_image: e_R of every pixel.  hr_read_robust_noise_trim: the trim that the estimate took, pixel by
 *     pixel — hr_read_robust_trim's values without an hr_robust.
 *   - hr_select_tiles_robust (needs "sample_counts" as well) is hr_select_tiles with e_R in place of e: a tile stays active iff e_R > threshold
 *     for at least one of its in-region pixels — exactly the value hr_read_robust_noise_image returns — ANDed with the mask in force, compacted as
 *     there.
 *   - They work on the region, synchronise, put their time into hr_stats.post_kernel_ms, and touch neither R, the buckets, the moments nor the
 *     counts (R stays valid). */
int hr_robust_noise_estimate(hr_ctx *ctx, double floor, double threshold, hr_noise *out);
int hr_read_robust_noise_image(hr_ctx *ctx, double floor, double *host /* w*h */);
int hr_read_robust_noise_trim(hr_ctx *ctx, double floor, uint8_t *host /* w*h */);
int hr_select_tiles_robust(hr_ctx *ctx, double floor, double threshold, uint32_t *active /* may be NULL */);
/* The robust denoiser: hr_denoise's filter on the robust radiance and a robust variance — not on the accumulator and the raw
 * moments, which the few paths that R leaves out dominate.  Per pixel, with n_b, m_b,c, y_b, their ascending order (y_b, b) and trim exactly as
 * hr_robust's (the definition is robust_pixel_cv_k in csrc/robust_core.h, to the bit: f64, + - x /, comparisons and one truncation, NO sqrt):
 *         kept = K - 2 trim;   C_c = (m_(trim+1),c + .. + m_(K-trim),c) / kept                  (float)C_c is hr_robust's R_c
 *         w_i,c = m_(i),c with i clamped to [trim + 1, K - trim]: winsorized by the RANK in y, per channel, i = 1 .. K
 *         wbar_c = (sum_i w_i,c) / K;   ss_c = sum_i (w_i,c - wbar_c)^2;   f = K / kept;   V_c = ss_c / (K - 1) / K x f x f
 *     V_c is the Tukey-McLaughlin variance of the trimmed mean, per channel; 0 by construction with trim = (K - 1) / 2.  {C, V} take the place of
 *     hr_denoise's {C0, V0}; demodulation, the levels and the final pass are hr_denoise's (csrc/denoise_core.h), unchanged.
 *   - It writes the same D as hr_denoise: hr_read_denoised and hr_resolve_denoised serve both, D is whichever call succeeded last.  With
 *     levels = 0, D is R bit for bit and hr_resolve_denoised gives the bytes of hr_resolve_robust.
 *   - It needs "robust_buckets" on ("moments" is not needed), works on the region, runs hr_render_guides itself when there are no guide planes,
 *     synchronises, and puts its time into hr_stats.post_kernel_ms.  With "sample_counts" on every pixel has its own n.
 *   - HR_ERR_INVALID — and D, R, the buckets, the counts and the mask stay exactly as they were — with the option off, while any pixel of the
 *     region has fewer than K samplings, with "sample_counts" on when a count exceeds the samplings behind the buckets, and for the parameters
 *     hr_denoise refuses.
 *   - A D made by this call is valid until anything on hr_denoise's list changes, and also until "robust_buckets" is switched (every hr_write_*,
 *     hr_write_buckets among them, is on that list already).  A D made by hr_denoise keeps its own rules.  The call touches neither R's validity,
 *     the buckets, the accumulator, the moments nor the counts. */
int hr_denoise_robust(hr_ctx *ctx, const hr_denoise_params *p /* NULL = defaults */);

/* ---- the restored robust resolve R' (csrc/restore_core.h is the definition) -------------------------------------------------------
 * R is biased dark where it trims: a trimmed bucket's energy is gone.  R' gives it back without giving the hot pixel back: per pixel and channel the
 * excess X = what the t hot buckets hold above the highest kept bucket mean, over K (robust_pixel_excess_k: never negative, 0 where nothing is
 * trimmed), is spread over `levels` a-trous levels along the guide planes — each pixel hands X w(p,q) / sum_q w(p,q) to its 5 x 5 taps, w the
 * denoiser's tap weight without its colour term (h K(x_n) K(x_a) K(x_z) K(x_h)), written as a gather since w is symmetric to the bit — and added:
 * R'_c = (float)(base_c + X_L,c).  base 0: C, the robust radiance before its rounding; base 1: D of hr_denoise_robust.  All f64, + - x / max only:
 * the device, the header under a host compiler and a numpy restatement agree bit for bit.
 *   - Needs "robust_buckets" != 0; works on the region and with "sample_counts" (every pixel's own n); renders the guide planes itself
 *     (hr_render_guides) when there are none; synchronises; its time goes to hr_stats.post_kernel_ms.
 *   - HR_ERR_INVALID, with R', R, D, the buckets, the counts and the mask exactly as they were: the option off; a pixel of the region with fewer
 *     than K samplings; a count beyond the samplings behind the buckets; levels > 5; a sigma that is not positive and finite; base > 1; base 1
 *     without a valid D made by hr_denoise_robust.
 *   - R' is valid until anything that invalidates a D of hr_denoise_robust happens (hr_render, hr_render_debug, hr_clear, every hr_write_*,
 *     hr_render_guides, "guide_bounces", switching "robust_buckets", "moments" or "sample_counts", the target), and with base 1 until a new D is
 *     made.  The call touches neither R's nor D's validity, nor the buckets, nor the accumulator.  hr_read_restored and hr_resolve_restored return
 *     HR_ERR_INVALID without a valid R'.
 *   - levels = 0, base 0: R' = (float)(C + X); where no pixel trims R' is R bit for bit and hr_resolve_restored gives hr_resolve_robust's bytes.
 *   - What it is not: X is noisy — it is the firefly energy itself — so R' has a larger error than R (DESIGN.md 4.14 has the measured rows). */
typedef struct hr_restore_params {
    uint32_t levels;   /* 0..5 */
    uint32_t base;     /* 0: the robust radiance | 1: the denoised robust radiance of hr_denoise_robust */
    double sigma_n, sigma_a, sigma_z;
} hr_restore_params;
int hr_restore_default_params(hr_restore_params *out);     /* 4, 0, 0.5, 0.25, 0.1 */
int hr_robust_restore(hr_ctx *ctx, const hr_restore_params *p /* NULL = defaults */);
int hr_read_restored(hr_ctx *ctx, float *host /* w*h*3 radiance */);
int hr_resolve_restored(hr_ctx *ctx, uint8_t *host_rgb8);  /* renderer.rs:64-90 on R' with scale 1.0f */

/* ---- the denoiser that picks its level per pixel: S and its level plane L (csrc/select_core.h is the definition) ------------------
 * hr_denoise applies one `levels` to the whole frame, and a level too many RAISES the error of a converged pixel.  hr_denoise_select runs
 * hr_denoise's filter through every level 0 .. levels and keeps, per pixel, the level whose held-out error is the lowest.  The pixel's K sample
 * buckets split into two halves for free (even and odd b); each half is filtered on its own — the same levels, the same guides — and judged
 * against the RAW pixel of the other half, which its noise is independent of:
 *         n_b = (n - b + K - 1) / K;   n_A, n_B: the samplings of the even and of the odd buckets;   A0_c = (sum_{b even} B[b][c]) / n_A / 4, B0 likewise
 *         states {C, V}:  W = hr_denoise's {C0, V0};   A = {A0, V0 n / n_A};   B = {B0, V0 n / n_B}   (demodulated as hr_denoise's, A0 and B0 too)
 *         F_X,l = state X after l levels;   e_l = sum_c (F_A,l,c - B0_c)^2 + (F_B,l,c - A0_c)^2
 *         e_l smoothed by `smooth` passes of the 5 x 5 a-trous kernel (steps 1, 2, 4; weights h alone);   L = the lowest l with the smallest e_l
 *         (strict comparison: ties and NaN keep the lower level);   S = hr_denoise's final pass on F_W,L
 *     All f64, + - x / and comparisons only: the device, the header under a host compiler and a numpy restatement agree bit for bit.  Where
 *     L(p) = l, S(p) has the bits of hr_denoise(levels = l)'s D at p; with levels = 0 hr_resolve_selected gives hr_resolve's bytes.
 *   - Needs "robust_buckets" != 0 AND "moments" on; works on the region (the taps stop at its edge) and with "sample_counts" (every pixel's own
 *     n); renders the guide planes itself (hr_render_guides) when there are none; synchronises; its time goes to hr_stats.post_kernel_ms.
 *   - HR_ERR_INVALID, decided before anything is touched — an earlier S stays readable and unchanged: either option off; a pixel of the region
 *     with fewer than 2 samplings; moments, buckets (and counts) that do not cover the same samplings; the parameters hr_denoise refuses;
 *     smooth > 3; reserved != 0.
 *   - S and L are valid until the accumulator, the moments, the counts, the buckets, the guides, the scene or the target change (hr_render,
 *     hr_clear, every hr_write_*, hr_render_guides, "guide_bounces", switching "robust_buckets", "moments" or "sample_counts", hr_upload_scene,
 *     hr_set_resolution, hr_set_region).  A new D, R or R' and hr_set_tile_mask leave them alone, and the call touches none of D, R, R'.
 *     hr_read_selected, hr_read_selected_levels and hr_resolve_selected return HR_ERR_INVALID with "robust_buckets" off or without a valid S.
 *   - Memory for the call: about 360 bytes per pixel (746 MB at 1920x1080) — the three states twice, the halves' raw radiance, two error planes
 *     and the best error; S (12 B) and L (1 B) per pixel stay.  HR_ERR_DEVICE "out of memory" when the device has no room; nothing is written then.
 *   - What it is not: e_l is the error of filters on n / 2 samplings, so it leans towards more smoothing than the whole buffer needs; with
 *     smooth = 0 the pick is correlated with the pixel's own noise (the default, 2, has the lowest worst case of DESIGN.md 4.16's table; 0 is the
 *     better choice for short renders with first-hit guides); it is the plain estimator, not the robust one; there is no temporal part.
 *     Cost at 1920x1080 with K = 9 and levels 4 on one MI355X: 5.0 ms of hr_stats.post_kernel_ms with smooth 0, 5.3 ms with smooth 2 — 0.63 of
 *     three hr_denoise calls (tools/select_rate.py). */
typedef struct hr_select_params {
    uint32_t smooth;     /* 0..3 passes over the error planes */
    uint32_t reserved;   /* 0 */
} hr_select_params;
int hr_select_default_params(hr_select_params *out);       /* 2, 0; needs no device */
int hr_denoise_select(hr_ctx *ctx, const hr_denoise_params *p /* NULL = defaults */, const hr_select_params *s /* NULL = defaults */);
int hr_read_selected(hr_ctx *ctx, float *host /* w*h*3 radiance */);
int hr_read_selected_levels(hr_ctx *ctx, uint8_t *host /* w*h: the level each pixel took */);
int hr_resolve_selected(hr_ctx *ctx, uint8_t *host_rgb8);  /* renderer.rs:64-90 on S with scale 1.0f */

/* ---- the error estimate of S, its stop rule and its tile selection (csrc/select_noise_core.h is the definition) -----------------
 * hr_noise_estimate judges the raw mean and hr_robust_noise_estimate judges R; these four judge S, the image hr_denoise_select makes with the
 * parameters handed in (NULL = defaults).  Per level l and pixel, from the states of hr_denoise_select above (k_c = (A_c + eps)^2 with
 * demodulate && levels, else no factor at all):
 *         m_l = sum_c k_c (((F_A,l,c - B0_c)^2 + (F_B,l,c - A0_c)^2) - (V_A,0,c + V_B,0,c)) / 2      the held-out MSE of a half filter: half A is
 *               independent of B0, so E[(F_A,l - B0)^2] = MSE(F_A,l) + Var(B0), and Var(B0) is the level-0 variance that is subtracted
 *         m^_l = m_l through the same `smooth` passes as e_l;   vh = sum_c k_c (V_A,l,c + V_B,l,c) / 2;   vw = sum_c k_c V_W,l,c
 *         mse_l = vw + max(0, m^_l - vh)        the whole-buffer filter's propagated variance plus the half filters' squared bias
 *         M = mse_L at the level L the pick takes;   e_S = sqrt(M) / (S_r + S_g + S_b + 3 floor), 0 where that denominator is not positive
 *     M is f64, + - x / and comparisons only: the device, the header under a host compiler and a numpy restatement agree bit for bit.
 *   - hr_selected_noise_estimate: hr_noise of e_S (samplings: the count behind the moments), reduced on the device in a fixed order — two calls
 *     return identical bits.  hr_read_selected_noise_image: e_S of every pixel.  hr_read_selected_mse: M of every pixel (radiance squared).
 *   - hr_select_tiles_selected (needs "sample_counts" as well) is hr_select_tiles with e_S in place of e: a tile stays active iff e_S > threshold
 *     for one of its in-region pixels, e_S exactly the value hr_read_selected_noise_image returns; ANDed with the mask in force, compacted alike.
 *   - Each call runs hr_denoise_select's pipeline in memory of its own, S and L included, and leaves every kept image and its validity exactly
 *     as it was: S, L, D, R, R'.  The guide planes are the exception: they are rendered when there are none, as hr_denoise_select does.
 *   - HR_ERR_INVALID, decided before anything is touched: whatever hr_denoise_select refuses, in its order; floor <= 0 or not finite;
 *     threshold < 0; hr_select_tiles_selected without "sample_counts".
 *   - All four work on the region, synchronise, and book their time to hr_stats.post_kernel_ms.
 *   - Memory for the call: about 453 bytes per pixel (939 MB at 1920x1080) — hr_denoise_select's 360, the two level-0 variances (48), two planes
 *     of m (16), M (8), e_S (8) and the call's own S and L (13); nothing stays.  HR_ERR_DEVICE "out of memory" when the device has no room; nothing
 *     is touched then.
 *   - What it is not: the bias is that of filters on n / 2 samplings, whose colour kernel is wider — the estimate is conservative; the colour
 *     weights of A and B use V_W of all samplings; at L = 0 the clamp lets the positive half of the noise of m^_0 - vh_0 through; it is blind to
 *     what both halves share (guide errors, fireflies that have not happened yet). */
int hr_selected_noise_estimate(hr_ctx *ctx, const hr_denoise_params *p, const hr_select_params *s, double floor, double threshold, hr_noise *out);
int hr_read_selected_noise_image(hr_ctx *ctx, const hr_denoise_params *p, const hr_select_params *s, double floor, double *host /* w*h: e_S */);
int hr_read_selected_mse(hr_ctx *ctx, const hr_denoise_params *p, const hr_select_params *s, double *host /* w*h: M */);
int hr_select_tiles_selected(hr_ctx *ctx, const hr_denoise_params *p, const hr_select_params *s, double floor, double threshold, uint32_t *active /* may be NULL */);

/* ---- sharded statistics: buckets by sampling, and the fold into rank 0 ----------------------------------------------------------
 * Contexts that shard the samplings (hr_render's stride) each hold a share of every additive plane.  hr_fold_statistics moves the shares to
 * rank 0 of the communicator, so that ONE context answers every question with the functions above, unchanged: hr_noise_estimate,
 * hr_select_tiles, hr_denoise, hr_robust, hr_robust_noise_estimate, hr_select_tiles_robust, hr_denoise_robust, hr_resolve_counted, hr_read_*.
 *   - Option "bucket_by_sampling" 0 (default) / 1.  With 1 sampling s goes into bucket (s - 1) mod K whatever the pixel has received before; s is
 *     the index hr_render renders (s_begin, s_begin + stride, ..), and no count is read.  With 0 nothing differs by a bit from the ordinal form
 *     above.  hr_robust, the robust noise family and hr_denoise_robust are unchanged: they take bucket b to hold n_b = (n - b + K - 1) / K
 *     samplings, which is right if and only if the pixel has received samplings 1 .. n — on whatever contexts, once their buckets are added.  One
 *     context rendering 1 .. n from a clear gets buckets bit-identical to the ordinal form's; a host that skips or repeats indices gets what it
 *     asked for.  Switching the option while "robust_buckets" is on starts the buckets over exactly as another K does (the counts and the moments
 *     with them while "sample_counts" is on; R and a D of hr_denoise_robust are invalid); with "robust_buckets" off the value is only recorded.
 *     Any value other than 0 or 1 is HR_ERR_INVALID and changes nothing.
 *   - What a fold moves: the accumulator (fp32), and where their option is on the moments (f64) with their count, the sample counts (u32) and
 *     the buckets (f64) with their count.  Afterwards rank 0's own planes hold the sum over all ranks and its two counts are the sums; every
 *     other rank's planes are zero and its counts 0.  The global sum is preserved, so every rank simply goes on rendering and a later fold adds
 *     what came since.  A bound accumulator (hr_bind_accumulator) is folded in place.
 *   - Contexts that share one device (HR_COMM_SAME_DEVICE_SUM): a kernel adds rank 1, 2, .. to rank 0 in rank order — ((r0 + r1) + r2) .. to the
 *     bit in every type — and zeroes them; its time goes to rank 0's hr_stats.post_kernel_ms.  RCCL groups and ranks: one ncclReduce per plane in
 *     place to root 0, behind the render work on the context's stream, then the plane is zeroed on the other ranks; the summation order is
 *     RCCL's, so the result is equal to rounding, not to the bit.
 *   - hr_fold_statistics is the form of one process per GPU (hr_comm_init_rank; every rank calls it); hr_fold_statistics_group the form of one
 *     process with n contexts (hr_comm_init_local; ctxs in the order the group was made of, one ncclGroupStart / ncclGroupEnd).  For a context of
 *     a same-device group hr_fold_statistics folds the whole group, whichever context asks.
 *   - Both synchronise.  On EVERY rank the all-reduced total (hr_total_device_ptr), R and D are invalid afterwards; the tile mask, the guide
 *     planes, the options and hr_stats.paths stay.  (A host that selects tiles on rank 0 sets rank 0's mask on the others itself.)
 *   - HR_ERR_INVALID, and nothing is touched: no communicator; n is not the group's size or ctxs are not the contexts of ONE hr_comm_init_local call in its order; the
 *     contexts of the group differ in resolution, region, which of "moments", "sample_counts", "robust_buckets" are on, or K; "robust_buckets" is
 *     on with "bucket_by_sampling" 0 (ordinal buckets of different contexts do not add up); hr_fold_statistics on a context of an
 *     hr_comm_init_local group of several devices.  In the one-process-per-GPU form each rank can check only itself: ranks that differ there hand
 *     RCCL buffers of different sizes, which is the host's to avoid.  HR_ERR_NO_TARGET without a resolution, HR_ERR_UNSUPPORTED when RCCL is
 *     needed and cannot be loaded.  A group of one is a valid fold that moves nothing and still invalidates.
 *   - HR_ERR_DEVICE (a launch, a copy or an RCCL call failed on the way) is no refusal: some planes may have moved and others not, the counts are
 *     as they were, and the total, R and D are invalid on every rank.  The group's statistics cannot be trusted after it: hr_clear every context. */
int hr_fold_statistics(hr_ctx *ctx);
int hr_fold_statistics_group(hr_ctx **ctxs, int n);

/* ---- camera moves that keep their history ------------------------------------------------------------------------------------
 * The scene description carries its camera, and hr_upload_scene flattens, builds and uploads everything again.  A turntable or fly-through
 * changes the camera only:
 *   - hr_set_camera replaces the camera of the scene in place — the fp32 camera the kernels take and the f64 one on the device — with the
 *     conversions of hr_upload_scene.  After it every entry point gives the bits that a fresh context gives after hr_upload_scene of the same
 *     description with camera = cam: hr_render, hr_render_debug, the guide passes and the hr_debug_* queries, both shading modes, both trace
 *     pipelines, both node formats.  HR_ERR_NO_SCENE before a scene is uploaded; a camera that is not finite is HR_ERR_INVALID and the camera in
 *     place stays.  It synchronises, drops the guide planes and the motion plane (they show the old view) and makes every derived image that shows
 *     the scene stale, as hr_upload_scene does.  It touches neither the accumulator, the counts, the moments, the buckets, the tile mask, the
 *     region, the BVH, the textures nor hr_stats.bvh_build_ms / bvh_builder_used: what is accumulated stays accumulated — a host that wants a fresh
 *     frame calls hr_clear, one that wants to carry the old frame over calls hr_reproject.
 *   - hr_get_camera: the f64 camera in place, as it was uploaded or set (HR_ERR_NO_SCENE without a scene).
 *   - The motion plane: h x w x 4 x 3 floats, row-major, top row first: {mx, my, code} for each of a pixel's 2x2 sub-samples in the kernels' lane
 *     order (sub-sample s has sx = s & 1, sy = s >> 1 of renderer.rs:51-53).  (mx, my): where the point this sub-sample sees was in an EARLIER
 *     frame, as an offset in pixels from the pixel itself, y pointing down — the history of pixel (px, py) is at (px + mx, py + my) of the old
 *     planes.  code: 0 = may be reused; 1 = behind the old camera or off its frame; 2 = hidden from the old eye; 3 = a view-dependent surface
 *     (mirror, glass, smooth GGX); anything but 0 is "no history".  hr_read_motion returns the plane as an output in its own right (an AOV: motion
 *     vectors; HR_ERR_INVALID without a valid plane); hr_write_motion replaces it (synthetic inputs, stitched tiles; HR_ERR_NO_TARGET without a
 *     target).  The plane is allocated on first use and goes stale with hr_set_camera, hr_upload_scene, hr_set_resolution and hr_set_region;
 *     hr_clear keeps it.
 *   - hr_render_motion(ctx, from, params) renders the plane for the camera in place against the earlier camera `from`: one pass of the production
 *     traversal, two walks per sub-sample at most.  The scene is static and the library owns a ray tracer, so whether a history sample is valid is
 *     asked exactly, with a visibility ray from the old eye, not by comparing depth and normal planes.  Per sub-sample (motion_point and
 *     motion_verdict in csrc/pt_core.h; the f64 steps are reproject_project and reproject_motion in csrc/reproject_core.h, to the bit):
 *       1. the PINHOLE ray of the frame pixel and sub-sample (the rays of hr_render_debug and hr_render_guides), closest hit;
 *       2. a hit on Specular, Refraction or GGXRefraction, or on GGX with roughness below min_roughness, is view-dependent: {0, 0, 3}.  Otherwise the
 *          point is the fp32 hit point x, or for a miss the point at infinity along the ray direction d;
 *       3. into `from`, in f64: v = x - eye0 (a miss: v = d);  c = v . forward0, c <= 0: {0, 0, 1};  k = c / focus0;
 *          ncx = (v . phr0) / ((phr0 . phr0) k), ncy likewise with phu0 — the inverse of camera.rs:98-107, which needs `from` as Camera::new builds
 *          it (camera.rs:45-64): right, up and forward orthogonal, plane_half_right along right, plane_half_up along up.  With m = min(W, H):
 *          fx = (ncx m + W) / 2, fy = (ncy m + H) / 2 (renderer.rs:36,53-54), the sub-sample's own gx = px + ox, gy = (H - py) + oy;
 *          mx = fx - gx, my = gy - fy, a component with |.| < 2^-10 stored as 0 (a camera that did not move hands every pixel its own history
 *          exactly); fx outside [-1, W + 1] or fy outside [-1, H + 1]: {mx, my, 1};
 *       4. the sub-samples still at code 0 send a ray from (float)eye0 along normalize((float)v), closest hit: a point is visible when the walk
 *          hits with |t - |v|| <= depth_tolerance |v| (fp32), a sky direction when it misses; otherwise code 2.
 *     It follows hr_render_guides: the whole region whatever the tile mask; a region's plane is the frame's window bit for bit; it touches neither
 *     the accumulator, the statistics planes nor hr_stats.paths; one launch, timed into debug_kernel_ms / debug_launches; it does not synchronise.
 *     params = NULL: the defaults; the parameters hr_reproject refuses are refused here.  The lens is ignored, as the guide planes ignore it: with
 *     depth of field the motion is that of the pinhole image.
 *   - hr_reproject replaces the region's accumulator, counts and (with option "moments" on) moments by the history gathered along the motion
 *     plane; the next hr_render adds the new frame's samplings on top, and hr_resolve_counted, the noise estimate, tile selection and hr_denoise
 *     work as before, because every pixel knows its count.  The definition is reproject_pixel in csrc/reproject_core.h, to the bit (f64; + - x /,
 *     floor and comparisons, one IEEE operation per step, no FMA).  For each sub-sample with code 0 and a finite motion with |component| <= 2^20:
 *         u = px + mx,  v = py + my;  x0 = floor(u),  y0 = floor(v);  ax = u - x0,  ay = v - y0;  taps (x0 + i, y0 + j), i, j in {0, 1}, j outer;
 *         w = (i ? ax : 1 - ax) (j ? ay : 1 - ay); a tap is skipped when w == 0, outside the region, or when its old count n_q is 0; else
 *         Wp += w,  N += w n_q,  A_c += w (acc_q,c / n_q),  and with moments  M1_c += w (S1_q,c / n_q),  M2_c += w (S2_q,c / n_q)
 *     and per pixel n' = min(max_history, floor(N / 4)) — sub-samples and taps without history count as none, so a half-disoccluded pixel gets
 *     proportionally less —;  Wp == 0 or n' == 0: every plane of the pixel is 0;  else acc'_c = (float)((A_c / Wp) n'), S1'_c = (M1_c / Wp) n',
 *     S2' likewise, count' = n'.  The samplings behind the moments become the largest count written (no count exceeds them).  It reads a copy of
 *     the old planes that lives for the call (w x h x (12 + 4 + 48) bytes), synchronises, and puts its time into hr_stats.post_kernel_ms.
 *     HR_ERR_INVALID: no valid motion plane, "sample_counts" off, a tile mask set, max_history == 0, or a min_roughness or depth_tolerance that is
 *     not finite and >= 0.  HR_ERR_UNSUPPORTED: "robust_buckets" on (buckets are not carried).  What is refused touches nothing.  On success
 *     everything made of the accumulator, the moments or the counts is stale (D, R', S, the all-reduced total).
 *   - hr_reproject_params: max_history caps the count a pixel carries over — the weight of the past against the new frame's samplings —;
 *     min_roughness and depth_tolerance are hr_render_motion's (steps 2 and 4), and hr_reproject only checks them.  params = NULL: hr_reproject_default_params' (32, 0.3, 1e-3; it needs no device).  These are design parameters nobody has measured.
 *   - The caller's rule: a path's seed depends only on its pixel, sub-sample and sampling index.  A sequence must therefore give every frame fresh
 *     sampling indices — frame f renders samplings f S + 1 .. (f + 1) S —, or a still camera adds the history's own samples a second time.
 *   - What it is not: depth of field is ignored.  GGX above min_roughness is reused although it is mildly view-dependent.  Lighting on a reused diffuse point is
 *     view-independent only up to what it sees through glossy occluders: max_history is the limit on that.  A silhouette pixel of the old frame is
 *     a blend and hands the blend on: there is no per-tap validation.  Buckets are not carried.  Geometry does not move. */
typedef struct hr_reproject_params {
    uint32_t max_history;     /* > 0 */
    uint32_t _pad;
    double min_roughness;     /* >= 0 */
    double depth_tolerance;   /* >= 0 */
} hr_reproject_params;
int hr_set_camera(hr_ctx *ctx, const hr_camera *cam);
int hr_get_camera(hr_ctx *ctx, hr_camera *out);
int hr_render_motion(hr_ctx *ctx, const hr_camera *from, const hr_reproject_params *p /* NULL = defaults */);
int hr_read_motion(hr_ctx *ctx, float *host /* w*h*12 */);
int hr_write_motion(hr_ctx *ctx, const float *host);
int hr_reproject_default_params(hr_reproject_params *out);
int hr_reproject(hr_ctx *ctx, const hr_reproject_params *p /* NULL = defaults */);

int hr_get_stats(hr_ctx *ctx, hr_stats *out);
/* Options that leave the image as the reference computes it (the summation order of the accumulator aside):
 *   "counters"      0 / 1: instrumented build of the trace kernel (fills the counter fields of hr_stats)
 *   "batch"         samplings per launch, 1..64; 0 = automatic (about 33 M paths per launch: 4 at 1080p, up to 64 for small images)
 *   "trace_boost"   -1 = the two kernels are balanced from their own time stamps, on the device, launch by launch (default): five
 *                   levels from "the seed kernel's producer waves above the trace kernel" (0) over "alternating" (1) and "equal" (2)
 *                   to "the trace kernel's box phase (3) and leaf phase (4) above the producer waves" — and, where the trace kernel is
 *                   the faster kernel of the pair by a margin, how many of its persistent workgroups stay (its surplus waves only slow
 *                   the seed kernel beside it); 0 .. 4 = fixed level, every workgroup kept
 *                   (hr_stats.governor_level / governor_budget say where it stands)
 *   "max_tail_gib"  cap of each seed -> trace hand-off buffer, 1..128 GiB (default 20)
 *   "rng_window"    fixed: 64
 *   "precise_shading"  the GEOMETRY of every bounce in the reference's own f64: hit distance again from the f64 ray and the f64 primitive, hit
 *                   point, normal, mirror / Snell / Fresnel (material.rs:154-199) and the sampled lobe directions, FROM THE REFERENCE'S f64 DRAWS
 *                   (the seed kernel hands over what rounding a draw to fp32 took away as well: the hand-off record doubles); roughness maps are
 *                   read at f64 texture coordinates; the ray is carried as fp32 + residual, the walk stays fp32.  Same estimator, closer to the
 *                   reference: the paths that take the reference's branches and still differ by more than 1e-3 — refraction chains through
 *                   faceted glass, bounces off small spheres, GGX lobes driven by a roughness map — fall from 90 - 990 per million to 0 - 6
 *                   (BASELINE config 2: none in 10^6 paths, worst path 4e-5).  Two implementations that render the same bits:
 *                   in the megakernel at 128 VGPRs (2 - 4 % slower on scenes without meshes) and in the split pipeline's shading kernel
 *                   (7 - 30 % on mesh scenes); the library takes the faster one for the scene.
 *                   -1 (default) = automatic: ON for scenes without triangle meshes (BASELINE config 2: small spheres are what multiplies an
 *                   fp32 ray's error, and there it costs little), OFF for the others; 0 = off; 1 = on.  hr_stats.shading_in_force says
 *                   what runs.  (1 excludes "russian_roulette": whichever of the two is asked for second is refused with HR_ERR_UNSUPPORTED and
 *                   what was in force stays; -1 stands back when the roulette is on.)
 *   "moments"       0 (default) / 1: keep per-pixel first and second moments of the per-sampling values for hr_noise_estimate (see there);
 *                   the image does not change by a bit
 *   "sample_counts" 0 (default) / 1: keep per-pixel counts of the samplings received, for hr_set_tile_mask / hr_select_tiles /
 *                   hr_resolve_counted (see there); the image does not change by a bit
 *   "robust_buckets" 0 (default) / K in {3, 5, .., 15}: keep K sample buckets per pixel for hr_robust (see there; 3 K doubles per pixel); the
 *                   image does not change by a bit
 *   "bucket_by_sampling" 0 (default) / 1: with 1 sampling s goes into bucket (s - 1) mod K instead of the pixel's j-th into j mod K, so that the
 *                   buckets of contexts that shard the samplings add up (see hr_fold_statistics); the image does not change by a bit
 *   next hr_render_guides:
 *   "guide_bounces" 0 (default) .. 8, a whole number: how many mirrors and glass surfaces the guide rays follow to the first rough hit (see
 *                   "guide planes" above).  A new value drops the guide planes and the denoised image; the value it already has changes
 *                   nothing; anything else is HR_ERR_INVALID and changes nothing.  No rendered image depends on it.
 *   next hr_upload_scene:
 *   "bvh_builder"   -1 = by scene size (default): the host's binned-SAH build below 200,000 primitives (the best tree; one host thread,
 *                   < 1 s), the device PLOC build from there on (0.97 - 0.99 of that tree's quality; 4 x 10^6 triangles in 38 ms instead of
 *                   25 s); 0 = host build, 1 = LBVH, 2 = PLOC on the device — replaces bvh.rs:107-211 (hr_stats.bvh_builder_used)
 *   "max_leaf"      BVH leaf size, 1..15 (default 4)
 *   "split_ratio"   early split clipping of long thin triangles in the host builder: -1 = automatic (kept when it cuts the SAH
 *                   cost by more than 7 %, default), 0 = off, > 0 = always, with that box / triangle area ratio
 *   "quant_nodes"   1 = the trace kernel walks the 16-byte quantised node records (default), 0 = the 32-byte fp32 records of the
 *                   same tree.  Identical hits, bit for bit, for ray origins within about three scene extents of the scene by
 *                   construction (the quantised planes' margin covers the fp32 error of the box test) and, measured, on every
 *                   ray tried up to 1,000 extents; from 3,000 extents on a few rays per thousand whose hit fp32 no longer
 *                   resolves return another primitive (2 of 6,000 at 3,000 extents, 5 at 10,000, 49 at 100,000 on primitives
 *                   of 0.01 - 0.1 extents; none of 1,800 on primitives of 0.2 extents and more: profiles/trace_sweeps.txt)
 * One option that does NOT preserve the image (off by default; every parity test runs with it off):
 *   "russian_roulette"  0 = off.  k in 2..9: from path iteration k on a path survives with probability q = min(1, max(reflectance))
 *                   and its reflectance is divided by q.  The reference has no Russian roulette (renderer.rs:174-200 runs every
 *                   path to the bounce limit); the estimator stays unbiased (the decisions come from a hash of the path's
 *                   indices, not from its ISAAC-64 stream, whose draws the reference estimator has all spoken for); its noise
 *                   changes, it traces ~10 % fewer rays. */
int hr_set_option(hr_ctx *ctx, const char *key, double value);
/* The measurement knobs (hr_set_debug_option) and the unit-level entry points of the parity tests (hr_debug_*) live in
 * hanamaru_hip_debug.h: same library, but a product host — the Rust shell of INTEGRATION.md, the hanamaru-hip CLI — includes and binds
 * this header only (tests/test_abi.py checks that the CLI binary imports no hr_debug_* symbol). */

#ifdef __cplusplus
}
#endif
#endif
