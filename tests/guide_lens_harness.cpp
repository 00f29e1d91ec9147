// Host form of the lens-sampled guide planes (csrc/pt_core.h: guide_lens_point, guide_lens_ray, guide_chain_link; hr_render_guides_lens) — TEST
// INFRASTRUCTURE ONLY, built by tests/guide_lens.py with g++ -ffp-contract=off and linked with flatten.cpp and bvh_build.cpp as
// tests/guide_chain_harness.cpp is.  The very functions guide_lens_kernel runs per lane, driven one (sub-sample, lens point) at a time with the
// scalar walk (trace_step), summed in the kernel's order; nothing in the product loads this.
#include <cstdint>
#include <cstdio>
#include <string>

#include "flatten.h"
#include "pt_core.h"

using namespace hr;

struct gl_scene { HostScene hs; Scene view; };

static RenderParams frame(uint32_t W, uint32_t H) {
    RenderParams rp{};
    rp.width = W; rp.height = H;
    return rp;
}
// One ray's chain as guide_lens_kernel runs it per lane and lens point, with the scalar walk in place of the wave's.
// info = {hits along the chain, element of the last hit or -1}
static void chain_ray(const Scene &sc, Ray ray, uint32_t bounces, float *g, int32_t *info) {
    GuideChain gc;
    guide_chain_begin(gc, g);
    info[0] = 0; info[1] = -1;
    for (uint32_t j = 0;; j++) {
        TraceState ts;
        trace_begin(ts, T_INF);
        while (ts.cur != NODE_END) trace_step<false>(sc, ray, ts, nullptr);
        if (ts.prim >= 0) { info[0]++; info[1] = hit_element(sc, ts); }
        if (!guide_chain_link(sc, ray, ts, j >= bounces, gc, g)) return;
    }
}

extern "C" {

int gl_scene_create(const hr_scene_desc *sd, gl_scene **out) {
    gl_scene *e = new gl_scene;
    std::string err;
    int rc = flatten_scene(sd, e->hs, err);
    if (rc) { fprintf(stderr, "guide_lens_harness: %s\n", err.c_str()); delete e; return rc; }
    e->view = e->hs.view();
    *out = e;
    return 0;
}
void gl_scene_destroy(gl_scene *e) { delete e; }

// guide_lens_point as the kernel calls it: uv = {u, v} of point i of L
void gl_point(int lens_shape, uint32_t L, uint32_t i, float *uv) { guide_lens_point(lens_shape, L, i, uv[0], uv[1]); }

// guide_lens_ray through the points uv[n][2] (any points, the table's or not): org, dir: h x w x 4 x n x 3
void gl_rays(const gl_scene *e, uint32_t W, uint32_t H, uint32_t n, const float *uv, float *org, float *dir) {
    const RenderParams rp = frame(W, H);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++)
            for (uint32_t k = 0; k < 4; k++)
                for (uint32_t l = 0; l < n; l++) {
                    Ray ray;
                    guide_lens_ray(e->view, rp, x, y, k, uv[2 * l], uv[2 * l + 1], ray);
                    const size_t at = ((((size_t)y * W + x) * 4 + k) * n + l) * 3;
                    org[at] = ray.o.x; org[at + 1] = ray.o.y; org[at + 2] = ray.o.z;
                    dir[at] = ray.d.x; dir[at + 1] = ray.d.y; dir[at + 2] = ray.d.z;
                }
}
// debug_camera_ray: org, dir: h x w x 4 x 3
void gl_pinhole_rays(const gl_scene *e, uint32_t W, uint32_t H, float *org, float *dir) {
    const RenderParams rp = frame(W, H);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++)
            for (uint32_t k = 0; k < 4; k++) {
                Ray ray;
                debug_camera_ray(e->view, rp, x, y, k, ray);
                const size_t at = (((size_t)y * W + x) * 4 + k) * 3;
                org[at] = ray.o.x; org[at + 1] = ray.o.y; org[at + 2] = ray.o.z;
                dir[at] = ray.d.x; dir[at + 1] = ray.d.y; dir[at + 2] = ray.d.z;
            }
}
// The planes of hr_render_guides_lens(L) with guide_bounces = bounces over the window (x0, y0, w, h) of the W x H frame; step > 1: at the w x h
// frame pixels (x0 + i step, y0 + j step) only (tools/guide_lens_quality.py looks for its windows on such a grid).
// ray: h x w x 4 x L x 8 (per sub-sample and lens point), info: h x w x 4 x L x 2 — either may be null —, pix: h x w x 8 (the planes): per
// sub-sample the fp32 sum over l = 0 .. L - 1 in order, then (s0 + s1) + (s2 + s3), then x 0.25f / L.  L = 1 is the camera without an aperture's one
// lens point: debug_camera_ray, the planes of hr_render_guides.
void gl_lens_window(const gl_scene *e, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t step, uint32_t bounces, uint32_t L, float *ray, int32_t *info,
                    float *pix) {
    const RenderParams rp = frame(W, H);
    const int shape = e->view.cam.lens_shape;
    const float scale = 0.25f / (float)L;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            const size_t p = (size_t)y * w + x;
            float sub[4][8];
            for (uint32_t k = 0; k < 4; k++) {
                for (int c = 0; c < 8; c++) sub[k][c] = 0.0f;
                for (uint32_t l = 0; l < L; l++) {
                    float u, v, g[8];
                    int32_t inf[2];
                    Ray r;
                    if (L == 1) debug_camera_ray(e->view, rp, x0 + x * step, y0 + y * step, k, r);
                    else {
                        guide_lens_point(shape, L, l, u, v);
                        guide_lens_ray(e->view, rp, x0 + x * step, y0 + y * step, k, u, v, r);
                    }
                    chain_ray(e->view, r, bounces, g, inf);
                    for (int c = 0; c < 8; c++) sub[k][c] += g[c];
                    const size_t at = (p * 4 + k) * L + l;
                    if (ray) for (int c = 0; c < 8; c++) ray[at * 8 + c] = g[c];
                    if (info) { info[at * 2] = inf[0]; info[at * 2 + 1] = inf[1]; }
                }
            }
            for (int c = 0; c < 8; c++) pix[p * 8 + c] = ((sub[0][c] + sub[1][c]) + (sub[2][c] + sub[3][c])) * scale;
        }
}

}
