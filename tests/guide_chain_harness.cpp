// Host form of the guide chain (csrc/pt_core.h: guide_chain_link) — TEST INFRASTRUCTURE ONLY, built by
// tests/test_guide_chain_cpu.py with g++ -ffp-contract=off and linked with flatten.cpp and bvh_build.cpp as tests/emu is.  The very functions
// guide_chain_kernel runs per lane, driven one sub-sample at a time with the scalar walk (trace_step); nothing in the product loads this.
#include <cstdint>
#include <cstdio>
#include <string>

#include "flatten.h"
#include "pt_core.h"

using namespace hr;

struct gc_scene { HostScene hs; Scene view; };

static RenderParams frame(uint32_t W, uint32_t H) {
    RenderParams rp{};
    rp.width = W; rp.height = H;
    return rp;
}
// One sub-sample's chain as guide_chain_kernel runs it per lane, with the scalar walk (one node + its leaf per step) in place of the wave's.
// info = {hits along the chain, element of the last hit or -1}
static void chain_sub(const Scene &sc, const RenderParams &rp, uint32_t px, uint32_t py, uint32_t sub, uint32_t bounces, float *g, int32_t *info) {
    Ray ray;
    debug_camera_ray(sc, rp, px, py, sub, ray);
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
// the kernel's sum of a pixel's four sub-samples: two lane exchanges, (s0 + s1) + (s2 + s3), then x 0.25f
static void pixel_mean(const float *sub, float *pix) {
    for (int k = 0; k < 8; k++) pix[k] = ((sub[k] + sub[8 + k]) + (sub[16 + k] + sub[24 + k])) * 0.25f;
}

extern "C" {

int gc_scene_create(const hr_scene_desc *sd, gc_scene **out) {
    gc_scene *e = new gc_scene;
    std::string err;
    int rc = flatten_scene(sd, e->hs, err);
    if (rc) { fprintf(stderr, "guide_chain_harness: %s\n", err.c_str()); delete e; return rc; }
    e->view = e->hs.view();
    *out = e;
    return 0;
}
void gc_scene_destroy(gc_scene *e) { delete e; }

// sub: h x w x 4 x 8 (per sub-sample), info: h x w x 4 x 2, pix: h x w x 8 (the planes)
void gc_chain(const gc_scene *e, uint32_t W, uint32_t H, uint32_t bounces, float *sub, int32_t *info, float *pix) {
    const RenderParams rp = frame(W, H);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            float *s = sub + ((size_t)y * W + x) * 32;
            for (uint32_t k = 0; k < 4; k++) chain_sub(e->view, rp, x, y, k, bounces, s + 8 * k, info + (((size_t)y * W + x) * 4 + k) * 2);
            pixel_mean(s, pix + ((size_t)y * W + x) * 8);
        }
}
// the same through guide_primary, what guide_render_kernel runs
void gc_primary(const gc_scene *e, uint32_t W, uint32_t H, float *sub, float *pix) {
    const RenderParams rp = frame(W, H);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            float *s = sub + ((size_t)y * W + x) * 32;
            for (uint32_t k = 0; k < 4; k++) {
                Ray ray;
                debug_camera_ray(e->view, rp, x, y, k, ray);
                TraceState ts;
                trace_begin(ts, T_INF);
                while (ts.cur != NODE_END) trace_step<false>(e->view, ray, ts, nullptr);
                guide_primary(e->view, ray, ts, s + 8 * k);
            }
            pixel_mean(s, pix + ((size_t)y * W + x) * 8);
        }
}

}
