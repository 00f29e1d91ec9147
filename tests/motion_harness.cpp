// Host form of the motion plane (csrc/pt_core.h: motion_point, motion_verdict; hr_render_motion) — TEST INFRASTRUCTURE ONLY, built by
// tests/reproject_cores.py with g++ -ffp-contract=off and linked with flatten.cpp and bvh_build.cpp as tests/guide_lens_harness.cpp is.  The very
// functions motion_kernel runs per lane, driven one sub-sample at a time with the scalar walk (trace_step); nothing in the product loads this.
#include <cstdint>
#include <cstdio>
#include <string>

#include "flatten.h"
#include "pt_core.h"

using namespace hr;

struct mh_scene { HostScene hs; Scene view; };

static void walk(const Scene &sc, const Ray &ray, TraceState &ts) {
    trace_begin(ts, T_INF);
    while (ts.cur != NODE_END) trace_step<false>(sc, ray, ts, nullptr);
}

extern "C" {

int mh_scene_create(const hr_scene_desc *sd, mh_scene **out) {
    mh_scene *e = new mh_scene;
    std::string err;
    int rc = flatten_scene(sd, e->hs, err);
    if (rc) { fprintf(stderr, "motion_harness: %s\n", err.c_str()); delete e; return rc; }
    e->view = e->hs.view();
    *out = e;
    return 0;
}
void mh_scene_destroy(mh_scene *e) { delete e; }

// The plane of hr_render_motion(from) over the window (x0, y0, w, h) of the W x H frame, with the scene's own camera: motion h x w x 4 x 3.
// elem: h x w x 4, the element the primary ray hits or -1 (may be null).  from: hr_camera.
int mh_motion(const mh_scene *e, const hr_camera *from, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, double min_roughness, double depth_tolerance,
              float *motion, int32_t *elem) {
    CameraF camf;
    CameraD camd;
    std::string err;
    int rc = flatten_camera(*from, camf, camd, err);
    if (rc) return rc;
    ReprojectCam rc0;
    for (int k = 0; k < 3; k++) { rc0.eye[k] = camd.eye[k]; rc0.forward[k] = camd.forward[k]; rc0.phr[k] = camd.phr[k]; rc0.phu[k] = camd.phu[k]; }
    rc0.focus = camd.focus_distance;
    RenderParams rp{};
    rp.width = W; rp.height = H;
    const Scene &sc = e->view;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++)
            for (uint32_t sub = 0; sub < 4; sub++) {
                const size_t at = ((size_t)y * w + x) * 4 + sub;
                Ray ray, second;
                debug_camera_ray(sc, rp, x0 + x, y0 + y, sub, ray);
                TraceState ts;
                walk(sc, ray, ts);
                if (elem) elem[at] = ts.prim >= 0 ? hit_element(sc, ts) : -1;
                float *out = motion + at * 3, len;
                second = ray;
                if (motion_point(sc, rp, rc0, (float)min_roughness, ray, ts, x0 + x, y0 + y, sub, out, second, len)) {
                    TraceState ts2;
                    walk(sc, second, ts2);
                    motion_verdict(ts2, len, (float)depth_tolerance, out);
                }
            }
    return 0;
}

}
