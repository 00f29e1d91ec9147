// The point queries hr_debug_surface / hr_debug_sky / hr_debug_texture (hanamaru_hip_debug.h), one point per call: unpack the arguments, call the
// product's functions (pt_core.h, prec_core.h), pack what they return.  No arithmetic of their own.  __host__ __device__: the kernels of
// trace_kernel.h run them one point per lane, the host emulation (tests/emu) one point after the other.
#pragma once
#include "pt_core.h"

namespace hr {

static const int QUERY_SURFACE_FLOATS = 24;
// out[24] = {hit, t, pos xyz, n xyz, u, v, face, surface, param, albedo rgb, emission rgb, roughness, cur_refl, sampled, transmitted, 0}; a miss:
// {0, the search limit, zeros}, element -1.  face: cuboid_face_of(n) for a cuboid, -1 otherwise.
//   precise == 0: hit_surface (with the ray fix, or none) + material_at; slots 20 .. 23 are 0.
//   precise != 0: shade_hit_f64 with the fix and the draws; n = PrecHit::nf, u / v / element = PrecHit::s, the material PrecHit::m, pos = the fp32
//                 walk's o + t d (shade_hit_f64 keeps its f64 hit point to itself: it shows in out64 = {no xyz, nd xyz}).
HD void query_surface(const Scene &sc, const float *ray6, const float *fix6, const double *draws2, bool precise, float *o, double *o64, int32_t *elem) {
    Ray r;
    ray_set(r, v3(ray6[0], ray6[1], ray6[2]), v3(ray6[3], ray6[4], ray6[5]));
    TraceState ts;
    trace_begin(ts, T_INF);
    LaneCounters lc = {0, 0, 0, 0, 0, 0};
    while (ts.cur != NODE_END) trace_step<false>(sc, r, ts, &lc);
    for (int k = 0; k < QUERY_SURFACE_FLOATS; k++) o[k] = 0.0f;
    if (o64) for (int k = 0; k < 6; k++) o64[k] = 0.0;
    o[1] = ts.t;
    *elem = -1;
    if (ts.prim < 0) return;
    RayFix fix = no_ray_fix();
    if (fix6) { fix.o = v3(fix6[0], fix6[1], fix6[2]); fix.d = v3(fix6[3], fix6[4], fix6[5]); }
    o[0] = 1.0f;
    Surf s;
    PointMat m;
    if (!precise) {
        hit_surface(sc, r, ts, material_needs_uv(sc, hit_element(sc, ts)), s, fix);
        material_at(sc, s.elem, s.u, s.v, m);
    } else {
        PrecHit x;
        shade_hit_f64(sc, r.o, r.d, fix.o, fix.d, ts, draws2 ? draws2[0] : 0.5, draws2 ? draws2[1] : 0.5, x);
        s = x.s; s.n = x.nf; s.pos = r.o + r.d * ts.t;
        m = x.m;
        o[20] = x.sampled ? x.cur_refl : 0.0f; o[21] = x.sampled ? 1.0f : 0.0f; o[22] = x.transmitted ? 1.0f : 0.0f;
        if (o64) { o64[0] = x.no.x; o64[1] = x.no.y; o64[2] = x.no.z; o64[3] = x.nd.x; o64[4] = x.nd.y; o64[5] = x.nd.z; }
    }
    *elem = s.elem;
    o[2] = s.pos.x; o[3] = s.pos.y; o[4] = s.pos.z; o[5] = s.n.x; o[6] = s.n.y; o[7] = s.n.z; o[8] = s.u; o[9] = s.v;
    o[10] = ts.type == 2 ? (float)cuboid_face_of(s.n) : -1.0f;
    o[11] = (float)m.surface; o[12] = m.param;
    o[13] = m.albedo.x; o[14] = m.albedo.y; o[15] = m.albedo.z; o[16] = m.emission.x; o[17] = m.emission.y; o[18] = m.emission.z; o[19] = m.roughness;
}

// rgb = sky_sample in the form the scene has; where = {face + 8 when the lookup went through the footprint table (Scene::sky_quads), x1, y1}
HD void query_sky(const Scene &sc, const float *d3, float *rgb, uint32_t *where) {
    const V3f d = v3(d3[0], d3[1], d3[2]);
    const V3f c = sky_sample(sc, d);
    const SkyWhere sw = sky_where(sc, d);
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    where[0] = (uint32_t)sw.face + (sc.sky_quads ? 8u : 0u); where[1] = sw.x1; where[2] = sw.y1;
}

// rgb = sample_bilinear at the coordinates narrowed to fp32, rough64 = roughness_map_f64 at the f64 coordinates, quad[4] = the fp32 form's corner
// (ix1, iy1), then the f64 read's own
HD void query_texture(const Scene &sc, int32_t image, const double *uv, float *rgb, float *rough64, uint32_t *quad) {
    const float u = (float)uv[0], v = (float)uv[1];
    const V3f c = sample_bilinear(sc, image, u, v);
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    *rough64 = roughness_map_f64(sc, image, uv[0], uv[1], quad + 2);
    quad_corner(sc, image, u, v, quad[0], quad[1]);
}

}  // namespace hr
