// Temporal reuse: where a point was in an earlier camera's frame, and the gather of a frame's history along a motion plane.  All f64,
// host-compilable like denoise_core.h.  THIS HEADER IS THE DEFINITION: every operation is a single IEEE f64 operation in the order written
// (+ - x /, floor and comparisons only; no FMA — contraction is switched off below, a host compiler that contracts by default wants
// -ffp-contract=off), so the device, a host build and any restatement of these lines agree bit for bit.
//   reproject_project   the camera `from` as Camera::new builds it (camera.rs:45-64: right, up, forward orthogonal, plane_half_right along right,
//                       plane_half_up along up), which inverts camera.rs:98-107:
//                           v = (double)x - eye0 (a point), or (double)d (a direction: a point at infinity);  c = v . forward0;  c <= 0: behind
//                           k = c / focus0;   ncx = (v . phr0) / ((phr0 . phr0) k);   ncy = (v . phu0) / ((phu0 . phu0) k)
//                       every dot product is ((a0 b0 + a1 b1) + a2 b2)
//   reproject_motion    with m = min(W, H):  fx = (ncx m + W) / 2,  fy = (ncy m + H) / 2  (the fragment coordinates of renderer.rs:36,53-54 in `from`);
//                       the sub-sample's own gx = px + ox, gy = (H - py) + oy;  mx = fx - gx,  my = gy - fy  (pixels, y down);  a component with
//                       |.| < 2^-10 is 0 (a camera that did not move hands every pixel its own history exactly);  fx outside [-1, W + 1] or
//                       fy outside [-1, H + 1]: off the frame
//   reproject_pixel     one pixel of hr_reproject.  motion[4][3] = {mx, my, code} of its sub-samples in lane order; a sub-sample counts when its
//                       code is 0 and both components are finite with |.| <= 2^20 (so a written plane can never index out of range).  For those
//                           u = px + mx,  v = py + my;   x0 = floor(u),  y0 = floor(v);   ax = u - x0,  ay = v - y0
//                           taps (x0 + i, y0 + j), j outer, i inner;   w = (i ? ax : 1 - ax) (j ? ay : 1 - ay)
//                           a tap is skipped when w == 0, when it lies outside the region (asked in f64, before any index is formed), or when its
//                           old count n_q is 0;  else  Wp += w,  N += w n_q,  A_c += w (acc_q,c / n_q),  M1_c += w (S1_q,c / n_q),  M2_c likewise
//                       n' = min(max_history, floor(N / 4));   Wp == 0 or n' == 0: every plane of the pixel is 0;   else
//                           acc'_c = (float)((A_c / Wp) n'),  S1'_c = (M1_c / Wp) n',  S2'_c = (M2_c / Wp) n',  count' = n'
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HR_REPROJECT_HD __host__ __device__ __forceinline__
#else
#define HR_REPROJECT_HD inline
#endif

namespace hr {

constexpr double REPROJECT_SNAP = 0.0009765625;    // 2^-10 px: motion below it is stored as 0
constexpr double REPROJECT_MAX_MOTION = 1048576.0; // 2^20 px: a component beyond it makes the sub-sample invalid
// the code of a sub-sample of the motion plane: 0 may be reused; 1 behind or off the frame of `from`; 2 hidden from `from`; 3 view-dependent surface
enum { REPROJECT_OK = 0, REPROJECT_OFF_FRAME = 1, REPROJECT_OCCLUDED = 2, REPROJECT_VIEW_DEPENDENT = 3 };

// what reproject_project reads of the camera `from` (hr_camera's f64 values)
struct ReprojectCam { double eye[3], forward[3], phr[3], phu[3], focus; };

HR_REPROJECT_HD double reproject_dot(const double *a, const double *b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2];
    const double s = p0 + p1;
    return s + p2;
}

// x: the fp32 point, or with at_infinity the fp32 direction.  v[3]: the vector from eye0 (the direction).  false: behind `from` (c <= 0 or a NaN)
HR_REPROJECT_HD bool reproject_project(const ReprojectCam &from, const float *x, bool at_infinity, double *v, double &ncx, double &ncy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int k = 0; k < 3; k++) v[k] = at_infinity ? (double)x[k] : (double)x[k] - from.eye[k];
    const double c = reproject_dot(v, from.forward);
    ncx = 0.0; ncy = 0.0;
    if (!(c > 0.0)) return false;
    const double k = c / from.focus;
    const double rr = reproject_dot(from.phr, from.phr), uu = reproject_dot(from.phu, from.phu);
    const double dr = rr * k, du = uu * k;
    ncx = reproject_dot(v, from.phr) / dr;
    ncy = reproject_dot(v, from.phu) / du;
    return true;
}

// (px, py): the FRAME pixel; (ox, oy): the sub-sample's offset (renderer.rs:53: -0.5 or 0).  false: off the frame of `from` (or a NaN)
HR_REPROJECT_HD bool reproject_motion(double ncx, double ncy, uint32_t W, uint32_t H, uint32_t px, uint32_t py, double ox, double oy, double &mx, double &my) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double w = (double)W, h = (double)H, m = w < h ? w : h;
    const double fx = (ncx * m + w) / 2.0, fy = (ncy * m + h) / 2.0;
    const double gx = (double)px + ox, gy = (h - (double)py) + oy;
    mx = fx - gx; my = gy - fy;
    if (mx < REPROJECT_SNAP && mx > -REPROJECT_SNAP) mx = 0.0;
    if (my < REPROJECT_SNAP && my > -REPROJECT_SNAP) my = 0.0;
    return fx >= -1.0 && fx <= w + 1.0 && fy >= -1.0 && fy <= h + 1.0;
}

// One pixel (px, py) of the w x h region.  acc (3 floats per pixel), counts, mom (6 doubles per pixel, or nullptr: option "moments" off) are the OLD
// planes; out_mom may be nullptr with mom.  Returns the count written.
HR_REPROJECT_HD uint32_t reproject_pixel(const float *motion, const float *acc, const uint32_t *counts, const double *mom, uint32_t w, uint32_t h, uint32_t px, uint32_t py,
                                         uint32_t max_history, float *out_acc, double *out_mom) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double wd = (double)w, hd = (double)h;
    double Wp = 0.0, N = 0.0, A[3] = {0.0, 0.0, 0.0}, M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < 4; s++) {
        const float fmx = motion[s * 3], fmy = motion[s * 3 + 1], code = motion[s * 3 + 2];
        if (!(code == 0.0f)) continue;
        const double mx = (double)fmx, my = (double)fmy;
        if (!(mx >= -REPROJECT_MAX_MOTION && mx <= REPROJECT_MAX_MOTION && my >= -REPROJECT_MAX_MOTION && my <= REPROJECT_MAX_MOTION)) continue;   // (a NaN fails too)
        const double u = (double)px + mx, v = (double)py + my;
        const double x0 = floor(u), y0 = floor(v);
        const double ax = u - x0, ay = v - y0;
        for (int j = 0; j < 2; j++) {
            const double ty = y0 + (double)j, wy = j ? ay : 1.0 - ay;
            for (int i = 0; i < 2; i++) {
                const double tx = x0 + (double)i, wx = i ? ax : 1.0 - ax;
                const double wt = wx * wy;
                if (wt == 0.0) continue;
                if (!(tx >= 0.0 && tx < wd && ty >= 0.0 && ty < hd)) continue;
                const size_t q = (size_t)(uint32_t)ty * w + (uint32_t)tx;
                const uint32_t nq = counts[q];
                if (nq == 0u) continue;
                const double nd = (double)nq;
                Wp = Wp + wt;
                N = N + wt * nd;
                for (int c = 0; c < 3; c++) {
                    const double mean = (double)acc[q * 3 + c] / nd;
                    A[c] = A[c] + wt * mean;
                }
                if (mom)
                    for (int c = 0; c < 6; c++) {
                        const double mean = mom[q * 6 + c] / nd;
                        M[c] = M[c] + wt * mean;
                    }
            }
        }
    }
    const double quarter = floor(N / 4.0), cap = (double)max_history;
    const double nn = quarter < cap ? quarter : cap;
    const bool none = !(Wp > 0.0) || !(nn >= 1.0);
    const uint32_t n_new = none ? 0u : (uint32_t)nn;
    for (int c = 0; c < 3; c++) out_acc[c] = none ? 0.0f : (float)((A[c] / Wp) * nn);
    if (out_mom)
        for (int c = 0; c < 6; c++) out_mom[c] = none ? 0.0 : (M[c] / Wp) * nn;
    return n_new;
}

}  // namespace hr
