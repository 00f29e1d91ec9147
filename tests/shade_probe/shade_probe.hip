// Shading-function probe — TEST INFRASTRUCTURE ONLY (tests/shade_sweeps.py, tests/test_shade_functions_*.py).
//
// The material functions of csrc/pt_core.h, the f64 forms of precise shading (csrc/prec_core.h) and the tone-map curve of csrc/post_core.h, each
// asked one point at a time with explicit arguments — no Scene —, so that the tests can put the same question to the f64 oracle.
// One source, two builds:
//   * hipcc, the product Makefile's HIPFLAGS (target `shade_probe` of hanamaru-renderer_amd/Makefile): one kernel per entry, one thread per point;
//     the C entry allocates, copies in, launches, copies back and returns the HIP error code (0 = ok) — it never aborts;
//   * g++ -x c++ with the flags of tests/emu: the same per-point function in a loop (libm where the device has v_rcp / v_rsq / v_sin / v_exp).
// The per-point functions below only unpack arguments and call the product's function: there is no arithmetic of the probe's own.
//
// LIMIT: this is the product's source and flags inside ANOTHER kernel.  FMA contraction and instruction scheduling are decided per kernel, so a
// value here may differ from the trace kernel's by an ulp; the whole-path tests (hr_debug_path_log against the oracle's path log) remain the check
// on the kernel itself.  Nothing in hanamaru-renderer_amd/ loads this library.
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <vector>
#endif

#include "pt_core.h"
#include "post_core.h"

using namespace hr;

// ---------------------------------------------------------------------------------------------
// per-point functions
struct EvalArgs { const int32_t *surface; const float *param, *roughness, *view, *n, *light; float *out; };
HD void point_bsdf_eval(const EvalArgs &a, size_t i) {
    a.out[i] = bsdf_eval(a.surface[i], a.param[i], a.roughness[i], v3(a.view + 3 * i), v3(a.n + 3 * i), v3(a.light + 3 * i));
}

struct SampleArgs { const int32_t *surface; const float *param, *roughness, *r0, *r1, *pos, *view, *n; int32_t *some, *transmitted; float *origin, *dir, *refl; };
HD void point_bsdf_sample(const SampleArgs &a, size_t i) {
    PointMat m;
    m.surface = a.surface[i]; m.param = a.param[i]; m.roughness = a.roughness[i];
    m.albedo = v3(1, 1, 1); m.emission = v3(0, 0, 0);
    V3f no = v3(0, 0, 0), nd = v3(0, 0, 0);
    float refl = 0.0f;
    bool transmitted = false;
    const bool some = bsdf_sample(m, a.r0[i], a.r1[i], v3(a.pos + 3 * i), v3(a.view + 3 * i), v3(a.n + 3 * i), no, nd, refl, transmitted);
    a.some[i] = some ? 1 : 0; a.transmitted[i] = transmitted ? 1 : 0;
    a.origin[3 * i] = no.x; a.origin[3 * i + 1] = no.y; a.origin[3 * i + 2] = no.z;
    a.dir[3 * i] = nd.x; a.dir[3 * i + 1] = nd.y; a.dir[3 * i + 2] = nd.z;
    a.refl[i] = refl;
}

struct SincosArgs { const double *r; double *sn, *cs; };
HD void point_sincos_f64(const SincosArgs &a, size_t i) { sincos_2pi_f64(a.r[i], a.sn[i], a.cs[i]); }

struct LobeArgs { const double *r0, *r1, *n, *alpha2; double *out; };
HD void store3(double *p, D3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
HD D3 load3(const double *p) { return dv(p[0], p[1], p[2]); }
HD void point_diffuse_f64(const LobeArgs &a, size_t i) { store3(a.out + 3 * i, sample_diffuse_f64(a.r0[i], a.r1[i], load3(a.n + 3 * i))); }
HD void point_ggx_half_f64(const LobeArgs &a, size_t i) { store3(a.out + 3 * i, sample_ggx_half_f64(a.r0[i], a.r1[i], load3(a.n + 3 * i), a.alpha2[i])); }

struct RefractArgs { const double *r0, *pos, *in, *n, *ior; int32_t *transmitted; double *origin, *dir; float *refl; };
HD void point_refraction_f64(const RefractArgs &a, size_t i) {
    D3 no = dv(0, 0, 0), nd = dv(0, 0, 0);
    float refl = 0.0f;
    bool transmitted = false;
    sample_refraction_f64(a.r0[i], load3(a.pos + 3 * i), load3(a.in + 3 * i), load3(a.n + 3 * i), a.ior[i], no, nd, refl, transmitted);
    a.transmitted[i] = transmitted ? 1 : 0;
    store3(a.origin + 3 * i, no); store3(a.dir + 3 * i, nd);
    a.refl[i] = refl;
}

struct GgxReflArgs { const double *ln, *vn, *vh, *hn; const float *alpha2, *f0; double *out; };
HD void point_ggx_refl_f64(const GgxReflArgs &a, size_t i) { a.out[i] = ggx_refl_f64(a.ln[i], a.vn[i], a.vh[i], a.hn[i], a.alpha2[i], a.f0[i]); }

struct TonemapArgs { const float *rgb, *scale; float *out; };
HD void point_tonemap_gamma(const TonemapArgs &a, size_t i) { tonemap_gamma(a.rgb[3 * i], a.rgb[3 * i + 1], a.rgb[3 * i + 2], a.scale[i], a.out + 3 * i); }

struct GammaArgs { const float *v; float *out; };
HD void point_gamma_to_linear(const GammaArgs &a, size_t i) { a.out[i] = gamma_to_linear(a.v[i]); }

// ---------------------------------------------------------------------------------------------
// the two ways to run a per-point function over n points
#if defined(__HIPCC__)
template <class A, void (*F)(const A &, size_t)>
__global__ void __launch_bounds__(256) probe_kernel(A a, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    F(a, i);
}
// device copies of an entry's arrays; the first HIP error sticks and every later step is skipped
struct Bufs {
    struct Out { void *host, *dev; size_t bytes; };
    std::vector<void *> owned;
    std::vector<Out> outs;
    hipError_t err = hipSuccess;
    void *alloc(size_t bytes) {
        void *d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, bytes ? bytes : 1);
        if (err == hipSuccess) owned.push_back(d); else d = nullptr;
        return d;
    }
    template <class T> const T *in(const T *h, size_t count) {
        void *d = alloc(count * sizeof(T));
        if (err == hipSuccess) err = hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice);
        return (const T *)d;
    }
    template <class T> T *out(T *h, size_t count) {
        void *d = alloc(count * sizeof(T));
        if (err == hipSuccess) err = hipMemset(d, 0, count * sizeof(T));
        if (err == hipSuccess) outs.push_back(Out{h, d, count * sizeof(T)});
        return (T *)d;
    }
    template <class A, void (*F)(const A &, size_t)> int run(const A &a, size_t n) {
        if (err == hipSuccess && n > 0) {
            probe_kernel<A, F><<<dim3((unsigned)((n + 255u) / 256u)), dim3(256)>>>(a, n);
            err = hipGetLastError();
            if (err == hipSuccess) err = hipDeviceSynchronize();
        }
        for (const Out &o : outs)
            if (err == hipSuccess) err = hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost);
        for (void *d : owned) (void)hipFree(d);
        return (int)err;
    }
};
#else
struct Bufs {
    template <class T> const T *in(const T *h, size_t) { return h; }
    template <class T> T *out(T *h, size_t) { return h; }
    template <class A, void (*F)(const A &, size_t)> int run(const A &a, size_t n) {
        for (size_t i = 0; i < n; i++) F(a, i);
        return 0;
    }
};
#endif

// ---------------------------------------------------------------------------------------------
// C entries: host arrays in, host arrays out, return 0 or the HIP error code.  Vectors are n x 3, tightly packed.
extern "C" {

int sp_is_device_build(void) {
#if defined(__HIPCC__)
    return 1;
#else
    return 0;
#endif
}

int sp_bsdf_eval(size_t n, const int32_t *surface, const float *param, const float *roughness, const float *view, const float *nrm, const float *light, float *out) {
    Bufs b;
    const EvalArgs a = {b.in(surface, n), b.in(param, n), b.in(roughness, n), b.in(view, 3 * n), b.in(nrm, 3 * n), b.in(light, 3 * n), b.out(out, n)};
    return b.run<EvalArgs, point_bsdf_eval>(a, n);
}

int sp_bsdf_sample(size_t n, const int32_t *surface, const float *param, const float *roughness, const float *r0, const float *r1, const float *pos,
                   const float *view, const float *nrm, int32_t *some, int32_t *transmitted, float *origin, float *dir, float *refl) {
    Bufs b;
    const SampleArgs a = {b.in(surface, n), b.in(param, n), b.in(roughness, n), b.in(r0, n), b.in(r1, n), b.in(pos, 3 * n), b.in(view, 3 * n), b.in(nrm, 3 * n),
                          b.out(some, n), b.out(transmitted, n), b.out(origin, 3 * n), b.out(dir, 3 * n), b.out(refl, n)};
    return b.run<SampleArgs, point_bsdf_sample>(a, n);
}

int sp_sincos_2pi_f64(size_t n, const double *r, double *sn, double *cs) {
    Bufs b;
    const SincosArgs a = {b.in(r, n), b.out(sn, n), b.out(cs, n)};
    return b.run<SincosArgs, point_sincos_f64>(a, n);
}

int sp_sample_diffuse_f64(size_t n, const double *r0, const double *r1, const double *nrm, double *out) {
    Bufs b;
    const LobeArgs a = {b.in(r0, n), b.in(r1, n), b.in(nrm, 3 * n), b.in(r0, n), b.out(out, 3 * n)};   // (alpha2: unused by this entry)
    return b.run<LobeArgs, point_diffuse_f64>(a, n);
}

int sp_sample_ggx_half_f64(size_t n, const double *r0, const double *r1, const double *nrm, const double *alpha2, double *out) {
    Bufs b;
    const LobeArgs a = {b.in(r0, n), b.in(r1, n), b.in(nrm, 3 * n), b.in(alpha2, n), b.out(out, 3 * n)};
    return b.run<LobeArgs, point_ggx_half_f64>(a, n);
}

int sp_sample_refraction_f64(size_t n, const double *r0, const double *pos, const double *in, const double *nrm, const double *ior, int32_t *transmitted,
                             double *origin, double *dir, float *refl) {
    Bufs b;
    const RefractArgs a = {b.in(r0, n), b.in(pos, 3 * n), b.in(in, 3 * n), b.in(nrm, 3 * n), b.in(ior, n), b.out(transmitted, n), b.out(origin, 3 * n),
                           b.out(dir, 3 * n), b.out(refl, n)};
    return b.run<RefractArgs, point_refraction_f64>(a, n);
}

int sp_ggx_refl_f64(size_t n, const double *ln, const double *vn, const double *vh, const double *hn, const float *alpha2, const float *f0, double *out) {
    Bufs b;
    const GgxReflArgs a = {b.in(ln, n), b.in(vn, n), b.in(vh, n), b.in(hn, n), b.in(alpha2, n), b.in(f0, n), b.out(out, n)};
    return b.run<GgxReflArgs, point_ggx_refl_f64>(a, n);
}

int sp_tonemap_gamma(size_t n, const float *rgb, const float *scale, float *out) {
    Bufs b;
    const TonemapArgs a = {b.in(rgb, 3 * n), b.in(scale, n), b.out(out, 3 * n)};
    return b.run<TonemapArgs, point_tonemap_gamma>(a, n);
}

int sp_gamma_to_linear(size_t n, const float *v, float *out) {
    Bufs b;
    const GammaArgs a = {b.in(v, n), b.out(out, n)};
    return b.run<GammaArgs, point_gamma_to_linear>(a, n);
}

}  // extern "C"
