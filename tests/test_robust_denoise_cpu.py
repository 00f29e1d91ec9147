"""The robust denoiser on the CPU tier: robust_pixel_cv_k / robust_pixel_k / robust_denoise_image of csrc/robust_core.h compiled
for the host against an independent numpy restatement of their definition — bit for bit: + - x /, comparisons and one truncation in f64 without
contraction, no sqrt —, their corner cases, their consistency with hr_robust's and the robust noise estimate's definitions, the quality figure on
the checker's per-sampling renders, and the entry point declared, exported and bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guide_chain as gc
import test_denoise_cpu as dn
from cli import run_cli
from test_robust_cpu import bits, fill_buckets, heavy_tailed, numpy_robust, rel_sq_error
from test_robust_noise_cpu import numpy_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_K = (3, 5, 7, 9, 11, 13, 15)
EPS, TINY = 1e-3, 1e-30

HARNESS = r'''
#include <vector>
#include "robust_core.h"
using namespace hr;
// counts may be null (every pixel: n_all)
extern "C" void robust_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, uint64_t pixels, float *R, uint8_t *trim) {
    robust_image(buckets, counts, n_all, K, (size_t)pixels, R, trim);
}
extern "C" void robust_error_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, double floor, uint64_t pixels, double *e, uint8_t *trim) {
    robust_error_image(buckets, counts, n_all, K, floor, (size_t)pixels, e, trim);
}
template <uint32_t K>
static void robust_k_image(const double *buckets, const uint32_t *counts, uint64_t n_all, size_t pixels, float *R, uint8_t *trim) {
    for (size_t p = 0; p < pixels; p++) robust_pixel_k<K>(buckets + p * K * 3, counts ? (uint64_t)counts[p] : n_all, R + p * 3, trim + p);
}
extern "C" int robust_k_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, uint64_t pixels, float *R, uint8_t *trim) {
    switch (K) {
    case 3: robust_k_image<3>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 5: robust_k_image<5>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 7: robust_k_image<7>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 9: robust_k_image<9>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 11: robust_k_image<11>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 13: robust_k_image<13>(buckets, counts, n_all, pixels, R, trim); return 0;
    case 15: robust_k_image<15>(buckets, counts, n_all, pixels, R, trim); return 0;
    }
    return 1;
}
extern "C" void robust_cv_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, uint64_t pixels, double *cv, uint8_t *trim) {
    for (size_t p = 0; p < pixels; p++) robust_pixel_cv(buckets + p * K * 3, K, counts ? (uint64_t)counts[p] : n_all, cv + p * 6, trim + p);
}
// sig = {sigma_color, sigma_normal, sigma_albedo, sigma_depth}; state (may be null): the last level's {C, V} of every pixel, w*h*6 doubles
extern "C" void robust_denoise_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, const float *guides, uint32_t w, uint32_t h, uint32_t levels,
                                   int demodulate, const double *sig, float *d, double *state) {
    std::vector<double> work((size_t)w * h * 12);
    const int dem = demodulate && levels ? 1 : 0;
    robust_denoise_image(buckets, counts, n_all, K, guides, w, h, levels, dem, denoise_sigmas(sig[0], sig[1], sig[2], sig[3]), work.data(), d);
    if (state) for (size_t i = 0; i < (size_t)w * h * 6; i++) state[i] = work[(levels & 1u ? (size_t)w * h * 6 : 0) + i];
}
'''


def build_core(directory):
    src, so = directory / "robust_denoise_harness.cpp", directory / "librobust_denoise_harness.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "hanamaru-renderer_amd", "csrc"), "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    image = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.robust_run.argtypes = image
    lib.robust_k_run.argtypes = image
    lib.robust_cv_run.argtypes = image
    lib.robust_error_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.robust_denoise_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return build_core(tmp_path_factory.mktemp("robust_denoise"))


def _image_args(buckets, n):
    b = np.ascontiguousarray(buckets, dtype=np.float64)
    K, shape = b.shape[-2], b.shape[:-2]
    assert b.shape[-1] == 3
    counts = None if np.isscalar(n) else np.ascontiguousarray(n, dtype=np.uint32)
    assert counts is None or counts.shape == shape
    return b, K, shape, counts, (counts.ctypes.data if counts is not None else None), (int(n) if counts is None else 0)


def core_cv(lib, buckets, n):
    """robust_pixel_cv over buckets (.., K, 3); n: one count or per-pixel counts, every one >= K.  Returns (cv float64 (.., 6), trim uint8 (..))."""
    b, K, shape, counts, cp, n_all = _image_args(buckets, n)
    cv, trim = np.zeros(shape + (6,)), np.zeros(shape, dtype=np.uint8)
    lib.robust_cv_run(b.ctypes.data, cp, n_all, K, int(np.prod(shape, dtype=np.int64)), cv.ctypes.data, trim.ctypes.data)
    return cv, trim


def core_r(lib, buckets, n, templated=False):
    """robust_pixel (the run-time K definition) or robust_pixel_k<K>: (R float32 (.., 3), trim uint8 (..))."""
    b, K, shape, counts, cp, n_all = _image_args(buckets, n)
    R, trim = np.zeros(shape + (3,), dtype=np.float32), np.zeros(shape, dtype=np.uint8)
    if templated:
        assert lib.robust_k_run(b.ctypes.data, cp, n_all, K, int(np.prod(shape, dtype=np.int64)), R.ctypes.data, trim.ctypes.data) == 0
    else:
        lib.robust_run(b.ctypes.data, cp, n_all, K, int(np.prod(shape, dtype=np.int64)), R.ctypes.data, trim.ctypes.data)
    return R, trim


def core_e(lib, buckets, n, floor):
    b, K, shape, counts, cp, n_all = _image_args(buckets, n)
    e, trim = np.zeros(shape), np.zeros(shape, dtype=np.uint8)
    lib.robust_error_run(b.ctypes.data, cp, n_all, K, float(floor), int(np.prod(shape, dtype=np.int64)), e.ctypes.data, trim.ctypes.data)
    return e, trim


def core_filter(lib, buckets, n, guides, want_state=False, **over):
    """robust_denoise_image over an (h, w, K, 3) image of buckets with the rule of hr_denoise_robust: demodulate only with levels > 0."""
    params = dict(dn.DEFAULTS, **over)
    b, K, shape, counts, cp, n_all = _image_args(buckets, n)
    h, w = shape
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    assert guides.shape == (h, w, 8)
    d = np.zeros((h, w, 3), dtype=np.float32)
    state = np.zeros((h, w, 6)) if want_state else None
    sig = dn._sig(params)
    lib.robust_denoise_run(b.ctypes.data, cp, n_all, K, guides.ctypes.data, w, h, int(params["levels"]), int(params["demodulate"]), sig.ctypes.data,
                           d.ctypes.data, state.ctypes.data if want_state else None)
    return (d, state) if want_state else d


def numpy_cv(buckets, n):
    """The definition in the comment of robust_pixel_cv_k, restated on whole arrays: every line one IEEE f64 operation per element, every sum
    sequential from its first term.  Returns (cv (.., 6), trim)."""
    B = np.asarray(buckets, dtype=np.float64)
    K, shape = B.shape[-2], B.shape[:-2]
    B = B.reshape(-1, K, 3)
    P = B.shape[0]
    n = np.broadcast_to(np.asarray(n, dtype=np.uint64).reshape(-1), (P,))
    assert (n >= K).all()
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        nb = (n[:, None] - np.arange(K, dtype=np.uint64)[None, :] + np.uint64(K - 1)) // np.uint64(K)
        m = B / nb.astype(np.float64)[..., None] / 4.0
        y = (m[..., 0] + m[..., 1]) + m[..., 2]
        order = np.argsort(y, axis=1, kind="stable")                                  # ascending by (y, b)
        ys = np.take_along_axis(y, order, 1)
        ms = np.take_along_axis(m, order[..., None], 1)
        T = ys[:, 0].copy()
        Gn = float(1 - K) * ys[:, 0]
        for i in range(2, K + 1):
            T = T + ys[:, i - 1]
            Gn = Gn + float(2 * i - K - 1) * ys[:, i - 1]
        G = Gn / (float(K) * T)
        want = np.trunc(np.where((T > 0.0) & (G > 0.0), G * float(K) / 2.0, 0.0)).astype(np.int64)
        trim = np.minimum((K - 1) // 2, want)
        cv = np.zeros((P, 6))
        for t in range((K - 1) // 2 + 1):
            kept = float(K - 2 * t)
            s = ms[:, t, :].copy()
            for i in range(t + 1, K - t):
                s = s + ms[:, i, :]
            Cc = s / kept
            lo, hi = ms[:, t, :], ms[:, K - 1 - t, :]
            w = [lo if i < t else (hi if i >= K - t else ms[:, i, :]) for i in range(K)]
            ws = w[0].copy()
            for i in range(1, K):
                ws = ws + w[i]
            wbar = ws / float(K)
            ss = (w[0] - wbar) * (w[0] - wbar)
            for i in range(1, K):
                d = w[i] - wbar
                ss = ss + d * d
            f = float(K) / kept
            V = ss / float(K - 1) / float(K) * f * f
            cv = np.where((trim == t)[:, None], np.concatenate([Cc, V], axis=1), cv)
    return cv.reshape(shape + (6,)), trim.astype(np.uint8).reshape(shape)


def numpy_filter(cv, guides, want_state=False, **over):
    """denoise_core.h's demodulation, levels and final pass (restated as tests/test_denoise_cpu.py numpy_denoise does) on an initial
    state cv (h, w, 6) = {C, V}."""
    p = dict(dn.DEFAULTS, **over)
    g = np.asarray(guides, dtype=np.float32).astype(np.float64)
    h, w = cv.shape[:2]
    A, N, Z, H = g[..., 0:3], g[..., 3:6], g[..., 6], g[..., 7]
    levels = int(p["levels"])
    dem = bool(p["demodulate"]) and levels > 0
    a = A + EPS
    Cc, V = (cv[..., 0:3] / a, cv[..., 3:6] / (a * a)) if dem else (cv[..., 0:3], cv[..., 3:6])
    sc2, sn2, sa2, sz2 = (p[k] * p[k] for k in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"))
    k = (0.375, 0.25, 0.0625)
    with np.errstate(under="ignore"):
        for lev in range(levels):
            s = 1 << lev
            sw, sC, sV = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
            sumV = (V[..., 0] + V[..., 1]) + V[..., 2]
            for j in range(-2, 3):
                for i in range(-2, 3):
                    dx, dy = s * i, s * j
                    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                    if y0 >= y1 or x0 >= x1:
                        continue                                              # the tap is outside the image for every pixel: skipped
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                    dn_ = N[P] - N[Q]
                    xn = ((dn_[..., 0] * dn_[..., 0] + dn_[..., 1] * dn_[..., 1]) + dn_[..., 2] * dn_[..., 2]) / sn2
                    da = A[P] - A[Q]
                    xa = ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) / sa2
                    dz = Z[P] - Z[Q]
                    xz = (dz * dz) / (sz2 * (Z[P] * Z[P] + Z[Q] * Z[Q]) + TINY)
                    dh = H[P] - H[Q]
                    xh = dh * dh
                    dc = Cc[P] - Cc[Q]
                    xc = ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) / (sc2 * (sumV[P] + sumV[Q]) + TINY)
                    wt = ((((k[abs(i)] * k[abs(j)]) * dn._weight(xn)) * dn._weight(xa)) * dn._weight(xz)) * dn._weight(xh) * dn._weight(xc)
                    w2 = wt * wt
                    sw[P] = sw[P] + wt
                    sC[P] = sC[P] + wt[..., None] * Cc[Q]
                    sV[P] = sV[P] + w2[..., None] * V[Q]
            Cc, V = sC / sw[..., None], sV / (sw * sw)[..., None]
    out = (Cc * a if dem else Cc).astype(np.float32)
    return (out, np.concatenate([Cc, V], axis=-1)) if want_state else out


def tie_pixel(swap=False):
    """test_robust_cpu's tie, K = 9, n = 9: buckets 0 and 1 share the key y = 1 with different colours, two hot buckets make the trim 1 — the two tied
    buckets straddle the low trim boundary.  swap: the two change places."""
    B = np.zeros((9, 3))
    B[0], B[1] = [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]
    B[2:7] = [4.0, 4.0, 4.0]
    B[7:9] = [8.0, 8.0, 8.0]
    if swap:
        B[[0, 1]] = B[[1, 0]]
    return B


def plant(B, n=None):
    """The corner cases into the first pixels of an image of buckets (h, w, K, 3), wherever the image has room for them: equal buckets, one hot
    bucket, all zero, negative sums, tiny values (the squares of their differences are subnormal), and for K = 9 the tie of tie_pixel."""
    B = B.copy()
    K = B.shape[-2]
    flat = B.reshape(-1, K, 3)
    cases = [np.broadcast_to(np.float64([3.0, 10.0, 0.5]), (K, 3)), np.zeros((K, 3)), np.zeros((K, 3)), -np.abs(flat[0]) - 1.0, flat[0] * 1e-160]
    cases[1] = cases[1].copy()
    cases[1][K // 3] = [7.0, 14.0, 3.5]
    if K == 9:
        cases += [tie_pixel(), tie_pixel(True)]
    for i, c in enumerate(cases):
        if 2 * i + 1 < flat.shape[0]:
            flat[2 * i + 1] = c
    return B


def synthetic_buckets(seed, K, shape, n):
    """Heavy-tailed buckets with the planted cases.  n: a count for every pixel, or per-pixel counts (every pixel the buckets of its own prefix)."""
    rng = np.random.default_rng(seed)
    if np.isscalar(n):
        return plant(fill_buckets(heavy_tailed(rng, min(int(n), 96), shape), K))
    x = heavy_tailed(rng, int(n.max()), shape)
    x = x * (np.arange(x.shape[0])[:, None, None, None] < n[None, ..., None])
    return plant(fill_buckets(x, K))


# ---- the header against numpy ----
@pytest.mark.parametrize("K", ALL_K)
def test_core_against_numpy(core, K):
    shape = (23, 37)
    trimmed = 0
    for n in (K, 2 * K - 1, 64):
        B = synthetic_buckets(200 + K, K, shape, n)
        got, ref = core_cv(core, B, n), numpy_cv(B, n)
        assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(got[1], ref[1]), (K, n)
        assert np.isfinite(got[0]).all() and (got[0][..., 3:6] >= 0).all()
        trimmed += int((got[1] > 0).sum())
        assert (got[0][..., 3:6][got[1] == (K - 1) // 2] == 0).all()                  # the median bucket: no spread by construction
    assert trimmed > 0
    counts = np.random.default_rng(K).integers(K, 3 * K + 3, size=shape).astype(np.uint32)
    B = synthetic_buckets(300 + K, K, shape, counts)
    got, ref = core_cv(core, B, counts), numpy_cv(B, counts)
    assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("K", ALL_K)
def test_equal_buckets_have_no_variance(core, K):
    v = np.float64([0.75, 2.5, 0.125])
    for per in (1, 4):
        B = np.broadcast_to(v * 4.0 * per, (5, K, 3)).copy()
        cv, trim = core_cv(core, B, K * per)
        assert not trim.any() and (cv[..., 3:6] == 0).all() and np.array_equal(bits(cv[..., 0:3]), bits(np.broadcast_to(v, (5, 3))))


@pytest.mark.parametrize("K", ALL_K)
def test_one_hot_bucket_is_the_median_bucket_without_variance(core, K):
    """One bucket holds everything: where robust_pixel trims to the median bucket (K = 3, 9, 15 for every value; see test_robust_noise_cpu for 5 and
    13) C is that bucket's mean — zero — and V is 0 by construction; the trim is robust_pixel's whatever it is."""
    full = 0
    for hot in range(K):
        for value in (1.0, 3.7e5, 1e-3):
            B = np.zeros((1, K, 3))
            B[0, hot] = np.float64([value, 2.0 * value, 0.5 * value])
            cv, trim = core_cv(core, B, 2 * K)
            assert trim[0] == core_r(core, B, 2 * K)[1][0], (K, hot, value)
            assert np.array_equal(bits(cv), bits(numpy_cv(B, 2 * K)[0]))
            if K in (3, 9, 15):
                assert trim[0] == (K - 1) // 2, (K, hot, value)
            if trim[0] == (K - 1) // 2:
                assert (cv == 0).all() and not np.signbit(cv).any(), (K, hot, value)
                full += 1
    assert full > 0


@pytest.mark.parametrize("K", ALL_K)
def test_zero_negative_and_tiny_sums(core, K):
    cv, trim = core_cv(core, np.zeros((4, K, 3)), 64)
    assert not trim.any() and (cv == 0).all()
    rng = np.random.default_rng(1)
    pos = fill_buckets(heavy_tailed(rng, 64, (11,)), K)
    cv, trim = core_cv(core, -pos, 64)                                                 # T < 0: no trim, the plain spread of the bucket means
    ref = numpy_cv(-pos, 64)
    assert not trim.any() and (cv[..., 0:3] < 0).all() and (cv[..., 3:6] > 0).all()
    assert np.array_equal(bits(cv), bits(ref[0]))
    tiny = pos * 1e-160                                                                # the squared differences are subnormal or zero
    cv, trim = core_cv(core, tiny, 64)
    assert np.array_equal(bits(cv), bits(numpy_cv(tiny, 64)[0])) and np.array_equal(trim, core_cv(core, pos, 64)[1])
    assert (cv[..., 0:3] > 0).all() and (cv[..., 3:6] >= 0).all() and (cv[..., 3:6] < 1e-300).all()


def test_equal_keys_straddling_the_trim_are_ordered_by_bucket_index(core):
    """tie_pixel: buckets 0 (red) and 1 (green) share the key, one bucket goes at either end.  The stable order (y, b) drops bucket 0 and makes bucket
    1 the low winsorizing value: C and V are worked out by hand, and swapping the two buckets swaps red and green — other bits."""
    B, S = tie_pixel()[None], tie_pixel(True)[None]
    (cv, trim), (cs, ts) = core_cv(core, B, 9), core_cv(core, S, 9)
    assert trim[0] == 1 and ts[0] == 1
    # kept (t = 1): bucket 1 = (0, 1, 0), five of (1, 1, 1), one of (2, 2, 2); w = kept plus bucket 1 again (low) and (2, 2, 2) again (high)
    want_c = np.float64([7.0 / 7.0, 8.0 / 7.0, 7.0 / 7.0])
    assert np.array_equal(bits(cv[0, 0:3]), bits(want_c))
    w = {0: [0, 0, 1, 1, 1, 1, 1, 2, 2], 1: [1, 1, 1, 1, 1, 1, 1, 2, 2]}
    for c, ws in ((0, w[0]), (1, w[1]), (2, w[0])):                                    # (blue is 0 in both tied buckets, as red is in bucket 1)
        ws = np.float64(ws)
        acc = ws[0]
        for v in ws[1:]:
            acc = acc + v
        wbar = acc / 9.0
        ss = (ws[0] - wbar) * (ws[0] - wbar)
        for v in ws[1:]:
            ss = ss + (v - wbar) * (v - wbar)
        f = 9.0 / 7.0
        assert cv[0, 3 + c] == ss / 8.0 / 9.0 * f * f, c
    assert np.array_equal(bits(cs[0, [1, 0, 2, 4, 3, 5]]), bits(cv[0]))                # swapped buckets: red and green change places
    assert not np.array_equal(bits(cs[0]), bits(cv[0]))
    for X in (B, S):
        assert np.array_equal(bits(core_cv(core, X, 9)[0]), bits(numpy_cv(X, 9)[0]))


# ---- consistency with hr_robust and with the robust noise estimate ----
@pytest.mark.parametrize("K", ALL_K)
def test_c_is_r_and_the_trim_is_the_same_everywhere(core, K):
    shape = (23, 37)
    for n in (K, 2 * K - 1, 64):
        B = synthetic_buckets(400 + K, K, shape, n)
        cv, trim = core_cv(core, B, n)
        R, tr = core_r(core, B, n)
        assert np.array_equal(bits(cv[..., 0:3].astype(np.float32)), bits(R)) and np.array_equal(trim, tr), (K, n)
        assert np.array_equal(trim, core_e(core, B, n, 0.01)[1]), (K, n)
        assert np.array_equal(bits(R), bits(numpy_robust(B, n)[0]))


@pytest.mark.parametrize("K", ALL_K)
def test_robust_pixel_k_is_robust_pixel(core, K):
    """The templated resolve of robust_kernel<K> against the run-time K definition: every n from 0 to 3 K + 2 side by side, and equal counts."""
    shape = (23, 37)
    rng = np.random.default_rng(K)
    counts = rng.integers(0, 3 * K + 3, size=shape).astype(np.uint32)
    counts[0, :4] = [0, 1, K - 1, K]
    B = synthetic_buckets(500 + K, K, shape, counts)
    a, b = core_r(core, B, counts, templated=True), core_r(core, B, counts)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    assert np.array_equal(bits(a[0]), bits(numpy_robust(B, counts)[0]))
    assert (a[0][counts == 0] == 0).all() and not a[1][counts < K].any()
    for n in (0, 1, K - 1, K, K + 1, 64, 1000):
        B = synthetic_buckets(600 + K, K, shape, max(n, 1))
        a, b = core_r(core, B, n, templated=True), core_r(core, B, n)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (K, n)


@pytest.mark.parametrize("K", ALL_K)
def test_one_channel_has_the_variance_of_the_robust_noise_estimate(core, K):
    """With one channel non-zero the key y IS that channel's mean ((m + 0) + 0 is exact), so sum V = V_c is the square of §4.11's se = e_R den.
    Bound, in units u = 2^-53 of relative rounding error (each IEEE operation at most 1 u): V = q f f with f = fl(K / kept) carries 1 u twice for f
    and 1 u for each product, 4 u; se = fl(fl(fl(sqrt q) K) / kept) carries 3 u, e = fl(se / den) 4 u, fl(e den) 5 u, its square 10 u + 1 u.  Both
    start from the same q, so they differ by at most 15 u, first order; 16 u is asserted."""
    floor = 0.01
    rng = np.random.default_rng(700 + K)
    for c in range(3):
        B = np.zeros((23, 37, K, 3))
        B[..., c] = fill_buckets(heavy_tailed(rng, 64, (23, 37)), K)[..., c]
        cv, trim = core_cv(core, B, 64)
        e, te = core_e(core, B, 64, floor)
        assert np.array_equal(trim, te)
        sum_v = (cv[..., 3] + cv[..., 4]) + cv[..., 5]
        assert (cv[..., [3 + k for k in range(3) if k != c]] == 0).all()
        den = cv[..., c] + 3.0 * floor                                                 # Ry = C_c here, the same operations
        sq = (e * den) * (e * den)
        assert np.array_equal(bits(numpy_error(B, 64, floor, parts=True)[3]), bits(cv[..., c]))
        assert (np.abs(sum_v - sq) <= 16 * 2.0 ** -53 * np.maximum(sum_v, sq)).all(), (K, c)
        assert (sum_v > 0).any()


# ---- the whole filter ----
SHAPES = [(37, 23), (1, 1), (5, 1), (1, 5)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("K", [3, 9, 15])
def test_filter_against_numpy(core, w, h, K):
    g = dn.synthetic_inputs(11, w, h)[3]
    counts = np.random.default_rng(w * h + K).integers(K, 3 * K + 3, size=(h, w)).astype(np.uint32)
    for n in (2 * K + 1, counts):
        B = synthetic_buckets(800 + K, K, (h, w), n)
        cv0, _ = numpy_cv(B, n)
        R = core_r(core, B, n)[0]
        for levels in (0, 1, 5):
            for dem in (0, 1):
                got, st = core_filter(core, B, n, g, want_state=True, levels=levels, demodulate=dem)
                ref, st_ref = numpy_filter(cv0, g, want_state=True, levels=levels, demodulate=dem)
                assert np.array_equal(bits(got), bits(ref)) and np.array_equal(bits(st), bits(st_ref)), (w, h, K, levels, dem)
                assert np.isfinite(got).all()
                if levels == 0:
                    assert np.array_equal(bits(got), bits(R))                          # without a level D is R
        if (w, h) == (37, 23):
            assert not np.array_equal(core_filter(core, B, n, g, levels=1), R)         # a level does something, and V steers it:
            flat = core_filter(core, np.repeat(B.sum(axis=2, keepdims=True) / K, K, axis=2), K, g, levels=1)
            assert not np.array_equal(flat, core_filter(core, B, n, g, levels=1))


# ---- quality on the checker's per-sampling renders (the figures of DESIGN.md §4.12, with half the truth set of tools/robust_denoise_quality.py) ----
QW, QH, QN, QBOUNCES, QTRUTH = 96, 54, 16, 2, 512
_oracle = {}


def oracle_short_render(orc, scenes, name):
    """(per-sampling values x (QN, h, w, 3) fp32, fp32 accumulator, moments, guide planes with QBOUNCES bounces, truth radiance), once per scene."""
    if name not in _oracle:
        sc, osc = scenes(name)
        x = np.stack([osc.render(QW, QH, s, s + 1)[0] for s in range(1, QN + 1)]).astype(np.float32)
        acc = np.zeros((QH, QW, 3), dtype=np.float32)
        for s in range(QN):
            acc = acc + x[s]
        xd = x.astype(np.float64)
        mom = np.concatenate([xd.sum(axis=0), (xd * xd).sum(axis=0)], axis=-1)
        guides = gc.planes_of(gc.oracle_chain(orc, osc, sc.desc, QW, QH, QBOUNCES)[0]).astype(np.float32)
        truth, _ = osc.render(QW, QH, 100001, 100001 + QTRUTH)
        _oracle[name] = (x, acc, mom, guides, truth.astype(np.float64) / (4.0 * QTRUTH))
    return _oracle[name]


def quality_figures(core, dcore, x, acc, mom, guides, truth, K):
    """(R / mean, D / mean, DR / R, DR / D): relative squared errors of the robust radiance, today's denoiser and the robust denoiser."""
    n = x.shape[0]
    B = fill_buckets(x, K)
    e_mean = rel_sq_error(acc / np.float32(4 * n), truth)
    e_r = rel_sq_error(core_r(core, B, n)[0], truth)
    e_d = rel_sq_error(dn.core_denoise(dcore, acc, mom, n, guides), truth)
    e_dr = rel_sq_error(core_filter(core, B, n, guides), truth)
    return e_r / e_mean, e_d / e_mean, e_dr / e_r, e_dr / e_d


@pytest.mark.parametrize("name,measured", [("cornell_mini", (0.59, 0.59)), ("rtcamp6_v3_1", (0.66, 0.34))])
def test_quality_on_the_oracle(core, orc, scenes, tmp_path, name, measured):
    """96x54, 16 samplings, guide_bounces 2, default parameters: the denoised R beats R alone and beats today's denoiser on the same samplings.
    The truth is samplings 100001 .. 100512: half of the 1,024 behind DESIGN.md §4.12's table, to keep this test within the suite's budget (the
    oracle renders on the CPU; 47 s for both scenes on 8 cores) — the assertions and their bound are unchanged.  Measured with this truth, K = 5:
    cornell_mini DR / R 0.557, DR / D 0.584; rtcamp6_v3_1 0.676, 0.314.  K = 9 (printed, not asserted): 0.852 / 0.678 and 0.934 / 0.287."""
    dcore = dn.build_core(tmp_path)
    data = oracle_short_render(orc, scenes, name)
    for K in (5, 9):
        r_mean, d_mean, dr_r, dr_d = quality_figures(core, dcore, *data, K)
        print("%s n=%d K=%d: R/mean %.3f  D/mean %.3f  DR/R %.3f  DR/D %.3f  (a restatement measured DR/R %.2f, DR/D %.2f at K = 5)"
              % ((name, QN, K, r_mean, d_mean, dr_r, dr_d) + measured))
        if K == 5:
            assert dr_r < 1.0 and dr_d < 1.0


# ---- interface ----
def test_entry_point_declared_exported_and_bound(ha):
    raw = open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+hr_denoise_robust\s*\(\s*hr_ctx\s*\*\s*\w*\s*,\s*const\s+hr_denoise_params\s*\*\s*\w+\s*\)\s*;", text)
    assert int(re.search(r"#define\s+HR_ABI_VERSION\s+(\d+)", text).group(1)) == 7       # a function was added, none changed
    assert "robust_pixel_cv_k" in raw
    lib = C.CDLL(ha.HIP_LIB)
    assert hasattr(lib, "hr_denoise_robust")
    assert callable(getattr(ha.Renderer, "denoise_robust", None))
    assert len(ha.hip_lib().hr_denoise_robust.argtypes) == 2
    ffi = open(os.path.join(ROOT, "rust", "hip_ffi.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"pub fn hr_denoise_robust\(ctx: \*mut HrCtx, p: \*const HrDenoiseParams", ffi)
    assert "pub fn hr_denoise_robust(" in integration


def test_kernel_rows():
    kv = open(os.path.join(ROOT, "hanamaru-renderer_amd", "csrc", "kernel_variants.h")).read()
    for K in ALL_K:
        assert "HR_VARIANT(robust_denoise_init_kernel, %d)" % K in kv, K
        assert "HR_VARIANT(robust_kernel, %d)" % K in kv, K
        assert "HR_VARIANT(robust_noise_kernel, %d, true)" % K in kv, K                 # the estimate's rows are still there
    assert "select_robust_denoise_init_kernel" in kv and "select_robust_kernel" in kv


def test_cli_help_lists_the_flag(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--robust-denoise" in r.stdout
    assert "--robust-denoise" in open(os.path.join(ROOT, "README.md")).read()
    assert "robust_denoise_quality.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


@pytest.mark.parametrize("args,word", [(["--robust-denoise"], "--robust-denoise needs --robust"),
                                       (["--robust-denoise", "--denoise-levels", "2"], "--robust-denoise needs --robust"),
                                       (["--robust", "5", "--robust-denoise", "--gpus", "2"], "one device"),
                                       (["--robust", "5", "--robust-denoise", "--debug"], "--debug"),
                                       (["--robust", "5", "--robust-denoise", "--denoise"], "--denoise"),
                                       (["--robust", "5", "--robust-denoise", "--denoise-levels", "6"], "--denoise-levels"),
                                       (["--denoise-levels", "2"], "--denoise-levels needs --denoise"),
                                       (["--guide-bounces", "2"], "--guide-bounces needs --denoise or --guide-image")])
def test_cli_refuses_before_any_device(tmp_path, args, word):
    r = run_cli(["-w", "64", "-h", "48", "-s", "8"] + args, tmp_path)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not (tmp_path / "result.txt").exists()
