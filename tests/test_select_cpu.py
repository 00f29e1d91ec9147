"""The denoiser that picks its level per pixel on the CPU tier: csrc/select_core.h compiled for the host against an independent
numpy restatement of its definition — bit for bit: + - x / and comparisons in f64 without contraction —, its consequences (S against the fixed
levels, equal halves, a planted firefly), the entry points declared, exported and bound, and the quality ordering on the checker's renders."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guide_chain as gc
import test_denoise_cpu as dn
from cli import run_cli
from test_robust_cpu import bits, fill_buckets, rel_sq_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_K = (3, 5, 7, 9, 11, 13, 15)
EPS, TINY = 1e-3, 1e-30
ENTRY_POINTS = ("hr_select_default_params", "hr_denoise_select", "hr_read_selected", "hr_read_selected_levels", "hr_resolve_selected")

HARNESS = r'''
#include <vector>
#include "select_core.h"
using namespace hr;
// sig = {sigma_color, sigma_normal, sigma_albedo, sigma_depth}; counts may be null (every pixel: n_all); states (may be null): w*h*18 doubles
extern "C" void select_run(const double *buckets, uint32_t K, const uint32_t *counts, uint32_t n_all, const float *acc, const double *mom, const float *guides, uint32_t w, uint32_t h,
                           uint32_t levels, int demodulate, const double *sig, uint32_t smooth, float *S, uint8_t *L, double *states) {
    std::vector<double> work((size_t)w * h * 45);
    select_image(buckets, K, counts, n_all, acc, mom, guides, w, h, levels, demodulate, denoise_sigmas(sig[0], sig[1], sig[2], sig[3]), smooth, work.data(), S, L, states);
}
'''


def build_core(directory):
    src, so = directory / "select_harness.cpp", directory / "libselect_harness.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "hanamaru-renderer_amd", "csrc"), "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    lib.select_run.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
                               C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return build_core(tmp_path_factory.mktemp("select"))


@pytest.fixture(scope="module")
def dcore(tmp_path_factory):
    return dn.build_core(tmp_path_factory.mktemp("select_denoise"))


def core_select(lib, buckets, acc, mom, n, guides, smooth=0, want_states=False, **over):
    """select_image over an (h, w, K, 3) image of buckets.  n: one count for every pixel, or an (h, w) array.  Returns (S, L[, states (3, h, w, 6)])."""
    params = dict(dn.DEFAULTS, **over)
    b = np.ascontiguousarray(buckets, dtype=np.float64)
    h, w, K = b.shape[:3]
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    assert acc.shape == (h, w, 3) and mom.shape == (h, w, 6) and guides.shape == (h, w, 8) and b.shape[3] == 3
    counts = None if np.isscalar(n) else np.ascontiguousarray(n, dtype=np.uint32)
    S, L = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.uint8)
    states = np.zeros((3, h, w, 6)) if want_states else None
    sig = dn._sig(params)
    lib.select_run(b.ctypes.data, K, counts.ctypes.data if counts is not None else None, int(n) if counts is None else 0, acc.ctypes.data, mom.ctypes.data, guides.ctypes.data,
                   w, h, int(params["levels"]), int(params["demodulate"]), sig.ctypes.data, int(smooth), S.ctypes.data, L.ctypes.data,
                   states.ctypes.data if want_states else None)
    return (S, L, states) if want_states else (S, L)


# ---- the numpy restatement ----
def _taps(h, w, s):
    for j in range(-2, 3):
        for i in range(-2, 3):
            dx, dy = s * i, s * j
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if y0 < y1 and x0 < x1:                                                   # (else the tap is outside the image for every pixel: skipped)
                yield i, j, (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def _level(state, g, s, p):
    """denoise_core.h's level with step s on one state (h, w, 6)."""
    Cc, V = state[..., 0:3], state[..., 3:6]
    h, w = Cc.shape[:2]
    A, N, Z, H = g[..., 0:3], g[..., 3:6], g[..., 6], g[..., 7]
    sc2, sn2, sa2, sz2 = (p[k] * p[k] for k in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"))
    k = (0.375, 0.25, 0.0625)
    sw, sC, sV = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    sumV = (V[..., 0] + V[..., 1]) + V[..., 2]
    for i, j, P, Q in _taps(h, w, s):
        d = N[P] - N[Q]
        xn = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / sn2
        d = A[P] - A[Q]
        xa = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / sa2
        dz = Z[P] - Z[Q]
        xz = (dz * dz) / (sz2 * (Z[P] * Z[P] + Z[Q] * Z[Q]) + TINY)
        dh = H[P] - H[Q]
        xh = dh * dh
        d = Cc[P] - Cc[Q]
        xc = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / (sc2 * (sumV[P] + sumV[Q]) + TINY)
        wt = (((((k[abs(i)] * k[abs(j)]) * dn._weight(xn)) * dn._weight(xa)) * dn._weight(xz)) * dn._weight(xh)) * dn._weight(xc)
        w2 = wt * wt
        sw[P] = sw[P] + wt
        sC[P] = sC[P] + wt[..., None] * Cc[Q]
        sV[P] = sV[P] + w2[..., None] * V[Q]
    return np.concatenate([sC / sw[..., None], sV / (sw * sw)[..., None]], axis=-1)


def _smooth(e, s):
    h, w = e.shape
    k = (0.375, 0.25, 0.0625)
    se, sh = np.zeros((h, w)), np.zeros((h, w))
    for i, j, P, Q in _taps(h, w, s):
        hw = k[abs(i)] * k[abs(j)]
        se[P] = se[P] + hw * e[Q]
        sh[P] = sh[P] + hw
    return se / sh


def numpy_select(buckets, acc, mom, n, guides, smooth=0, **over):
    """The definition in the comment of select_core.h, restated on whole arrays: every line one IEEE f64 operation per element, every bucket sum
    sequential from its first term, the taps in row order.  Returns (S, L, states (3, h, w, 6))."""
    p = dict(dn.DEFAULTS, **over)
    B = np.asarray(buckets, dtype=np.float64)
    h, w, K = B.shape[:3]
    acc = np.asarray(acc, dtype=np.float32)
    mom = np.asarray(mom, dtype=np.float64)
    g = np.asarray(guides, dtype=np.float32).astype(np.float64)
    cnt = np.full((h, w), n, dtype=np.uint32) if np.isscalar(n) else np.asarray(n, dtype=np.uint32)
    assert (cnt >= 2).all()
    levels = int(p["levels"])
    dem = bool(p["demodulate"]) and levels > 0
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        nb = (cnt.astype(np.int64)[..., None] - np.arange(K)[None, None, :] + (K - 1)) // K
        nA, nB = nb[..., 0::2].sum(axis=-1).astype(np.float64)[..., None], nb[..., 1::2].sum(axis=-1).astype(np.float64)[..., None]
        sa, sb = B[..., 0, :].copy(), B[..., 1, :].copy()
        for b in range(2, K):
            if b & 1:
                sb = sb + B[..., b, :]
            else:
                sa = sa + B[..., b, :]
        A0, B0 = sa / nA / 4.0, sb / nB / 4.0
        scale = (np.float32(1.0) / (cnt * np.uint32(4)).astype(np.float32)).astype(np.float64)     # the resolve's fp32 scale, correctly rounded
        nd = cnt.astype(np.float64)[..., None]
        C0 = acc.astype(np.float64) * scale[..., None]
        s1, s2 = mom[..., 0:3], mom[..., 3:6]
        var = (s2 - s1 * (s1 / nd)) / (nd - 1.0)
        V0 = np.where(var > 0.0, var, 0.0) / nd / 16.0
        VA, VB = V0 * nd / nA, V0 * nd / nB
        a = g[..., 0:3] + EPS
        if dem:
            a2 = a * a
            C0, V0, A0, VA, B0, VB = C0 / a, V0 / a2, A0 / a, VA / a2, B0 / a, VB / a2
        FA, FB, FW = np.concatenate([A0, VA], axis=-1), np.concatenate([B0, VB], axis=-1), np.concatenate([C0, V0], axis=-1)
        best = S = L = None
        for lev in range(levels + 1):
            dA, dB = FA[..., 0:3] - B0, FB[..., 0:3] - A0
            e = ((dA[..., 0] * dA[..., 0] + dB[..., 0] * dB[..., 0]) + (dA[..., 1] * dA[..., 1] + dB[..., 1] * dB[..., 1])) + (dA[..., 2] * dA[..., 2] + dB[..., 2] * dB[..., 2])
            for t in range(int(smooth)):
                e = _smooth(e, 1 << t)
            final = (FW[..., 0:3] * a if dem else FW[..., 0:3]).astype(np.float32)
            if lev == 0:
                best, L, S = e, np.zeros((h, w), dtype=np.uint8), final
            else:
                take = e < best
                best, L, S = np.where(take, e, best), np.where(take, np.uint8(lev), L), np.where(take[..., None], final, S)
            if lev < levels:
                FA, FB, FW = _level(FA, g, 1 << lev, p), _level(FB, g, 1 << lev, p), _level(FW, g, 1 << lev, p)
    return S, L.astype(np.uint8), np.stack([FA, FB, FW])


def synthetic(seed, w, h, K, n, firefly=0.03):
    """Consistent inputs of one render: per-sampling values whose mean follows dn.synthetic_inputs' guides, with rare bright outliers, summed into
    the fp32 accumulator, the f64 moments and the K buckets (sampling j of a pixel into bucket j mod K).  n: one count, or per-pixel counts (a pixel
    holds its own prefix).  Returns (buckets, acc, mom, n, guides)."""
    rng = np.random.default_rng(seed)
    g = dn.synthetic_inputs(seed, w, h, n=2)[3]
    cnt = np.full((h, w), n, dtype=np.uint32) if np.isscalar(n) else np.asarray(n, dtype=np.uint32)
    mean = 4.0 * (g[..., 0:3].astype(np.float64) + 0.05)
    N = int(cnt.max())
    x = rng.gamma(2.0, 0.5, size=(N, h, w, 3)) * mean
    x = np.where(rng.random((N, h, w, 1)) < firefly, x * 200.0, x).astype(np.float32)
    x = x * (np.arange(N)[:, None, None, None] < cnt[None, ..., None])
    acc = np.zeros((h, w, 3), dtype=np.float32)
    for s in range(N):
        acc = acc + x[s]
    xd = x.astype(np.float64)
    mom = np.concatenate([xd.sum(axis=0), (xd * xd).sum(axis=0)], axis=-1)
    return fill_buckets(x, K), acc, mom, n, g


def unequal_counts(seed, w, h, K):
    """per-pixel counts 2 .. 3 K + 2: some no multiple of K, some below K, and n = 2 wherever the frame has room for it"""
    cnt = np.random.default_rng(seed).integers(2, 3 * K + 3, size=(h, w)).astype(np.uint32)
    cnt.reshape(-1)[:3] = [2, K + 1, 2 * K]
    return cnt


# ---- 1. the core against numpy, bit for bit ----
# 5x3: smaller than the reach at step 4 (the far taps are all skipped); 37x19 and 33x9: no multiple of anything
@pytest.mark.parametrize("w,h", [(5, 3), (37, 19), (33, 9)])
@pytest.mark.parametrize("K", [3, 9, 15])
def test_core_against_numpy(core, w, h, K):
    picked = set()
    for n in (2 * K + 1, unequal_counts(w * h + K, w, h, K)):
        B, acc, mom, n, g = synthetic(100 + K, w, h, K, n)
        for levels in (0, 1, 5):
            for dem in (0, 1):
                for smooth in (0, 2):
                    S, L, st = core_select(core, B, acc, mom, n, g, smooth=smooth, want_states=True, levels=levels, demodulate=dem)
                    rS, rL, rst = numpy_select(B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)
                    where = (w, h, K, levels, dem, smooth)
                    assert np.array_equal(bits(st), bits(rst)), where
                    assert np.array_equal(L, rL), where
                    assert np.array_equal(bits(S), bits(rS)), where
                    assert np.isfinite(S).all() and L.max() <= levels
                    picked |= set(np.unique(L).tolist())
    if (w, h) == (37, 19):
        assert len(picked) >= 3, picked                                               # the pick does pick


# ---- 2. S against the fixed levels ----
@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("dem", [0, 1])
def test_s_has_the_bits_of_the_fixed_level(core, dcore, K, dem):
    w, h, levels = 37, 19, 5
    for n in (2 * K + 1, unequal_counts(K, w, h, K)):
        B, acc, mom, n, g = synthetic(200 + K, w, h, K, n)
        S, L = core_select(core, B, acc, mom, n, g, levels=levels, demodulate=dem)
        seen = 0
        for lev in range(levels + 1):
            # (hr_denoise(levels = 0) drops the demodulation, a pixel that picks level 0 under it is (float)((C / a) a): the float of C unless C
            # lies within two f64 ulps of the boundary between two floats, which none of these does)
            D = dn.core_denoise(dcore, acc, mom, n, g, levels=lev, demodulate=dem)
            m = L == lev
            if m.any():
                assert np.array_equal(bits(S[m]), bits(D[m])), (K, dem, lev)
                seen += 1
        assert seen >= 2


def test_levels_zero_is_the_mean_rounded_once(core):
    w, h, K = 37, 19, 9
    cnt = unequal_counts(5, w, h, K)
    B, acc, mom, n, g = synthetic(300, w, h, K, cnt)
    scale = np.float32(1.0) / (cnt * np.uint32(4)).astype(np.float32)
    for dem in (0, 1):
        S, L = core_select(core, B, acc, mom, n, g, levels=0, demodulate=dem)
        assert not L.any() and np.array_equal(bits(S), bits(acc * scale[..., None]))


# ---- 3. equal halves ----
@pytest.mark.parametrize("smooth", [0, 2])
def test_equal_halves_give_level_zero(core, smooth):
    """A noisy image whose halves agree in every pixel: K = 3, n = 12, every bucket 16 r(p) — A0 = (16 r + 16 r) / 8 / 4 and B0 = 16 r / 4 / 4 are
    both r exactly.  e_0 = 0 and no error is negative, so the strict comparison keeps level 0 everywhere, smoothed or not."""
    w, h, K, n = 21, 11, 3, 12
    r = np.random.default_rng(17).gamma(2.0, 0.5, size=(h, w, 3)).astype(np.float32).astype(np.float64)
    B = np.repeat((16.0 * r)[:, :, None, :], K, axis=2)
    acc = (48.0 * r).astype(np.float32)
    mom = np.concatenate([48.0 * r, 1.5 * n * (4.0 * r) ** 2], axis=-1)
    g = dn.synthetic_inputs(3, w, h)[3]
    for dem in (0, 1):
        S, L, st = core_select(core, B, acc, mom, n, g, smooth=smooth, want_states=True, levels=4, demodulate=dem)
        assert not np.array_equal(bits(st[2]), bits(core_select(core, B, acc, mom, n, g, want_states=True, levels=0)[2][2]))   # the levels did filter
        assert not L.any()


# ---- 4. a planted firefly ----
def test_a_planted_firefly_is_filtered_and_the_rest_is_left_alone(core):
    """A flat image, every sampling 4 v: the halves agree everywhere and L = 0.  One hot sampling in bucket 0 (half A) of one pixel: at level 0 that
    pixel's A0 is off B0 by the whole firefly, at level 1 the filtered half A is pulled back to its neighbours — the pixel gets L > 0.  A pixel
    further than the filter's reach 2 (2^levels - 1) from it sees none of it in either half: its errors are all 0, L = 0, and S is the raw mean."""
    w, h, K, per, levels = 41, 21, 3, 4, 3
    px, py, reach = 20, 10, 2 * ((1 << levels) - 1)
    v = np.float32([0.75, 2.5, 0.125])
    x = np.broadcast_to(v * np.float32(4.0), (per * K, h, w, 3)).copy()
    x[3, py, px] += np.float32(4000.0)                                                # sampling 3: bucket 0, the even half
    acc = np.zeros((h, w, 3), dtype=np.float32)
    for s in range(per * K):
        acc = acc + x[s]
    xd = x.astype(np.float64)
    mom = np.concatenate([xd.sum(axis=0), (xd * xd).sum(axis=0)], axis=-1)
    g = np.zeros((h, w, 8), dtype=np.float32)
    g[..., 0:3], g[..., 5], g[..., 6], g[..., 7] = 0.5, 1.0, 4.0, 1.0
    for dem in (0, 1):
        S, L = core_select(core, fill_buckets(x, K), acc, mom, per * K, g, levels=levels, demodulate=dem)
        rS, rL, _ = numpy_select(fill_buckets(x, K), acc, mom, per * K, g, levels=levels, demodulate=dem)
        assert np.array_equal(L, rL) and np.array_equal(bits(S), bits(rS))
        assert L[py, px] > 0
        yy, xx = np.mgrid[0:h, 0:w]
        far = (np.abs(xx - px) > reach) | (np.abs(yy - py) > reach)
        assert far.any() and not L[far].any()
        raw = acc * (np.float32(1.0) / np.float32(4 * per * K))
        if not dem:
            assert np.array_equal(bits(S[far]), bits(raw[far]))
        else:                                                                         # (C / a) a, rounded once: within an ulp of the mean, and the mean's bits in numpy's own words
            a = g[..., 0:3].astype(np.float64) + EPS
            want = ((acc.astype(np.float64) * np.float64(np.float32(1.0) / np.float32(4 * per * K))) / a * a).astype(np.float32)
            assert np.array_equal(bits(S[far]), bits(want[far]))


# ---- 5. plumbing ----
def test_entry_points_declared_exported_and_bound(ha):
    raw = open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"typedef\s+struct\s+\w*\s*\{\s*uint32_t\s+smooth\s*;\s*uint32_t\s+reserved\s*;\s*\}\s*hr_select_params\s*;", text)
    assert re.search(r"int\s+hr_select_default_params\s*\(\s*hr_select_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"int\s+hr_denoise_select\s*\(\s*hr_ctx\s*\*\s*\w*\s*,\s*const\s+hr_denoise_params\s*\*\s*\w+\s*,\s*const\s+hr_select_params\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"int\s+hr_read_selected\s*\(\s*hr_ctx\s*\*\s*\w*\s*,\s*float\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"int\s+hr_read_selected_levels\s*\(\s*hr_ctx\s*\*\s*\w*\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;", text)
    assert re.search(r"int\s+hr_resolve_selected\s*\(\s*hr_ctx\s*\*\s*\w*\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;", text)
    assert int(re.search(r"#define\s+HR_ABI_VERSION\s+(\d+)", text).group(1)) == 7       # functions were added, none changed
    lib = C.CDLL(ha.HIP_LIB)
    ffi = open(os.path.join(ROOT, "rust", "hip_ffi.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    arity = {"hr_select_default_params": 1, "hr_denoise_select": 3}
    for fn in ENTRY_POINTS:
        assert hasattr(lib, fn), fn
        assert len(getattr(ha.hip_lib(), fn).argtypes) == arity.get(fn, 2)
        assert "pub fn %s(" % fn in ffi and "pub fn %s(" % fn in integration, fn
    assert "size_of::<HrSelectParams>() == 8" in ffi
    assert C.sizeof(ha.SelectParams) == 8
    for method in ("denoise_select", "read_selected", "read_selected_levels", "resolve_selected"):
        assert callable(getattr(ha.Renderer, method, None)), method
    p = ha.select_default_params()                                                      # needs no device
    assert (p.smooth, p.reserved) == (2, 0)                                             # (the lowest worst case of tools/select_quality.py's table)
    assert ha.hip_lib().hr_select_default_params(None) == -1


def test_kernel_rows():
    kv = open(os.path.join(ROOT, "hanamaru-renderer_amd", "csrc", "kernel_variants.h")).read()
    pk = open(os.path.join(ROOT, "hanamaru-renderer_amd", "csrc", "post_kernels.h")).read()
    for K in ALL_K:
        assert "HR_VARIANT(select_init_kernel, %d)" % K in kv, K
    assert "select_select_init_kernel" in kv
    for kernel in ("select_init_kernel", "atrous3_kernel", "select_pick_kernel", "select_smooth_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, pk), kernel


def test_cli_help_lists_the_flags(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0
    readme = open(os.path.join(ROOT, "README.md")).read()
    for flag in ("--denoise-auto", "--select-smooth", "--level-image"):
        assert flag in r.stdout and flag in readme, flag
    tools = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "select_quality.py" in tools and "select_rate.py" in tools


@pytest.mark.parametrize("args,word", [(["--denoise-auto", "9", "--robust", "5"], "--robust"),
                                       (["--denoise-auto", "9", "--denoise"], "--denoise"),
                                       (["--denoise-auto", "9", "--debug"], "--debug"),
                                       (["--denoise-auto", "9", "--gpus", "2"], "one device"),
                                       (["--denoise-auto", "4"], "--denoise-auto"),
                                       (["--denoise-auto", "9", "--select-smooth", "4"], "--select-smooth"),
                                       (["--select-smooth", "1"], "--select-smooth needs --denoise-auto"),
                                       (["--level-image", "l.png"], "--level-image needs --denoise-auto")])
def test_cli_refuses_before_any_device(tmp_path, args, word):
    r = run_cli(["-w", "64", "-h", "48", "-s", "8"] + args, tmp_path)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not (tmp_path / "result.txt").exists()


# ---- 6. quality on the checker's per-sampling renders (the figures of DESIGN.md §4.16, with half the truth set of tools/select_quality.py) ----
QW, QH, QK, QTRUTH = 96, 54, 9, 1024
_oracle = {}


def oracle_render(orc, scenes, name, n_max=64):
    """(per-sampling values x (n_max, h, w, 3) fp32, {bounces: guide planes}, truth radiance), once per scene"""
    if name not in _oracle:
        sc, osc = scenes(name)
        x = np.stack([osc.render(QW, QH, s, s + 1)[0] for s in range(1, n_max + 1)]).astype(np.float32)
        guides = {k: gc.planes_of(gc.oracle_chain(orc, osc, sc.desc, QW, QH, k)[0]).astype(np.float32) for k in (0, 2)}
        truth, _ = osc.render(QW, QH, 100001, 100001 + QTRUTH)
        _oracle[name] = (x, guides, truth.astype(np.float64) / (4.0 * QTRUTH))
    return _oracle[name]


def sums_of(x):
    """(fp32 accumulator, f64 moments) of the samplings x (n, h, w, 3), one sampling at a time"""
    acc = np.zeros(x.shape[1:], dtype=np.float32)
    for s in range(x.shape[0]):
        acc = acc + x[s]
    xd = x.astype(np.float64)
    return acc, np.concatenate([xd.sum(axis=0), (xd * xd).sum(axis=0)], axis=-1)


def quality_ratios(core, dcore, x, guides, truth, K, smooth=0):
    """(fixed-levels-4 / raw, select / raw): relative squared errors against the truth over the raw mean's"""
    n = x.shape[0]
    acc, mom = sums_of(x)
    e_raw = rel_sq_error(acc / np.float32(4 * n), truth)
    e_fixed = rel_sq_error(dn.core_denoise(dcore, acc, mom, n, guides), truth)
    e_sel = rel_sq_error(core_select(core, fill_buckets(x, K), acc, mom, n, guides, smooth=smooth)[0], truth)
    return e_fixed / e_raw, e_sel / e_raw


def test_quality_on_the_oracle(core, dcore, orc, scenes):
    """96x54, K = 9, default parameters, smooth 0, truth samplings 100001 .. 101024 (half of tools/select_quality.py's 2,048).  Asserted on
    rtcamp6_v3_1 with first-hit guides, the case of DESIGN.md §4.9's finding, at 16 and at 64 samplings: the selection's error is below the
    whole-buffer filter's at levels = 4.  A host prototype measured fixed -> select 0.52 -> 0.31 (n = 16) and 1.95 -> 1.03 (n = 64), a gap of
    1.7 - 1.9 x.  The guide_bounces 2 rows are printed.  Measured with this truth: first-hit guides 0.351 -> 0.216 (n = 16) and 0.905 -> 0.520
    (n = 64); guide_bounces 2: 0.234 -> 0.213 and 0.364 -> 0.324."""
    x, guides, truth = oracle_render(orc, scenes, "rtcamp6_v3_1")
    for bounces in (0, 2):
        for n in (16, 64):
            fixed, sel = quality_ratios(core, dcore, x[:n], guides[bounces], truth, QK)
            print("rtcamp6_v3_1 guide_bounces=%d n=%d K=%d: fixed-4 / raw %.3f  select / raw %.3f" % (bounces, n, QK, fixed, sel))
            if bounces == 0:
                assert sel < fixed, (n, fixed, sel)
