"""The robust noise estimate on the CPU tier: robust_pixel_error of csrc/robust_core.h compiled for the host against an independent
numpy restatement of its definition — bit for bit: + - x /, comparisons, one truncation and one correctly rounded sqrt in f64 without contraction —,
its corner cases, its calibration on the checker's per-sampling renders, and the entry points declared, exported and bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cli import run_cli
from test_robust_cpu import bits, core_robust, fill_buckets, heavy_tailed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hr_robust_noise_estimate", "hr_read_robust_noise_image", "hr_read_robust_noise_trim", "hr_select_tiles_robust")
ALL_K = (3, 5, 7, 9, 11, 13, 15)

HARNESS = r'''
#include "robust_core.h"
using namespace hr;
// counts may be null (every pixel: n_all)
extern "C" void robust_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, uint64_t pixels, float *R, uint8_t *trim) {
    robust_image(buckets, counts, n_all, K, (size_t)pixels, R, trim);
}
extern "C" void robust_error_run(const double *buckets, const uint32_t *counts, uint64_t n_all, uint32_t K, double floor, uint64_t pixels, double *e, uint8_t *trim) {
    robust_error_image(buckets, counts, n_all, K, floor, (size_t)pixels, e, trim);
}
'''


def build_error_core(directory):
    src, so = directory / "robust_noise_harness.cpp", directory / "librobust_noise_harness.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "hanamaru-renderer_amd", "csrc"), "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    lib.robust_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.robust_error_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return build_error_core(tmp_path_factory.mktemp("robust_noise"))


def core_error(lib, buckets, n, floor=0.01):
    """The host-compiled robust_error_image over buckets (.., K, 3).  n: one count for every pixel, or an array of per-pixel counts (every one >= K).
    Returns (e float64 (..), trim uint8 (..))."""
    b = np.ascontiguousarray(buckets, dtype=np.float64)
    K, shape = b.shape[-2], b.shape[:-2]
    assert b.shape[-1] == 3
    pixels = int(np.prod(shape, dtype=np.int64))
    counts = None if np.isscalar(n) else np.ascontiguousarray(n, dtype=np.uint32)
    assert counts is None or counts.shape == shape
    e = np.zeros(shape, dtype=np.float64)
    trim = np.zeros(shape, dtype=np.uint8)
    lib.robust_error_run(b.ctypes.data, counts.ctypes.data if counts is not None else None, int(n) if counts is None else 0, K, float(floor), pixels,
                         e.ctypes.data, trim.ctypes.data)
    return e, trim


def numpy_error(buckets, n, floor=0.01, parts=False):
    """The definition in the comment of robust_pixel_error, restated on whole arrays: every line one IEEE f64 operation per element, every sum
    sequential from its first term.  parts: (e, trim, se, Ry, ss) instead of (e, trim)."""
    B = np.asarray(buckets, dtype=np.float64)
    K, shape = B.shape[-2], B.shape[:-2]
    B = B.reshape(-1, K, 3)
    P = B.shape[0]
    n = np.broadcast_to(np.asarray(n, dtype=np.uint64).reshape(-1), (P,))
    assert (n >= K).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        nb = (n[:, None] - np.arange(K, dtype=np.uint64)[None, :] + np.uint64(K - 1)) // np.uint64(K)
        m = B / nb.astype(np.float64)[..., None] / 4.0
        y = (m[..., 0] + m[..., 1]) + m[..., 2]
        ys = np.take_along_axis(y, np.argsort(y, axis=1, kind="stable"), 1)            # ascending by (y, b)
        T = ys[:, 0].copy()
        Gn = float(1 - K) * ys[:, 0]
        for i in range(2, K + 1):
            T = T + ys[:, i - 1]
            Gn = Gn + float(2 * i - K - 1) * ys[:, i - 1]
        G = Gn / (float(K) * T)
        want = np.trunc(np.where((T > 0.0) & (G > 0.0), G * float(K) / 2.0, 0.0)).astype(np.int64)
        trim = np.minimum((K - 1) // 2, want)
        e = np.zeros(P)
        se_all, ry_all, ss_all = np.zeros(P), np.zeros(P), np.zeros(P)
        for t in range((K - 1) // 2 + 1):
            kept = float(K - 2 * t)
            s = ys[:, t].copy()
            for i in range(t + 1, K - t):
                s = s + ys[:, i]
            Ry = s / kept
            lo, hi = ys[:, t], ys[:, K - 1 - t]
            w = [lo if i < t else (hi if i >= K - t else ys[:, i]) for i in range(K)]
            ws = w[0].copy()
            for i in range(1, K):
                ws = ws + w[i]
            wbar = ws / float(K)
            ss = (w[0] - wbar) * (w[0] - wbar)
            for i in range(1, K):
                d = w[i] - wbar
                ss = ss + d * d
            se = np.sqrt(ss / float(K - 1) / float(K)) * float(K) / kept
            den = Ry + 3.0 * floor
            e_t = np.where(den > 0.0, se / den, 0.0)
            sel = trim == t
            e = np.where(sel, e_t, e)
            se_all, ry_all, ss_all = np.where(sel, se, se_all), np.where(sel, Ry, ry_all), np.where(sel, ss, ss_all)
    if parts:
        return e.reshape(shape), trim.astype(np.uint8).reshape(shape), se_all.reshape(shape), ry_all.reshape(shape), ss_all.reshape(shape)
    return e.reshape(shape), trim.astype(np.uint8).reshape(shape)


def plain_spread_error(buckets, n, floor=0.01):
    """The untrimmed counterpart: the standard error of the mean of the K bucket means of the channel sum, over that mean + 3 floor."""
    B = np.asarray(buckets, dtype=np.float64)
    K = B.shape[-2]
    nb = (np.uint64(n) - np.arange(K, dtype=np.uint64) + np.uint64(K - 1)) // np.uint64(K)
    y = (B / nb.astype(np.float64)[:, None] / 4.0).sum(axis=-1)
    se = y.std(axis=-1, ddof=1) / np.sqrt(K)
    den = y.mean(axis=-1) + 3.0 * floor
    return np.where(den > 0.0, se / np.where(den > 0.0, den, 1.0), 0.0)


@pytest.mark.parametrize("K", ALL_K)
def test_core_against_numpy(core, K):
    rng = np.random.default_rng(100 + K)
    shape = (23, 37)
    trimmed = 0
    for n in (K, K + 1, 2 * K - 1, 64, 1000):
        B = fill_buckets(heavy_tailed(rng, min(n, 96), shape), K)                     # (1,000 samplings: the buckets of 96, n only divides)
        got, ref = core_error(core, B, n), numpy_error(B, n)
        assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(got[1], ref[1]), (K, n)
        assert np.isfinite(got[0]).all() and (got[0] >= 0).all()
        assert np.array_equal(got[1], core_robust(core, B, n)[1]), (K, n)              # the trim is robust_pixel's
        trimmed += int((got[1] > 0).sum())
    assert K == 3 or trimmed > 0
    # unequal per-pixel counts, K .. 3 K + 2
    counts = rng.integers(K, 3 * K + 3, size=shape).astype(np.uint32)
    x = heavy_tailed(rng, int(counts.max()), shape)
    x = x * (np.arange(x.shape[0])[:, None, None, None] < counts[None, ..., None])
    B = fill_buckets(x, K)
    got, ref = core_error(core, B, counts), numpy_error(B, counts)
    assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[1], core_robust(core, B, counts)[1])


@pytest.mark.parametrize("K", ALL_K)
def test_equal_buckets_have_no_error(core, K):
    v = np.float64([0.75, 2.5, 0.125])
    for per in (1, 4):
        B = np.broadcast_to(v * 4.0 * per, (5, K, 3)).copy()
        e, trim = core_error(core, B, K * per)
        assert not trim.any() and (e == 0).all() and not np.signbit(e).any()


@pytest.mark.parametrize("K", ALL_K)
def test_one_hot_bucket_is_the_median_bucket_without_spread(core, K):
    """One bucket holds everything: t = (K - 1) / 2, every winsorized value is the median bucket's, se = 0 by construction.  (G K / 2 is (K - 1) / 2
    in exact arithmetic; where the rounding of G leaves it a hair below, robust_pixel truncates to one less — K = 5 and 13 with some values —, and
    the estimate follows it: the trim is robust_pixel's whatever it is.  K = 3, 9, 15 are the cases test_robust_cpu pins.)"""
    full = 0
    for hot in range(K):
        for value in (1.0, 3.7e5, 1e-3):
            B = np.zeros((1, K, 3))
            B[0, hot] = np.float64([value, 2.0 * value, 0.5 * value])
            e, trim = core_error(core, B, 2 * K)
            assert trim[0] == core_robust(core, B, 2 * K)[1][0], (K, hot, value)
            assert np.array_equal(bits(e), bits(numpy_error(B, 2 * K)[0]))
            if K in (3, 9, 15):
                assert trim[0] == (K - 1) // 2, (K, hot, value)
            if trim[0] == (K - 1) // 2:
                assert e[0] == 0.0 and not np.signbit(e[0]), (K, hot, value)
                full += 1
    assert full > 0


@pytest.mark.parametrize("K", ALL_K)
def test_zero_and_negative_sums(core, K):
    floor = 0.25
    e, trim = core_error(core, np.zeros((4, K, 3)), 64, floor)                         # den = 3 floor > 0, se = 0
    assert not trim.any() and (e == 0).all()
    _, _, se, ry, _ = numpy_error(np.zeros((4, K, 3)), 64, floor, parts=True)
    assert (se == 0).all() and (ry + 3.0 * floor == 0.75).all()
    rng = np.random.default_rng(1)
    neg = -fill_buckets(heavy_tailed(rng, 64, (11,)), K)                               # T < 0: no trim; den <= 0: e = 0 whatever the spread
    e, trim = core_error(core, neg, 64)
    _, _, se, ry, _ = numpy_error(neg, 64, parts=True)
    assert not trim.any() and (ry + 0.03 <= 0).all() and (se > 0).all() and (e == 0).all()


def test_ties_are_ordered_by_bucket_index(core):
    """test_robust_cpu's tie: buckets 0 and 1 share the key y = 1 with different colours, one bucket is trimmed at either end.  The low winsorizing
    edge lo = y_(2) is the tied key whichever of the two is dropped — only the keys enter e, so buckets with equal keys are interchangeable —: e is
    that of the sorted keys {1, 1, 3 x5, 6, 6}, worked out by hand below, and does not change when the two swap places.  The same at the high edge."""
    K = 9
    B = np.zeros((2, K, 3))
    B[:, 0] = [4.0, 0.0, 0.0]
    B[:, 1] = [0.0, 4.0, 0.0]
    B[:, 2:7] = [4.0, 4.0, 4.0]
    B[:, 7:9] = [8.0, 8.0, 8.0]
    B[1, [0, 1]] = B[1, [1, 0]]
    e, trim = core_error(core, B, K)
    assert (trim == 1).all() and e[0] == e[1]
    # by hand: w = {1, 1, 3, 3, 3, 3, 3, 6, 6}, wbar = 29 / 9, kept = 7, Ry = 22 / 7
    w = np.float64([1, 1, 3, 3, 3, 3, 3, 6, 6])
    wbar = w.sum() / 9.0
    ss = 0.0
    for v in w:
        ss = ss + (v - wbar) * (v - wbar)
    want = (np.sqrt(ss / 8.0 / 9.0) * 9.0 / 7.0) / (22.0 / 7.0 + 0.03)
    assert e[0] == want
    assert np.array_equal(bits(e), bits(numpy_error(B, K)[0]))
    # equal keys on either side of the HIGH edge (hi = y_(8) = 6, y_(9) = 6): dropping bucket 8 or bucket 7 leaves hi as it is
    B2 = B[:1].copy()
    B2[0, 8] = [24.0, 0.0, 0.0]                                                        # the same key 6, another colour
    assert core_error(core, B2, K)[0][0] == want


@pytest.mark.parametrize("K", [3, 9, 15])
def test_scaling_buckets_and_floor_by_two_changes_no_bit(core, K):
    rng = np.random.default_rng(7)
    B = fill_buckets(heavy_tailed(rng, 64, (19, 11)), K)
    for floor in (0.01, 0.3):
        e1, t1 = core_error(core, B, 64, floor)
        e2, t2 = core_error(core, 2.0 * B, 64, 2.0 * floor)
        assert np.array_equal(bits(e1), bits(e2)) and np.array_equal(t1, t2)


# ---- calibration on the checker's per-sampling renders (the figures of DESIGN.md §4.11) ----
QW, QH, QN, QK = 48, 27, 64, 9
_sets = {}


def oracle_sets(scenes, name):
    """The buckets of samplings 1 .. 64 and of 65 .. 128, K = 9, rendered once per scene."""
    if name not in _sets:
        _, osc = scenes(name)
        x = np.stack([osc.render(QW, QH, s, s + 1)[0] for s in range(1, 2 * QN + 1)]).astype(np.float32)
        _sets[name] = (fill_buckets(x[:QN], QK), fill_buckets(x[QN:], QK))
    return _sets[name]


def rms_z(core, A, B, n, floor=0.01):
    """z = (Ry_A - Ry_B) / sqrt(se_A^2 + se_B^2) per pixel: its RMS over the pixels with a non-zero denominator, and the share of those without."""
    eA, eB = core_error(core, A, n, floor)[0], core_error(core, B, n, floor)[0]
    _, _, seA, ryA, _ = numpy_error(A, n, floor, parts=True)
    _, _, seB, ryB, _ = numpy_error(B, n, floor, parts=True)
    assert np.array_equal(bits(eA), bits(numpy_error(A, n, floor)[0])) and np.array_equal(bits(eB), bits(numpy_error(B, n, floor)[0]))
    den = np.sqrt(seA ** 2 + seB ** 2)
    ok = den > 0
    z = (ryA[ok] - ryB[ok]) / den[ok]
    return float(np.sqrt(np.mean(z ** 2))), float(1.0 - ok.mean())


@pytest.mark.parametrize("name,measured", [("rtcamp6_v3_1", 1.09), ("cornell_mini", 1.07)])
def test_calibration_on_the_oracle(core, scenes, name, measured):
    A, B = oracle_sets(scenes, name)
    rms, excluded = rms_z(core, A, B, QN)
    print("%s: RMS z %.3f (a restatement measured %.2f), pixels without a spread in either set %.4f" % (name, rms, measured, excluded))
    assert 0.6 <= rms <= 1.6                                                           # §4.7's own gate
    assert excluded <= 0.05


def test_the_winsorized_error_is_below_the_plain_spread(core, scenes):
    A, B = oracle_sets(scenes, "rtcamp6_v3_1")
    for S in (A, B):
        e_r, e_p = core_error(core, S, QN)[0].mean(), plain_spread_error(S, QN).mean()
        print("rtcamp6_v3_1 n=64 K=9: mean e_R %.4f, plain spread of the bucket means %.4f (measured 0.078 / 0.129)" % (e_r, e_p))
        assert e_r < e_p


# ---- interface ----
def test_entry_points_declared_exported_and_bound(ha):
    raw = open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    c = r"hr_ctx\s*\*\s*\w*"
    assert re.search(r"int\s+hr_robust_noise_estimate\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*hr_noise\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_read_robust_noise_image\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_read_robust_noise_trim\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_select_tiles_robust\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert int(re.search(r"#define\s+HR_ABI_VERSION\s+(\d+)", text).group(1)) == 7       # functions were added, none changed
    lib = C.CDLL(ha.HIP_LIB)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    for m in ("robust_noise_estimate", "robust_noise_image", "robust_noise_trim", "select_tiles_robust"):
        assert callable(getattr(ha.Renderer, m, None)), m
    L = ha.hip_lib()
    assert len(L.hr_robust_noise_estimate.argtypes) == 4 and len(L.hr_read_robust_noise_image.argtypes) == 3
    assert len(L.hr_read_robust_noise_trim.argtypes) == 3 and len(L.hr_select_tiles_robust.argtypes) == 4
    ffi = open(os.path.join(ROOT, "rust", "hip_ffi.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"pub fn %s\(ctx: \*mut HrCtx" % name, ffi), name
        assert "pub fn %s(" % name in integration, name


def test_robust_noise_kernel_rows():
    kv = open(os.path.join(ROOT, "hanamaru-renderer_amd", "csrc", "kernel_variants.h")).read()
    for K in ALL_K:
        assert "HR_VARIANT(robust_noise_kernel, %d, true)" % K in kv, K
    assert "select_robust_noise_kernel" in kv


def test_cli_help_lists_the_flag(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--robust-noise" in r.stdout
    assert "--robust-noise" in open(os.path.join(ROOT, "README.md")).read()


@pytest.mark.parametrize("args", [["--robust-noise"], ["--robust-noise", "--noise-target", "0.05"], ["--robust-noise", "--adaptive", "0.05"]])
def test_cli_refuses_the_flag_without_robust_before_any_device(tmp_path, args):
    r = run_cli(["-w", "64", "-h", "48", "-s", "8"] + args, tmp_path)
    assert r.returncode == 1, r.stdout
    assert "--robust-noise needs --robust" in r.stdout
    assert not (tmp_path / "result.txt").exists()
