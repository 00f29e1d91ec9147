"""The restored robust resolve R'  on the CPU tier: robust_pixel_excess_k / restore_norm / restore_gather / restore_image of
csrc/restore_core.h compiled for the host against an independent numpy restatement of their definition — bit for bit: + - x / max and comparisons
in f64 without contraction —, the properties of the excess X, exact impulse cases, the conservation of the spread energy within a bound derived
from the operation count, the quality figures on the checker's per-sampling renders, and the entry points declared, exported and bound."""
import math
import re

import numpy as np
import pytest

import interface_checks as ic
from cli import run_cli
from post_cores import core, core_excess, core_r, core_restore, core_spread  # noqa: F401  (core: the g++-built harness, a fixture)
from post_numpy import ALL_K
from post_numpy import RESTORE_DEFAULTS as DEFAULTS
from post_numpy import bits, flat_guides, heavy_tailed, numpy_excess, numpy_restore, numpy_spread, synthetic_buckets, synthetic_inputs, tie_pixel
from post_quality import SHORT_N as QN
from post_quality import oracle_short_render, restore_figures

U = 2.0 ** -53


# ---- 1. the header against numpy ----
@pytest.mark.parametrize("K", ALL_K)
def test_excess_against_numpy(core, K):
    shape = (23, 37)
    trimmed = 0
    for n in (K, 2 * K - 1, 64):
        B = synthetic_buckets(200 + K, K, shape, n)                                # the planted cases: equal buckets, one hot bucket, zeros,
        got, ref = core_excess(core, B, n), numpy_excess(B, n)                        # negative sums, tiny values, equal keys straddling the trim
        assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(got[1], ref[1]), (K, n)
        assert np.isfinite(got[0]).all()
        trimmed += int((got[0][..., 3:6] > 0).sum())
    assert trimmed > 0
    counts = np.random.default_rng(K).integers(K, 3 * K + 3, size=shape).astype(np.uint32)
    B = synthetic_buckets(300 + K, K, shape, counts)
    got, ref = core_excess(core, B, counts), numpy_excess(B, counts)
    assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(got[1], ref[1])
    for X in (tie_pixel()[None], tie_pixel(True)[None]) if K == 9 else ():
        assert np.array_equal(bits(core_excess(core, X, 9)[0]), bits(numpy_excess(X, 9)[0]))


# ---- 2. properties of X and C ----
@pytest.mark.parametrize("K", ALL_K)
def test_c_is_r_and_x_is_zero_without_a_trim(core, K):
    shape = (23, 37)
    counts = np.random.default_rng(K).integers(0, 3 * K + 3, size=shape).astype(np.uint32)
    counts[0, :4] = [0, 1, K - 1, K]
    for n in (K, 2 * K - 1, 64, counts):
        B = synthetic_buckets(400 + K, K, shape, n)
        cx, trim = core_excess(core, B, n)
        R, tr = core_r(core, B, n)
        assert np.array_equal(bits(cx[..., 0:3].astype(np.float32)), bits(R)) and np.array_equal(trim, tr), K   # n = 0 and n < K among the counts
        assert (cx[..., 3:6][trim == 0] == 0).all() and not np.signbit(cx[..., 3:6]).any()
        assert (cx[..., 3:6] >= 0).all()
        assert (trim > 0).any()


@pytest.mark.parametrize("K", ALL_K)
def test_one_hot_bucket_in_one_channel(core, K):
    """Every bucket mean (b, b, b) but one, whose channel c is b + v: the keys put it last and the Gini coefficient trims it — G K / 2 is
    (K - 1) / 2 with b = 0 and (K - 1) / 2 x v / (3 K b + v) otherwise, at least 1 for b = 1, v >= 64 from K = 5 (with K = 3 it stays below 1: no
    trim, so b = 1 is left out there).  The highest kept bucket is (b, b, b) and the other trimmed buckets hold exactly that:
    X_c = ((b + v) - b) / K, the other channels 0, C = b — exactly."""
    per = 2
    for b in (0.0, 1.0) if K > 3 else (0.0,):
        for hot in (0, K // 2, K - 1):
            for c in range(3):
                for v in (64.0, 3.0e5):
                    B = np.full((1, K, 3), 4.0 * per * b)
                    B[0, hot, c] = 4.0 * per * (b + v)
                    cx, trim = core_excess(core, B, K * per)
                    assert trim[0] >= 1, (K, b, hot, c, v)
                    want = np.zeros(3)
                    want[c] = ((b + v) - b) / float(K)
                    assert np.array_equal(bits(cx[0, 3:6]), bits(want)), (K, b, hot, c, v)
                    assert np.array_equal(bits(cx[0, 0:3]), bits(np.full(3, b)))


# ---- 3. the spread and the whole thing against numpy ----
SHAPES = [(37, 23), (1, 1), (5, 1), (1, 5)]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("K", [3, 9, 15])
def test_restore_against_numpy(core, w, h, K):
    g = synthetic_inputs(11, w, h)[3]
    counts = np.random.default_rng(w * h + K).integers(K, 3 * K + 3, size=(h, w)).astype(np.uint32)
    D = np.random.default_rng(K).gamma(2.0, 0.5, size=(h, w, 3)).astype(np.float32)
    for n in (2 * K + 1, counts):
        B = synthetic_buckets(800 + K, K, (h, w), n)
        for levels in (0, 1, 5):
            for base in (0, 1):
                got, x = core_restore(core, B, n, g, D=D if base else None, want_x=True, levels=levels, base=base)
                ref, x_ref = numpy_restore(B, n, g, D=D if base else None, levels=levels)
                assert np.array_equal(bits(got), bits(ref)) and np.array_equal(bits(x), bits(x_ref)), (w, h, K, levels, base)
                assert np.isfinite(got).all() and (x >= 0).all()
        if (w, h) == (37, 23):
            x0 = core_restore(core, B, n, g, want_x=True, levels=0)[1]
            assert (x0 > 0).any() and not np.array_equal(x0, core_restore(core, B, n, g, want_x=True, levels=1)[1])


# ---- 4. exact impulse cases ----
def test_an_interior_impulse_is_the_tap_kernel(core):
    """Constant guides: every K(x) is 1, N = (3/8 + 2/4 + 2/16)^2 = 1 exactly, S = X, and one level hands k[|i|] k[|j|] to each of the 25 taps."""
    w, h, px, py = 11, 9, 5, 4
    X = np.zeros((h, w, 3))
    X[py, px] = [1.0, 2.0, 0.5]
    out = core_spread(core, X, flat_guides(w, h), levels=1)
    k = (0.375, 0.25, 0.0625)
    want = np.zeros((h, w, 3))
    for j in range(-2, 3):
        for i in range(-2, 3):
            want[py + j, px + i] = np.float64([1.0, 2.0, 0.5]) * (k[abs(i)] * k[abs(j)])
    assert np.array_equal(bits(out), bits(want))
    assert np.array_equal(bits(numpy_spread(X, flat_guides(w, h), levels=1)), bits(want))


def test_a_corner_impulse_stays_in_the_frame(core):
    """The same impulse at the corner pixel: 9 taps are inside, N = (3/8 + 1/4 + 1/16)^2 = (11/16)^2, nothing leaves the frame."""
    w, h = 11, 9
    X = np.zeros((h, w, 3))
    X[0, 0] = 1.0
    out = core_spread(core, X, flat_guides(w, h), levels=1)
    k = (0.375, 0.25, 0.0625)
    N = 0.0
    for j in range(3):
        for i in range(3):
            N = N + k[i] * k[j]
    assert N == (11.0 / 16.0) ** 2
    for j in range(h):
        for i in range(w):
            want = k[i] * k[j] * (1.0 / N) if i < 3 and j < 3 else 0.0
            assert (out[j, i] == want).all(), (i, j)
    for c in range(3):
        assert abs(math.fsum(out[..., c].ravel()) - 1.0) <= conservation_bound(1) * 1.0


# ---- 5. conservation ----
def conservation_bound(levels):
    """Relative, per channel.  In real numbers sum_q X'_q = sum_p X_p sum_q w(p, q) / N_p = sum_p X_p, and w(q, p) computed at q IS w(p, q) computed
    at p, so the rounding of the weights themselves cancels.  What does not: an output X'_q is 25 products fl(w S_p) added with 24 additions, S_p one
    quotient, N_p 24 additions — every term is non-negative, so each of these 1 + 1 + 24 + 24 = 50 roundings moves a term's share of the sum by at
    most one u = 2^-53, relative: (1 + u)^50 - 1 < 51 u per level.  math.fsum rounds each of the two sums once more (half a u each).  52 u < 64 u per
    level; the levels multiply: (1 + 64 u)^L - 1 <= 64 L u (1 + 320 u), and the last factor is below the slack of 12 u per level."""
    return 64.0 * levels * U


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_the_spread_conserves_the_excess(core, levels):
    w, h = 37, 23
    g = synthetic_inputs(11, w, h)[3]
    rng = np.random.default_rng(levels)
    X = heavy_tailed(rng, 1, (h, w))[0].astype(np.float64) * (rng.random((h, w, 1)) < 0.2)
    out = core_spread(core, X, g, levels=levels)
    assert (out >= 0).all() and not np.array_equal(out, X)
    for c in range(3):
        a, b = math.fsum(out[..., c].ravel()), math.fsum(X[..., c].ravel())
        print("levels %d channel %d: sum X_L / sum X - 1 = %.3g u (bound %g u)" % (levels, c, (a / b - 1.0) / U, conservation_bound(levels) / U))
        assert b > 0 and abs(a - b) <= conservation_bound(levels) * b


def test_an_edge_beyond_sigma_keeps_each_side_its_own(core):
    """Two halves whose normals differ by |dN|^2 = 2 > sigma_n^2: K(x_n) = 0 across the edge.  Each half conserves its own sum within the bound, and
    changing X in the right half changes no bit of the left half's output."""
    w, h, levels = 24, 9, 4
    g = flat_guides(w, h)
    g[:, w // 2:, 3:6] = [1.0, 0.0, 0.0]
    rng = np.random.default_rng(3)
    X = rng.gamma(2.0, 0.5, size=(h, w, 3)) * (rng.random((h, w, 1)) < 0.3)
    out = core_spread(core, X, g, levels=levels)
    for half in (np.s_[:, :w // 2], np.s_[:, w // 2:]):
        for c in range(3):
            a, b = math.fsum(out[half][..., c].ravel()), math.fsum(X[half][..., c].ravel())
            assert b > 0 and abs(a - b) <= conservation_bound(levels) * b
    X2 = X.copy()
    X2[:, w // 2:] = X2[:, w // 2:] * 3.0 + 1.0
    out2 = core_spread(core, X2, g, levels=levels)
    assert np.array_equal(bits(out2[:, :w // 2]), bits(out[:, :w // 2])) and not np.array_equal(out2[:, w // 2:], out[:, w // 2:])


# ---- 6. quality on the checker's per-sampling renders (the figures of DESIGN.md §4.14, with half the truth set of tools/restore_quality.py) ----
@pytest.mark.parametrize("name", ["rtcamp6_v3_1", "cornell_mini"])
def test_quality_on_the_oracle(core, orc, scenes, name):
    """96x54, 16 samplings, guide_bounces 2, default parameters, truth samplings 100001 .. 100512 (the renders test_robust_denoise_cpu.py shares).
    Asserted on rtcamp6_v3_1 at K = 5: R' is closer to the energy of the plain mean than R is, and its error is below the plain mean's.  Everything
    else is printed: R' / R is above 1 — restoring the energy costs error —, and on cornell_mini, which loses under 1 % of its energy, nothing is
    asserted.  Measured, K = 5: rtcamp6_v3_1 sum R / sum M 0.819, sum R' / sum M 0.999, R / mean 0.109, R' / mean 0.238, R' (base DR) / mean 0.223,
    R' / R 2.19; cornell_mini 0.997, 1.000, 0.586, 0.784, 0.663, 1.34.  K = 9: rtcamp6_v3_1 0.724, 1.004, 0.072, 0.246, 0.259, 3.43; cornell_mini
    0.992, 1.000, 0.445, 0.994, 1.034, 2.23 (R' on DR there is WORSE than the plain mean)."""
    x, _, _, guides, truth = oracle_short_render(orc, scenes, name)
    for K in (5, 9):
        f = restore_figures(core, x, guides, truth, K)
        print("%s n=%d K=%d: " % (name, QN, K) + "  ".join("%s %.3f" % kv for kv in f.items()))
        if name == "rtcamp6_v3_1" and K == 5:
            assert abs(f["sumR'/sumM"] - 1.0) < abs(f["sumR/sumM"] - 1.0)
            assert f["R'/mean"] < 1.0


# ---- 7. plumbing ----
def test_entry_points_declared_exported_and_bound(ha):
    text = ic.header_text()
    assert ic.declared(text, r"typedef\s+struct\s+hr_restore_params\s*\{\s*uint32_t\s+levels\s*;\s*uint32_t\s+base\s*;\s*double\s+sigma_n\s*,\s*sigma_a\s*,\s*sigma_z\s*;\s*\}\s*hr_restore_params\s*;")
    assert ic.declared(text, r"int\s+hr_restore_default_params\s*\(\s*hr_restore_params\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_robust_restore\s*\(\s*%s\s*,\s*const\s+hr_restore_params\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_restored\s*\(\s*%s\s*,\s*float\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_resolve_restored\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.abi_version(text) == 7       # functions were added, none changed
    ffi, integration = ic.rust_ffi(), ic.read("INTEGRATION.md")
    for fn in ("hr_restore_default_params", "hr_robust_restore", "hr_read_restored", "hr_resolve_restored"):
        assert not ic.exported_and_bound(ha, (fn,)), fn
        assert len(getattr(ha.hip_lib(), fn).argtypes) == (1 if fn == "hr_restore_default_params" else 2)
        assert "pub fn %s(" % fn in ffi and "pub fn %s(" % fn in integration, fn
    assert "size_of::<HrRestoreParams>() == 32" in ffi
    for method in ("robust_restore", "read_restored", "resolve_restored"):
        assert callable(getattr(ha.Renderer, method, None)), method
    p = ha.restore_default_params()                                                     # needs no device
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    assert ha.hip_lib().hr_restore_default_params(None) == -1


def test_kernel_rows():
    kv, pk = ic.kernel_variants(), ic.read("hanamaru-renderer_amd", "csrc", "post_kernels.h")
    for K in ALL_K:
        assert "HR_VARIANT(restore_init_kernel, %d)" % K in kv, K
    assert "select_restore_init_kernel" in kv
    for kernel in ("restore_init_kernel", "spread_norm_kernel", "spread_gather_kernel", "restore_final_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, pk), kernel


def test_cli_help_lists_the_flags(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0
    readme = ic.read("README.md")
    for flag in ("--robust-restore", "--restore-levels"):
        assert flag in r.stdout and flag in readme, flag
    tools = ic.read("tools", "README.md")
    assert "restore_quality.py" in tools and "restore_rate.py" in tools


@pytest.mark.parametrize("args,word", [(["--robust-restore"], "--robust-restore needs --robust"),
                                       (["--robust-restore", "--restore-levels", "2"], "--robust-restore needs --robust"),
                                       (["--robust", "5", "--restore-levels", "2"], "--restore-levels needs --robust-restore"),
                                       (["--robust", "5", "--robust-restore", "--restore-levels", "6"], "--restore-levels"),
                                       (["--robust", "5", "--robust-restore", "--gpus", "2"], "one device"),
                                       (["--robust", "5", "--robust-restore", "--denoise"], "--denoise")])
def test_cli_refuses_before_any_device(tmp_path, args, word):
    r, left_a_result = ic.cli_refused(tmp_path, args)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not left_a_result
