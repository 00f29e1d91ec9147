"""The robust noise estimate on the CPU tier: robust_pixel_error of csrc/robust_core.h compiled for the host against an independent
numpy restatement of its definition — bit for bit: + - x /, comparisons, one truncation and one correctly rounded sqrt in f64 without contraction —,
its corner cases, its calibration on the checker's per-sampling renders, and the entry points declared, exported and bound."""
import numpy as np
import pytest

import interface_checks as ic
from cli import run_cli
from post_cores import core, core_error, core_robust  # noqa: F401  (core: the g++-built harness, a fixture)
from post_numpy import ALL_K, bits, fill_buckets, heavy_tailed, numpy_error
from post_quality import QN, oracle_sets, plain_spread_error, rms_z

ENTRY_POINTS = ("hr_robust_noise_estimate", "hr_read_robust_noise_image", "hr_read_robust_noise_trim", "hr_select_tiles_robust")


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
    text = ic.header_text()
    assert ic.declared(text, r"int\s+hr_robust_noise_estimate\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*hr_noise\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_robust_noise_image\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_robust_noise_trim\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_select_tiles_robust\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.abi_version(text) == 7       # functions were added, none changed
    assert not ic.exported_and_bound(ha, ENTRY_POINTS)
    for m in ("robust_noise_estimate", "robust_noise_image", "robust_noise_trim", "select_tiles_robust"):
        assert callable(getattr(ha.Renderer, m, None)), m
    L = ha.hip_lib()
    assert len(L.hr_robust_noise_estimate.argtypes) == 4 and len(L.hr_read_robust_noise_image.argtypes) == 3
    assert len(L.hr_read_robust_noise_trim.argtypes) == 3 and len(L.hr_select_tiles_robust.argtypes) == 4
    ffi, integration = ic.rust_ffi(), ic.read("INTEGRATION.md")
    for name in ENTRY_POINTS:
        assert "pub fn %s(ctx: *mut HrCtx" % name in ffi, name
        assert "pub fn %s(" % name in integration, name


def test_robust_noise_kernel_rows():
    kv = ic.kernel_variants()
    for K in ALL_K:
        assert "HR_VARIANT(robust_noise_kernel, %d, true)" % K in kv, K
    assert "select_robust_noise_kernel" in kv


def test_cli_help_lists_the_flag(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--robust-noise" in r.stdout
    assert "--robust-noise" in ic.read("README.md")


@pytest.mark.parametrize("args", [["--robust-noise"], ["--robust-noise", "--noise-target", "0.05"], ["--robust-noise", "--adaptive", "0.05"]])
def test_cli_refuses_the_flag_without_robust_before_any_device(tmp_path, args):
    r, left_a_result = ic.cli_refused(tmp_path, args)
    assert r.returncode == 1, r.stdout
    assert "--robust-noise needs --robust" in r.stdout
    assert not left_a_result
