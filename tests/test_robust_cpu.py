"""Sample buckets and the firefly-robust resolve on the CPU tier: csrc/robust_core.h compiled for the host against an independent
numpy restatement of the definition in include/hanamaru_hip.h — bit for bit: the estimator is + - x /, comparisons and one truncation in f64 without
contraction —, its corner cases, its quality on the checker's per-sampling renders, and the entry points declared, exported and bound."""
import re

import numpy as np
import pytest

import interface_checks as ic
from cli import run_cli
from post_cores import core, core_robust  # noqa: F401  (core: the g++-built harness, a fixture)
from post_numpy import bits, fill_buckets, heavy_tailed, numpy_robust, rel_sq_error
from post_quality import QH, QK, QN, QTRUTH, QW, oracle_buckets_and_truth

ENTRY_POINTS = ("hr_read_buckets", "hr_write_buckets", "hr_robust", "hr_read_robust", "hr_read_robust_trim", "hr_resolve_robust")


@pytest.mark.parametrize("K", [3, 9, 15])
def test_core_against_numpy(core, K):
    rng = np.random.default_rng(K)
    shape = (23, 37)
    for n in (0, 1, K - 1, K, K + 1, 64):
        B = fill_buckets(heavy_tailed(rng, n, shape), K) if n else np.zeros(shape + (K, 3))
        got, ref = core_robust(core, B, n), numpy_robust(B, n)
        assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(got[1], ref[1]), (K, n)
        assert np.isfinite(got[0]).all()
        assert got[1].max() <= (K - 1) // 2                                           # never more than to the median
        if n >= K and K >= 9:                                                         # (K = 3 trims only when one bucket holds everything: G >= 2 / 3)
            assert got[1].max() > 0                                                   # it trimmed somewhere
        if n < K:
            assert not got[1].any()
    # unequal per-pixel counts, 0 .. 3 K + 2: every pixel's buckets are those of its own prefix
    counts = rng.integers(0, 3 * K + 3, size=shape).astype(np.uint32)
    x = heavy_tailed(rng, int(counts.max()), shape)
    x = x * (np.arange(x.shape[0])[:, None, None, None] < counts[None, ..., None])
    B = fill_buckets(x, K)
    got, ref = core_robust(core, B, counts), numpy_robust(B, counts)
    assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(got[1], ref[1])
    assert (got[0][counts == 0] == 0).all() and not got[1][counts < K].any()
    # the plain mean below K samplings is the accumulator's mean up to the order of the f64 additions
    few = (counts > 0) & (counts < K)
    mean = x.astype(np.float64).sum(axis=0) / np.maximum(counts, 1)[..., None] / 4.0
    assert np.allclose(got[0][few], mean[few].astype(np.float32), rtol=1e-6)


@pytest.mark.parametrize("K", [3, 9, 15])
def test_equal_buckets_are_the_bucket_mean(core, K):
    """Every bucket the same (dyadic values: every step exact): G = 0, trim = 0, R = the bucket mean."""
    v = np.float64([0.75, 2.5, 0.125])
    for per in (1, 4):                                  # samplings per bucket
        B = np.broadcast_to(v * 4.0 * per, (5, K, 3)).copy()
        R, trim = core_robust(core, B, K * per)
        assert not trim.any() and np.array_equal(bits(R), bits(np.broadcast_to(v.astype(np.float32), (5, 3))))
        assert np.array_equal(bits(numpy_robust(B, K * per)[0]), bits(R))


@pytest.mark.parametrize("K", [3, 9, 15])
def test_one_hot_bucket_is_the_median_bucket(core, K):
    """One bucket holds everything: G = (K - 1) / K, trim = (K - 1) / 2, R = the median bucket's mean — here one of the empty ones."""
    for hot in range(K):
        for value in (1.0, 3.7e5, 1e-3):
            B = np.zeros((1, K, 3))
            B[0, hot] = np.float64([value, 2.0 * value, 0.5 * value])
            R, trim = core_robust(core, B, 2 * K)
            assert trim[0] == (K - 1) // 2 and (R == 0).all(), (K, hot, value)
            assert np.array_equal(bits(R), bits(numpy_robust(B, 2 * K)[0])) and numpy_robust(B, 2 * K)[1][0] == trim[0]


def test_ties_are_ordered_by_bucket_index(core):
    """Buckets 0 and 1 have the same key y and different colours; two hot buckets make the estimator trim exactly one bucket at either end: the
    one that goes at the low end is bucket 0, the one with the smaller index."""
    K = 9
    B = np.zeros((1, K, 3))
    B[0, 0] = [4.0, 0.0, 0.0]
    B[0, 1] = [0.0, 4.0, 0.0]
    B[0, 2:7] = [4.0, 4.0, 4.0]
    B[0, 7:9] = [8.0, 8.0, 8.0]
    R, trim = core_robust(core, B, K)
    assert trim[0] == 1                                                               # T = 29, Gn = 70, G = 0.268: (int)(G 9 / 2) = 1
    assert np.array_equal(bits(R), bits(numpy_robust(B, K)[0]))
    # kept: buckets 1 .. 6 and bucket 7 -> red has 5 + 2, green 1 + 5 + 2
    assert np.array_equal(R[0], np.float32([1.0, 8.0 / 7.0, 1.0]))
    # the other way round the colours swap
    B[0, [0, 1]] = B[0, [1, 0]]
    R2, _ = core_robust(core, B, K)
    assert np.array_equal(R2[0], np.float32([8.0 / 7.0, 1.0, 1.0]))
    # all keys equal: nothing is trimmed and the sum runs in index order
    B = np.zeros((1, 3, 3))
    B[0, 0], B[0, 1], B[0, 2] = [12.0, 0, 0], [0, 12.0, 0], [0, 0, 12.0]
    R, trim = core_robust(core, B, 3)
    assert trim[0] == 0 and np.array_equal(R[0], np.float32([1.0, 1.0, 1.0]))


@pytest.mark.parametrize("K", [3, 9, 15])
def test_zero_and_negative_sums_trim_nothing(core, K):
    zero = np.zeros((4, K, 3))
    R, trim = core_robust(core, zero, 64)
    assert not trim.any() and (R == 0).all()                                          # T = 0
    rng = np.random.default_rng(1)
    neg = -fill_buckets(heavy_tailed(rng, 64, (11,)), K)
    R, trim = core_robust(core, neg, 64)
    ref = numpy_robust(neg, 64)
    assert not trim.any() and (R < 0).all()                                           # T < 0: the mean of the bucket means
    assert np.array_equal(bits(R), bits(ref[0])) and np.array_equal(trim, ref[1])


def test_valid_k(core):
    assert [k for k in range(0, 20) if core.robust_k_ok(float(k))] == [3, 5, 7, 9, 11, 13, 15]
    assert not core.robust_k_ok(4.5) and not core.robust_k_ok(-3.0)


# ---- quality on the checker's per-sampling renders (the figures of DESIGN.md §4.10, with a shorter truth set) ----
@pytest.mark.parametrize("name,measured", [("rtcamp6_v3_1", 0.034), ("cornell_mini", 0.297)])
def test_quality_on_the_oracle(core, scenes, name, measured):
    _, osc = scenes(name)
    bk, acc, truth = oracle_buckets_and_truth(osc, QW, QH, QN, (QK,), QTRUTH)
    R, trim = core_robust(core, bk[QK], QN)
    assert np.array_equal(bits(R), bits(numpy_robust(bk[QK], QN)[0]))
    e_mean, e_rob = rel_sq_error(acc / np.float32(4 * QN), truth), rel_sq_error(R, truth)
    ratio = e_rob / e_mean
    print("%s: relMSE mean %.4g robust %.4g ratio %.3f (against a 4,096-sampling truth: %.3f), energy kept %.3f, pixels trimmed %.3f"
          % (name, e_mean, e_rob, ratio, measured, R.astype(np.float64).sum() / (acc.astype(np.float64).sum() / (4 * QN)), (trim > 0).mean()))
    assert ratio < 1.0


def test_a_quiet_scene_is_left_alone(core, scenes):
    _, osc = scenes("spheres")
    x = np.stack([osc.render(QW, QH, s, s + 1)[0] for s in range(1, QN + 1)]).astype(np.float32)
    _, trim = core_robust(core, fill_buckets(x, QK), QN)
    print("spheres: pixels trimmed %.4f" % (trim > 0).mean())
    assert (trim > 0).mean() <= 0.05                                                   # measured 0.008


# ---- interface ----
def test_entry_points_declared_exported_and_bound(ha):
    raw, text = ic.header_text(raw=True), ic.header_text()
    assert ic.declared(text, r"int\s+hr_read_buckets\s*\(\s*%s\s*,\s*double\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_write_buckets\s*\(\s*%s\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_robust\s*\(\s*%s\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_robust\s*\(\s*%s\s*,\s*float\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_robust_trim\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_resolve_robust\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.abi_version(text) == 7       # functions were added, none changed
    assert "448 MB" in raw                                                              # the memory figure
    debug = ic.read("include", "hanamaru_hip_debug.h")
    assert "robust" not in debug and "bucket" not in debug
    assert not ic.exported_and_bound(ha, ENTRY_POINTS)
    for m in ("read_buckets", "write_buckets", "robust", "read_robust", "read_robust_trim", "resolve_robust"):
        assert callable(getattr(ha.Renderer, m, None)), m
    L = ha.hip_lib()
    assert len(L.hr_read_buckets.argtypes) == 3 and len(L.hr_write_buckets.argtypes) == 3 and len(L.hr_robust.argtypes) == 1
    assert len(L.hr_read_robust.argtypes) == 2 and len(L.hr_read_robust_trim.argtypes) == 2 and len(L.hr_resolve_robust.argtypes) == 2
    ffi = ic.rust_ffi()
    for name in ENTRY_POINTS:
        assert re.search(r"pub fn %s\(ctx: \*mut HrCtx" % name, ffi), name


def test_bucket_kernel_rows():
    kv = ic.kernel_variants()
    for row in ("HR_VARIANT(bucket_kernel, false, false)", "HR_VARIANT(bucket_kernel, true, false)", "HR_VARIANT(bucket_kernel, true, true)"):
        assert row in kv, row
    assert "select_bucket_kernel" in kv
    # every row of the accumulate family is still there: the buckets are a kernel of their own
    for row in ("HR_VARIANT(accumulate_kernel, false, false, false)", "HR_VARIANT(accumulate_kernel, true, true, true)"):
        assert row in kv, row


def test_cli_help_lists_the_robust_flags(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0
    for flag in ("--robust K", "--robust-image FILE.png"):
        assert flag in r.stdout, flag
    readme = ic.read("README.md")
    assert "--robust K" in readme and "--robust-image" in readme


@pytest.mark.parametrize("args,word", [(["--robust", "4"], "--robust"), (["--robust", "17"], "--robust"), (["--robust", "nine"], "--robust"),
                                       (["--robust", "1"], "--robust"), (["--robust", "9", "--denoise"], "--denoise"),
                                       (["--robust", "9", "--gpus", "2"], "one device"), (["--robust", "9", "--gpu-ids", "0,1"], "one device"),
                                       (["--robust", "9", "--debug"], "--debug"), (["--robust-image", "t.png"], "--robust")])
def test_cli_refuses_before_any_device(tmp_path, args, word):
    r, left_a_result = ic.cli_refused(tmp_path, args)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not left_a_result
