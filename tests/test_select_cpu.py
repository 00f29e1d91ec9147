"""The denoiser that picks its level per pixel on the CPU tier: csrc/select_core.h compiled for the host against an independent
numpy restatement of its definition — bit for bit: + - x / and comparisons in f64 without contraction —, its consequences (S against the fixed
levels, equal halves, a planted firefly), the entry points declared, exported and bound, and the quality ordering on the checker's renders."""
import ctypes as C
import re

import numpy as np
import pytest

import guide_chain as gc
import interface_checks as ic
from cli import run_cli
from post_cores import core, core_denoise, core_select  # noqa: F401  (core: the g++-built harness, a fixture)
from post_numpy import ALL_K, EPS, bits, fill_buckets, numpy_select, rel_sq_error, sums_of, synthetic_inputs

ENTRY_POINTS = ("hr_select_default_params", "hr_denoise_select", "hr_read_selected", "hr_read_selected_levels", "hr_resolve_selected")


def synthetic(seed, w, h, K, n, firefly=0.03):
    """Consistent inputs of one render: per-sampling values whose mean follows synthetic_inputs' guides, with rare bright outliers, summed into
    the fp32 accumulator, the f64 moments and the K buckets (sampling j of a pixel into bucket j mod K).  n: one count, or per-pixel counts (a pixel
    holds its own prefix).  Returns (buckets, acc, mom, n, guides)."""
    rng = np.random.default_rng(seed)
    g = synthetic_inputs(seed, w, h, n=2)[3]
    cnt = np.full((h, w), n, dtype=np.uint32) if np.isscalar(n) else np.asarray(n, dtype=np.uint32)
    mean = 4.0 * (g[..., 0:3].astype(np.float64) + 0.05)
    N = int(cnt.max())
    x = rng.gamma(2.0, 0.5, size=(N, h, w, 3)) * mean
    x = np.where(rng.random((N, h, w, 1)) < firefly, x * 200.0, x).astype(np.float32)
    x = x * (np.arange(N)[:, None, None, None] < cnt[None, ..., None])
    acc, mom = sums_of(x)
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
def test_s_has_the_bits_of_the_fixed_level(core, K, dem):
    w, h, levels = 37, 19, 5
    for n in (2 * K + 1, unequal_counts(K, w, h, K)):
        B, acc, mom, n, g = synthetic(200 + K, w, h, K, n)
        S, L = core_select(core, B, acc, mom, n, g, levels=levels, demodulate=dem)
        seen = 0
        for lev in range(levels + 1):
            # (hr_denoise(levels = 0) drops the demodulation, a pixel that picks level 0 under it is (float)((C / a) a): the float of C unless C
            # lies within two f64 ulps of the boundary between two floats, which none of these does)
            D = core_denoise(core, acc, mom, n, g, levels=lev, demodulate=dem)
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
    g = synthetic_inputs(3, w, h)[3]
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
    text = ic.header_text()
    assert ic.declared(text, r"typedef\s+struct\s+\w*\s*\{\s*uint32_t\s+smooth\s*;\s*uint32_t\s+reserved\s*;\s*\}\s*hr_select_params\s*;")
    assert ic.declared(text, r"int\s+hr_select_default_params\s*\(\s*hr_select_params\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_denoise_select\s*\(\s*%s\s*,\s*const\s+hr_denoise_params\s*\*\s*\w+\s*,\s*const\s+hr_select_params\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_selected\s*\(\s*%s\s*,\s*float\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_selected_levels\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_resolve_selected\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.abi_version(text) == 7       # functions were added, none changed
    ffi, integration = ic.rust_ffi(), ic.read("INTEGRATION.md")
    arity = {"hr_select_default_params": 1, "hr_denoise_select": 3}
    for fn in ENTRY_POINTS:
        assert not ic.exported_and_bound(ha, (fn,)), fn
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
    kv, pk = ic.kernel_variants(), ic.read("hanamaru-renderer_amd", "csrc", "post_kernels.h")
    for K in ALL_K:
        assert "HR_VARIANT(select_init_kernel, %d)" % K in kv, K
    assert "select_select_init_kernel" in kv
    for kernel in ("select_init_kernel", "atrous3_kernel", "select_pick_kernel", "select_smooth_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, pk), kernel


def test_cli_help_lists_the_flags(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0
    readme = ic.read("README.md")
    for flag in ("--denoise-auto", "--select-smooth", "--level-image"):
        assert flag in r.stdout and flag in readme, flag
    tools = ic.read("tools", "README.md")
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
    r, left_a_result = ic.cli_refused(tmp_path, args)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not left_a_result


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


def quality_ratios(core, x, guides, truth, K, smooth=0):
    """(fixed-levels-4 / raw, select / raw): relative squared errors against the truth over the raw mean's"""
    n = x.shape[0]
    acc, mom = sums_of(x)
    e_raw = rel_sq_error(acc / np.float32(4 * n), truth)
    e_fixed = rel_sq_error(core_denoise(core, acc, mom, n, guides), truth)
    e_sel = rel_sq_error(core_select(core, fill_buckets(x, K), acc, mom, n, guides, smooth=smooth)[0], truth)
    return e_fixed / e_raw, e_sel / e_raw


def test_quality_on_the_oracle(core, orc, scenes):
    """96x54, K = 9, default parameters, smooth 0, truth samplings 100001 .. 101024 (half of tools/select_quality.py's 2,048).  Asserted on
    rtcamp6_v3_1 with first-hit guides, the case of DESIGN.md §4.9's finding, at 16 and at 64 samplings: the selection's error is below the
    whole-buffer filter's at levels = 4.  A host prototype measured fixed -> select 0.52 -> 0.31 (n = 16) and 1.95 -> 1.03 (n = 64), a gap of
    1.7 - 1.9 x.  The guide_bounces 2 rows are printed.  Measured with this truth: first-hit guides 0.351 -> 0.216 (n = 16) and 0.905 -> 0.520
    (n = 64); guide_bounces 2: 0.234 -> 0.213 and 0.364 -> 0.324."""
    x, guides, truth = oracle_render(orc, scenes, "rtcamp6_v3_1")
    for bounces in (0, 2):
        for n in (16, 64):
            fixed, sel = quality_ratios(core, x[:n], guides[bounces], truth, QK)
            print("rtcamp6_v3_1 guide_bounces=%d n=%d K=%d: fixed-4 / raw %.3f  select / raw %.3f" % (bounces, n, QK, fixed, sel))
            if bounces == 0:
                assert sel < fixed, (n, fixed, sel)
