"""The error estimate of hr_denoise_select's image on the CPU tier: csrc/select_noise_core.h compiled for the host against an
independent numpy restatement of its definition — M bit for bit, S and L equal to select_image's —, the identities that need no tolerance, e_S and
the tile rule on the host, the entry points declared, exported and bound, and the CLI's refusals."""
import ctypes as C
import re

import numpy as np
import pytest

import interface_checks as ic
from cli import run_cli
from post_cores import core, core_select  # noqa: F401  (core: the g++-built harness, a fixture)
from post_numpy import EPS, bits, fill_buckets, initial_state, sums_of, synthetic_inputs
from select_noise_cores import core_errors, core_select_noise, core_tile_rule, noise_core  # noqa: F401  (noise_core: a fixture)
from select_noise_numpy import numpy_error, numpy_select_noise, numpy_tile_rule, synthetic

ENTRY_POINTS = ("hr_selected_noise_estimate", "hr_read_selected_noise_image", "hr_read_selected_mse", "hr_select_tiles_selected")


def mixed_counts(seed, w, h):
    """per-pixel counts 2 .. 64, with 2 and 64 present"""
    cnt = np.random.default_rng(seed).integers(2, 65, size=(h, w)).astype(np.uint32)
    cnt.reshape(-1)[:2] = [2, 64]
    return cnt


# ---- 1. the core against numpy, bit for bit ----
# 13x7: the level-3 taps (step 4, reach 8) leave the image; 37x19: ragged 4x4 tiles, no multiple of anything
@pytest.mark.parametrize("w,h", [(13, 7), (37, 19)])
@pytest.mark.parametrize("K", [3, 9, 15])
def test_core_against_numpy(core, noise_core, w, h, K):
    picked, positive_bias = set(), 0
    for n in (2, K - 1, 64, mixed_counts(w * h + K, w, h)):      # n = 2: n_A = n_B = 1; n = K - 1: the last bucket is empty
        B, acc, mom, n, g = synthetic(100 + K, w, h, K, n)
        for levels in (0, 1, 3):
            for dem in (0, 1):
                for smooth in (0, 2):
                    where = (w, h, K, n if np.isscalar(n) else "mixed", levels, dem, smooth)
                    S, L, M = core_select_noise(noise_core, B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)
                    rS, rL, rM, per_level = numpy_select_noise(B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)
                    assert np.array_equal(bits(M), bits(rM)), where
                    assert np.array_equal(L, rL) and np.array_equal(bits(S), bits(rS)), where
                    sS, sL = core_select(core, B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)   # select_image's bits
                    assert np.array_equal(L, sL) and np.array_equal(bits(S), bits(sS)), where
                    assert np.isfinite(M).all() and (M >= 0.0).all(), where
                    yy, xx = np.mgrid[0:h, 0:w]
                    assert np.array_equal(bits(M), bits(per_level[L, yy, xx])), where                       # M = mse_L
                    picked |= set(np.unique(L).tolist())
                    positive_bias += int((M > 0.0).sum())
    assert positive_bias > 0
    if (w, h) == (37, 19):
        assert len(picked) >= 3, picked


# ---- 2. identities without a tolerance ----
def _equal_halves(w, h, spread):
    """K = 3, n = 12, every bucket 16 r(p), r a multiple of 1 / 8: A0 = 32 r / 8 / 4 and B0 = 16 r / 4 / 4 are both r exactly, every product below
    is exact.  spread: the second moment over that of twelve equal samplings (1: no variance at all)."""
    K, n = 3, 12
    r = np.random.default_rng(17).integers(1, 64, size=(h, w, 3)).astype(np.float64) / 8.0
    B = np.repeat((16.0 * r)[:, :, None, :], K, axis=2)
    acc = (48.0 * r).astype(np.float32)
    mom = np.concatenate([48.0 * r, spread * n * (4.0 * r) ** 2], axis=-1)
    return B, acc, mom, n, synthetic_inputs(3, w, h)[3]


@pytest.mark.parametrize("smooth", [0, 2])
def test_equal_samplings_give_zero(noise_core, smooth):
    B, acc, mom, n, g = _equal_halves(21, 11, 1.0)
    for levels in (0, 3):
        for dem in (0, 1):
            S, L, M = core_select_noise(noise_core, B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)
            assert not L.any() and not M.any(), (levels, dem)                     # (+0.0 everywhere: not a bit is set)
            assert np.array_equal(bits(M), bits(numpy_select_noise(B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)[2]))


@pytest.mark.parametrize("smooth", [0, 2])
def test_equal_halves_give_the_propagated_variance_of_level_zero(noise_core, smooth):
    """The halves agree in every pixel but the moments say the samplings vary: e_0 = 0 keeps L = 0; m_0 = -(va0 + vb0) / 2 is negative, so is
    m^_0 - vh_0, the clamp leaves M = vw_0 = sum_c k_c V_W,c — in the stated order: V / a^2 first, then times k, then (r + g) + b."""
    w, h = 21, 11
    B, acc, mom, n, g = _equal_halves(w, h, 1.5)
    V0 = initial_state(acc, mom, np.full((h, w), n, dtype=np.uint32))[0][..., 3:6]
    assert (V0 > 0.0).all()
    a = g[..., 0:3].astype(np.float64) + EPS
    for levels in (0, 4):
        for dem in (0, 1):
            S, L, M = core_select_noise(noise_core, B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)
            v = (V0 / (a * a)) * (a * a) if dem and levels else V0
            assert not L.any()
            assert np.array_equal(bits(M), bits((v[..., 0] + v[..., 1]) + v[..., 2])), (levels, dem)


@pytest.mark.parametrize("smooth", [0, 2])
def test_a_nan_stays_within_reach(noise_core, smooth):
    """A NaN in one bucket of one pixel: level l of the filter carries it 2 (2^l - 1) pixels, the smoothing of the error planes 2 (2^smooth - 1)
    further.  Every pixel beyond both has the bits it has without the NaN, in M, S and L."""
    w, h, K, levels = 41, 21, 3, 2
    px, py, reach = 20, 10, 2 * ((1 << levels) - 1) + 2 * ((1 << smooth) - 1)
    B, acc, mom, n, g = synthetic(7, w, h, K, 12)
    hot = B.copy()
    hot[py, px, 1, 0] = np.nan
    yy, xx = np.mgrid[0:h, 0:w]
    far = (np.abs(xx - px) > reach) | (np.abs(yy - py) > reach)
    assert far.any() and not far.all()
    for dem in (0, 1):
        S, L, M = core_select_noise(noise_core, B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)
        hS, hL, hM = core_select_noise(noise_core, hot, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)
        assert np.array_equal(bits(M[far]), bits(hM[far])) and np.array_equal(bits(S[far]), bits(hS[far])) and np.array_equal(L[far], hL[far])
        rM = numpy_select_noise(hot, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)[2]
        assert np.array_equal(bits(hM), bits(rM))                                 # (where the NaN does reach, both say the same)


# ---- 3. e_S and the tile rule ----
@pytest.mark.parametrize("w,h", [(13, 7), (37, 19)])
def test_error_and_tile_rule_on_the_host(noise_core, w, h):
    K = 9
    B, acc, mom, n, g = synthetic(55, w, h, K, mixed_counts(3, w, h))
    S, L, M = core_select_noise(noise_core, B, acc, mom, n, g, smooth=2)
    M[0, 0] = 0.0
    M[1, 1] = np.nan                                                               # a NaN is never above a threshold
    S2 = S.copy()
    S2[2, 2] = -1.0                                                                # a denominator that is not positive: e_S = 0
    for floor in (0.01, 0.25):
        e = core_errors(noise_core, M, S2, floor)
        ref = numpy_error(M, S2, floor)
        assert np.array_equal(bits(e), bits(ref))                                  # (the square root is correctly rounded on both sides)
        assert e[0, 0] == 0.0 and e[2, 2] == 0.0 and np.isnan(e[1, 1])
        for threshold in (0.0, float(np.nanmedian(ref)), float(np.nanmax(ref))):
            mask = core_tile_rule(noise_core, e, threshold)
            assert np.array_equal(mask, numpy_tile_rule(ref, threshold)), (floor, threshold)
        assert 0 < core_tile_rule(noise_core, e, float(np.nanmedian(ref))).sum() < mask.size
        assert not core_tile_rule(noise_core, e, float(np.nanmax(ref))).any()


# ---- 4. plumbing ----
def test_entry_points_declared_exported_and_bound(ha):
    text = ic.header_text()
    sel = r"\s*%s\s*,\s*const\s+hr_denoise_params\s*\*\s*\w+\s*,\s*const\s+hr_select_params\s*\*\s*\w+\s*,"
    assert ic.declared(text, r"int\s+hr_selected_noise_estimate\s*\(" + sel + r"\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*hr_noise\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_selected_noise_image\s*\(" + sel + r"\s*double\s+\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_selected_mse\s*\(" + sel + r"\s*double\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_select_tiles_selected\s*\(" + sel + r"\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.abi_version(text) == 7       # functions were added, none changed
    assert ha.hip_lib().hr_abi_version() == 7
    assert C.sizeof(ha.Stats) == 368
    ffi, integration = ic.rust_ffi(), ic.read("INTEGRATION.md")
    arity = {"hr_selected_noise_estimate": 6, "hr_read_selected_noise_image": 5, "hr_read_selected_mse": 4, "hr_select_tiles_selected": 6}
    for fn in ENTRY_POINTS:
        assert not ic.exported_and_bound(ha, (fn,)), fn
        assert len(getattr(ha.hip_lib(), fn).argtypes) == arity[fn]
        assert "pub fn %s(" % fn in ffi and fn in integration, fn
    for method in ("selected_noise_estimate", "selected_noise_image", "selected_mse", "select_tiles_selected"):
        assert callable(getattr(ha.Renderer, method, None)), method
    for fn in ENTRY_POINTS:                                                        # a null context is refused, not dereferenced
        args = [None] * (arity[fn] - 1)
        if fn != "hr_read_selected_mse":
            args[2] = 0.01
        if arity[fn] == 6:
            args[3] = 0.05
        assert getattr(ha.hip_lib(), fn)(None, *args) == -1, fn


def test_kernels_and_documents():
    pk = ic.read("hanamaru-renderer_amd", "csrc", "post_kernels.h")
    for kernel in ("select_noise_kernel", "select_noise_error_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, pk), kernel
    design = ic.read("DESIGN.md")
    assert "4.17" in design
    for profile in ("select_noise_quality.txt", "select_noise_rate.txt", "select_noise_kernel_resources.txt"):
        assert ic.read("profiles", profile).strip() and profile in design, profile
    tools = ic.read("tools", "README.md")
    assert "select_noise_quality.py" in tools and "select_noise_rate.py" in tools


def test_cli_help_lists_the_flag(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0
    assert "--auto-noise" in r.stdout and "--auto-noise" in ic.read("README.md")


@pytest.mark.parametrize("args,word", [(["--auto-noise", "--noise-target", "0.05"], "--auto-noise needs --denoise-auto"),
                                       (["--denoise-auto", "9", "--auto-noise", "--robust-noise", "--noise-target", "0.05"], "--robust-noise"),
                                       (["--denoise-auto", "9", "--auto-noise", "--resume", "state.bin"], "--resume"),
                                       (["--denoise-auto", "9", "--auto-noise", "--gpus", "2"], "one device")])
def test_cli_refuses_before_any_device(tmp_path, args, word):
    r, left_a_result = ic.cli_refused(tmp_path, args)
    assert r.returncode == 1, r.stdout
    assert "--auto-noise" in r.stdout and word in r.stdout, r.stdout
    assert not left_a_result
