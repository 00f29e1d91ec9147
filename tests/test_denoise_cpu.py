"""The à-trous denoiser on the CPU tier: csrc/denoise_core.h compiled for the host against an independent numpy restatement of
the formulas in include/hanamaru_hip.h — bit for bit: the filter is + - x / max in f64 without contraction —, its invariants, and the entry
points declared, exported and bound."""
import ctypes as C
import re

import numpy as np
import pytest

import interface_checks as ic
from cli import run_cli
from post_cores import core, core_denoise, core_one_level  # noqa: F401  (core: the g++-built harness, a fixture)
from post_numpy import DENOISE_DEFAULTS as DEFAULTS
from post_numpy import bits, numpy_denoise, synthetic_inputs, ulp_distance

ENTRY_POINTS = ("hr_denoise_default_params", "hr_render_guides", "hr_read_guides", "hr_write_guides", "hr_denoise", "hr_read_denoised", "hr_resolve_denoised")

# (w, h, levels): reach 32 beyond either edge distance (skipped taps dominate), a single pixel, a row and a column
SHAPES = [(37, 23, 5), (1, 1, 5), (5, 1, 3), (1, 5, 3), (37, 23, 1)]


@pytest.mark.parametrize("w,h,levels", SHAPES)
@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("unequal", [False, True])
def test_core_against_numpy(core, w, h, levels, demodulate, unequal):
    counts = np.random.default_rng(3).integers(2, 20, size=(h, w)) if unequal else None
    acc, mom, n, g = synthetic_inputs(7, w, h, counts)
    got, st = core_denoise(core, acc, mom, n, g, want_state=True, levels=levels, demodulate=demodulate)
    ref, st_ref = numpy_denoise(acc, mom, n, g, want_state=True, levels=levels, demodulate=demodulate)
    assert np.isfinite(got).all()
    assert np.array_equal(bits(st), bits(st_ref))
    assert np.array_equal(bits(got), bits(ref))
    if (w, h) == (37, 23) and levels == 5:
        raw = core_denoise(core, acc, mom, n, g, levels=0)
        assert not np.array_equal(bits(got), bits(raw))                       # it filtered


def test_levels_zero_is_the_mean_rounded_once(core):
    counts = np.random.default_rng(5).integers(2, 300, size=(23, 37))
    acc, mom, n, g = synthetic_inputs(11, 37, 23, counts)
    scale = np.float32(1.0) / (n * np.uint32(4)).astype(np.float32)
    want = (acc.astype(np.float64) * scale.astype(np.float64)[..., None]).astype(np.float32)
    assert np.array_equal(bits(want), bits(acc * scale[..., None]))              # the resolve's own fp32 product
    for dem in (0, 1):
        assert np.array_equal(bits(core_denoise(core, acc, mom, n, g, levels=0, demodulate=dem)), bits(want))
    one = synthetic_inputs(2, 1, 1)
    assert np.array_equal(bits(core_denoise(core, *one, levels=5)), bits(core_denoise(core, *one, levels=0)))   # 1 x 1: nothing to average with


def _flat(w, h):
    g = np.zeros((h, w, 8), dtype=np.float32)
    g[..., 0:3] = 0.5
    g[..., 5] = 1.0
    g[..., 6] = 2.0
    g[..., 7] = 1.0
    return g


@pytest.mark.parametrize("guide", ["normal", "albedo", "coverage", "depth"])
def test_a_guide_edge_with_zero_weight_separates_the_sides(core, guide):
    """A step in one guide that K() sends to zero: the left side's output does not depend on the right side's colours, and the other way round."""
    w, h = 24, 9
    g = _flat(w, h)
    right = np.arange(w) >= 11
    if guide == "normal":
        g[:, right, 3:6] = np.float32([1.0, 0.0, 0.0])          # |dN|^2 = 2 >= sigma_n^2
    elif guide == "albedo":
        g[:, right, 0:3] = np.float32([0.9, 0.5, 0.1])          # |dA|^2 = 0.32 >= sigma_a^2 = 0.0625
    elif guide == "coverage":
        g[:, right, :] = 0.0                                    # a miss: x_h = 1
    else:
        g[:, right, 6] = 3.0                                    # (3 - 2)^2 / (0.01 x 13) > 1
    acc, mom, n, _ = synthetic_inputs(21, w, h)
    acc2, mom2, _, _ = synthetic_inputs(22, w, h)
    for dem in (0, 1):
        base = core_denoise(core, acc, mom, n, g, demodulate=dem)
        a, m = acc.copy(), mom.copy()
        a[:, right], m[:, right] = acc2[:, right], mom2[:, right]
        other = core_denoise(core, a, m, n, g, demodulate=dem)
        assert np.array_equal(bits(base[:, ~right]), bits(other[:, ~right]))
        assert not np.array_equal(bits(base[:, right]), bits(other[:, right]))
        a, m = acc.copy(), mom.copy()
        a[:, ~right], m[:, ~right] = acc2[:, ~right], mom2[:, ~right]
        other = core_denoise(core, a, m, n, g, demodulate=dem)
        assert np.array_equal(bits(base[:, right]), bits(other[:, right]))
    # without the edge the sides do mix
    flat = _flat(w, h)
    base = core_denoise(core, acc, mom, n, flat)
    a, m = acc.copy(), mom.copy()
    a[:, right], m[:, right] = acc2[:, right], mom2[:, right]
    assert not np.array_equal(bits(base[:, ~right]), bits(core_denoise(core, a, m, n, flat)[:, ~right]))


def test_zero_variance_returns_the_input(core):
    """Every sampling of a pixel the same value: V = 0, so x_c is 0 between equal neighbours and huge between different ones — a pixel averages with
    its equals only.  The weighted mean of equal values is the value up to the roundings of sum w C / sum w: at most 25 products and 25 additions
    above, 25 additions below, one division — under 80 roundings of 2^-53, i.e. under 80 f64 ulp per level's state without demodulation.  In fp32
    that is 2^-22 of an ulp (demodulation adds a division and a product by the same A + eps): 1 fp32 ulp covers the final rounding falling on the
    other side."""
    w, h, n = 19, 11, 8
    rng = np.random.default_rng(4)
    x = rng.choice(np.float32([0.25, 1.5, 3.0, 0.0]), size=(h, w, 1)).repeat(3, axis=2) * np.float32([1.0, 0.5, 2.0])
    acc = (x * np.float32(n)).astype(np.float32)
    mom = np.concatenate([x.astype(np.float64) * n, x.astype(np.float64) ** 2 * n], axis=-1)
    want, st0 = core_denoise(core, acc, mom, n, _flat(w, h), want_state=True, levels=0)
    for dem in (0, 1):
        for levels in (1, 4, 5):
            got, st = core_denoise(core, acc, mom, n, _flat(w, h), want_state=True, levels=levels, demodulate=dem)
            assert (np.abs(bits(got).astype(np.int64) - bits(want).astype(np.int64)) <= 1).all()
            if not dem:
                assert ulp_distance(st[..., 0:3], st0[..., 0:3]).max() <= 80 * levels
                assert (st[..., 3:6] == 0.0).all()


def test_a_level_does_not_raise_the_variance(core):
    """V'_c = sum w^2 V_c / (sum w)^2 <= max V_c over the taps, since sum w^2 <= (sum w)^2.  That is exact in real numbers; in f64 a pixel whose
    only tap with weight is the centre gets fl(fl(w^2 V) / fl(w^2)), which can land an ulp above V.  So the bound is asserted within the roundings
    — at most 25 products and 25 additions above, a product and a division below, under 64 roundings of 2^-53: a factor 1 + 2^-46 — for every
    value; how many meet it exactly is printed (DESIGN.md §4.9 says the same)."""
    w, h = 37, 23
    acc, mom, n, g = synthetic_inputs(9, w, h, np.random.default_rng(8).integers(2, 30, size=(h, w)))
    _, st = core_denoise(core, acc, mom, n, g, want_state=True, levels=0)
    for lev in range(5):
        s = 1 << lev
        out = core_one_level(core, st, g, s)
        V = st[..., 3:6]
        pad = np.full((h + 4 * s, w + 4 * s, 3), -np.inf)
        pad[2 * s:2 * s + h, 2 * s:2 * s + w] = V
        vmax = np.max([pad[2 * s + j * s:2 * s + j * s + h, 2 * s + i * s:2 * s + i * s + w] for j in range(-2, 3) for i in range(-2, 3)], axis=0)
        assert (out[..., 3:6] <= vmax * (1.0 + 2.0 ** -46)).all()
        exact = (out[..., 3:6] <= vmax).mean()
        print("level %d: V' <= max V exactly at %.4f of the values" % (lev, exact))
        assert (out[..., 3:6] >= 0).all() and np.isfinite(out).all()
        st = out


def test_entry_points_declared_exported_and_bound(ha):
    text = ic.header_text()
    assert re.search(r"typedef\s+struct\s+hr_denoise_params\s*\{\s*uint32_t\s+levels\s*;\s*uint32_t\s+demodulate\s*;\s*double\s+sigma_color\s*,\s*sigma_normal\s*,\s*sigma_albedo\s*,\s*sigma_depth\s*;\s*\}\s*hr_denoise_params\s*;", text)
    assert re.search(r"int\s+hr_denoise_default_params\s*\(\s*hr_denoise_params\s*\*\s*\w+\s*\)\s*;", text)
    assert ic.declared(text, r"int\s+hr_render_guides\s*\(\s*%s\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_guides\s*\(\s*%s\s*,\s*float\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_write_guides\s*\(\s*%s\s*,\s*const\s+float\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_denoise\s*\(\s*%s\s*,\s*const\s+hr_denoise_params\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_denoised\s*\(\s*%s\s*,\s*float\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_resolve_denoised\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.abi_version(text) == 7       # functions and one new struct were added, none changed
    debug = ic.read("include", "hanamaru_hip_debug.h")
    assert "denoise" not in debug and "guides" not in debug
    assert not ic.exported_and_bound(ha, ENTRY_POINTS + ("hr_denoise_default_params",))
    assert C.sizeof(ha.Stats) == 46 * 8 and C.sizeof(ha.DenoiseParams) == 40
    for m in ("render_guides", "read_guides", "write_guides", "denoise", "read_denoised", "resolve_denoised"):
        assert callable(getattr(ha.Renderer, m, None)), m
    L = ha.hip_lib()
    assert len(L.hr_denoise.argtypes) == 2 and len(L.hr_read_guides.argtypes) == 2 and len(L.hr_render_guides.argtypes) == 1
    ffi = ic.rust_ffi()
    for name in ENTRY_POINTS[1:]:
        assert re.search(r"pub fn %s\(ctx: \*mut HrCtx" % name, ffi), name
    assert "pub fn hr_denoise_default_params(out: *mut HrDenoiseParams)" in ffi and "size_of::<HrDenoiseParams>() == 40" in ffi


def test_default_params_need_no_device(ha):
    p = ha.denoise_default_params()
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    assert ha.hip_lib().hr_denoise_default_params(None) == -1


def test_guide_kernel_has_a_row_per_node_format():
    kv = ic.kernel_variants()
    for row in ("HR_VARIANT(guide_render_kernel, true)", "HR_VARIANT(guide_render_kernel, false)"):
        assert row in kv, row


def test_cli_help_lists_the_denoise_flags(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0
    for flag in ("--denoise ", "--denoise-levels N", "--guide-image PREFIX"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,word", [(["--denoise", "--gpus", "2"], "one device"), (["--denoise", "--gpu-ids", "0,1"], "one device"),
                                       (["--denoise", "--debug"], "--debug"), (["--guide-image", "g", "--gpus", "2"], "one device"),
                                       (["--guide-image", "g", "--debug"], "--debug"), (["--denoise", "--denoise-levels", "6"], "--denoise-levels"),
                                       (["--denoise", "--denoise-levels", "two"], "--denoise-levels"), (["--denoise-levels", "2"], "--denoise")])
def test_cli_refuses_before_any_device(tmp_path, args, word):
    r, left_a_result = ic.cli_refused(tmp_path, args)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not left_a_result
