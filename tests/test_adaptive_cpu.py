"""Adaptive sampling on the CPU tier: csrc/adapt_core.h compiled for the host — the step from a launch's dense work item to the
tile it renders, the rule that keeps a tile active, the noise estimate with a count per pixel — and the entry points declared, exported and bound."""
import ctypes as C
import re

import numpy as np
import pytest

import interface_checks as ic
from cli import run_cli
from post_cores import core  # noqa: F401  (the g++-built harness, a fixture)
from post_numpy import noise_reference, ulp_distance

ENTRY_POINTS = ("hr_read_sample_counts", "hr_write_sample_counts", "hr_resolve_counted", "hr_set_tile_mask", "hr_get_tile_mask", "hr_select_tiles")


def _geometry(frame, region):
    x0, y0, w, h = region if region else (0, 0) + frame
    return np.array([frame[0], frame[1], x0, y0, w, h], dtype=np.uint32), (w + 3) // 4, (h + 3) // 4


def _synthetic(rng, h, w, counts):
    """Moments of counts[y, x] fp32 values per pixel and channel, added one at a time in f64."""
    mom = np.zeros((h, w, 6))
    for k in range(int(counts.max())):
        x = rng.gamma(0.7, 1.0, size=(h, w, 3)).astype(np.float32).astype(np.float64) * (counts > k)[..., None]
        mom[..., 0:3] += x
        mom[..., 3:6] += x * x
    return mom


@pytest.mark.parametrize("frame,region", [((37, 23), None), ((64, 48), (5, 3, 37, 23)), ((8, 8), None), ((5, 1), None)])
def test_list_lookup_against_tile_lane_pixel(core, frame, region):
    g, tx, ty = _geometry(frame, region)
    tiles = tx * ty
    assert core.default_params_mean_no_list() == 1                  # RenderParams rp{} means every tile, as it always did
    full = np.zeros((tiles, 64, 3), dtype=np.uint32)
    assert core.lane_pixels(g.ctypes.data, None, 0, full.ctypes.data) == tiles
    # what tile_lane_frame_pixel has always given: tile t -> pixels (4 tx + .., 4 ty + ..) + origin, lane = pixel * 4 + sub-sample
    for t in (0, tiles - 1, tiles // 2):
        j = np.arange(64)
        assert np.array_equal(full[t, :, 0], g[2] + 4 * (t % tx) + (j >> 2 & 3)) and np.array_equal(full[t, :, 1], g[3] + 4 * (t // tx) + (j >> 4))
        assert np.array_equal(full[t, :, 2], j & 3)
    rng = np.random.default_rng(11)
    for lst in [np.arange(tiles), np.array([tiles - 1]), np.array([0]), np.sort(rng.choice(tiles, size=max(1, tiles // 3), replace=False)), np.arange(0, tiles, 2)]:
        lst = np.ascontiguousarray(lst, dtype=np.uint32)
        out = np.zeros((len(lst), 64, 3), dtype=np.uint32)
        assert core.lane_pixels(g.ctypes.data, lst.ctypes.data, len(lst), out.ctypes.data) == len(lst)
        assert np.array_equal(out, full[lst])                       # dense item d renders exactly what tile list[d] renders without a list


@pytest.mark.parametrize("frame,region", [((37, 23), None), ((64, 48), (5, 3, 37, 23))])
def test_tile_rule_on_synthetic_moments(core, frame, region):
    g, tx, ty = _geometry(frame, region)
    w, h = int(g[4]), int(g[5])
    rng = np.random.default_rng(5)
    counts = rng.integers(2, 40, size=(h, w)).astype(np.uint32)
    mom = _synthetic(rng, h, w, counts)
    floor = 0.01
    e = noise_reference(mom, counts, floor)
    got_e = np.zeros(h * w)
    core.pixel_errors(mom.ctypes.data, counts.ctypes.data, floor, h * w, got_e.ctypes.data)
    pad = np.full((ty * 4, tx * 4), -np.inf)
    pad[:h, :w] = got_e.reshape(h, w)
    tmax = pad.reshape(ty, 4, tx, 4).max(axis=(1, 3))
    for thr in (0.0, float(np.median(tmax)), float(tmax.max()), float(np.sort(tmax.ravel())[3])):
        out = np.zeros(tx * ty, dtype=np.uint8)
        core.tile_rule(g.ctypes.data, mom.ctypes.data, counts.ctypes.data, floor, thr, out.ctypes.data)
        assert np.array_equal(out.reshape(ty, tx) != 0, tmax > thr), thr         # strictly greater; exactly the per-pixel value
    assert ulp_distance(got_e, e.ravel()).max() <= 4
    # the lanes that overhang the region are ignored: the buffers end with the region (a read past them would be out of bounds), and a tile
    # whose only hot pixel would be an overhanging one stays inactive — make every in-region pixel of the last tile constant (e = 0)
    assert w % 4 and h % 4
    quiet = mom.copy()
    ys, xs = slice(4 * (ty - 1), h), slice(4 * (tx - 1), w)
    c = counts[ys, xs].astype(np.float64)[..., None]
    quiet[ys, xs, 0:3] = c * 0.5
    quiet[ys, xs, 3:6] = c * 0.25
    out = np.zeros(tx * ty, dtype=np.uint8)
    core.tile_rule(g.ctypes.data, quiet.ctypes.data, counts.ctypes.data, floor, 0.0, out.ctypes.data)
    assert out[-1] == 0 and out[:-1].all()


def test_noise_pixel_error_with_a_count_per_pixel(core):
    rng = np.random.default_rng(20261017)
    counts = np.concatenate([np.full(64, 2), rng.integers(2, 200, size=4000), np.full(32, 100000)]).astype(np.uint32)
    mom = _synthetic(rng, 1, len(counts), np.minimum(counts, 64)[None, :])[0]
    for floor in (0.01, 0.5, 1e-6):
        got = np.zeros(len(counts))
        core.pixel_errors(mom.ctypes.data, counts.ctypes.data, floor, len(counts), got.ctypes.data)
        d = ulp_distance(got, noise_reference(mom, counts, floor))
        print("floor %g: worst %d ulp" % (floor, int(d.max())))
        assert np.isfinite(got).all() and d.max() <= 4


def test_entry_points_declared_exported_and_bound(ha):
    text = ic.header_text()
    assert ic.declared(text, r"int\s+hr_read_sample_counts\s*\(\s*%s\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_write_sample_counts\s*\(\s*%s\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_resolve_counted\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_set_tile_mask\s*\(\s*%s\s*,\s*const\s+uint8_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_get_tile_mask\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_select_tiles\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.abi_version(text) == 7       # functions were added, no struct changed
    assert '"sample_counts"' in ic.header_text(raw=True)
    assert not ic.exported_and_bound(ha, ENTRY_POINTS)
    assert C.sizeof(ha.Stats) == 46 * 8
    for m in ("read_sample_counts", "write_sample_counts", "resolve_counted", "set_tile_mask", "tile_mask", "select_tiles"):
        assert callable(getattr(ha.Renderer, m, None)), m
    L = ha.hip_lib()
    assert len(L.hr_select_tiles.argtypes) == 4 and len(L.hr_get_tile_mask.argtypes) == 3 and len(L.hr_set_tile_mask.argtypes) == 2
    ffi = ic.rust_ffi()
    for name in ENTRY_POINTS:
        assert re.search(r"pub fn %s\(ctx: \*mut HrCtx" % name, ffi), name


def test_list_forms_are_rows_of_the_variant_tables():
    """The list forms are instantiations of their own, selected by a fact of the launch — not a branch in the kernels that run without a mask."""
    kv = ic.kernel_variants()
    for row in ("HR_VARIANT(trace_kernel, false, 5, true, false, false, false, true)", "HR_VARIANT(trace_kernel, false, 5, false, false, false, false, true)",
                "HR_VARIANT(trace_kernel, false, 4, true, false, false, true, true)", "HR_VARIANT(trace_kernel, false, 4, false, false, false, true, true)",
                "HR_VARIANT(wf_start_kernel, false, true)", "HR_VARIANT(wf_start_kernel, true, true)",
                "seed_seg_kernel<false, false, true>", "seed_seg_kernel<false, true, true>",
                "HR_VARIANT(accumulate_kernel, false, true, true)", "HR_VARIANT(accumulate_kernel, true, true, true)"):
        assert row in kv, row


def test_cli_help_lists_the_adaptive_flags(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0
    for flag in ("--adaptive E", "--sample-image FILE.png"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,word", [(["--adaptive", "0.1", "--gpus", "2"], "one device"), (["--adaptive", "0.1", "--gpu-ids", "0,1"], "one device"),
                                       (["--adaptive", "0.1", "--noise-target", "0.05"], "two stop rules"), (["--adaptive", "0"], "--adaptive"),
                                       (["--adaptive", "-0.5"], "--adaptive"), (["--adaptive", "nan"], "--adaptive"), (["--adaptive", "soon"], "--adaptive"),
                                       (["--sample-image", "s.png", "--gpus", "2"], "one device"), (["--adaptive", "0.1", "--debug"], "--debug")])
def test_cli_refuses_before_any_device(tmp_path, args, word):
    r, left_a_result = ic.cli_refused(tmp_path, args)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not left_a_result
