"""Adaptive sampling on the CPU tier: csrc/adapt_core.h compiled for the host — the step from a launch's dense work item to the
tile it renders, the rule that keeps a tile active, the noise estimate with a count per pixel — and the entry points declared, exported and bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cli import run_cli
from test_moments_cpu import ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("hr_read_sample_counts", "hr_write_sample_counts", "hr_resolve_counted", "hr_set_tile_mask", "hr_get_tile_mask", "hr_select_tiles")

HARNESS = r'''
#include "adapt_core.h"
using namespace hr;
static RenderParams params(const uint32_t *g, const uint32_t *list, uint32_t count) {
    RenderParams rp{};
    rp.width = g[0]; rp.height = g[1]; rp.org_x = g[2]; rp.org_y = g[3]; rp.reg_w = g[4]; rp.reg_h = g[5];
    rp.tiles_x = (g[4] + 3) / 4; rp.tiles_y = (g[5] + 3) / 4;
    rp.tile_list = list; rp.tile_count = count;
    return rp;
}
// frame pixel and sub-sample of lane j of every dense tile of a launch, with and without a list: out[dense][64][3]
extern "C" uint32_t lane_pixels(const uint32_t *g, const uint32_t *list, uint32_t count, uint32_t *out) {
    const RenderParams rp = params(g, list, count);
    const uint32_t n = list ? launch_tiles<true>(rp) : launch_tiles<false>(rp);
    for (uint32_t d = 0; d < n; d++)
        for (uint32_t j = 0; j < 64; j++) {
            uint32_t *o = out + ((size_t)d * 64 + j) * 3;
            tile_lane_frame_pixel(rp, list ? launch_tile<true>(rp, d) : launch_tile<false>(rp, d), j, o[0], o[1], o[2]);
        }
    return n;
}
extern "C" void tile_rule(const uint32_t *g, const double *moments, const uint32_t *counts, double floor, double threshold, unsigned char *out) {
    const RenderParams rp = params(g, nullptr, 0);
    for (uint32_t t = 0; t < rp.tiles_x * rp.tiles_y; t++) out[t] = adapt_tile_active(rp, t, moments, counts, floor, threshold) ? 1 : 0;
}
extern "C" void pixel_errors(const double *moments, const uint32_t *counts, double floor, int n, double *out) {
    for (int i = 0; i < n; i++) out[i] = noise_pixel_error(moments + 6 * (size_t)i, counts[i], floor);
}
extern "C" uint32_t default_params_mean_no_list() { RenderParams rp{}; return rp.tile_list == nullptr && rp.tile_count == 0u; }
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("adapt")
    src, so = d / "adapt_harness.cpp", d / "libadapt_harness.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "hanamaru-renderer_amd", "csrc"), "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    lib.lane_pixels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.lane_pixels.restype = C.c_uint32
    lib.tile_rule.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    lib.pixel_errors.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p]
    lib.default_params_mean_no_list.restype = C.c_uint32
    return lib


def _geometry(frame, region):
    x0, y0, w, h = region if region else (0, 0) + frame
    return np.array([frame[0], frame[1], x0, y0, w, h], dtype=np.uint32), (w + 3) // 4, (h + 3) // 4


def _noise_reference(mom, n, floor):
    """The definition (include/hanamaru_hip.h) with a count per pixel, every step one IEEE f64 operation in noise_core.h's order."""
    mom = np.asarray(mom, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)[..., None]
    s1, s2 = mom[..., 0:3], mom[..., 3:6]
    m = s1 / n
    var = np.maximum(0.0, (s2 - s1 * m) / (n - 1.0))
    se = np.sqrt(var / n) / 4.0
    mu = m / 4.0
    return ((se[..., 0] + se[..., 1]) + se[..., 2]) / (((mu[..., 0] + mu[..., 1]) + mu[..., 2]) + 3.0 * np.float64(floor))


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
    e = _noise_reference(mom, counts, floor)
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
        d = ulp_distance(got, _noise_reference(mom, counts, floor))
        print("floor %g: worst %d ulp" % (floor, int(d.max())))
        assert np.isfinite(got).all() and d.max() <= 4


def test_entry_points_declared_exported_and_bound(ha):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read(), flags=re.S)
    c = r"hr_ctx\s*\*\s*\w*"
    assert re.search(r"int\s+hr_read_sample_counts\s*\(\s*%s\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_write_sample_counts\s*\(\s*%s\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_resolve_counted\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_set_tile_mask\s*\(\s*%s\s*,\s*const\s+uint8_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_get_tile_mask\s*\(\s*%s\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_select_tiles\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert int(re.search(r"#define\s+HR_ABI_VERSION\s+(\d+)", text).group(1)) == 7       # functions were added, no struct changed
    assert '"sample_counts"' in open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read()
    lib = C.CDLL(ha.HIP_LIB)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert C.sizeof(ha.Stats) == 46 * 8
    for m in ("read_sample_counts", "write_sample_counts", "resolve_counted", "set_tile_mask", "tile_mask", "select_tiles"):
        assert callable(getattr(ha.Renderer, m, None)), m
    L = ha.hip_lib()
    assert len(L.hr_select_tiles.argtypes) == 4 and len(L.hr_get_tile_mask.argtypes) == 3 and len(L.hr_set_tile_mask.argtypes) == 2
    ffi = open(os.path.join(ROOT, "rust", "hip_ffi.rs")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"pub fn %s\(ctx: \*mut HrCtx" % name, ffi), name


def test_list_forms_are_rows_of_the_variant_tables():
    """The list forms are instantiations of their own, selected by a fact of the launch — not a branch in the kernels that run without a mask."""
    kv = open(os.path.join(ROOT, "hanamaru-renderer_amd", "csrc", "kernel_variants.h")).read()
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
    r = run_cli(["-w", "64", "-h", "48", "-s", "8"] + args, tmp_path)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not (tmp_path / "result.txt").exists()
