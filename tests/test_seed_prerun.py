"""The pre-run form of the three-run seed kernel's window (csrc/seed_kernels.h, debug option "seed_prerun", the default): all 128 lanes of a
half's two waves have a run of the init sweep, and a producer lane computes the first blocks of its run before the window, into registers.
It must hand the trace kernel exactly the draws of the three equal runs (seed_prerun = 0) and of the fused kernel (seed_mode = 0): the
accumulators are compared bit for bit.  The decomposition itself (entry states per generator class + pre-run blocks + window runs = the 256
words of isaac_init_final) is checked on the host by a stand-alone program built here with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from gpu_helpers import bits as _bits, options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hanamaru-renderer_amd", "csrc")


def test_decomposition_reproduces_isaac_init_final_on_the_host(tmp_path):
    exe = str(tmp_path / "seed_prerun_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-parameter",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "emu", "seed_prerun_check.cpp")], check=True)
    r = subprocess.run([exe, "100"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)   # 100 x 40 columns = 4,000 seeds
    assert r.returncode == 0, r.stdout
    assert "seed_prerun_check ok: 4000 seeds" in r.stdout, r.stdout


def test_every_three_run_row_has_a_pre_run_twin():
    kv = open(os.path.join(CSRC, "kernel_variants.h")).read()
    for args in ("false, false, false", "true, false, false", "false, true, false", "true, true, false", "false, false, true", "false, true, true"):
        assert "seed_seg_kernel<%s, true>" % args in kv, args
    assert '"seed_prerun"' in open(os.path.join(CSRC, "hr_api.hip")).read()
    assert '"seed_prerun"' in open(os.path.join(ROOT, "include", "hanamaru_hip_debug.h")).read()


@pytest.fixture(scope="module")
def r(ha):
    rr = ha.Renderer(0)
    yield rr
    rr.close()


def _render(r, args):
    r.clear()
    r.render(*args)
    acc = r.read_accumulator()
    assert np.isfinite(acc).all()
    return acc


def _forms(r, args, fused=True):
    """The accumulator of render(*args) from the default, from seed_prerun = 0 and (fused) from seed_mode = 0; options restored."""
    with options(r) as opt:
        out = {"default": _render(r, args)}
        opt.set("seed_prerun", 0)
        out["seed_prerun=0"] = _render(r, args)
        opt.set("seed_prerun", 1)
        if fused:
            opt.set("seed_mode", 0)
            out["seed_mode=0"] = _render(r, args)
        return out


def _assert_same(out, what):
    ref = out["default"]
    assert ref.sum() > 0, what
    for k, acc in out.items():
        assert np.array_equal(_bits(ref), _bits(acc)), (what, k, int((_bits(ref) != _bits(acc)).sum()), float(np.abs(ref.astype(np.float64) - acc).max()))


# 1x1 and 3x2: fewer groups than CUs, one partial group.  130x71x6: ragged tiles and a partial last group, out-of-range lanes in both generator
# classes.  640x360x9: many groups per workgroup.  (1, 20, 3): a strided range.
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,args", [(1, 1, (1, 3)), (3, 2, (1, 4)), (130, 71, (1, 7)), (640, 360, (1, 10)), (130, 71, (1, 20, 3))])
def test_default_matches_three_equal_runs_and_the_fused_kernel(r, scenes, w, h, args):
    sc, _ = scenes("rtcamp6_v3_1")
    r.upload_scene(sc)
    r.set_resolution(w, h)
    _assert_same(_forms(r, args), (w, h, args))


@pytest.mark.gpu
def test_every_workgroup_gets_exactly_one_group(r, scenes):
    """64x20 pixels = 80 tiles, 4 samplings in one launch: 20,480 paths = 256 groups of 80 — one per workgroup on a chip of 256 CUs (on a
    smaller chip the first workgroups get two): the first window, whose pre-run has its own pair of barriers, is then also the last."""
    sc, _ = scenes("rtcamp6_v3_1")
    r.upload_scene(sc)
    r.set_resolution(64, 20)
    with options(r, {"batch": 4}):
        _assert_same(_forms(r, (1, 5)), "one group per workgroup")


@pytest.mark.gpu
def test_under_a_tile_mask(r, scenes):
    """The LIST row.  The fused kernel has no list form: it renders without the mask and is compared on the mask's pixels (one sampling per
    launch in both, so that the launch cuts are the same)."""
    sc, _ = scenes("rtcamp6_v3_1")
    r.upload_scene(sc)
    w, h = 130, 71
    r.set_resolution(w, h)
    ty, tx = (h + 3) // 4, (w + 3) // 4
    yy, xx = np.mgrid[0:ty, 0:tx]
    mask = (((xx * 7 + yy * 3) % 5) < 2).astype(np.uint8)     # 40 % of the tiles, the ragged last column and row among them
    mask[ty - 1, tx - 1] = 1
    pix = np.kron(mask != 0, np.ones((4, 4), bool))[:h, :w]
    with options(r, {"sample_counts": 1, "batch": 1}) as opt:      # (the mask goes with the counts)
        r.set_tile_mask(mask)
        out = _forms(r, (1, 6), fused=False)
        _assert_same(out, "tile mask")
        r.set_tile_mask(None)
        opt.set("seed_mode", 0)
        full = _render(r, (1, 6))
        assert np.array_equal(_bits(out["default"]), _bits(np.where(pix[..., None], full, np.float32(0))))


@pytest.mark.gpu
def test_precise_shading_on_spheres(r, scenes):
    """The LO row (the records' twin with the draws' residuals).  The fused kernel writes no residuals: it is compared with draw_residuals = 0,
    where precise shading runs on the fp32 draws alone."""
    sc, _ = scenes("spheres")
    r.upload_scene(sc)
    r.set_resolution(130, 71)
    with options(r, {"precise_shading": 1}) as opt:
        _assert_same(_forms(r, (1, 7), fused=False), "precise shading, residual twin")
        opt.set("draw_residuals", 0)
        _assert_same(_forms(r, (1, 7)), "precise shading, fp32 draws alone")
