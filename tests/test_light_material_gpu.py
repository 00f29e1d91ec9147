"""Light and material scenes (tests/light_material_scenes.py) on the MI355X: hr_debug_path_log against the oracle's path log, path by path, with
the accounting and the limits of the CPU tier (tests/test_light_material_cpu.py runs the same cases through the host emulation, which has libm
where the device has v_rcp / v_rsq / v_sin / v_exp / v_log); nee_setup's shortcuts on against off; the split pipeline against the megakernel;
and the other trees."""
import numpy as np
import pytest

import light_material_scenes as lm
from gpu_helpers import options
from test_corners_gpu import _log_and_render

pytestmark = pytest.mark.gpu

ALL = sorted(lm.CASES)
LIGHT_CASES = sorted(lm.LIGHT_CASES)


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("name", ALL)
def test_light_material_scene_path_by_path(gpu, ha, orc, name, precise):
    s, ref = lm.get(ha, orc, name)
    gpu.upload_scene(s)
    with options(gpu, {"precise_shading": precise}):
        g = _log_and_render(gpu, s)
    assert np.isfinite(g[0]).all()
    lm.check(name, g, ref, "device, precise_shading %d" % precise)


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("name", LIGHT_CASES)
def test_nee_culls_do_not_change_a_bit_here_either(gpu, ha, orc, name, precise):
    """tests/test_gpu_parity.py test_nee_culls_do_not_change_a_bit on the light cases: debug option nee_cull 7 (nee_setup's shortcuts, the
    default) against 0 (every shadow ray traced) — the accumulator of samplings 1 .. 4 and the path log are the same bits, the rays not traced
    are the rays the uncut kernel traces besides, and no shortcut fires on an emitter whose whole diameter lies inside the proximity window."""
    s, _ = lm.get(ha, orc, name)
    gpu.upload_scene(s)
    gpu.set_resolution(s.w, s.h)
    out = {}
    with options(gpu, {"precise_shading": precise}) as opt:
        for cull in (7, 0):
            opt.set("nee_cull", cull)
            opt.set("counters", 1)
            gpu.clear()
            gpu.render(1, 5)
            st = gpu.stats()
            opt.set("counters", 0)
            out[cull] = (gpu.read_accumulator().copy(), st, gpu.debug_path_log(1))
    (a, sa, la), (b, sb, lb) = out[7], out[0]
    assert a.sum() > 0 and np.isfinite(a).all() and np.array_equal(a, b), (name, np.abs(a - b).max())
    for x, y in zip(la, lb):
        assert np.array_equal(x, y), name
    print("%s, precise_shading %d: %d of %d rays not traced" % (name, precise, sa["shadow_culled"], sb["rays"]))
    assert sb["shadow_culled"] == 0 and sa["rays"] + sa["shadow_culled"] == sb["rays"], (name, sa["rays"], sa["shadow_culled"], sb["rays"])
    if lm.light_case(name) == "tiny":
        assert sa["shadow_culled"] == 0
    else:
        assert sa["shadow_culled"] > 0


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("name", ALL)
def test_split_pipeline_renders_the_same_bits(gpu, ha, orc, name, precise):
    """debug option trace_mode 1 (wf_core.h: nee_setup's and the shadow branch's other written home) against 0: the accumulator of samplings
    1 .. 2 and the path log, bit for bit"""
    s, _ = lm.get(ha, orc, name)
    gpu.upload_scene(s)
    gpu.set_resolution(s.w, s.h)
    out = []
    with options(gpu, {"precise_shading": precise}) as opt:
        for mode in (0, 1):
            opt.set("trace_mode", mode)
            gpu.clear()
            gpu.render(1, 3)
            out.append((gpu.read_accumulator().copy(), gpu.debug_path_log(1)))
    (a, la), (b, lb) = out
    assert a.sum() > 0 and np.isfinite(a).all() and np.array_equal(a, b), (name, np.abs(a - b).max())
    for x, y in zip(la, lb):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("option,value,default", [("quant_nodes", 0, 1), ("bvh_builder", 2, -1)])
@pytest.mark.parametrize("name", ["tiny-diffuse", "tiny-ggx", "shell_emits-diffuse", "shell_emits-ggx", "corridor", "mat_ggx_ior"])
def test_light_material_scene_on_the_other_trees(gpu, ha, orc, name, option, value, default):
    """the 32-byte nodes and the device-built PLOC tree: the same limits"""
    s, ref = lm.get(ha, orc, name)
    with options(gpu, {option: value, "precise_shading": 0}):
        gpu.upload_scene(s)
        g = _log_and_render(gpu, s)
    lm.check(name, g, ref, "device, %s %d" % (option, value))
