"""The device BVH builders on edge geometry, GPU tier: the cases of tests/bvh_edge_scenes.py through hr_upload_scene with the host-SAH
tree (bvh_builder 0) and the device builders (1 LBVH, 2 PLOC: csrc/gpu_bvh.h, build_bvh_on_device), over max_leaf, quant_nodes, the debug
option ploc_top and split_ratio.  Per combination: the upload succeeds and reports the input's primitives, an odd record count and the
builder asked for; the production traversal (hr_debug_trace) returns the scalar walk's (hr_debug_intersect) bits; every tree returns the
same hit flags and distances, bit for bit, and the same elements except on equal-t ties; and the hits are the brute force's (plain f64,
every ray against every primitive) to the bounds of bvh_edge_scenes.check_against_brute.  tests/test_bvh_edges_cpu.py asserts the same
of the emulation."""
import numpy as np
import pytest

import bvh_edge_scenes as bes
from gpu_helpers import options
from schedule_knobs import ALL_DEFAULTS

pytestmark = pytest.mark.gpu


def _upload_and_query(gpu, ha, case, builder, max_leaf=4, quant=1, split_ratio=-1.0, ploc_top=ALL_DEFAULTS["ploc_top"]):
    """upload under the options, check the stats and that the two walks agree to the bit; returns (hits, elements, stats)"""
    with options(gpu, {"bvh_builder": builder, "max_leaf": max_leaf, "quant_nodes": quant, "split_ratio": split_ratio}, {"ploc_top": ploc_top}):
        gpu.upload_scene(case.scene_holder(ha))          # raises unless hr_upload_scene returns HR_OK
    st = gpu.stats()
    what = (case.name, "builder %d max_leaf %d quant %d split %g ploc_top %d" % (builder, max_leaf, quant, split_ratio, ploc_top))
    nt, ns, nc = case.g.counts
    assert (st["spheres"], st["cuboids"]) == (ns, nc), (what, st["spheres"], st["cuboids"])
    assert st["triangles"] == nt or (split_ratio != 0.0 and st["triangles"] > nt), (what, st["triangles"])
    assert st["bvh_nodes"] % 2 == 1, (what, st["bvh_nodes"])
    assert st["bvh_builder_used"] == builder, what
    got, gel = gpu.debug_trace(case.rays)
    scalar, sel = gpu.debug_intersect(case.rays)
    assert np.array_equal(got.view(np.uint32), scalar.view(np.uint32)) and np.array_equal(gel, sel), (what, "production traversal and scalar walk differ")
    return got, gel, st


@pytest.mark.parametrize("name", sorted(bes.CASES))
def test_edge_case_on_the_device(gpu, ha, name):
    case = bes.get(name)
    n = sum(case.g.counts)
    ms = {}
    base, base_el, _ = _upload_and_query(gpu, ha, case, 0)
    bes.check_against_brute(case, base, base_el, "builder 0")
    for max_leaf in (1, 4, 15):
        for builder in (0, 1, 2):
            got, gel, st = _upload_and_query(gpu, ha, case, builder, max_leaf=max_leaf)
            bes.check_same_hits(case, got, gel, base, base_el, "builder %d max_leaf %d" % (builder, max_leaf))
            if max_leaf == 4:
                ms[builder] = st["bvh_build_ms"]
    if bes.in_group(name, "ADE"):
        for builder in (0, 1, 2):
            got, gel, _ = _upload_and_query(gpu, ha, case, builder, quant=0)
            bes.check_same_hits(case, got, gel, base, base_el, "builder %d, 32-byte records" % builder)
    for top in [1, 2, 64] + ([n - 1, n] if bes.in_group(name, "A") and n > 2 else []):
        got, gel, _ = _upload_and_query(gpu, ha, case, 2, ploc_top=top)
        bes.check_same_hits(case, got, gel, base, base_el, "ploc_top %d" % top)
    if bes.in_group(name, "DFG"):
        for ratio in (0.0, 1.01, 1000.0):
            for builder in (0, 1, 2):
                got, gel, _ = _upload_and_query(gpu, ha, case, builder, split_ratio=ratio)
                bes.check_same_hits(case, got, gel, base, base_el, "builder %d split_ratio %g" % (builder, ratio))
    print("%s: %d primitives, bvh_build_ms LBVH %.3f PLOC %.3f" % (case.name, n, ms[1], ms[2]))


@pytest.mark.parametrize("name", sorted(bes.CASES))
def test_edge_case_renders(gpu, ha, name):
    """one short render over the device-built trees: the accumulator is finite and not empty"""
    case = bes.get(name)
    for builder in (1, 2):
        with options(gpu, {"bvh_builder": builder}):
            gpu.upload_scene(case.scene_holder(ha))
            gpu.set_resolution(32, 18)
            gpu.clear()
            gpu.render(1, 3)
            acc = gpu.read_accumulator()
            assert np.isfinite(acc).all() and (acc != 0).any(), (name, builder)


@pytest.mark.parametrize("name", sorted(bes.LOOP_CASES))
def test_merge_loop_that_makes_one_merge_per_iteration_on_the_device(gpu, ha, scenes, name):
    """Copies of one triangle, and concentric spheres: one merge per iteration (tests/test_bvh_edges_cpu.py says why).  With ploc_top = 1 the
    loop overran its old bound of 4,096 iterations and hr_upload_scene failed with an unnamed device error; it now hands the clusters that
    are left to the top-down build.  The upload succeeds, the hits are the host tree's and the brute force's, and the context goes on
    working: another scene uploads and renders."""
    case = bes.get(name)
    base, base_el, _ = _upload_and_query(gpu, ha, case, 0)
    bes.check_against_brute(case, base, base_el, "builder 0")
    for top in (1, ALL_DEFAULTS["ploc_top"]):
        got, gel, st = _upload_and_query(gpu, ha, case, 2, ploc_top=top)
        bes.check_same_hits(case, got, gel, base, base_el, "builder 2 ploc_top %d" % top)
        print("%s ploc_top %d: bvh_build_ms %.3f, %d records" % (name, top, st["bvh_build_ms"], st["bvh_nodes"]))
    sc, _ = scenes("cornell_mini")
    gpu.upload_scene(sc)
    gpu.set_resolution(32, 18)
    gpu.clear()
    gpu.render(1, 3)
    acc = gpu.read_accumulator()
    assert np.isfinite(acc).all() and (acc != 0).any()
