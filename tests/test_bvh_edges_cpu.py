"""The device BVH builders on edge geometry, CPU tier: the cases of tests/bvh_edge_scenes.py through the emulation of csrc/lbvh_core.h
(tests/emu: the builders' per-thread code run sequentially, the merge loop under the device loop's own control, PlocLoop) for the
host-SAH tree and builders 1 (LBVH) and 2 (PLOC).  The build succeeds, nodes == 2 leaves - 1, hit flag and t are bit-identical
between the three trees and between the walk on the 32-byte records and the one on the 16-byte quantised records, and the hits are
the brute force's.  tests/test_bvh_edges_gpu.py asserts the same of the kernels."""
import numpy as np
import pytest

import bvh_edge_scenes as bes

MAX_LEAVES = (1, 4, 15)


def _build(emu, ha, case, **options):
    emu.set_build_options(**options)
    try:
        return emu.EmuScene(case.scene_holder(ha).desc_ptr)
    finally:
        emu.set_build_options()


def _hits(emu, e):
    """(hits, elements) of the case's rays on the 32-byte records, after checking that the quantised walk returns the same bits"""
    def run(case):
        got, gel = e.intersect(case.rays)
        emu.set_walk_mode(2)
        try:
            gq, gelq = e.intersect(case.rays)
        finally:
            emu.set_walk_mode(0)
        assert np.array_equal(got.view(np.uint32), gq.view(np.uint32)) and np.array_equal(gel, gelq), (case.name, "quantised walk differs")
        return got, gel
    return run


def _check_tree(case, e, split):
    st = e.stats()
    nt, ns, nc = case.g.counts
    assert st["nodes"] == 2 * st["leaves"] - 1, (case.name, st)
    assert (st["spheres"], st["cuboids"]) == (ns, nc) and (st["tris"] >= nt if split else st["tris"] == nt), (case.name, st)


@pytest.mark.parametrize("name", sorted(bes.CASES))
def test_edge_case_through_the_emulated_builders(ha, emu, name):
    case = bes.get(name)
    n = sum(case.g.counts)
    base = None
    for max_leaf in MAX_LEAVES:
        for builder in (0, 1, 2):
            e = _build(emu, ha, case, max_leaf=max_leaf, builder=builder, split_ratio=0.0)
            _check_tree(case, e, False)
            got, gel = _hits(emu, e)(case)
            what = "builder %d max_leaf %d" % (builder, max_leaf)
            if base is None:
                base = (got, gel)
                bes.check_against_brute(case, got, gel, what)
            else:
                bes.check_same_hits(case, got, gel, base[0], base[1], what)
    tops = [1, 2, 64] + ([n - 1, n] if bes.in_group(name, "A") and n > 2 else [])
    for top in tops:
        e = _build(emu, ha, case, builder=2, split_ratio=0.0, ploc_top=max(1, top))
        _check_tree(case, e, False)
        its, left = emu.last_ploc_loop()
        assert (its == 0) == (n <= top) and min(n - 1, 1) <= left <= n, (name, top, its, left)   # (n = 1: no loop at all)
        got, gel = _hits(emu, e)(case)
        bes.check_same_hits(case, got, gel, base[0], base[1], "ploc_top %d" % top)
    if bes.in_group(name, "DFG"):
        for ratio in (-1.0, 1.01, 1000.0):
            for builder in (0, 1, 2):
                e = _build(emu, ha, case, builder=builder, split_ratio=ratio)
                _check_tree(case, e, True)
                got, gel = _hits(emu, e)(case)
                bes.check_same_hits(case, got, gel, base[0], base[1], "builder %d split_ratio %g" % (builder, ratio))


@pytest.mark.parametrize("name", sorted(bes.CASES))
def test_brute_force_against_the_oracle(ha, orc, name):
    """A second opinion on the reference hits: the oracle (f64, the reference's own median-split BVH and primitive tests) finds the brute
    force's hits.  The two see the same fp32-rounded coordinates; the oracle forms a triangle's edges in f64 where the brute force takes
    the fp32 edges of the kernels' record, so distances agree to an fp32 rounding of the edges, not to the bit."""
    case = bes.get(name)
    b = case.ref
    ref, rel = orc.OracleScene(case.scene_holder(ha).desc_ptr).intersect(case.rays.astype(np.float64))
    assert np.array_equal(ref[:, 0] == 1, b.hit), (name, np.where((ref[:, 0] == 1) != b.hit)[0][:10])
    err = np.abs(ref[b.hit, 1] - b.t[b.hit]) / np.where(b.kind[b.hit] == bes.TRI, b.scale[b.hit], np.maximum(1.0, b.t[b.hit]))
    assert err.max() < 4 * bes.EPS32, (name, err.max())
    if not case.ties:
        assert np.array_equal(rel[b.hit], b.elem[b.hit]), name


@pytest.mark.parametrize("name", sorted(bes.LOOP_CASES))
def test_merge_loop_that_makes_one_merge_per_iteration(ha, emu, name):
    """Copies of one triangle (every pair of the window has the same union area) and concentric spheres (boxes nested in Morton order):
    all clusters but one point at the same neighbour, an iteration makes ONE merge.  With ploc_top = 1 and more than 4,097 primitives
    that overran the loop's old bound of 4,096 iterations, and hr_upload_scene failed with an unnamed device error.  The loop now
    notices (PlocLoop: fewer than 1/64 of the clusters merged per iteration) and hands what is left to the top-down build."""
    case = bes.get(name)
    n = sum(case.g.counts)
    assert n > 4096 + 1
    e0 = _build(emu, ha, case, builder=0, split_ratio=0.0)
    base = _hits(emu, e0)(case)
    bes.check_against_brute(case, base[0], base[1], "builder 0")
    for top in (1, bes_default_top(emu)):
        e = _build(emu, ha, case, builder=2, split_ratio=0.0, ploc_top=top)
        _check_tree(case, e, False)
        its, left = emu.last_ploc_loop()
        print("%s ploc_top %d: %d iterations, %d clusters to the top-down build" % (name, top, its, left))
        assert its <= 64 * np.log(n) + 128 and left <= n, (its, left)
        got, gel = _hits(emu, e)(case)
        bes.check_same_hits(case, got, gel, base[0], base[1], "builder 2 ploc_top %d" % top)


def bes_default_top(emu):
    return emu.PLOC_TOP_DEFAULT


def test_merge_loop_control():
    """PlocLoop's rule in numbers, as lbvh_core.h states it: no stall while every iteration merges 1/64 of the clusters, a stall below
    that, never a stall under 128 clusters where one merge per iteration is all an iteration can be asked for."""
    def run(n, top, shrink):
        m_known, m, since, its = n, n, 0, 0
        while m_known > top:
            m = max(1, shrink(m)); its += 1; since += 1
            if since == 4 or m_known <= 4 * top:
                if m > top and m_known - m < since * max(1, m_known >> 6):
                    return its, m, True
                m_known, since = m, 0
        return its, m, False
    assert run(1 << 20, 8192, lambda m: m - m // 5)[2] is False
    assert run(5000, 1, lambda m: m - 1) == (4, 4996, True)
    assert run(100, 1, lambda m: m - 1) == (99, 1, False)
    assert run(1 << 24, 1, lambda m: m - max(1, m >> 6))[0] <= 64 * np.log(1 << 24) + 128
