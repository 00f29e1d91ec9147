"""The walk, ray by ray, GPU tier: the sets of tests/trace_sweeps.py through hr_debug_trace (the production traversal: traverse_wave on the record
format the renderer walks, box and leaf phases, two parked leaves, for shadow queries nee_setup's search limit and shadow_early_out) and
hr_debug_intersect (the scalar walk on the 32-byte records).  The judge is the brute force of tests/bvh_edge_scenes.py — plain f64, every ray
against every primitive — and the rule is ZERO disagreeing usable rays: hit flag, element, t within that module's bounds, in every direction
octant, from outside and inside, from surface points +- OFFSET, with direction components down to a denormal and +-0.0 (v_rcp_f32 on the device,
a division in the emulation), from origins up to 1,000 scene extents away, for closest-hit and shadow queries — and whatever else shares the
wave: a ray's answer is the same bits in every order, beside idle lanes, beside shadow queries, under the schedule's edge values.
tests/test_trace_sweeps_cpu.py asserts the same of the emulation and shows that four wrong walks are noticed."""
import time

import numpy as np
import pytest

import trace_sweeps as ts
from gpu_helpers import options, same

pytestmark = pytest.mark.gpu


def _upload(gpu, holder, builder=-1, max_leaf=4, quant=1, split=-1.0):
    with options(gpu, {"bvh_builder": builder, "max_leaf": max_leaf, "quant_nodes": quant, "split_ratio": split}):
        gpu.upload_scene(holder)
    st = gpu.stats()
    assert builder < 0 or st["bvh_builder_used"] == builder, (builder, st["bvh_builder_used"])
    return st


def _both_walks(gpu, s, what):
    """the set through the production traversal and the scalar walk: the same bits on EVERY ray, and the brute force's hits on the usable ones"""
    got, gel = gpu.debug_trace(s.rays)
    scalar, sel = gpu.debug_intersect(s.rays)
    diff = ts.differing(got, gel, scalar, sel)
    assert not diff.any() and same(got, scalar), (s.name, what, "production traversal and scalar walk differ on rays", np.where(diff)[0][:10].tolist(),
                                                   [(s.rays[i].tolist(), got[i, :2].tolist(), scalar[i, :2].tolist()) for i in np.where(diff)[0][:3]])
    ts.check_walk(s, got, gel, what)
    return got, gel


_base = {}


@pytest.mark.parametrize("builder", [0, 1, 2])
def test_octants_and_near_axis_on_every_tree(gpu, ha, builder):
    """sets 1 and 3 for this builder x quant_nodes 0 / 1 x max_leaf 1 / 4 / 15, and split_ratio 0 / 1000 on both record formats"""
    sw = ts.sweep()
    t0 = time.perf_counter()
    configs = [(max_leaf, quant, -1.0) for max_leaf in (1, 4, 15) for quant in (1, 0)] + [(4, quant, split) for split in (0.0, 1000.0) for quant in (1, 0)]
    base = _base          # the first configuration's answer of the first builder run, kept unchanged: every tree of every builder returns the same hits
    for max_leaf, quant, split in configs:
        st = _upload(gpu, sw.scene_holder(ha), builder, max_leaf, quant, split)
        what = "builder %d max_leaf %d quant_nodes %d split_ratio %g" % (builder, max_leaf, quant, split)
        assert st["triangles"] == sw.g.counts[0], (what, st["triangles"])
        for s in (sw.octants, sw.near_axis):
            got, gel = _both_walks(gpu, s, what)
            print("%s %s: worst |dt| per kind %s" % (s.name, what, ts.t_errors(s, got)))
            if s.name not in base:
                base[s.name] = (got, gel)
            else:
                ts.check_same(s, got, gel, base[s.name][0], base[s.name][1], what)
    # split_ratio 1000 still cuts the thin long triangles: with one primitive per leaf the tree has 2 x references - 1 records
    nodes = {split: _upload(gpu, sw.scene_holder(ha), builder, 1, 1, split)["bvh_nodes"] for split in (0.0, 1000.0)}
    assert nodes[0.0] == 2 * sum(sw.g.counts) - 1 and nodes[1000.0] > nodes[0.0], nodes
    print("wall time %.2f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("quant", [1, 0])
def test_secondary_inside_and_ragged_sets(gpu, ha, quant):
    """sets 2, 4 and 5 on the default tree, both record formats; a prefix of n rays (n = 1 too: a wave with 63 idle lanes) returns what those
    rays return inside the whole set"""
    sw = ts.sweep()
    t0 = time.perf_counter()
    _upload(gpu, sw.scene_holder(ha), quant=quant)
    what = "default tree quant_nodes %d" % quant
    for s in (sw.secondary, sw.inside, sw.plus37):
        got, gel = _both_walks(gpu, s, what)
        print("%s %s: worst |dt| per kind %s" % (s.name, what, ts.t_errors(s, got)))
    full, full_el = gpu.debug_trace(sw.octants.rays)
    for n in ts.RAGGED:
        got, gel = gpu.debug_trace(sw.octants.rays[:n])
        scalar, sel = gpu.debug_intersect(sw.octants.rays[:n])
        assert not ts.differing(got, gel, full[:n], full_el[:n]).any() and not ts.differing(scalar, sel, full[:n], full_el[:n]).any(), (what, n)
    got, gel = gpu.debug_trace(sw.plus37.rays)          # 4,037 rays: the last wave holds 5
    assert not ts.differing(got[:len(full)], gel[:len(full)], full, full_el).any(), (what, "set 1 inside set 1 plus 37")
    print("wall time %.2f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("quant", [1, 0])
def test_shadow_queries(gpu, ha, quant):
    """hit && (t - L)^2 < 4e-4 of the device's answer is the brute force's verdict on every kept query; where visible, the bits are the closest-hit query's"""
    sw = ts.sweep()
    sh = sw.shadow
    t0 = time.perf_counter()
    _upload(gpu, sw.scene_holder(ha), quant=quant)
    got, gel = gpu.debug_trace(sh.rays, sh.length)
    closest, cel = gpu.debug_trace(sh.rays)
    n_vis = ts.check_shadow(sh, got, gel, closest, cel, "quant_nodes %d" % quant)
    v = ts.shadow_verdict(got, sh.length)
    print("shadow quant_nodes %d: %d kept queries, %d visible; of the %d dropped ones %d differ from the brute force's verdict; wall time %.2f s"
          % (quant, int(sh.keep.sum()), n_vis, int((~sh.keep).sum()), int((~sh.keep & (v != sh.visible)).sum()), time.perf_counter() - t0))


def _in_order(gpu, s, order, base, base_el, what):
    got, gel = gpu.debug_trace(s.rays[order])
    back, back_el = np.empty_like(got), np.empty_like(gel)
    back[order], back_el[order] = got, gel
    n = ts.check_same_bits(s, back, back_el, base, base_el, what)
    print("octants %s: %d of the %d fragile rays differ" % (what, n, int((~s.usable).sum())))


def test_neighbours_do_not_matter(gpu, ha):
    """Set 1 through hr_debug_trace as generated, sorted by octant, under three permutations, one-to-63 among rays that miss the scene box at
    once, lane by lane beside shadow queries, and under the edge values of leaf_den and node_unroll: every usable ray returns the same bits."""
    sw = ts.sweep()
    s, sh = sw.octants, sw.shadow
    t0 = time.perf_counter()
    _upload(gpu, sw.scene_holder(ha))
    base, base_el = gpu.debug_trace(s.rays)
    ts.check_walk(s, base, base_el, "as generated")
    n = len(s)
    _in_order(gpu, s, np.argsort(s.octant, kind="stable"), base, base_el, "sorted by octant")
    for seed in (1, 2, 3):
        _in_order(gpu, s, np.random.default_rng(seed).permutation(n), base, base_el, "permutation %d" % seed)
    # one ray and 63 lanes that are done after the root: the first 160 rays, each in lane (7 k mod 64) of a wave of its own
    lo, hi = sw.g.bounds()
    away = np.concatenate([hi + 1.0, np.full(3, 3.0 ** -0.5)]).astype(np.float32)
    k = 160
    rays = np.tile(away, (64 * k, 1))
    lanes = np.arange(k) * 64 + (7 * np.arange(k)) % 64
    rays[lanes] = s.rays[:k]
    got, gel = gpu.debug_trace(rays)
    idle = np.ones(64 * k, dtype=bool)
    idle[lanes] = False
    assert (got[idle, 0] == 0).all(), "the filler rays hit something"
    first = ts.differing(got[lanes], gel[lanes], base[:k], base_el[:k])
    assert not (first & s.usable[:k]).any(), ("alone in the wave", np.where(first & s.usable[:k])[0][:10].tolist())
    print("octants one ray per wave: %d of the %d fragile rays differ" % (int((first & ~s.usable[:k]).sum()), int((~s.usable[:k]).sum())))
    # closest-hit and shadow queries alternating lane by lane
    alone, alone_el = gpu.debug_trace(sh.rays[:n], sh.length[:n])
    rays = np.empty((2 * n, 6), dtype=np.float32)
    sl = np.zeros(2 * n, dtype=np.float32)
    rays[0::2], rays[1::2], sl[1::2] = s.rays, sh.rays[:n], sh.length[:n]
    got, gel = gpu.debug_trace(rays, sl)
    m = ts.check_same_bits(s, got[0::2], gel[0::2], base, base_el, "beside shadow queries")
    d = ts.differing(got[1::2], gel[1::2], alone, alone_el)
    assert not (d & sh.keep[:n]).any(), ("shadow queries beside closest-hit queries", np.where(d & sh.keep[:n])[0][:10].tolist())
    print("octants beside shadow queries: %d of the %d fragile rays differ; shadow queries beside closest-hit queries: %d of the %d dropped ones differ"
          % (m, int((~s.usable).sum()), int((d & ~sh.keep[:n]).sum()), int((~sh.keep[:n]).sum())))
    for dbg in ({"leaf_den": 1}, {"leaf_den": 64}, {"node_unroll": 1}, {"node_unroll": 2}, {"leaf_den": 64, "node_unroll": 1}):
        with options(gpu, dbg=dbg):
            got, gel = gpu.debug_trace(s.rays)
        m = ts.check_same_bits(s, got, gel, base, base_el, str(dbg))
        print("octants %s: %d of the %d fragile rays differ" % (dbg, m, int((~s.usable).sum())))
    print("wall time %.2f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("spheres", [False, True])
def test_ladder(gpu, ha, spheres):
    """Origins 1 .. 1,000 scene extents from the target (and, counted only, two rungs beyond): the usable rays agree with the brute force at every
    rung on both record formats, and up to 1,000 extents quant_nodes 1 returns quant_nodes 0's bits on EVERY ray."""
    L = ts.ladder(spheres)
    t0 = time.perf_counter()
    for builder in (0, 1, 2):
        res = {}
        for quant in (0, 1):
            _upload(gpu, ts.ladder_holder(ha, spheres), builder, quant=quant)
            for s in L.rungs + L.beyond:
                got, gel = gpu.debug_trace(s.rays)
                scalar, sel = gpu.debug_intersect(s.rays)
                if s in L.rungs:
                    ts.check_rung(s, got, gel, "builder %d quant_nodes %d" % (builder, quant))
                    ts.check_rung(s, scalar, sel, "builder %d scalar walk" % builder)
                if quant == 0 or s.D <= ts.LADDER_BITS_TOP:
                    d = ts.differing(got, gel, scalar, sel)
                    assert not d.any(), (s.name, builder, quant, "production traversal and scalar walk differ on rays", np.where(d)[0][:10].tolist())
                res[quant, s.name] = (got, gel)
        for s in L.rungs + L.beyond:
            d = ts.differing(res[1, s.name][0], res[1, s.name][1], res[0, s.name][0], res[0, s.name][1])
            print("%s%s builder %d: quant_nodes 1 differs from quant_nodes 0 on %d of %d rays (%d usable of them)"
                  % (s.name, " with spheres" if spheres else "", builder, int(d.sum()), len(s), int((d & s.usable).sum())))
            if s.D <= ts.LADDER_BITS_TOP:
                assert not d.any(), (s.name, builder, np.where(d)[0][:10].tolist(), [(s.rays[i].tolist(), res[1, s.name][0][i, :2].tolist(), res[0, s.name][0][i, :2].tolist()) for i in np.where(d)[0][:3]])
    print("wall time %.2f s" % (time.perf_counter() - t0))


def test_small_primitives_from_far_away(gpu, ha):
    """The sweep scene from 1 .. 1e5 extents away.  No judge — the brute force calls every such ray fragile from 100 extents on.  On the
    32-byte records the production traversal returns the scalar walk's bits up to 1,000 extents (beyond, t has so few digits left that unlike
    primitives tie, and which one a walk keeps depends on the leaves it visits: counted); quant_nodes 1 returns quant_nodes 0's on every ray at 1
    extent, where the planes' margin covers the fp32 error (trace_sweeps.FAR_EQUAL); further out the count is printed."""
    sw = ts.sweep()
    t0 = time.perf_counter()
    for builder in (0, 1, 2):
        res, parked = {}, {}
        for quant in (0, 1):
            _upload(gpu, sw.scene_holder(ha), builder, quant=quant)
            for D in ts.FAR_EQUAL + ts.FAR_COUNTED:
                rays = ts.far_rays(sw.g, D)
                res[quant, D] = gpu.debug_trace(rays)
                if quant == 0:
                    scalar, sel = gpu.debug_intersect(rays)
                    parked[D] = int(ts.differing(res[0, D][0], res[0, D][1], scalar, sel).sum())
                    assert D > ts.LADDER_BITS_TOP or not parked[D], (D, builder, "production traversal and scalar walk differ")
        for D in ts.FAR_EQUAL + ts.FAR_COUNTED:
            d = ts.differing(res[1, D][0], res[1, D][1], res[0, D][0], res[0, D][1])
            print("sweep scene from %g extents, builder %d: quant_nodes 1 differs from quant_nodes 0 on %d of %d rays, the production traversal from the scalar walk on %d, %d rays hit"
                  % (D, builder, int(d.sum()), len(d), parked[D], int((res[0, D][0][:, 0] == 1).sum())))
            assert D not in ts.FAR_EQUAL or not d.any(), (D, builder, np.where(d)[0][:10].tolist())
    print("wall time %.2f s" % (time.perf_counter() - t0))
