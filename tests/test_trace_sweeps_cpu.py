"""The walk, ray by ray, CPU tier: the sets of tests/trace_sweeps.py through the emulation (tests/emu: the product's own ray_set, ray_quantise,
trace_node / trace_qnode, node_advance, trace_leaf_next, the primitive tests and shadow_early_out, one lane at a time) in walk modes 0 (node + leaf
per visit), 1 (two parked leaves, 32-byte records) and 2 (two parked leaves, 16-byte quantised records), for the host-SAH tree and the emulated
device builders at max_leaf 1, 4 and 15 with split_ratio 0 and 1000.  No usable ray may differ from the brute force (hit flag, element, t within
the bounds of tests/bvh_edge_scenes.py); the three walks agree bit for bit on every ray; the shadow verdict is the brute force's on every kept
query; and four deliberately wrong walks and trees each make these checks raise.  The emulation's reciprocal is a division where the device has
v_rcp_f32, and its waves are one lane wide: tests/test_trace_sweeps_gpu.py asserts the same of the kernels."""
import numpy as np
import pytest

import trace_sweeps as ts

CONFIGS = [(builder, max_leaf, split) for builder in (0, 1, 2) for max_leaf in (1, 4, 15) for split in (0.0, 1000.0)]


def _build(emu, holder, builder=0, max_leaf=4, split=-1.0):
    emu.set_build_options(max_leaf=max_leaf, split_ratio=split, builder=builder)
    try:
        return emu.EmuScene(holder.desc_ptr)
    finally:
        emu.set_build_options()


def _modes(emu, e, rays, shadow_len=None):
    """the query in walk modes 0, 1 and 2"""
    out = []
    for mode in (0, 1, 2):
        emu.set_walk_mode(mode)
        try:
            out.append(e.trace(rays, shadow_len))
        finally:
            emu.set_walk_mode(0)
    return out


def _check_closest(emu, e, s, what):
    """a closest-hit set: walk 0 against the brute force, walks 1 and 2 the same bits on EVERY ray.  Returns walk 0's answer."""
    res = _modes(emu, e, s.rays)
    ts.check_walk(s, res[0][0], res[0][1], what + " walk 0")
    for mode in (1, 2):
        ts.check_same_bits(s, res[mode][0], res[mode][1], res[0][0], res[0][1], what + " walk %d against walk 0" % mode, every_ray=True)
    return res[0]


def _check_shadow(emu, e, sh, what):
    closest = _modes(emu, e, sh.rays)
    res = _modes(emu, e, sh.rays, sh.length)
    for mode in (0, 1, 2):
        ts.check_shadow(sh, res[mode][0], res[mode][1], closest[mode][0], closest[mode][1], what + " walk %d" % mode)
        assert not ts.differing(res[mode][0], res[mode][1], res[0][0], res[0][1]).any(), (what, "shadow queries: walk %d differs from walk 0" % mode)


_base = {}


@pytest.mark.parametrize("builder,max_leaf,split", CONFIGS)
def test_every_set_in_every_walk(ha, emu, builder, max_leaf, split):
    sw = ts.sweep()
    e = _build(emu, sw.scene_holder(ha), builder, max_leaf, split)
    what = "builder %d max_leaf %d split_ratio %g" % (builder, max_leaf, split)
    assert (e.stats()["tris"] > sw.g.counts[0]) == (split == 1000.0), (what, e.stats()["tris"])     # the thin long triangles' records are duplicated
    for s in sw.closest + [sw.plus37]:
        got, gel = _check_closest(emu, e, s, what)
        print("%s %s: worst |dt| per kind %s" % (s.name, what, ts.t_errors(s, got)))
        if s.name not in _base:
            _base[s.name] = (got, gel)          # the first configuration's answer, kept unchanged: every tree returns the same hits
        else:
            ts.check_same(s, got, gel, _base[s.name][0], _base[s.name][1], what)
    _check_shadow(emu, e, sw.shadow, what)


def test_ragged_prefixes_on_the_host(ha, emu):
    """the first 1, 63, 64 and 65 rays of set 1 return what they return inside the whole set (the host has no wave: this pins the entry's indexing)"""
    sw = ts.sweep()
    e = _build(emu, sw.scene_holder(ha))
    full, full_el = e.trace(sw.octants.rays)
    for n in ts.RAGGED:
        got, gel = e.trace(sw.octants.rays[:n])
        assert not ts.differing(got, gel, full[:n], full_el[:n]).any(), n


@pytest.mark.parametrize("spheres", [False, True])
def test_ladder_on_the_host(ha, emu, spheres):
    """Usable rays agree with the brute force at every rung; up to 1,000 extents the walk on the 16-byte records returns the 32-byte walk's bits on
    EVERY ray; beyond, the count of differing rays is printed."""
    L = ts.ladder(spheres)
    for builder in (0, 1, 2):
        e = _build(emu, ts.ladder_holder(ha, spheres), builder, split=0.0)
        for s in L.rungs + L.beyond:
            res = _modes(emu, e, s.rays)
            judged = s in L.rungs
            if judged:
                ts.check_rung(s, res[0][0], res[0][1], "builder %d walk 0" % builder)
                ts.check_same_bits(s, res[1][0], res[1][1], res[0][0], res[0][1], "walk 1 against walk 0", every_ray=True)
            diff = ts.differing(res[2][0], res[2][1], res[1][0], res[1][1])
            print("%s%s builder %d: 16-byte walk differs from the 32-byte walk on %d of %d rays (%d usable of them)"
                  % (s.name, " with spheres" if spheres else "", builder, int(diff.sum()), len(s), int((diff & s.usable).sum())))
            if s.D <= ts.LADDER_BITS_TOP:
                assert not diff.any(), (s.name, builder, np.where(diff)[0][:10].tolist())
            elif judged:
                ts.check_rung(s, res[2][0], res[2][1], "builder %d walk 2" % builder)


def test_small_primitives_from_far_away_on_the_host(ha, emu):
    """the sweep scene from 1 .. 1e5 extents away: no judge (every such ray is fragile from 100 extents on).  Walk 1 returns walk 0's bits up to 1,000
    extents (beyond, t has so few digits left that unlike primitives tie, and which one a walk keeps depends on the leaves it visits: counted); the 16-byte walk returns the 32-byte walk's on every ray at 1 extent, where the planes' margin covers the fp32 error (trace_sweeps.FAR_EQUAL);
    further out the count is printed"""
    sw = ts.sweep()
    for builder in (0, 1, 2):
        e = _build(emu, sw.scene_holder(ha), builder, split=0.0)
        for D in ts.FAR_EQUAL + ts.FAR_COUNTED:
            res = _modes(emu, e, ts.far_rays(sw.g, D))
            parked = ts.differing(res[1][0], res[1][1], res[0][0], res[0][1])
            assert D > ts.LADDER_BITS_TOP or not parked.any(), (D, builder, "walk 1 against walk 0")
            diff = ts.differing(res[2][0], res[2][1], res[1][0], res[1][1])
            print("sweep scene from %g extents, builder %d: 16-byte walk differs from the 32-byte walk on %d of %d rays, walk 1 from walk 0 on %d, %d rays hit"
                  % (D, builder, int(diff.sum()), len(diff), int(parked.sum()), int((res[1][0][:, 0] == 1).sum())))
            assert D not in ts.FAR_EQUAL or not diff.any(), (D, builder, np.where(diff)[0][:10].tolist())


def test_sets_are_what_they_claim():
    """the honesty conditions hold (Sweep and Ladder assert them when they are made) and the classes of the near-axis set are all there"""
    sw, L = ts.sweep(), ts.ladder()
    s3 = sw.near_axis
    for k, m in enumerate(ts.SMALL_COMPONENTS):
        sel = s3.usable & (s3.m_index == k)
        assert sel.sum() >= 100, (m, int(sel.sum()))
        small = np.abs(s3.rays[sel, 3:]).min(axis=1)
        assert (small == np.float32(m)).all(), m          # the component survives the fp32 rounding as given (1e-42: a denormal; 0.0: both signs)
    zero = s3.rays[s3.m_index == len(ts.SMALL_COMPONENTS) - 1, 3:]
    assert (np.signbit(zero) & (zero == 0)).any() and (~np.signbit(zero) & (zero == 0)).any()
    assert L.rungs[-1].D >= 1e3
    print(ts.report())


# ------------------------------------------------------------------------------------------ the checks notice a wrong walk

def test_a_swapped_octant_copy_is_noticed(ha, emu):
    sw = ts.sweep()
    e = _build(emu, sw.scene_holder(ha))
    e.break_octant_planes(5, 1)
    with pytest.raises(AssertionError):
        _check_closest(emu, e, sw.octants, "octant 5 with y near / far exchanged")


def test_quantised_boxes_two_steps_too_small_are_noticed(ha, emu):
    sw = ts.sweep()
    e = _build(emu, sw.scene_holder(ha))
    _check_closest(emu, e, sw.octants, "before")
    e.shrink_qboxes(2)
    with pytest.raises(AssertionError):
        _check_closest(emu, e, sw.octants, "quantised boxes shrunk by two steps")


def test_a_dropped_second_parked_leaf_is_noticed(ha, emu):
    sw = ts.sweep()
    e = _build(emu, sw.scene_holder(ha))
    emu.set_walk_mutant(emu.WALK_MUTANT_DROP_SECOND_LEAF)
    try:
        with pytest.raises(AssertionError):
            _check_closest(emu, e, sw.octants, "second parked leaf dropped")
    finally:
        emu.set_walk_mutant(0)


def test_a_shadow_limit_without_its_margin_is_noticed(ha, emu):
    sw = ts.sweep()
    e = _build(emu, sw.scene_holder(ha))
    _check_shadow(emu, e, sw.shadow, "before")
    emu.set_walk_mutant(emu.WALK_MUTANT_BARE_SHADOW_LIMIT)
    try:
        with pytest.raises(AssertionError):
            _check_shadow(emu, e, sw.shadow, "search limit shadow_len")
    finally:
        emu.set_walk_mutant(0)
