"""Sharded statistics on the MI355X: sample buckets indexed by the sampling (option bucket_by_sampling) and hr_fold_statistics,
which moves every rank's accumulator, moments, counts and buckets to rank 0.  Same-device groups are checked to the bit against numpy's rank-order
sums; against ONE context that rendered every sampling the f64 planes are held to the summation bound n * 2^-52 (all terms are non-negative).

Shapes: an 80x45 frame (20x12 tiles, the bottom row of tiles overhangs) and a 5x3 region at (3, 2) of a 16x12 frame — 45 floats, 90 and 75 doubles,
15 u32: none a multiple of the 16-byte vector, so every plane goes through fold_plane_kernel's vector loop AND its scalar tail."""
import numpy as np
import pytest

import post_cores as pc
from gpu_helpers import error_of, retarget, same

pytestmark = pytest.mark.gpu

HR_ERR_INVALID, HR_ERR_NO_TARGET, HR_ERR_UNSUPPORTED = -1, -4, -6
SCENE = "cornell_mini"
K = 5
TARGETS = {"frame": ((80, 45), None), "region": ((16, 12), (3, 2, 5, 3))}
SHAPES = {"frame": (45, 80), "region": (3, 5)}          # (h, w) of the accumulator
EPS = 2.0 ** -52


def _contexts(ha, sc, n):
    rs = []
    try:
        for _ in range(n):
            rs.append(ha.Renderer(0))
            rs[-1].upload_scene(sc)
    except Exception:
        _close(rs)
        raise
    return rs


def _close(rs):
    for r in rs:
        r.close()


def _aim(r, target, moments=False, counts=False, buckets=0, by_sampling=0):
    retarget(r, *TARGETS[target], moments=moments, counts=counts, buckets=buckets)
    r.set_option("bucket_by_sampling", by_sampling)
    if counts:
        r.set_tile_mask(None)
    r.clear()


def _planes(r, moments=True, counts=True, buckets=True):
    """every plane a fold moves, with the samplings behind it: {name: (array, n)}"""
    out = {"accumulator": (r.read_accumulator(), None)}
    if moments:
        out["moments"] = r.read_moments()
    if counts:
        out["sample_counts"] = (r.read_sample_counts(), None)
    if buckets:
        out["buckets"] = r.read_buckets()
    return out


def _unchanged(before, after):
    return before.keys() == after.keys() and all(same(before[k][0], after[k][0]) and before[k][1] == after[k][1] for k in before)


def _pixels(mask, shape):
    """the tile mask as a per-pixel mask of the (h, w) region"""
    return np.kron(np.asarray(mask, dtype=np.uint8), np.ones((4, 4), dtype=np.uint8))[:shape[0], :shape[1]] != 0


def _within_sum_bound(got, ref, n):
    """|got - ref| <= n * 2^-52 * ref, element by element: two f64 sums of the same n non-negative terms in different orders"""
    assert (ref >= 0).all()
    return (np.abs(got - ref) <= n * EPS * ref).all()


# ---- 1. by-sampling equals ordinal on one context ----
@pytest.mark.parametrize("counts", [False, True], ids=["uniform", "sample_counts"])
def test_by_sampling_equals_ordinal_on_one_context(ha, scenes, counts):
    rs = _contexts(ha, scenes(SCENE)[0], 2)
    try:
        for target in sorted(TARGETS):
            for pieces in ([(1, 12)], [(1, 4), (4, 12)]):
                got = []
                for by_sampling, r in enumerate(rs):
                    _aim(r, target, counts=counts, buckets=K, by_sampling=by_sampling)
                    for piece in pieces:
                        r.render(*piece)
                    got.append(r.read_buckets())
                assert got[0][1] == got[1][1] == 11, (target, pieces)
                assert got[0][0].shape == SHAPES[target] + (K, 3) and got[0][0].sum() > 0
                assert same(got[0][0], got[1][0]), (target, pieces)
    finally:
        _close(rs)


# ---- 2. by-sampling under a stride, and under a tile mask ----
def test_by_sampling_under_a_stride_and_a_tile_mask(ha, scenes):
    samplings = list(range(2, 15, 3))          # render(2, 15, 3): 2, 5, 8, 11, 14
    masks = {"frame": (np.add.outer(np.arange(12), np.arange(20)) % 3 != 0), "region": np.array([[1, 0]])}
    rs = _contexts(ha, scenes(SCENE)[0], 1)
    try:
        r = rs[0]
        for target in sorted(TARGETS):
            _aim(r, target)
            want = np.zeros(SHAPES[target] + (K, 3))
            for s in samplings:                 # x_s: what a launch of ONE sampling adds to a zeroed pixel, added in the order rendered
                r.clear()
                r.render(s, s + 1)
                want[:, :, (s - 1) % K, :] += r.read_accumulator().astype(np.float64)
            assert want.sum() > 0
            _aim(r, target, buckets=K, by_sampling=1)
            r.render(2, 15, 3)
            got, n = r.read_buckets()
            assert n == len(samplings) and same(got, want), target
            # under a tile mask (it needs the counts): inactive tiles keep all-zero buckets, active ones hold the same sums
            _aim(r, target, counts=True, buckets=K, by_sampling=1)
            r.set_tile_mask(masks[target])
            r.render(2, 15, 3)
            got, n = r.read_buckets()
            pix = _pixels(masks[target], SHAPES[target])
            assert pix.any() and not pix.all()
            assert n == len(samplings) and same(got, np.where(pix[..., None, None], want, 0.0)), target
            assert np.array_equal(r.read_sample_counts(), np.where(pix, len(samplings), 0).astype(np.uint32))
            r.set_tile_mask(None)
    finally:
        _close(rs)


# ---- 3. / 4. the same-device fold ----
def _render_shards(rs, target):
    """three ranks, moments + counts + K buckets by sampling; rank k renders samplings 1 + k, 4 + k, .. below 11: 4 / 3 / 3 of them"""
    for r in rs:
        _aim(r, target, moments=True, counts=True, buckets=K, by_sampling=1)
    for k, r in enumerate(rs):
        r.render(1 + k, 11, 3)


def test_same_device_fold_is_rank_order_addition_to_the_bit(ha, scenes):
    rs = _contexts(ha, scenes(SCENE)[0], 3)
    try:
        ha.comm_init_local(rs)
        assert [r.comm_info()["path"] for r in rs] == ["same-device-fallback"] * 3
        for target in sorted(TARGETS):
            _render_shards(rs, target)
            parts = [_planes(r) for r in rs]
            assert [p["moments"][1] for p in parts] == [4, 3, 3] and [p["buckets"][1] for p in parts] == [4, 3, 3]
            post_before = rs[0].stats()["post_kernel_ms"]
            ha.fold_statistics(rs)
            got = [_planes(r) for r in rs]
            assert rs[0].stats()["post_kernel_ms"] > post_before          # the fold kernels ran, on rank 0's clock
            for name, dtype in (("accumulator", np.float32), ("moments", np.float64), ("sample_counts", np.uint32), ("buckets", np.float64)):
                p = [part[name][0] for part in parts]
                assert p[0].dtype == dtype and all(x.any() for x in p), (target, name)
                assert same(got[0][name][0], (p[0] + p[1]) + p[2]), (target, name)
                for k in (1, 2):
                    assert not got[k][name][0].any(), (target, name, k)
            assert got[0]["moments"][1] == 10 and got[0]["buckets"][1] == 10
            assert [got[k]["moments"][1] for k in (1, 2)] == [0, 0] and [got[k]["buckets"][1] for k in (1, 2)] == [0, 0]
            assert (got[0]["sample_counts"][0] == 10).all()
    finally:
        _close(rs)


def test_fold_equals_one_context_within_the_rounding_bound(ha, scenes):
    core = pc.lib()
    rs = _contexts(ha, scenes(SCENE)[0], 4)
    one, rs = rs[3], rs[:3]
    try:
        ha.comm_init_local(rs)
        for target in sorted(TARGETS):
            _render_shards(rs, target)
            ha.fold_statistics(rs)
            _aim(one, target, moments=True, counts=True, buckets=K)
            one.render(1, 11)
            got, ref = _planes(rs[0]), _planes(one)
            assert np.array_equal(got["sample_counts"][0], ref["sample_counts"][0])
            assert got["moments"][1] == ref["moments"][1] == 10 and got["buckets"][1] == ref["buckets"][1] == 10
            for name in ("moments", "buckets"):
                print("%s %s: largest |fold - one| / one = %.3g (bound %.3g)" % (target, name, np.max(np.abs(got[name][0] - ref[name][0]) / np.maximum(ref[name][0], 1e-300)), 10 * EPS))
                assert ref[name][0].any() and _within_sum_bound(got[name][0], ref[name][0], 10), (target, name)
            acc, racc = got["accumulator"][0].astype(np.float64), ref["accumulator"][0].astype(np.float64)
            assert np.abs(acc - racc).max() <= 1e-5 * max(1.0, np.abs(racc).max()), target
            # R of rank 0 is the CPU definition's R of the buckets rank 0 holds, bit for bit (no trim decision is judged across two roundings)
            rs[0].robust()
            R, trim = pc.core_robust(core, got["buckets"][0], got["sample_counts"][0])
            assert same(rs[0].read_robust(), R) and np.array_equal(rs[0].read_robust_trim(), trim), target
            assert R.any()
    finally:
        _close(rs + [one])


# ---- 5. a sharded adaptive render ----
def test_sharded_adaptive_render_equals_the_one_context_one(ha, scenes):
    target, floor = "frame", 0.01
    rs = _contexts(ha, scenes(SCENE)[0], 3)
    ctl, rs = rs[2], rs[:2]
    try:
        ha.comm_init_local(rs)
        for r in rs + [ctl]:
            _aim(r, target, moments=True, counts=True)
        ctl.render(1, 17)
        # the threshold: the midpoint of the widest gap between consecutive sorted e of the control's middle half — no pixel's decision can flip
        # on the rounding of an f64 sum (1e-15 relative)
        e = np.sort(ctl.noise_image(floor).ravel())
        mid = e[len(e) // 4: 3 * len(e) // 4]
        i = int(np.argmax(np.diff(mid)))
        lo, hi = mid[i], mid[i + 1]
        threshold = 0.5 * (lo + hi)
        assert (hi - lo) > 1e-9 * threshold and (e > threshold).any() and (e < threshold).any()
        ctl_active = ctl.select_tiles(floor, threshold)
        ctl.render(17, 33)
        for k, r in enumerate(rs):
            r.render(1 + k, 17, 2)
        ha.fold_statistics(rs)
        assert (rs[0].read_sample_counts() == 16).all() and rs[0].read_moments()[1] == 16
        active = rs[0].select_tiles(floor, threshold)
        mask = rs[0].tile_mask()[0]
        rs[1].set_tile_mask(mask)
        print("threshold %.6g (gap %.3g relative): %d of %d tiles stay active" % (threshold, (hi - lo) / threshold, active, mask.size))
        assert active == ctl_active and np.array_equal(mask, ctl.tile_mask()[0]) and active > 0
        for k, r in enumerate(rs):
            r.render(17 + k, 33, 2)
        ha.fold_statistics(rs)
        assert np.array_equal(rs[0].tile_mask()[0], mask) and np.array_equal(rs[1].tile_mask()[0], mask)      # a fold leaves the masks
        counts = rs[0].read_sample_counts()
        assert np.array_equal(counts, ctl.read_sample_counts()) and set(np.unique(counts)) <= {16, 32} and (counts == 32).any()
        assert not rs[1].read_sample_counts().any() and not rs[1].read_accumulator().any()
        got, ref = rs[0].read_moments(), ctl.read_moments()
        assert got[1] == ref[1] == 32 and _within_sum_bound(got[0], ref[0], 32)
        a, b = rs[0].resolve_counted().astype(int), ctl.resolve_counted().astype(int)
        assert np.abs(a - b).max() <= 1 and b.std() > 1
    finally:
        _close(rs + [ctl])


# ---- 6. refusals ----
def test_refusals_touch_nothing(ha, scenes):
    rs = _contexts(ha, scenes(SCENE)[0], 2)
    try:
        target = "region"
        # no resolution yet
        ha.comm_init_local(rs)
        assert error_of(ha, ha.fold_statistics, rs)[0] == HR_ERR_NO_TARGET
        for r in rs:
            r.comm_destroy()

        def shards(by_sampling, ks=(K, K), moments=(True, True)):
            for k, r in enumerate(rs):
                _aim(r, target, moments=moments[k], counts=True, buckets=ks[k], by_sampling=by_sampling)
                r.render(1 + k, 8, 2)
            return [_planes(r, moments=moments[k]) for k, r in enumerate(rs)]

        def refused(before, fn, *args, word=None, moments=(True, True)):
            code, text = error_of(ha, fn, *args)
            assert code == HR_ERR_INVALID and (word is None or word in text), text
            assert all(_unchanged(before[k], _planes(r, moments=moments[k])) for k, r in enumerate(rs)), text

        # no communicator
        before = shards(1)
        refused(before, rs[0].fold_statistics, word="no communicator")
        refused(before, ha.fold_statistics, rs, word="no communicator")
        ha.comm_init_local(rs)
        # n is not the group's size; the contexts out of rank order
        refused(before, ha.fold_statistics, rs[:1])
        refused(before, ha.fold_statistics, rs[::-1])
        # bucket_by_sampling 2 is no value, and nothing starts over
        code, _ = error_of(ha, rs[0].set_option, "bucket_by_sampling", 2)
        assert code == HR_ERR_INVALID and all(_unchanged(before[k], _planes(r)) for k, r in enumerate(rs))
        # ordinal buckets do not add up
        before = shards(0)
        refused(before, ha.fold_statistics, rs, word="bucket_by_sampling")
        refused(before, rs[1].fold_statistics, word="bucket_by_sampling")
        # another K, other options
        before = shards(1, ks=(K, 9))
        refused(before, ha.fold_statistics, rs, word="differ")
        before = shards(1, moments=(True, False))
        refused(before, ha.fold_statistics, rs, word="differ", moments=(True, False))
        # another region
        before = shards(1)
        rs[1].set_region(3, 2, 4, 3)
        rs[1].render(1, 3)
        before[1] = _planes(rs[1])
        refused(before, ha.fold_statistics, rs, word="region")
        # and with everything in line the same group folds: whichever context of a same-device group asks, the group is folded
        before = shards(1)
        rs[1].fold_statistics()
        assert same(rs[0].read_buckets()[0], before[0]["buckets"][0] + before[1]["buckets"][0]) and not rs[1].read_buckets()[0].any()
        # switching the rule while the buckets run starts them over, as another K does — the counts and the moments with them
        rs[0].set_option("bucket_by_sampling", 1)          # the value it has: nothing happens
        assert rs[0].read_buckets()[1] == 7 and rs[0].read_buckets()[0].any()
        acc = rs[0].read_accumulator()
        rs[0].set_option("bucket_by_sampling", 0)
        assert rs[0].read_buckets()[1] == 0 and not rs[0].read_buckets()[0].any()
        assert not rs[0].read_sample_counts().any() and rs[0].read_moments()[1] == 0 and not rs[0].read_moments()[0].any()
        assert same(rs[0].read_accumulator(), acc)
    finally:
        _close(rs)


def test_bound_accumulators_are_folded_in_place(ha, scenes):
    """hr_bind_accumulator: the fold reads and writes the callers' buffers.  Rank 0's sits 4 bytes into its allocation — not 16-byte aligned, so
    fold_plane_kernel takes the plane element by element (no vector loop) —, rank 1's is aligned; the other planes stay the contexts' own."""
    import torch
    rs = _contexts(ha, scenes(SCENE)[0], 2)
    try:
        ha.comm_init_local(rs)
        for target in sorted(TARGETS):
            h, w = SHAPES[target]
            bufs = [torch.zeros((h * w * 3 + 1,), dtype=torch.float32, device="cuda:0"), torch.zeros((h * w * 3,), dtype=torch.float32, device="cuda:0")]
            views = [bufs[0][1:], bufs[1]]
            assert views[0].data_ptr() % 16 == 4 and views[1].data_ptr() % 16 == 0
            for k, r in enumerate(rs):
                _aim(r, target, moments=True, counts=True, buckets=K, by_sampling=1)
                r.bind_accumulator(views[k].data_ptr())
                r.clear()
                r.render(1 + k, 8, 2)
            parts = [_planes(r) for r in rs]
            assert all(same(views[k].cpu().numpy().reshape(h, w, 3), parts[k]["accumulator"][0]) and parts[k]["accumulator"][0].any() for k in (0, 1))
            ha.fold_statistics(rs)
            torch.cuda.synchronize()
            assert same(views[0].cpu().numpy().reshape(h, w, 3), parts[0]["accumulator"][0] + parts[1]["accumulator"][0]), target
            assert float(bufs[0][0]) == 0.0 and not views[1].cpu().numpy().any(), target          # the float in front of rank 0's window is not touched
            got = [_planes(r) for r in rs]
            for name in ("accumulator", "moments", "sample_counts", "buckets"):
                assert same(got[0][name][0], parts[0][name][0] + parts[1][name][0]) and not got[1][name][0].any(), (target, name)
            for r in rs:
                r.bind_accumulator(0)
    finally:
        _close(rs)


def _rccl_or_skip(ha):
    try:
        return ha.comm_unique_id()
    except ha.HipError as e:
        if e.code != HR_ERR_UNSUPPORTED:
            raise
        pytest.skip(str(e))


def _one_rank_fold(ha, r, fold):
    """a fold over one rank moves nothing — every plane bit for bit, the counts kept — and still invalidates R"""
    for target in sorted(TARGETS):
        _aim(r, target, moments=True, counts=True, buckets=K, by_sampling=1)
        r.render(1, 8)
        before = _planes(r)
        r.robust()
        assert r.read_robust().any()
        fold()
        assert _unchanged(before, _planes(r)) and before["buckets"][1] == 7 and before["moments"][1] == 7, target
        assert error_of(ha, r.read_robust)[0] == HR_ERR_INVALID
        r.render(8, 10)                                    # the context goes on rendering behind a fold
        assert r.read_buckets()[1] == 9


def test_a_group_of_one_is_a_fold_that_moves_nothing(ha, scenes):
    _rccl_or_skip(ha)                                      # (one context is no same-device group: hr_comm_init_local makes an RCCL communicator)
    rs = _contexts(ha, scenes(SCENE)[0], 1)
    try:
        ha.comm_init_local(rs)
        assert rs[0].comm_info()["path"] == "rccl-group"
        _one_rank_fold(ha, rs[0], lambda: ha.fold_statistics(rs))
    finally:
        _close(rs)


# ---- 7. the RCCL lines ----
def test_rccl_rank_fold_on_one_gpu(ha, scenes):
    uid = _rccl_or_skip(ha)
    rs = _contexts(ha, scenes(SCENE)[0], 1)
    try:
        rs[0].comm_init_rank(uid, 1, 0)
        assert rs[0].comm_info()["nranks"] == 1
        _one_rank_fold(ha, rs[0], rs[0].fold_statistics)
    finally:
        _close(rs)


def _two_gpus():
    import torch
    return torch.cuda.device_count() >= 2


@pytest.mark.skipif("not _two_gpus()", reason="needs two GPUs (skipped on the 1-GPU box, live on any bigger one)")
def test_rccl_group_fold_over_two_devices(ha, scenes):
    """ncclReduce to root 0 over two devices.  The summation order is RCCL's, but a sum of TWO terms is one rounding in either order: every plane
    of rank 0 is numpy's p0 + p1 to the bit."""
    _rccl_or_skip(ha)
    sc = scenes(SCENE)[0]
    rs = [ha.Renderer(0), ha.Renderer(1)]
    try:
        for r in rs:
            r.upload_scene(sc)
        ha.comm_init_local(rs)
        assert [r.comm_info()["path"] for r in rs] == ["rccl-group"] * 2
        for target in sorted(TARGETS):
            for k, r in enumerate(rs):
                _aim(r, target, moments=True, counts=True, buckets=K, by_sampling=1)
                r.render(1 + k, 11, 2)
            parts = [_planes(r) for r in rs]
            ha.fold_statistics(rs)
            got = [_planes(r) for r in rs]
            assert same(got[0]["sample_counts"][0], parts[0]["sample_counts"][0] + parts[1]["sample_counts"][0])
            assert same(got[0]["accumulator"][0], parts[0]["accumulator"][0] + parts[1]["accumulator"][0])      # (two terms: one rounding, either order)
            for name in ("moments", "buckets"):
                assert same(got[0][name][0], parts[0][name][0] + parts[1][name][0]) and got[0][name][1] == 10, (target, name)
                assert got[1][name][1] == 0
            assert all(not got[1][name][0].any() for name in got[1]), target
    finally:
        _close(rs)
