"""Sample buckets and the firefly-robust resolve on the MI355X: the buckets bucket_kernel keeps against a sequential f64 loop over
the library's own per-sampling renders, under launch cuts, strides, pipelines, regions and tile masks — bit for bit —, hr_robust against the host
build of csrc/robust_core.h — bit for bit —, the state rules of R, the quality figure on the device, and the CLI."""
import numpy as np
import pytest

import ckpt
import post_cores as pc
import post_numpy as pn
import post_quality as pq
from cli import ASSETS, run_cli
from gpu_helpers import bits, error_of, renderer, retarget, same
from post_cores import core  # noqa: F401  (the g++-built harness, a fixture)
from test_adaptive_gpu import MASKS, MODES, RH, RW, SCENES, TARGETS, _pixels

pytestmark = pytest.mark.gpu

HR_ERR_INVALID, HR_ERR_NO_TARGET, HR_ERR_UNSUPPORTED = -1, -4, -6
BUCKET_MODES = ["fp32-mega", "precise-mega", "fp32-split"]
N = 20                                                   # samplings of the rendered cases: 9 does not divide it, 3 does not either


def _make(ha, sc, mode="fp32-mega", target="frame", K=0, moments=False, counts=False):
    return renderer(ha, sc, *MODES[mode], *TARGETS[target], moments=moments, counts=counts, buckets=K)


def _aim(r, target, K=0, moments=False, counts=False):
    retarget(r, *TARGETS[target], moments=moments, counts=counts, buckets=K)


_x_cache = {}


def per_sampling(ha, scenes, name, mode, target, n=N):
    """x_s of samplings 1 .. n, (n, RH, RW, 3) fp32: what a launch of ONE sampling adds to a zeroed pixel (clear; render(s, s + 1); read_accumulator),
    rendered once per (scene, mode, target) by a context without the option and shared."""
    key = (name, mode, target)
    if key not in _x_cache:
        with _make(ha, scenes(name)[0], mode, target) as r:
            xs = []
            for s in range(1, n + 1):
                r.clear()
                r.render(s, s + 1)
                xs.append(r.read_accumulator())
        _x_cache[key] = np.stack(xs)
        assert np.isfinite(_x_cache[key]).all() and _x_cache[key].sum() > 0
    return _x_cache[key]


def sequential_buckets(x, samplings, K, counts=None):
    """The definition as a loop: the j-th sampling a pixel receives adds (double)x_s to its bucket j mod K.  samplings: 1-based indices in the order
    rendered; counts (h, w): only the pixel's first counts[p] samplings of the list reach it."""
    B = np.zeros(x.shape[1:3] + (K, 3))
    for j, s in enumerate(samplings):
        add = x[s - 1].astype(np.float64)
        if counts is not None:
            add = add * (j < counts)[..., None]
        B[:, :, j % K, :] += add
    return B


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("mode", BUCKET_MODES)
def test_buckets_equal_a_sequential_f64_loop(ha, scenes, name, mode):
    with _make(ha, scenes(name)[0], mode) as r:
        for target in sorted(TARGETS):
            x = per_sampling(ha, scenes, name, mode, target)
            for K in (3, 9):
                _aim(r, target, K)
                assert r.read_buckets()[0].shape == (RH, RW, K, 3) and not r.read_buckets()[0].any()
                for batch in (0, 1, 5):
                    r.set_option("batch", batch)
                    for pieces, samplings in [([(1, N + 1, 1)], range(1, N + 1)), ([(1, 8, 1), (8, N + 1, 1)], range(1, N + 1)), ([(1, 9, 2)], range(1, 9, 2))]:
                        what = (name, mode, target, K, batch, pieces)
                        r.clear()
                        for args in pieces:
                            r.render(*args)
                        got, n = r.read_buckets()
                        assert n == len(samplings), what
                        assert same(got, sequential_buckets(x, samplings, K)), what
                r.set_option("batch", 0)


@pytest.mark.parametrize("name", SCENES)
def test_the_option_changes_nothing_else(ha, scenes, name):
    sc = scenes(name)[0]
    off, on = _make(ha, sc, moments=True, counts=True), _make(ha, sc, K=9, moments=True, counts=True)
    try:
        for target in sorted(TARGETS):
            _aim(off, target, 0, True, True)
            _aim(on, target, 9, True, True)
            launches = []
            for r in (off, on):
                r.set_tile_mask(None)
                r.render(1, 8)
                r.set_tile_mask(MASKS["checker"])
                r.render(8, 13)
                launches.append(r.stats()["trace_launches"])
            assert same(off.read_accumulator(), on.read_accumulator()) and same(off.read_moments()[0], on.read_moments()[0])
            assert np.array_equal(off.read_sample_counts(), on.read_sample_counts()) and off.read_moments()[1] == on.read_moments()[1]
            assert launches[0] == launches[1]
            assert error_of(ha, off.read_buckets)[0] == HR_ERR_INVALID and on.read_buckets()[1] == 12
    finally:
        off.close()
        on.close()


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("target", sorted(TARGETS))
def test_tile_masks(ha, scenes, core, name, target):
    K = 9
    x = per_sampling(ha, scenes, name, "fp32-mega", target)
    with _make(ha, scenes(name)[0], "fp32-mega", target, K, counts=True) as r:
        full = sequential_buckets(x, range(1, 13), K)
        r.render(1, 13)
        assert same(r.read_buckets()[0], full)
        for mname in ("first", "last", "scattered", "none"):
            pix = _pixels(MASKS[mname])
            r.clear()
            r.set_tile_mask(MASKS[mname])
            r.render(1, 13)
            got, n = r.read_buckets()
            assert n == 12, mname
            assert same(got, np.where(pix[..., None, None], full, 0.0)), mname
            assert np.array_equal(r.read_sample_counts(), np.where(pix, 12, 0).astype(np.uint32)), mname
        # a second render under a smaller mask: every pixel holds the buckets of its own prefix 1 .. n_p
        wide = np.maximum(MASKS["checker"], MASKS["scattered"])
        r.clear()
        r.set_tile_mask(wide)
        r.render(1, 6)
        r.set_tile_mask(MASKS["scattered"])
        r.render(6, 13)
        counts = np.where(_pixels(MASKS["scattered"]), 12, np.where(_pixels(wide), 5, 0)).astype(np.uint32)
        assert np.array_equal(r.read_sample_counts(), counts)
        assert same(r.read_buckets()[0], sequential_buckets(x, range(1, 13), K, counts))
        # .. and the robust radiance takes every pixel's own count
        r.robust()
        R, trim = pc.core_robust(core, r.read_buckets()[0], counts)
        assert same(r.read_robust(), R) and np.array_equal(r.read_robust_trim(), trim)
        assert (r.read_robust()[counts == 0] == 0).all()


def _resolve_of(r, R):
    """hr_resolve's chain applied to a radiance image: the accumulator 4 R (exact) resolved with one sampling, scale 1 / 4 (exact)."""
    r.write_accumulator(R * np.float32(4))
    return r.resolve(1)


@pytest.mark.parametrize("name", SCENES)
def test_robust_equals_the_host_core(ha, scenes, core, name):
    with _make(ha, scenes(name)[0]) as r:
        for target in sorted(TARGETS):
            for K in (9, 3):
                # rendered buckets, equal counts
                _aim(r, target, K)
                r.render(1, N + 1)
                B, n = r.read_buckets()
                assert n == N
                r.robust()
                R, trim = pc.core_robust(core, B, N)
                got = r.read_robust()
                assert same(got, R) and np.array_equal(r.read_robust_trim(), trim), (target, K)
                assert np.isfinite(got).all() and got.sum() > 0
                if K == 9 and name == "rtcamp6_v3_1":
                    assert trim.max() > 0                                           # the fireflies of this scene are trimmed somewhere
                img = r.resolve_robust()
                assert img.shape == (RH, RW, 3) and np.array_equal(img, _resolve_of(r, got)), (target, K)
                # rendered buckets, per-pixel counts
                _aim(r, target, K, counts=True)
                r.render(1, 8)
                r.set_tile_mask(MASKS["checker"])
                r.render(8, N + 1)
                counts = r.read_sample_counts()
                assert set(np.unique(counts)) == {7, N}
                r.robust()
                R, trim = pc.core_robust(core, r.read_buckets()[0], counts)
                assert same(r.read_robust(), R) and np.array_equal(r.read_robust_trim(), trim), (target, K)
                # written synthetic buckets and counts: n = 0, n < K, n = K, n > K side by side
                rng = np.random.default_rng(K)
                counts = rng.integers(0, 3 * K + 3, size=(RH, RW)).astype(np.uint32)
                counts[0, :4] = [0, 1, K - 1, K]
                x = pn.heavy_tailed(rng, int(counts.max()), (RH, RW))
                x = x * (np.arange(x.shape[0])[:, None, None, None] < counts[None, ..., None])
                B = pn.fill_buckets(x, K)
                r.write_buckets(B, 123)
                r.write_sample_counts(counts)
                back, n = r.read_buckets()
                assert same(back, B) and n == 123
                r.robust()
                R, trim = pc.core_robust(core, B, counts)
                assert same(r.read_robust(), R) and np.array_equal(r.read_robust_trim(), trim), (target, K)
                assert np.array_equal(r.resolve_robust(), _resolve_of(r, R))
                # without the counts every pixel has the samplings behind the buckets
                _aim(r, target, K)
                B = pn.fill_buckets(pn.heavy_tailed(rng, 2 * K + 1, (RH, RW)), K)
                r.write_buckets(B, 2 * K + 1)
                r.robust()
                R, trim = pc.core_robust(core, B, 2 * K + 1)
                assert same(r.read_robust(), R) and np.array_equal(r.read_robust_trim(), trim), (target, K)
                # every bucket equal: R is that mean, and the bytes are hr_resolve's of it
                v = (rng.integers(1, 2 ** 12, size=(RH, RW, 3)) / 256.0).astype(np.float32)
                r.write_buckets(np.repeat((v.astype(np.float64) * 8.0)[:, :, None, :], K, axis=2), 2 * K)
                r.robust()
                assert same(r.read_robust(), v) and not r.read_robust_trim().any()
                assert np.array_equal(r.resolve_robust(), _resolve_of(r, v))


def test_state_rules(ha, scenes):
    sc = scenes("cornell_mini")[0]
    with ha.Renderer(0) as r:
        r.upload_scene(sc)
        assert error_of(ha, r.set_option, "robust_buckets", 9)[0] == HR_ERR_NO_TARGET
        r.set_resolution(RW, RH)
        # K = 0: every entry point is refused
        for fn in (r.read_buckets, r.robust, r.read_robust, r.read_robust_trim, r.resolve_robust):
            assert error_of(ha, fn)[0] == HR_ERR_INVALID
        assert r.L.hr_write_buckets(r._h, np.zeros(RH * RW * 27).ctypes.data, 0) == HR_ERR_INVALID
        r.set_option("robust_buckets", 9)
        r.render(1, 10)
        B, n = r.read_buckets()
        assert n == 9 and B.any()
        # bad values change nothing
        for bad in (4, 17, 1, 2, -3, 9.5, 16):
            assert error_of(ha, r.set_option, "robust_buckets", bad)[0] == HR_ERR_INVALID
        assert same(r.read_buckets()[0], B)
        r.set_option("robust_buckets", 9)                                           # the value it has: what was gathered stays
        assert same(r.read_buckets()[0], B) and r.read_buckets()[1] == 9
        assert error_of(ha, r.render_debug, 2)[0] == HR_ERR_UNSUPPORTED
        # no R before hr_robust; stale after everything it was made of changes
        for fn in (r.read_robust, r.read_robust_trim, r.resolve_robust):
            assert error_of(ha, fn)[0] == HR_ERR_INVALID
        r.set_option("moments", 1)
        acc, mom = r.read_accumulator(), r.read_moments()[0]

        def fresh():
            r.robust()
            hw = r._acc_hw()
            assert r.read_robust().shape == hw + (3,) and r.read_robust_trim().shape == hw and r.resolve_robust().shape == hw + (3,)

        def stale(what):
            for fn in (r.read_robust, r.read_robust_trim, r.resolve_robust):
                assert error_of(ha, fn)[0] == HR_ERR_INVALID, what

        for what, call in [("render", lambda: r.render(10, 11)), ("clear", r.clear), ("write_accumulator", lambda: r.write_accumulator(acc)),
                           ("write_moments", lambda: r.write_moments(mom, 9)), ("write_buckets", lambda: r.write_buckets(B, 9)),
                           ("bind_accumulator", lambda: r.bind_accumulator(None)), ("sample_counts on", lambda: r.set_option("sample_counts", 1)),
                           ("write_sample_counts", lambda: r.write_sample_counts(np.full((RH, RW), 9, np.uint32))),
                           ("sample_counts off", lambda: r.set_option("sample_counts", 0)), ("moments off", lambda: r.set_option("moments", 0)),
                           ("another K", lambda: r.set_option("robust_buckets", 5))]:
            fresh()
            call()
            stale(what)
        # another K started the buckets over
        B5, n5 = r.read_buckets()
        assert B5.shape == (RH, RW, 5, 3) and not B5.any() and n5 == 0
        # clear zeroes them; a round trip through write and read keeps every bit
        r.render(1, 4)
        assert r.read_buckets()[0].any()
        r.clear()
        assert not r.read_buckets()[0].any() and r.read_buckets()[1] == 0
        data = np.random.default_rng(2).standard_normal((RH, RW, 5, 3)) * 1e3
        r.write_buckets(data, 2 ** 40 + 3)
        back, n = r.read_buckets()
        assert same(back, data) and n == 2 ** 40 + 3
        # a new region or target zeroes them at the new size and drops R
        fresh()
        r.set_region(2, 1, 9, 6)
        stale("set_region")
        assert r.read_buckets()[0].shape == (6, 9, 5, 3) and not r.read_buckets()[0].any()
        r.render(1, 3)
        fresh()
        r.set_resolution(16, 8)
        stale("set_resolution")
        assert r.read_buckets()[0].shape == (8, 16, 5, 3) and r.read_buckets()[1] == 0
        # buckets and counts start over together: the count is the ordinal of a pixel's next sampling
        r.set_option("sample_counts", 1)
        r.render(1, 4)
        assert (r.read_sample_counts() == 3).all()
        r.set_option("robust_buckets", 3)
        assert not r.read_sample_counts().any() and not r.read_buckets()[0].any()
        r.render(1, 3)
        r.set_option("sample_counts", 0)
        r.set_option("sample_counts", 1)
        assert not r.read_buckets()[0].any()
        # off: the buckets go, and R with them
        fresh()
        r.set_option("robust_buckets", 0)
        for fn in (r.read_buckets, r.robust, r.read_robust, r.read_robust_trim, r.resolve_robust):
            assert error_of(ha, fn)[0] == HR_ERR_INVALID
        r.set_option("sample_counts", 0)
        r.render_debug(2)                                                            # allowed again


@pytest.mark.parametrize("name", SCENES)
def test_quality_ratio_on_the_device(ha, scenes, core, name):
    w, h, n, K, truth_n = pq.QW, pq.QH, pq.QN, pq.QK, pq.QTRUTH
    with ha.Renderer(0) as r:
        r.upload_scene(scenes(name)[0])
        r.set_resolution(w, h)
        r.set_option("robust_buckets", K)
        r.render(1, n + 1)
        acc = r.read_accumulator()
        r.robust()
        R, trim = r.read_robust(), r.read_robust_trim()
        assert same(R, pc.core_robust(core, r.read_buckets()[0], n)[0])
        r.set_option("robust_buckets", 0)
        r.clear()
        r.render(100001, 100001 + truth_n)                                           # the truth: 2,048 further samplings
        truth = r.read_accumulator().astype(np.float64) / (4.0 * truth_n)
        e_mean, e_rob = pn.rel_sq_error(acc / np.float32(4 * n), truth), pn.rel_sq_error(R, truth)
        print("%s on the device: relMSE mean %.4g robust %.4g ratio %.3f, energy kept %.3f, pixels trimmed %.3f"
              % (name, e_mean, e_rob, e_rob / e_mean, R.astype(np.float64).sum() / (acc.astype(np.float64).sum() / (4 * n)), (trim > 0).mean()))
        assert e_rob / e_mean < 1.0


# ---------------------------------------------------------------------------------------------------------------- the CLI

CW, CH = 32, 16
CLI_ARGS = ["--assets", ASSETS, "--scene", "cornell_mini", "-w", str(CW), "-h", str(CH), "-t", "1000", "-i", "1000"]


def _checkpoint_buckets(path, K):
    """The last trailer of a checkpoint written with --robust K: {"HRBK", K, samplings, w*h*3K doubles}."""
    c = ckpt.read(path)
    assert c.has_buckets and c.buckets_k == K and c.complete == ckpt.S_BUCKETS and c.used == c.size and c.buckets.shape == (CH, CW, K, 3)
    return c.buckets, c.buckets_n, c.size - (16 + CW * CH * 3 * K * 8)


def test_cli_robust_images_and_resume(tmp_path):
    one, two = tmp_path / "one", tmp_path / "two"
    r = run_cli(CLI_ARGS + ["-s", "16", "--robust", "9", "--robust-image", "trim.png", "--checkpoint", "c.ckpt"], one, timeout=120)
    assert r.returncode == 0, r.stdout
    for f in ("result.png", "trim.png", "c.ckpt"):
        assert (one / f).stat().st_size > 0, f
    assert "robust: buckets=9" in r.stdout
    # 8 + 8 samplings across a checkpoint: the bytes of the unsplit 16
    r = run_cli(CLI_ARGS + ["-s", "8", "--robust", "9", "--checkpoint", "a.ckpt"], two, timeout=120)
    assert r.returncode == 0, r.stdout
    r = run_cli(CLI_ARGS + ["-s", "16", "--robust", "9", "--robust-image", "trim.png", "--resume", "a.ckpt", "--checkpoint", "b.ckpt"], two, timeout=120)
    assert r.returncode == 0 and "resumed at 8x4 sampled" in r.stdout, r.stdout
    for f in ("result.png", "trim.png"):
        assert (one / f).read_bytes() == (two / f).read_bytes(), f
    b_one, n_one, head_one = _checkpoint_buckets(str(one / "c.ckpt"), 9)
    b_two, n_two, _ = _checkpoint_buckets(str(two / "b.ckpt"), 9)
    assert n_one == n_two == 16 and b_one.any() and np.array_equal(bits(b_one), bits(b_two))
    assert head_one == 20 + CW * CH * 12                                             # no other trailer: the header and the accumulator
    # another K, or a file without buckets, is refused together with --robust; without the flag the file keeps the bytes it always had
    r = run_cli(CLI_ARGS + ["-s", "20", "--robust", "5", "--resume", "a.ckpt"], two, timeout=120)
    assert r.returncode == 1 and "another K" in r.stdout, r.stdout
    r = run_cli(CLI_ARGS + ["-s", "4", "--checkpoint", "plain.ckpt"], two, timeout=120)
    assert r.returncode == 0 and (two / "plain.ckpt").stat().st_size == 20 + CW * CH * 12, r.stdout
    r = run_cli(CLI_ARGS + ["-s", "8", "--robust", "9", "--resume", "plain.ckpt"], two, timeout=120)
    assert r.returncode == 1 and "no sample buckets" in r.stdout, r.stdout
    # with --adaptive the buckets follow every pixel's own count, through the checkpoint as well
    r = run_cli(CLI_ARGS + ["-s", "24", "--robust", "9", "--adaptive", "0.05", "--noise-check", "8", "--checkpoint", "ad.ckpt"], two, timeout=120)
    assert r.returncode == 0 and "adaptive:" in r.stdout, r.stdout
    r = run_cli(CLI_ARGS + ["-s", "32", "--robust", "9", "--adaptive", "0.05", "--noise-check", "8", "--resume", "ad.ckpt"], two, timeout=120)
    assert r.returncode == 0, r.stdout
    r = run_cli(CLI_ARGS + ["-s", "32", "--robust", "9", "--resume", "ad.ckpt"], two, timeout=120)             # per-pixel ordinals need the counts
    assert r.returncode == 1 and "per-pixel" in r.stdout, r.stdout
