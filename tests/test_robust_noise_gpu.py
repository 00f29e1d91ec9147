"""The robust noise estimate on the MI355X: robust_noise_kernel<K> against the host build of csrc/robust_core.h — within the 4 ulp
of the device's f64 sqrt, bit for bit where the spread is 0 —, its fixed-order summary, per-pixel counts, the selection of tiles by e_R, what is
refused, that nothing else moves, the calibration on rendered buckets, and the CLI's --robust-noise."""
import re

import numpy as np
import pytest

import post_cores as pc
import post_numpy as pn
import post_quality as pq
from cli import ASSETS, run_cli
from gpu_helpers import error_of, renderer, retarget, same
from post_cores import core  # noqa: F401  (the g++-built harness, a fixture)
from test_adaptive_gpu import MASKS, RH, RW, TARGETS, TX, TY, _pixels

pytestmark = pytest.mark.gpu

HR_ERR_INVALID = -1
FLOOR = 0.01
BLOCKS, THREADS = 1024, 256                             # robust_noise_kernel's grid (post_kernels.h)


def ulp_distance(a, b):
    """non-negative finite doubles: the distance of their bit patterns"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def fixed_order_sum(img):
    """The kernel's reduction of an image, step by step: every thread its strided pixels in order, a wave's lanes by halving (shfl_down 32 .. 1), the
    four waves of a workgroup left to right, the workgroups in index order on the host."""
    flat = img.reshape(-1)
    per = np.zeros(BLOCKS * THREADS)
    for first in range(0, flat.size, BLOCKS * THREADS):
        chunk = flat[first:first + BLOCKS * THREADS]
        per[:chunk.size] = per[:chunk.size] + chunk
    a = per.reshape(BLOCKS, THREADS // 64, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        a[..., :off] = a[..., :off] + a[..., off:2 * off]
    w = a[..., 0]
    blocks = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    total = 0.0
    for b in blocks:
        total = total + b
    return total


def synthetic_buckets(K, n=64, seed=0):
    """Heavy-tailed buckets of n samplings for the 37x23 window with the corner cases planted — the last pixel of the last row among them."""
    rng = np.random.default_rng(1000 * K + seed)
    B = pn.fill_buckets(pn.heavy_tailed(rng, n, (RH, RW)), K)
    B[0, 0] = np.float64([3.0, 10.0, 0.5]) * 4.0 * (n // K)                            # equal buckets (n a multiple of K or not: the keys differ then)
    B[0, 1] = 0.0
    B[0, 1, K // 2] = [1.0, 2.0, 0.5]                                                  # one hot bucket
    B[RH - 1, RW - 1] = 0.0                                                            # all zero, the last pixel of the last row
    B[RH - 1, 0] = -np.abs(B[RH - 1, 0])                                               # negative sums: den <= 0
    B[5, 5, 0], B[5, 5, 1] = [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]                          # equal keys, different colours
    B[RH - 1, RW - 2] = B[3, 3] * 1e-30                                                # tiny: the floor decides
    return B


def check_against_host(core, r, B, n, K, what):
    e, trim = pc.core_error(core, B, n, FLOOR)
    ss = pn.numpy_error(B, n, FLOOR, parts=True)[4]
    img = r.robust_noise_image(FLOOR)
    assert img.shape == (RH, RW) and np.isfinite(img).all() and (img >= 0).all(), what
    d = ulp_distance(img, e)
    assert d.max() <= 4, (what, int(d.max()))
    assert np.array_equal(img[ss == 0], e[ss == 0]) and (ss == 0).sum() >= 1, what     # no sqrt to differ by
    assert np.array_equal(r.robust_noise_trim(FLOOR), trim), what
    r.robust()
    assert np.array_equal(r.read_robust_trim(), trim), what
    return img, int(d.max())


@pytest.mark.parametrize("K", pn.ALL_K)
def test_image_and_summary_against_the_host_core(ha, scenes, core, K):
    worst = 0
    with renderer(ha, scenes("cornell_mini")[0], None, None, *TARGETS["frame"], buckets=K) as r:
        for target in sorted(TARGETS):
            for n in (64, K, 2 * K - 1):
                retarget(r, *TARGETS[target], buckets=K)
                B = synthetic_buckets(K, n, seed=n)
                r.write_buckets(B, n)
                img, d = check_against_host(core, r, B, n, K, (K, target, n))
                worst = max(worst, d)
                assert img[RH - 1, RW - 1] == 0 and img[RH - 1, 0] == 0 and img[0, 1] >= 0
                if n % K == 0:
                    assert img[0, 0] == 0
                thr = float(np.median(img))
                est = r.robust_noise_estimate(FLOOR, thr)
                assert est["samplings"] == n and est["pixels"] == RW * RH
                assert est["max_error"] == img.max() and est["pixels_above"] == int((img > thr).sum()) and 0 < est["pixels_above"] < RW * RH
                assert np.float64(est["mean_error"]).tobytes() == np.float64(fixed_order_sum(img) / (RW * RH)).tobytes(), (K, target, n)
                again = r.robust_noise_estimate(FLOOR, thr)
                assert again == est and np.float64(again["mean_error"]).tobytes() == np.float64(est["mean_error"]).tobytes()
                assert same(r.robust_noise_image(FLOOR), img)
                assert same(r.read_buckets()[0], B) and r.read_buckets()[1] == n      # untouched
            # every pixel its own n (written counts, K .. 3 K + 2)
            retarget(r, *TARGETS[target], counts=True, buckets=K)
            rng = np.random.default_rng(K)
            counts = rng.integers(K, 3 * K + 3, size=(RH, RW)).astype(np.uint32)
            x = pn.heavy_tailed(rng, int(counts.max()), (RH, RW))
            B = pn.fill_buckets(x * (np.arange(x.shape[0])[:, None, None, None] < counts[None, ..., None]), K)
            r.write_buckets(B, int(counts.max()))
            r.write_sample_counts(counts)
            e, trim = pc.core_error(core, B, counts, FLOOR)
            img = r.robust_noise_image(FLOOR)
            assert ulp_distance(img, e).max() <= 4 and np.array_equal(r.robust_noise_trim(FLOOR), trim), (K, target)
    print("K = %d: worst %d ulp" % (K, worst))


def test_per_pixel_counts_through_a_render(ha, scenes, core):
    K = 3
    with renderer(ha, scenes("cornell_mini")[0], None, None, *TARGETS["region"], counts=True, buckets=K) as r:
        wide = np.maximum(MASKS["checker"], MASKS["scattered"])
        r.set_tile_mask(wide)
        r.render(1, 6)
        r.set_tile_mask(MASKS["scattered"])
        r.render(6, 13)
        counts = np.where(_pixels(MASKS["scattered"]), 12, np.where(_pixels(wide), 5, 0)).astype(np.uint32)
        assert np.array_equal(r.read_sample_counts(), counts)
        for fn in (r.robust_noise_estimate, r.robust_noise_image, r.select_tiles_robust):
            assert error_of(ha, fn, FLOOR)[0] == HR_ERR_INVALID                       # pixels without a sampling: n < K
        r.set_tile_mask(None)
        r.render(13, 16)
        counts = r.read_sample_counts()
        assert set(np.unique(counts)) == {3, 8, 15}
        B, n = r.read_buckets()
        assert n == 15
        e, trim = pc.core_error(core, B, counts, FLOOR)
        img = r.robust_noise_image(FLOOR)
        assert ulp_distance(img, e).max() <= 4 and np.array_equal(r.robust_noise_trim(FLOOR), trim)
        assert not same(img, pc.core_error(core, B, 15, FLOOR)[0])                    # (the pixel's n matters)


def _tiles_above(img, thr):
    hot = np.zeros((TY * 4, TX * 4), bool)
    hot[:RH, :RW] = img > thr
    return hot.reshape(TY, 4, TX, 4).any(axis=(1, 3))


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_select_tiles_robust(ha, scenes, target):
    K = 9
    with renderer(ha, scenes("cornell_mini")[0], None, None, *TARGETS[target], counts=True, buckets=K) as r:
        B = synthetic_buckets(K, 64, seed=5)
        B[RH - 4:, RW - 4:] = synthetic_buckets(K, 64, seed=6)[RH - 4:, RW - 4:]      # the overhanging corner tile holds spread, not planted zeros
        r.write_buckets(B, 64)
        r.write_sample_counts(np.full((RH, RW), 64, np.uint32))
        img = r.robust_noise_image(FLOOR)
        padded = np.zeros((TY * 4, TX * 4))
        padded[:RH, :RW] = img
        thr = float(np.median(padded.reshape(TY, 4, TX, 4).max(axis=(1, 3))))          # between the tiles' largest e_R: about half of them stay
        hot = _tiles_above(img, thr)
        assert 0 < hot.sum() < TX * TY and 0 < (hot & (MASKS["checker"] != 0)).sum() < (MASKS["checker"] != 0).sum()
        # no mask in force
        assert r.select_tiles_robust(FLOOR, thr) == int(hot.sum())
        assert np.array_equal(r.tile_mask()[0] != 0, hot)
        # under a mask: AND, it only removes tiles, two calls agree
        for mname in ("checker", "scattered", "last"):
            old = MASKS[mname] != 0
            r.set_tile_mask(MASKS[mname])
            active = r.select_tiles_robust(FLOOR, thr)
            mask, n = r.tile_mask()
            assert np.array_equal(mask != 0, old & hot) and active == n == int((old & hot).sum()), mname
            assert r.select_tiles_robust(FLOOR, thr) == active and np.array_equal(r.tile_mask()[0], mask), mname
        assert same(r.robust_noise_image(FLOOR), img) and same(r.read_buckets()[0], B)
        # a lower threshold cannot bring a tile back
        before = r.tile_mask()[0]
        r.select_tiles_robust(FLOOR, 0.0)
        assert (r.tile_mask()[0] <= before).all()
        # above the maximum: no tile is left, and a render enqueues nothing
        r.set_tile_mask(None)
        assert r.select_tiles_robust(FLOOR, float(img.max())) == 0 and not r.tile_mask()[0].any()
        launches = r.stats()["trace_launches"]
        r.render(65, 67)
        assert r.stats()["trace_launches"] == launches and same(r.read_buckets()[0], B)
        assert (r.read_sample_counts() == 64).all()


def test_what_is_refused_touches_nothing(ha, scenes):
    K = 9
    with renderer(ha, scenes("cornell_mini")[0], None, None, *TARGETS["frame"], counts=True) as r:
        every = (r.robust_noise_estimate, r.robust_noise_image, r.robust_noise_trim, r.select_tiles_robust)
        for fn in every:
            assert error_of(ha, fn, FLOOR)[0] == HR_ERR_INVALID                       # option off
        retarget(r, *TARGETS["frame"], counts=True, buckets=K)
        B = synthetic_buckets(K, 64, seed=9)
        counts = np.full((RH, RW), 64, np.uint32)
        r.write_buckets(B, 64)
        r.write_sample_counts(counts)
        r.set_tile_mask(MASKS["checker"])
        r.robust()
        R = r.read_robust()

        def untouched(what):
            assert same(r.read_robust(), R), what                                      # still valid, still the same
            assert same(r.read_buckets()[0], B) and r.read_buckets()[1] == 64, what
            assert np.array_equal(r.read_sample_counts(), counts) and np.array_equal(r.tile_mask()[0], MASKS["checker"]), what

        for floor in (0.0, -0.01, float("inf"), float("nan")):
            for fn in every:
                assert error_of(ha, fn, floor)[0] == HR_ERR_INVALID, floor
        for fn in (r.robust_noise_estimate, r.select_tiles_robust):
            assert error_of(ha, fn, FLOOR, -1e-9)[0] == HR_ERR_INVALID
            assert error_of(ha, fn, FLOOR, float("nan"))[0] == HR_ERR_INVALID
        untouched("floor / threshold")
        # a successful estimate leaves R valid too
        r.robust_noise_estimate(FLOOR, 0.05)
        untouched("an estimate")
        # a count above the samplings behind the buckets; a count below K
        for bad in (65, K - 1):
            c2 = counts.copy()
            c2[RH - 1, RW - 1] = bad
            r.write_sample_counts(c2)
            for fn in every:
                assert error_of(ha, fn, FLOOR)[0] == HR_ERR_INVALID, bad
            assert same(r.read_buckets()[0], B) and np.array_equal(r.read_sample_counts(), c2) and np.array_equal(r.tile_mask()[0], MASKS["checker"])
        # without the counts: the selection is refused, the estimate asks the buckets' n
        retarget(r, *TARGETS["frame"], buckets=K)
        r.write_buckets(B, 64)
        assert error_of(ha, r.select_tiles_robust, FLOOR)[0] == HR_ERR_INVALID
        assert r.robust_noise_estimate(FLOOR, 0.05)["samplings"] == 64
        r.write_buckets(B, K - 1)
        for fn in every[:3]:
            assert error_of(ha, fn, FLOOR)[0] == HR_ERR_INVALID
        assert same(r.read_buckets()[0], B) and r.read_buckets()[1] == K - 1


def test_asking_changes_nothing_else(ha, scenes):
    sc = scenes("rtcamp6_v3_1")[0]
    quiet = renderer(ha, sc, None, None, *TARGETS["region"], moments=True, counts=True, buckets=9)
    asked = renderer(ha, sc, None, None, *TARGETS["region"], moments=True, counts=True, buckets=9)
    try:
        for r in (quiet, asked):
            r.render(1, 10)
            if r is asked:
                est = r.robust_noise_estimate(FLOOR, 0.05)
                assert est["samplings"] == 9 and est["mean_error"] > 0
                post = r.stats()["post_kernel_ms"]
                assert post > 0
            r.set_tile_mask(MASKS["checker"])
            r.render(10, 14)
        assert same(quiet.read_accumulator(), asked.read_accumulator()) and same(quiet.read_moments()[0], asked.read_moments()[0])
        assert np.array_equal(quiet.read_sample_counts(), asked.read_sample_counts())
        assert same(quiet.read_buckets()[0], asked.read_buckets()[0]) and quiet.read_buckets()[1] == asked.read_buckets()[1] == 13
        assert quiet.stats()["trace_launches"] == asked.stats()["trace_launches"]
    finally:
        quiet.close()
        asked.close()


def test_calibration_on_rendered_buckets(ha, scenes):
    """rtcamp6_v3_1 at 48x27, K = 9, samplings 1 .. 64 against 65 .. 128: z = (Ry_A - Ry_B) / sqrt(se_A^2 + se_B^2) with the device's e_R (se = e_R den,
    den and Ry from the read-back buckets), RMS within §4.7's gate."""
    w, h, n, K = pq.QW, pq.QH, pq.QN, pq.QK
    with ha.Renderer(0) as r:
        r.upload_scene(scenes("rtcamp6_v3_1")[0])
        r.set_resolution(w, h)
        r.set_option("robust_buckets", K)
        sets = []
        for first in (1, n + 1):
            r.clear()
            r.render(first, first + n)
            B, got = r.read_buckets()
            assert got == n
            e = r.robust_noise_image(FLOOR)
            ref, _, _, ry, _ = pn.numpy_error(B, n, FLOOR, parts=True)
            assert ulp_distance(e, ref).max() <= 4
            sets.append((ry, e * (ry + 3.0 * FLOOR)))
    (ra, sa), (rb, sb) = sets
    den = np.sqrt(sa ** 2 + sb ** 2)
    ok = den > 0
    rms = float(np.sqrt(np.mean(((ra - rb)[ok] / den[ok]) ** 2)))
    print("rtcamp6_v3_1 on the device: RMS z %.3f, pixels without a spread in either set %.4f" % (rms, 1.0 - ok.mean()))
    assert 0.6 <= rms <= 1.6 and 1.0 - ok.mean() <= 0.05


# ---------------------------------------------------------------------------------------------------------------- the CLI
BASE = ["--assets", ASSETS, "--scene", "rtcamp6_v3_1", "-w", RW, "-h", RH, "-t", 1000, "-i", 1000, "--robust", 9, "--robust-noise", "--noise-check", 16,
        "--launch", 1]                                  # one sampling a launch: the checks fall on 16, 32, 48


def _noise_lines(text):
    return [(int(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4)))
            for m in re.finditer(r"^noise: samplings=(\d+) mean=(\S+) max=(\S+) above=(\d+)$", text, re.M)]


def _sampled(text):
    return int(re.search(r"^sampled: (\d+)x4 spp\.$", text, re.M).group(1))


def test_cli_noise_target_asks_the_buckets(tmp_path, ha, scenes):
    """A trial run with the target 0 prints the robust estimate at every check; the target is set just above the SECOND check's mean, so the run has
    to pass the first check and stop at the second — where the library's own hr_robust_noise_estimate says the same."""
    trial = run_cli(BASE + ["-s", 64, "--noise-target", 0], tmp_path / "trial", timeout=120)
    assert trial.returncode == 0, trial.stdout
    lines = _noise_lines(trial.stdout)
    print("trial:", lines)
    assert len(lines) >= 3 and lines[0][1] > lines[1][1] > 0, lines                   # the estimate falls from the first check to the second
    E = float("%.6g" % (0.5 * (lines[0][1] + lines[1][1])))
    assert lines[1][1] <= E < lines[0][1]
    run = run_cli(BASE + ["-s", 64, "--noise-target", E, "--noise-image", "noise.png"], tmp_path / "a", timeout=120)
    assert run.returncode == 0 and "reached noise target" in run.stdout, run.stdout
    got, done = _noise_lines(run.stdout), _sampled(run.stdout)
    assert done == lines[1][0] and got[0][:3] == lines[0][:3] and got[0][1] > E and got[-1][0] == done and got[-1][1] <= E, run.stdout
    assert all(m > E for _, m, _, _ in got[:-2])
    with renderer(ha, scenes("rtcamp6_v3_1")[0], None, None, (RW, RH), buckets=9) as r:
        r.render(1, done + 1)
        est = r.robust_noise_estimate(FLOOR, E)
        e_img = r.robust_noise_image(FLOOR)
    assert got[-1] == (done, float("%.9g" % est["mean_error"]), float("%.9g" % est["max_error"]), est["pixels_above"])
    grey = ha.decode_image(str(tmp_path / "a" / "noise.png"))
    assert np.array_equal(grey[..., 0], (np.minimum(1.0, e_img / E) * 255.0 + 0.5).astype(np.uint8))
    # without the flag the same command asks the moments: another estimate
    plain = [a for a in BASE if a != "--robust-noise"]
    raw = run_cli(plain + ["-s", 32, "--noise-target", 0], tmp_path / "raw", timeout=120)
    assert raw.returncode == 0 and _noise_lines(raw.stdout)[0][0] == lines[0][0] and _noise_lines(raw.stdout)[0][1] != lines[0][1], raw.stdout
    # a checkpoint at the first check, resumed: the same stop, the same bytes
    first = run_cli(BASE + ["-s", lines[0][0], "--noise-target", E, "--checkpoint", "c.ckpt"], tmp_path / "b", timeout=120)
    assert first.returncode == 0 and _sampled(first.stdout) == lines[0][0], first.stdout
    rest = run_cli(BASE + ["-s", 64, "--noise-target", E, "--noise-image", "noise.png", "--resume", "c.ckpt"], tmp_path / "b", timeout=120)
    assert rest.returncode == 0 and "reached noise target" in rest.stdout and _sampled(rest.stdout) == done, rest.stdout
    for f in ("result.png", "noise.png"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f


def test_cli_adaptive_asks_the_buckets(tmp_path, ha, scenes):
    # a threshold between the tiles' largest e_R after the first phase: some tiles stop at the first check, some go on
    with renderer(ha, scenes("rtcamp6_v3_1")[0], None, None, (RW, RH), buckets=9) as r:
        r.render(1, 17)
        img = np.zeros((TY * 4, TX * 4))
        img[:RH, :RW] = r.robust_noise_image(FLOOR)
    E = float("%.6g" % np.median(img.reshape(TY, 4, TX, 4).max(axis=(1, 3))))
    run = run_cli(BASE + ["-s", 48, "--adaptive", E, "--sample-image", "samples.png", "--checkpoint", "a.ckpt"], tmp_path, timeout=120)
    assert run.returncode == 0, run.stdout
    checks = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"^adaptive: samplings=(\d+) active=(\d+) tiles=(\d+)$", run.stdout, re.M)]
    assert checks and checks[0][0] == 16 and 0 < checks[0][1] < checks[0][2] == TX * TY, run.stdout
    assert all(b[1] <= a[1] for a, b in zip(checks, checks[1:]))
    grey = ha.decode_image(str(tmp_path / "samples.png"))
    assert grey.shape[:2] == (RH, RW) and grey[..., 0].max() == 255 and len(np.unique(grey[..., 0])) >= 2
    # resumed: the tiles are chosen again, by the buckets, before anything is rendered
    again = run_cli(BASE + ["-s", 64, "--adaptive", E, "--resume", "a.ckpt"], tmp_path, timeout=120)
    assert again.returncode == 0, again.stdout
    first = re.search(r"adaptive: samplings=(\d+) active=(\d+)", again.stdout)
    assert first and int(first.group(1)) == int(re.search(r"resumed at (\d+)x4 sampled", again.stdout).group(1)), again.stdout
