"""The restored robust resolve R'  on the MI355X: hr_robust_restore against csrc/restore_core.h compiled for the host — bit for bit:
f64, + - x / max and comparisons, no contraction —, levels 0 without a trim against hr_robust byte for byte, the refusals and state rules, that
asking changes nothing else, the quality figures on the device, and the CLI."""
import numpy as np
import pytest

import post_cores as pc
import post_numpy as pn
from cli import ASSETS, run_cli
from gpu_helpers import error_of, renderer, retarget, same
from post_cores import core  # noqa: F401  (the g++-built harness, a fixture)
from post_numpy import rel_sq_error, synthetic_inputs
from test_adaptive_gpu import MASKS

pytestmark = pytest.mark.gpu

HR_ERR_INVALID = -1
ALL_K = pn.ALL_K
RW, RH = 37, 23
# the 80 x 45 frame (3,600 pixels: 14 full spans of 256 and one of 16), a 37 x 23 region (851 pixels: a partial last span), one pixel
TARGETS = {"frame": ((80, 45), None, (80, 45)), "region": ((64, 48), (5, 3, RW, RH), (RW, RH)), "1x1": ((1, 1), None, (1, 1))}


def _counts(K, shape):
    return np.random.default_rng(K + shape[0]).integers(K, 3 * K + 3, size=shape).astype(np.uint32)


def _err(ha, fn, *a, **kw):
    return error_of(ha, fn, *a, **kw)[0]


# ---------------------------------------------------------------------------------------------------------------- R' against the host core

@pytest.mark.parametrize("K", ALL_K)
def test_restored_equals_the_host_core(ha, scenes, core, K):
    """Written synthetic buckets (heavy tails and the planted corner cases of the CPU tier) and written guides: R' is restore_image's, bit for bit,
    with levels 0, 1 and 4, on the robust radiance (base 0) and on the D that hr_denoise_robust has just made (base 1), on the frame, the region and
    one pixel, with one count for every pixel and with per-pixel counts.  K = 15 is the row with 92,160 B of LDS."""
    with renderer(ha, scenes("cornell_mini")[0]) as r:
        for target in sorted(TARGETS):
            frame, region, (w, h) = TARGETS[target]
            g = synthetic_inputs(5, w, h)[3]
            for n in (2 * K + 1, _counts(K, (h, w))):
                per_pixel = not np.isscalar(n)
                retarget(r, frame, region, counts=per_pixel, buckets=K)
                B = pn.synthetic_buckets(900 + K, K, (h, w), n)
                r.write_buckets(B, int(n.max()) if per_pixel else n)
                if per_pixel:
                    r.write_sample_counts(n)
                r.write_guides(g)
                r.denoise_robust()
                D = r.read_denoised()
                for levels in (0, 1, 4):
                    for base in (0, 1):
                        r.robust_restore(levels=levels, base=base)
                        want = pc.core_restore(core, B, n, g, D=D if base else None, levels=levels, base=base)
                        assert same(r.read_restored(), want), (K, target, per_pixel, levels, base)
                assert same(r.read_denoised(), D)                                      # D is still valid, and the same
                if target == "frame" and not per_pixel:
                    assert not same(pc.core_restore(core, B, n, g, levels=4), pc.core_restore(core, B, n, g, levels=0))
                    r.robust()
                    assert not same(pc.core_restore(core, B, n, g, levels=0), r.read_robust())   # X is somewhere


# ---------------------------------------------------------------------------------------------------------------- entry points and state

@pytest.mark.parametrize("K", [9, 3])
def test_levels_zero_without_a_trim_is_the_robust_image(ha, scenes, core, K):
    """Equal buckets trim nowhere: X = 0, and with levels 0 R' is R bit for bit and hr_resolve_restored gives hr_resolve_robust's bytes.  On rendered
    buckets, with the guide planes the call renders itself, R' = (float)(C + X) of the host core: K = 9 trims somewhere on 20 samplings of this
    scene and R' is brighter than R; K = 3 trims only a pixel two of whose three buckets are zero — none here — and R' stays R for every level."""
    with renderer(ha, scenes("rtcamp6_v3_1")[0]) as r:
        for target in ("frame", "region"):
            frame, region, (w, h) = TARGETS[target]
            retarget(r, frame, region, buckets=K)
            v = np.random.default_rng(K).gamma(2.0, 0.5, size=(h, w, 1, 3))
            r.write_buckets(np.repeat(v, K, axis=2) * 8.0, 2 * K)
            r.robust()
            assert not r.read_robust_trim().any()
            r.robust_restore(levels=0)
            assert same(r.read_restored(), r.read_robust()) and np.array_equal(r.resolve_restored(), r.resolve_robust()), (K, target)
            r.clear()
            r.render(1, 21)
            r.robust()
            R = r.read_robust()
            trims = bool(r.read_robust_trim().any())
            assert trims or K != 9
            r.robust_restore(levels=0)
            B, n = r.read_buckets()
            assert n == 20 and same(r.read_restored(), pc.core_restore(core, B, n, r.read_guides(), levels=0))
            assert r.read_guides().any() and same(r.read_restored(), R) == (not trims)  # the call rendered the guides; X is where a pixel trims
            assert same(r.read_robust(), R)                                            # R is still valid
            r.robust_restore()
            assert same(r.read_restored(), pc.core_restore(core, B, n, r.read_guides()))
            if trims:
                assert r.read_restored().astype(np.float64).sum() > R.astype(np.float64).sum()
            else:
                assert same(r.read_restored(), R)


def _state(r):
    return r.read_robust(), r.read_buckets(), r.read_sample_counts(), r.tile_mask()


def _same_state(a, b):
    return same(a[0], b[0]) and same(a[1][0], b[1][0]) and a[1][1] == b[1][1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3][0], b[3][0]) and a[3][1] == b[3][1]


def test_refusals_touch_nothing(ha, scenes):
    K = 9
    frame, region, (w, h) = TARGETS["region"]
    g = synthetic_inputs(5, w, h)[3]
    with renderer(ha, scenes("cornell_mini")[0], None, None, frame, region, counts=True) as r:
        assert _err(ha, r.robust_restore) == HR_ERR_INVALID                            # the option is off
        assert _err(ha, r.read_restored) == HR_ERR_INVALID and _err(ha, r.resolve_restored) == HR_ERR_INVALID
        r.set_option("robust_buckets", K)
        counts = _counts(K, (h, w))
        B = pn.synthetic_buckets(1, K, (h, w), counts)
        r.write_buckets(B, int(counts.max()))
        r.write_sample_counts(counts)
        r.write_guides(g)
        r.set_tile_mask(MASKS["checker"])
        r.robust()
        assert _err(ha, r.robust_restore, base=1) == HR_ERR_INVALID                    # base 1 without a D
        assert _err(ha, r.read_restored) == HR_ERR_INVALID
        r.denoise_robust()
        r.robust_restore(base=1)
        Rp, D, before = r.read_restored(), r.read_denoised(), _state(r)
        # the parameter refusals: R' stays, valid; so do R and D
        for bad in ({"levels": 6}, {"base": 2}, {"sigma_n": 0.0}, {"sigma_a": -1.0}, {"sigma_z": float("nan")}, {"sigma_n": float("inf")}):
            assert _err(ha, r.robust_restore, **bad) == HR_ERR_INVALID, bad
            assert same(r.read_restored(), Rp) and same(r.read_denoised(), D) and _same_state(_state(r), before), bad
        # a pixel with fewer than K samplings; a count beyond the samplings behind the buckets.  (Writing the counts has invalidated R', D and R
        # already: R is made again, R' and D stay invalid, and nothing else moves.)
        low, high = counts.copy(), counts.copy()
        low[7, 9] = K - 1
        high[7, 9] = int(counts.max()) + 1
        for bad in (low, high):
            r.write_sample_counts(bad)
            r.robust()
            before = _state(r)
            assert _err(ha, r.robust_restore) == HR_ERR_INVALID
            assert _err(ha, r.read_restored) == HR_ERR_INVALID and _err(ha, r.read_denoised) == HR_ERR_INVALID and _same_state(_state(r), before)
        r.write_sample_counts(counts)
        r.robust()
        before = _state(r)
        assert _err(ha, r.robust_restore, base=1) == HR_ERR_INVALID                    # D went with the counts
        assert _same_state(_state(r), before)
        r.denoise_robust()
        r.robust_restore(base=1)
        assert same(r.read_restored(), Rp) and same(r.read_denoised(), D)
        # without the counts: fewer samplings behind the buckets than buckets
        r.set_tile_mask(None)
        retarget(r, frame, region, buckets=K)
        r.write_buckets(B, K - 1)
        r.write_guides(g)
        assert _err(ha, r.robust_restore) == HR_ERR_INVALID and _err(ha, r.read_restored) == HR_ERR_INVALID
        assert same(r.read_buckets()[0], B) and r.read_buckets()[1] == K - 1
        r.write_buckets(B, K)
        r.robust_restore()
    # base 1 with a D that hr_denoise made, not hr_denoise_robust
    with renderer(ha, scenes("cornell_mini")[0], None, None, frame, region, moments=True, buckets=K) as r:
        r.render(1, 12)
        r.denoise()
        D = r.read_denoised()
        assert _err(ha, r.robust_restore, base=1) == HR_ERR_INVALID
        assert same(r.read_denoised(), D) and _err(ha, r.read_restored) == HR_ERR_INVALID
        r.robust_restore()
        assert same(r.read_denoised(), D)


def test_validity(ha, scenes):
    """R' goes stale with everything a D of hr_denoise_robust goes stale with, and with base 1 with a new D; with base 0 a new D is none of its
    business.  hr_robust, and the call itself, touch neither R's nor D's validity."""
    K = 9
    frame, region, (w, h) = TARGETS["region"]
    with renderer(ha, scenes("cornell_mini")[0], None, None, frame, region, buckets=K) as r:
        r.render(1, 12)
        B, n = r.read_buckets()
        acc = r.read_accumulator()

        def fresh(base):
            """K buckets of 11 samplings, R, a D of hr_denoise_robust and an R' on `base`"""
            r.set_option("sample_counts", 0)
            r.set_option("robust_buckets", K)
            r.write_buckets(B, n)
            r.robust()
            r.denoise_robust()
            r.robust_restore(base=base)
            assert r.read_restored().shape == (h, w, 3) and r.resolve_restored().shape == (h, w, 3)

        fresh(0)
        g, Rp = r.read_guides(), r.read_restored()
        r.set_option("robust_buckets", K)                                              # the value it has: R' stays
        r.robust()                                                                     # R again: R' is not made of R
        assert same(r.read_restored(), Rp) and r.read_denoised().shape == (h, w, 3) and r.read_robust().shape == (h, w, 3)
        for base in (0, 1):
            for what, call in [("render", lambda: r.render(12, 13)), ("write_buckets", lambda: r.write_buckets(B, n)),
                               ("another K", lambda: r.set_option("robust_buckets", 5)), ("robust_buckets off", lambda: r.set_option("robust_buckets", 0)),
                               ("clear", r.clear), ("write_accumulator", lambda: r.write_accumulator(acc)), ("write_guides", lambda: r.write_guides(g)),
                               ("render_guides", r.render_guides), ("guide_bounces", lambda: r.set_option("guide_bounces", 2)),
                               ("sample_counts on", lambda: r.set_option("sample_counts", 1))]:
                fresh(base)
                call()
                assert _err(ha, r.read_restored) == HR_ERR_INVALID and _err(ha, r.resolve_restored) == HR_ERR_INVALID, (base, what)
            r.set_option("guide_bounces", 0)
        fresh(1)
        r.denoise_robust(levels=1)                                                     # a new D: an R' on the old one is stale
        assert _err(ha, r.read_restored) == HR_ERR_INVALID
        fresh(0)
        Rp = r.read_restored()
        r.denoise_robust(levels=1)                                                     # base 0: R' is not made of D
        assert same(r.read_restored(), Rp)


def test_asking_changes_nothing_else(ha, scenes):
    sc = scenes("rtcamp6_v3_1")[0]
    frame, region, _ = TARGETS["region"]
    quiet, asks = (renderer(ha, sc, None, None, frame, region, counts=True, buckets=9) for _ in range(2))
    try:
        launches = []
        for r in (quiet, asks):
            r.render(1, 10)
            if r is asks:
                before = r.stats()
                r.robust_restore()
                after = r.stats()
                assert after["post_kernel_ms"] > before["post_kernel_ms"] and after["trace_launches"] == before["trace_launches"]
            r.set_tile_mask(MASKS["checker"])
            r.render(10, 15)
            launches.append(r.stats()["trace_launches"])
        assert same(quiet.read_accumulator(), asks.read_accumulator())
        assert np.array_equal(quiet.read_sample_counts(), asks.read_sample_counts())
        assert same(quiet.read_buckets()[0], asks.read_buckets()[0]) and quiet.read_buckets()[1] == asks.read_buckets()[1]
        assert launches[0] == launches[1]
    finally:
        quiet.close()
        asks.close()


# ---------------------------------------------------------------------------------------------------------------- quality

@pytest.mark.parametrize("name", ["rtcamp6_v3_1", "cornell_mini"])
def test_quality_on_the_device(ha, scenes, name):
    """48x27, 16 samplings, guide_bounces 2, default parameters, the truth rendered by hr_render from samplings 100001 .. 101024.  Asserted on
    rtcamp6_v3_1 at K = 5, as on the CPU tier: R' is closer to the energy of the plain mean of the bucket means than R is, and its error is below the
    plain mean's.  Everything else is printed."""
    w, h, n, truth_n = 48, 27, 16, 1024
    with ha.Renderer(0) as r:
        r.upload_scene(scenes(name)[0])
        r.set_resolution(w, h)
        r.set_option("guide_bounces", 2)
        got = {}
        for K in (5, 9):
            r.set_option("robust_buckets", K)
            r.clear()
            r.render(1, n + 1)
            mean = r.read_accumulator() / np.float32(4 * n)
            B, nn = r.read_buckets()
            nb = (nn - np.arange(K) + K - 1) // K
            M = (B / nb[:, None] / 4.0).mean(axis=-2)
            r.robust()
            R = r.read_robust()
            r.robust_restore()
            Rp = r.read_restored()
            r.denoise_robust()
            r.robust_restore(base=1)
            got[K] = (mean, R, Rp, r.read_restored(), M)
        r.set_option("robust_buckets", 0)
        r.clear()
        r.render(100001, 100001 + truth_n)
        truth = r.read_accumulator().astype(np.float64) / (4.0 * truth_n)
    for K in (5, 9):
        mean, R, Rp, Rpd, M = got[K]
        e_mean, e_r, e_rp, e_rpd = (rel_sq_error(x, truth) for x in (mean, R, Rp, Rpd))
        s_r, s_rp = R.astype(np.float64).sum() / M.sum(), Rp.astype(np.float64).sum() / M.sum()
        print("%s on the device n=%d K=%d: R/mean %.3f  R'/mean %.3f  R'(DR)/mean %.3f  sumR/sumM %.4f  sumR'/sumM %.4f  R'/R %.3f"
              % (name, n, K, e_r / e_mean, e_rp / e_mean, e_rpd / e_mean, s_r, s_rp, e_rp / e_r))
        if name == "rtcamp6_v3_1" and K == 5:
            assert abs(s_rp - 1.0) < abs(s_r - 1.0)
            assert e_rp / e_mean < 1.0


# ---------------------------------------------------------------------------------------------------------------- the CLI

CLI_ARGS = ["--assets", ASSETS, "--scene", "cornell_mini", "-w", "48", "-h", "27", "-t", "1000", "-i", "1000", "-s", "16", "--robust", "5"]


def test_cli_robust_restore(ha, scenes, tmp_path):
    plain, denoised, two = tmp_path / "plain", tmp_path / "denoised", tmp_path / "two"
    r = run_cli(CLI_ARGS + ["--robust-restore"], plain, timeout=120)
    assert r.returncode == 0 and "is not restored" not in r.stdout, r.stdout
    r = run_cli(CLI_ARGS + ["--robust-restore", "--robust-denoise"], denoised, timeout=120)
    assert r.returncode == 0 and "is not restored" not in r.stdout and "is not denoised" not in r.stdout, r.stdout
    r = run_cli(CLI_ARGS + ["--robust-restore", "--restore-levels", "2"], two, timeout=120)
    assert r.returncode == 0, r.stdout
    with renderer(ha, scenes("cornell_mini")[0], None, None, (48, 27), buckets=5) as lib:
        lib.render(1, 17)
        lib.robust_restore()
        assert np.array_equal(ha.decode_image(str(plain / "result.png"))[..., :3], lib.resolve_restored())
        lib.robust()
        assert not np.array_equal(lib.resolve_robust(), lib.resolve_restored())
        lib.robust_restore(levels=2)
        assert np.array_equal(ha.decode_image(str(two / "result.png"))[..., :3], lib.resolve_restored())
        lib.denoise_robust()
        lib.robust_restore(base=1)
        assert np.array_equal(ha.decode_image(str(denoised / "result.png"))[..., :3], lib.resolve_restored())
        assert not np.array_equal(lib.resolve_denoised(), lib.resolve_restored())
