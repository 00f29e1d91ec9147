"""The robust denoiser on the MI355X: hr_denoise_robust against csrc/robust_core.h + csrc/denoise_core.h compiled for the host — bit
for bit: f64, + - x /, comparisons and one truncation, no sqrt, no contraction —, levels 0 against hr_robust byte for byte, hr_robust's per-K kernel
against the run-time K definition, the refusals and state rules, that asking changes nothing else, the quality figure on the device, and the CLI."""
import numpy as np
import pytest

import post_cores as pc
import post_numpy as pn
import post_quality as pq
from cli import ASSETS, run_cli
from gpu_helpers import error_of, renderer, retarget, same
from post_cores import core  # noqa: F401  (the g++-built harness, a fixture)
from post_numpy import rel_sq_error, synthetic_inputs
from test_adaptive_gpu import MASKS, RH, RW, TARGETS

pytestmark = pytest.mark.gpu

HR_ERR_INVALID = -1
ALL_K = pn.ALL_K


def _counts(K, shape, low=None):
    """Per-pixel counts K .. 3 K + 2 (low: from there instead — 0 puts pixels without samplings and with fewer than K side by side)."""
    c = np.random.default_rng(K + shape[0]).integers(K if low is None else low, 3 * K + 3, size=shape).astype(np.uint32)
    if low is not None and c.size >= 4:
        c.reshape(-1)[:4] = [0, 1, K - 1, K]
    return c


def _err(ha, fn, *a, **kw):
    return error_of(ha, fn, *a, **kw)[0]


# ---------------------------------------------------------------------------------------------------------------- D against the host core

@pytest.mark.parametrize("K", ALL_K)
def test_d_equals_the_host_core(ha, scenes, core, K):
    """Written synthetic buckets (heavy tails and the planted corner cases of the CPU tier) and written guides: D is robust_denoise_image's, bit for
    bit, with levels 0, 1 and 4 (a level is what exposes V), demodulate 0 and 1, on the frame and the region — 851 pixels: three full spans of 256
    and a partial one —, with one count for every pixel and with per-pixel counts; and on a 1 x 1 frame.  K = 15 is the row with 92,160 B of LDS."""
    with renderer(ha, scenes("cornell_mini")[0]) as r:
        for target in sorted(TARGETS) + ["1x1"]:
            frame, region = TARGETS.get(target, ((1, 1), None))
            h, w = (RH, RW) if target != "1x1" else (1, 1)
            g = synthetic_inputs(5, w, h)[3]
            for n in (2 * K + 1, _counts(K, (h, w))):
                per_pixel = not np.isscalar(n)
                retarget(r, frame, region, counts=per_pixel, buckets=K)
                B = pn.synthetic_buckets(900 + K, K, (h, w), n)
                r.write_buckets(B, int(n.max()) if per_pixel else n)
                if per_pixel:
                    r.write_sample_counts(n)
                r.write_guides(g)
                for levels in (0, 1, 4):
                    for dem in (0, 1):
                        r.denoise_robust(levels=levels, demodulate=dem)
                        want = pc.core_filter(core, B, n, g, levels=levels, demodulate=dem)
                        assert same(r.read_denoised(), want), (K, target, per_pixel, levels, dem)
                if target == "frame" and not per_pixel:
                    assert not same(pc.core_filter(core, B, n, g, levels=1), pc.core_filter(core, B, n, g, levels=0))


@pytest.mark.parametrize("K", [9, 3])
def test_levels_zero_is_the_robust_image(ha, scenes, K):
    """Rendered buckets, guide planes the call renders itself: with levels = 0 D is R bit for bit and its resolve is hr_resolve_robust's bytes."""
    with renderer(ha, scenes("rtcamp6_v3_1")[0]) as r:
        for target in sorted(TARGETS):
            retarget(r, *TARGETS[target], buckets=K)
            r.render(1, 21)
            r.robust()
            R, img = r.read_robust(), r.resolve_robust()
            for dem in (0, 1):
                r.denoise_robust(levels=0, demodulate=dem)
                assert same(r.read_denoised(), R) and np.array_equal(r.resolve_denoised(), img), (K, target, dem)
            assert r.read_guides().any()                                               # the call rendered them
            assert same(r.read_robust(), R)                                            # R is still valid
            r.denoise_robust()
            assert not same(r.read_denoised(), R) and np.isfinite(r.read_denoised()).all()


@pytest.mark.parametrize("K", ALL_K)
def test_robust_equals_the_run_time_definition(ha, scenes, core, K):
    """hr_robust runs robust_kernel<K>: R and the trim plane against the host build of robust_pixel (run-time K), bit for bit, with counts that
    include 0 and values below K, and with one count for every pixel — below K, K, and more."""
    with renderer(ha, scenes("cornell_mini")[0]) as r:
        for target in sorted(TARGETS):
            counts = _counts(K, (RH, RW), low=0)
            retarget(r, *TARGETS[target], counts=True, buckets=K)
            B = pn.synthetic_buckets(950 + K, K, (RH, RW), counts)
            r.write_buckets(B, 123)
            r.write_sample_counts(counts)
            r.robust()
            R, trim = pc.core_r(core, B, counts)
            assert same(r.read_robust(), R) and np.array_equal(r.read_robust_trim(), trim), (K, target)
            assert (r.read_robust()[counts == 0] == 0).all()
            retarget(r, *TARGETS[target], buckets=K)
            for n in (0, K - 1, K, 2 * K + 1):
                B = pn.synthetic_buckets(960 + K, K, (RH, RW), max(n, 1))
                r.write_buckets(B, n)
                r.robust()
                R, trim = pc.core_r(core, B, n)
                assert same(r.read_robust(), R) and np.array_equal(r.read_robust_trim(), trim), (K, target, n)


# ---------------------------------------------------------------------------------------------------------------- refusals and state

def _state(r):
    return r.read_robust(), r.read_buckets(), r.read_sample_counts(), r.tile_mask()


def _same_state(a, b):
    return same(a[0], b[0]) and same(a[1][0], b[1][0]) and a[1][1] == b[1][1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3][0], b[3][0]) and a[3][1] == b[3][1]


def test_refusals_touch_nothing(ha, scenes):
    K = 9
    g = synthetic_inputs(5, RW, RH)[3]
    with renderer(ha, scenes("cornell_mini")[0], None, None, *TARGETS["frame"], counts=True) as r:
        assert _err(ha, r.denoise_robust) == HR_ERR_INVALID                            # the option is off
        r.set_option("robust_buckets", K)
        counts = _counts(K, (RH, RW))
        B = pn.synthetic_buckets(1, K, (RH, RW), counts)
        r.write_buckets(B, int(counts.max()))
        r.write_sample_counts(counts)
        r.write_guides(g)
        r.set_tile_mask(MASKS["checker"])
        r.robust()
        r.denoise_robust()
        D, before = r.read_denoised(), _state(r)
        # hr_denoise's parameter refusals: D stays, valid
        for bad in ({"levels": 6}, {"demodulate": 2}, {"sigma_color": 0.0}, {"sigma_normal": -1.0}, {"sigma_albedo": float("inf")}, {"sigma_depth": float("nan")}):
            assert _err(ha, r.denoise_robust, **bad) == HR_ERR_INVALID, bad
            assert same(r.read_denoised(), D) and _same_state(_state(r), before), bad
        # a pixel with fewer than K samplings; a count beyond the samplings behind the buckets.  (Writing the counts has invalidated D and R
        # already: R is made again, D stays invalid, and nothing else moves.)
        low, high = counts.copy(), counts.copy()
        low[7, 9] = K - 1
        high[7, 9] = int(counts.max()) + 1
        for bad in (low, high):
            r.write_sample_counts(bad)
            r.robust()
            before = _state(r)
            assert _err(ha, r.denoise_robust) == HR_ERR_INVALID
            assert _err(ha, r.read_denoised) == HR_ERR_INVALID and _same_state(_state(r), before)
        r.write_sample_counts(counts)
        r.denoise_robust()
        assert same(r.read_denoised(), D)
        # without the counts: fewer samplings behind the buckets than buckets
        r.set_tile_mask(None)
        retarget(r, *TARGETS["frame"], buckets=K)
        r.write_buckets(B, K - 1)
        r.write_guides(g)
        assert _err(ha, r.denoise_robust) == HR_ERR_INVALID and _err(ha, r.read_denoised) == HR_ERR_INVALID
        assert same(r.read_buckets()[0], B) and r.read_buckets()[1] == K - 1
        r.write_buckets(B, K)
        r.denoise_robust()


def test_validity(ha, scenes):
    """A D of hr_denoise_robust goes stale with everything a D of hr_denoise goes stale with (DESIGN.md §4.9's list — every hr_write_*,
    hr_write_buckets among them, is on it) AND with switching robust_buckets; a D of hr_denoise keeps its own rules: another K leaves it readable."""
    K = 9
    sc = scenes("cornell_mini")[0]
    with renderer(ha, sc, None, None, *TARGETS["frame"], moments=True, buckets=K) as r:
        r.render(1, 12)
        B, n = r.read_buckets()
        acc, g = r.read_accumulator(), None

        def fresh():
            """K buckets of 11 samplings without per-pixel counts, and a D of hr_denoise_robust made of them"""
            r.set_option("sample_counts", 0)
            r.set_option("robust_buckets", K)
            r.write_buckets(B, n)
            r.denoise_robust()
            assert r.read_denoised().shape == (RH, RW, 3) and r.resolve_denoised().shape == (RH, RW, 3)

        fresh()
        g = r.read_guides()
        r.set_option("robust_buckets", K)                                              # the value it has: D stays
        assert r.read_denoised().shape == (RH, RW, 3)
        for what, call in [("write_buckets", lambda: r.write_buckets(B, n)), ("another K", lambda: r.set_option("robust_buckets", 5)),
                           ("robust_buckets off", lambda: r.set_option("robust_buckets", 0)), ("render", lambda: r.render(12, 13)), ("clear", r.clear),
                           ("write_accumulator", lambda: r.write_accumulator(acc)), ("write_guides", lambda: r.write_guides(g)),
                           ("render_guides", r.render_guides), ("guide_bounces", lambda: r.set_option("guide_bounces", 2)),
                           ("sample_counts on", lambda: r.set_option("sample_counts", 1))]:
            fresh()
            call()
            assert _err(ha, r.read_denoised) == HR_ERR_INVALID and _err(ha, r.resolve_denoised) == HR_ERR_INVALID, what
        r.set_option("sample_counts", 0)
        # a D of hr_denoise: switching robust_buckets is none of its business, as before; hr_write_buckets invalidates it, as every hr_write_* does
        r.set_option("guide_bounces", 0)
        r.set_option("robust_buckets", K)
        r.clear()
        r.render(1, 12)
        r.denoise()
        D = r.read_denoised()
        r.set_option("robust_buckets", 5)
        assert same(r.read_denoised(), D)
        r.set_option("robust_buckets", 0)
        assert same(r.read_denoised(), D)
        # the context remembers which call made D: the last one
        r.set_option("robust_buckets", K)
        r.write_buckets(B, n)
        r.denoise_robust()
        r.denoise()
        r.set_option("robust_buckets", 5)
        assert same(r.read_denoised(), D)
        r.write_buckets(np.zeros((RH, RW, 5, 3)), 5)
        assert _err(ha, r.read_denoised) == HR_ERR_INVALID


def test_asking_changes_nothing_else(ha, scenes):
    sc = scenes("rtcamp6_v3_1")[0]
    quiet, asks = (renderer(ha, sc, None, None, *TARGETS["frame"], moments=True, counts=True, buckets=9) for _ in range(2))
    try:
        launches = []
        for r in (quiet, asks):
            r.render(1, 10)
            if r is asks:
                before = r.stats()
                r.denoise_robust()
                after = r.stats()
                assert after["post_kernel_ms"] > before["post_kernel_ms"] and after["trace_launches"] == before["trace_launches"]
            r.set_tile_mask(MASKS["checker"])
            r.render(10, 15)
            launches.append(r.stats()["trace_launches"])
        assert same(quiet.read_accumulator(), asks.read_accumulator()) and same(quiet.read_moments()[0], asks.read_moments()[0])
        assert np.array_equal(quiet.read_sample_counts(), asks.read_sample_counts()) and quiet.read_moments()[1] == asks.read_moments()[1]
        assert same(quiet.read_buckets()[0], asks.read_buckets()[0]) and quiet.read_buckets()[1] == asks.read_buckets()[1]
        assert launches[0] == launches[1]
    finally:
        quiet.close()
        asks.close()


# ---------------------------------------------------------------------------------------------------------------- quality

@pytest.mark.parametrize("name", ["cornell_mini", "rtcamp6_v3_1"])
def test_quality_on_the_device(ha, scenes, name):
    """The CPU tier's configuration — 96x54, 16 samplings, guide_bounces 2, default parameters — with the truth rendered by hr_render from
    samplings 100001 .. 101024: the denoised R beats R alone and beats hr_denoise on the same samplings (K = 5 asserted, K = 9 printed)."""
    w, h, n, truth_n = pq.SHORT_W, pq.SHORT_H, pq.SHORT_N, 1024
    with ha.Renderer(0) as r:
        r.upload_scene(scenes(name)[0])
        r.set_resolution(w, h)
        r.set_option("guide_bounces", pq.SHORT_BOUNCES)
        r.set_option("moments", 1)
        got = {}
        for K in (5, 9):
            r.set_option("robust_buckets", K)
            r.clear()
            r.render(1, n + 1)
            mean = r.read_accumulator() / np.float32(4 * n)
            r.robust()
            R = r.read_robust()
            r.denoise()
            D = r.read_denoised()
            r.denoise_robust()
            got[K] = (mean, R, D, r.read_denoised())
        r.set_option("robust_buckets", 0)
        r.set_option("moments", 0)
        r.clear()
        r.render(100001, 100001 + truth_n)
        truth = r.read_accumulator().astype(np.float64) / (4.0 * truth_n)
    for K in (5, 9):
        e_mean, e_r, e_d, e_dr = (rel_sq_error(x, truth) for x in got[K])
        print("%s on the device n=%d K=%d: R/mean %.3f  D/mean %.3f  DR/R %.3f  DR/D %.3f" % (name, n, K, e_r / e_mean, e_d / e_mean, e_dr / e_r, e_dr / e_d))
        if K == 5:
            assert e_dr / e_r < 1.0 and e_dr / e_d < 1.0


# ---------------------------------------------------------------------------------------------------------------- the CLI

CLI_ARGS = ["--assets", ASSETS, "--scene", "cornell_mini", "-w", str(RW), "-h", str(RH), "-t", "1000", "-i", "1000"]


def test_cli_robust_denoise(ha, scenes, tmp_path):
    full, short = tmp_path / "full", tmp_path / "short"
    r = run_cli(CLI_ARGS + ["-s", "16", "--robust", "5", "--robust-denoise", "--guide-bounces", "2"], full, timeout=120)
    assert r.returncode == 0 and "is not denoised" not in r.stdout, r.stdout
    r = run_cli(CLI_ARGS + ["-s", "3", "--robust", "5", "--robust-denoise", "--guide-bounces", "2"], short, timeout=120)
    assert r.returncode == 0 and r.stdout.count("robust-denoise: fewer than K samplings behind a pixel, the robust image is not denoised.") == 1, r.stdout
    with renderer(ha, scenes("cornell_mini")[0], {"guide_bounces": 2}, None, (RW, RH), buckets=5) as lib:
        lib.render(1, 17)
        lib.denoise_robust()
        assert np.array_equal(ha.decode_image(str(full / "result.png"))[..., :3], lib.resolve_denoised())
        lib.robust()
        assert not np.array_equal(lib.resolve_robust(), lib.resolve_denoised())
        lib.clear()
        lib.render(1, 4)
        lib.robust()
        assert np.array_equal(ha.decode_image(str(short / "result.png"))[..., :3], lib.resolve_robust())
