"""The error estimate of hr_denoise_select's image on the MI355X: the four entry points against csrc/select_noise_core.h compiled
for the host — M bit for bit, e_S within 4 ulp — on written planes, the summary against the image it reads, the tile selection against the rule
applied to that image, the promise that the calls touch nothing, the refusals, a rendered case, and the CLI's --auto-noise."""
import ctypes as C
import re

import numpy as np
import pytest

from cli import ASSETS, run_cli
from gpu_helpers import error_of, renderer, retarget, same
from post_numpy import bits, ulp_distance
from select_noise_cores import core_errors, core_select_noise, noise_core  # noqa: F401  (noise_core: the g++-built harness, a fixture)
from select_noise_numpy import numpy_tile_rule, synthetic

pytestmark = pytest.mark.gpu

HR_ERR_INVALID = -1
FLOOR = 0.01
BLOCKS, THREADS = 1024, 256                        # select_noise_error_kernel's grid (post_kernels.h)


def _err(ha, fn, *a, **kw):
    return error_of(ha, fn, *a, **kw)[0]


def _checker(w, h):
    ty, tx = (h + 3) // 4, (w + 3) // 4
    yy, xx = np.mgrid[0:ty, 0:tx]
    return ((xx + yy) & 1).astype(np.uint8)


def mixed_counts(seed, w, h):
    cnt = np.random.default_rng(seed).integers(2, 65, size=(h, w)).astype(np.uint32)
    cnt.reshape(-1)[:2] = [2, 64]
    return cnt


def write_planes(r, B, acc, mom, n, g):
    """the five planes of a render, written: the context then holds what `synthetic` made"""
    per_pixel = not np.isscalar(n)
    n_all = int(n.max()) if per_pixel else int(n)
    r.write_accumulator(acc)
    r.write_moments(mom, n_all)
    r.write_buckets(B, n_all)
    if per_pixel:
        r.write_sample_counts(n)
    r.write_guides(g)


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


def check_against_core(r, noise_core, B, acc, mom, n, g, where):
    for levels in (0, 3):
        for smooth in (0, 2):
            for dem in (0, 1):
                S, L, M = core_select_noise(noise_core, B, acc, mom, n, g, smooth=smooth, levels=levels, demodulate=dem)
                got = r.selected_mse(smooth=smooth, levels=levels, demodulate=dem)
                assert same(got, M), where + (levels, smooth, dem)
                e = r.selected_noise_image(FLOOR, smooth=smooth, levels=levels, demodulate=dem)
                ref = core_errors(noise_core, M, S, FLOOR)
                assert ulp_distance(e, ref).max() <= 4, where + (levels, smooth, dem)
                assert (e[M == 0.0] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------- M and e_S against the host core

# 13x7: one partial workgroup, the level-3 taps leave the image; 37x19: two workgroups of the 32x8 kernels in either direction, ragged tiles
@pytest.mark.parametrize("w,h", [(13, 7), (37, 19)])
@pytest.mark.parametrize("K", [3, 9])
def test_m_and_error_equal_the_host_core(ha, scenes, noise_core, w, h, K):
    with renderer(ha, scenes("cornell_mini")[0]) as r:
        for n in (2 * K + 1, mixed_counts(w * h + K, w, h)):
            per_pixel = not np.isscalar(n)
            retarget(r, (w, h), None, moments=True, counts=per_pixel, buckets=K)
            B, acc, mom, n, g = synthetic(400 + K, w, h, K, n)
            write_planes(r, B, acc, mom, n, g)
            check_against_core(r, noise_core, B, acc, mom, n, g, (w, h, K, per_pixel))


def test_on_a_region_with_an_origin(ha, scenes, noise_core):
    w, h, K = 37, 19, 9
    with renderer(ha, scenes("cornell_mini")[0]) as r:
        retarget(r, (64, 48), (5, 3, w, h), moments=True, counts=True, buckets=K)
        B, acc, mom, n, g = synthetic(77, w, h, K, mixed_counts(9, w, h))
        write_planes(r, B, acc, mom, n, g)
        check_against_core(r, noise_core, B, acc, mom, n, g, ("region",))


def test_equal_samplings_give_zero_on_the_device(ha, scenes):
    """K = 3, n = 12, every bucket 16 r: no variance and equal halves — M is +0.0 and e_S is 0 in every pixel, whatever the levels."""
    w, h, K, n = 21, 11, 3, 12
    rr = np.random.default_rng(17).integers(1, 64, size=(h, w, 3)).astype(np.float64) / 8.0
    B = np.repeat((16.0 * rr)[:, :, None, :], K, axis=2)
    acc = (48.0 * rr).astype(np.float32)
    mom = np.concatenate([48.0 * rr, n * (4.0 * rr) ** 2], axis=-1)
    g = synthetic(3, w, h, K, 2)[4]
    with renderer(ha, scenes("cornell_mini")[0], None, None, (w, h), moments=True, buckets=K) as r:
        write_planes(r, B, acc, mom, n, g)
        for levels in (0, 3):
            for smooth in (0, 2):
                assert not bits(r.selected_mse(smooth=smooth, levels=levels)).any(), (levels, smooth)
                assert not r.selected_noise_image(FLOOR, smooth=smooth, levels=levels).any()


# ---------------------------------------------------------------------------------------------------------------- the estimate and the tiles

def test_the_estimate_is_the_summary_of_the_image(ha, scenes):
    w, h, K = 37, 19, 9
    with renderer(ha, scenes("cornell_mini")[0], None, None, (w, h), moments=True, counts=True, buckets=K) as r:
        B, acc, mom, n, g = synthetic(11, w, h, K, mixed_counts(4, w, h))
        write_planes(r, B, acc, mom, n, g)
        for kw in ({}, {"levels": 2, "smooth": 0}):
            img = r.selected_noise_image(FLOOR, **kw)
            assert np.isfinite(img).all() and (img >= 0.0).all()
            thr = float(np.median(img))
            est = r.selected_noise_estimate(FLOOR, thr, **kw)
            assert est["samplings"] == int(n.max()) and est["pixels"] == w * h
            assert est["pixels_above"] == int((img > thr).sum()) and 0 < est["pixels_above"] < w * h
            assert np.float64(est["max_error"]).tobytes() == np.float64(img.max()).tobytes()
            assert np.float64(est["mean_error"]).tobytes() == np.float64(fixed_order_sum(img) / (w * h)).tobytes(), kw
            again = r.selected_noise_estimate(FLOOR, thr, **kw)
            assert again == est and np.float64(again["mean_error"]).tobytes() == np.float64(est["mean_error"]).tobytes()
            assert same(r.selected_noise_image(FLOOR, **kw), img)


def test_select_tiles_selected_is_the_rule_on_the_image(ha, scenes):
    w, h, K = 37, 19, 9
    with renderer(ha, scenes("cornell_mini")[0], None, None, (w, h), moments=True, counts=True, buckets=K) as r:
        B, acc, mom, n, g = synthetic(12, w, h, K, mixed_counts(5, w, h))
        write_planes(r, B, acc, mom, n, g)
        img = r.selected_noise_image(FLOOR, levels=3)
        tile_max = np.zeros((((h + 3) // 4) * 4, ((w + 3) // 4) * 4))
        tile_max[:h, :w] = img
        thr = float(np.median(tile_max.reshape((h + 3) // 4, 4, (w + 3) // 4, 4).max(axis=(1, 3))))
        free = numpy_tile_rule(img, thr)
        assert 0 < free.sum() < free.size
        assert r.select_tiles_selected(FLOOR, thr, levels=3) == int(free.sum())        # no mask in force: the rule alone
        assert np.array_equal(r.tile_mask()[0], free)
        planted = _checker(w, h)
        r.set_tile_mask(planted)
        want = numpy_tile_rule(img, thr, prev=planted)
        assert 0 < want.sum() < planted.sum()
        active = r.select_tiles_selected(FLOOR, thr, levels=3)
        mask, n_active = r.tile_mask()
        assert np.array_equal(mask, want) and active == n_active == int(want.sum())
        assert r.select_tiles_selected(FLOOR, thr, levels=3) == active and np.array_equal(r.tile_mask()[0], want)   # a second call: the same mask
        assert same(r.selected_noise_image(FLOOR, levels=3), img) and np.array_equal(r.read_sample_counts(), n)
        r.set_tile_mask(None)
        assert r.select_tiles_selected(FLOOR, float(img.max()), levels=3) == 0 and not r.tile_mask()[0].any()


# ---------------------------------------------------------------------------------------------------------------- it touches nothing

def test_the_calls_touch_nothing(ha, scenes):
    w, h, K = 37, 19, 9
    with renderer(ha, scenes("cornell_mini")[0], None, None, (w, h), moments=True, counts=True, buckets=K) as r:
        kept = (r.read_selected, r.read_selected_levels, r.read_denoised, r.read_robust, r.read_restored)
        r.render(1, 12)
        r.render_guides()
        other = {"levels": 2, "smooth": 0, "sigma_color": 2.0}

        def ask():
            r.selected_noise_estimate(FLOOR, 0.05, **other)
            r.selected_noise_image(FLOOR, **other)
            r.selected_mse(**other)
            r.select_tiles_selected(FLOOR, 0.0, **other)
            r.set_tile_mask(None)

        ask()                                                                          # nothing was valid, nothing has become valid
        for read in kept:
            assert _err(ha, read) == HR_ERR_INVALID, read
        r.denoise_select(levels=4, smooth=2)
        r.robust()
        r.robust_restore()
        for read in (r.read_selected, r.read_selected_levels, r.read_robust, r.read_restored):
            read()
        assert _err(ha, r.read_denoised) == HR_ERR_INVALID                             # (no D has been made)
        ask()
        assert _err(ha, r.read_denoised) == HR_ERR_INVALID
        r.denoise()
        before_images = [read() for read in kept]
        acc, mom, B, counts, g = r.read_accumulator(), r.read_moments(), r.read_buckets(), r.read_sample_counts(), r.read_guides()
        before = r.stats()
        ask()
        after = r.stats()
        for read, was in zip(kept, before_images):
            assert same(read(), was), read
        assert same(r.read_accumulator(), acc) and same(r.read_moments()[0], mom[0]) and same(r.read_buckets()[0], B[0]) and r.read_moments()[1] == mom[1]
        assert np.array_equal(r.read_sample_counts(), counts) and same(r.read_guides(), g)
        moved = sorted(k for k in before if before[k] != after[k])
        assert moved == ["post_kernel_ms"] and after["post_kernel_ms"] > before["post_kernel_ms"], moved


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_refusals_touch_nothing(ha, scenes):
    w, h, K = 37, 19, 9
    with renderer(ha, scenes("cornell_mini")[0], None, None, (w, h), moments=True, counts=True, buckets=K) as r:
        r.render(1, 12)
        r.denoise_select()
        S, L = r.read_selected(), r.read_selected_levels()
        planted = _checker(w, h)
        r.set_tile_mask(planted)
        counts = r.read_sample_counts()
        calls = {"estimate": lambda **kw: r.selected_noise_estimate(kw.pop("floor", FLOOR), kw.pop("threshold", 0.05), **kw),
                 "image": lambda **kw: r.selected_noise_image(kw.pop("floor", FLOOR), **kw),
                 "mse": lambda **kw: r.selected_mse(**kw),
                 "tiles": lambda **kw: r.select_tiles_selected(kw.pop("floor", FLOOR), kw.pop("threshold", 0.05), **kw)}

        def untouched(what):
            assert np.array_equal(r.tile_mask()[0], planted) and np.array_equal(r.read_sample_counts(), counts), what
            assert same(r.read_selected(), S) and np.array_equal(r.read_selected_levels(), L), what

        # the parameters hr_denoise_select refuses
        for bad in ({"levels": 6}, {"demodulate": 2}, {"sigma_color": 0.0}, {"sigma_depth": float("nan")}, {"smooth": 4}):
            for name, call in calls.items():
                assert _err(ha, call, **bad) == HR_ERR_INVALID, (name, bad)
            untouched(bad)
        reserved, n_out, host = ha.SelectParams(0, 1), ha.Noise(), np.zeros((h, w))
        active = C.c_uint32()
        assert r.L.hr_selected_noise_estimate(r._h, None, C.byref(reserved), FLOOR, 0.05, C.byref(n_out)) == HR_ERR_INVALID
        assert r.L.hr_read_selected_noise_image(r._h, None, C.byref(reserved), FLOOR, host.ctypes.data) == HR_ERR_INVALID
        assert r.L.hr_read_selected_mse(r._h, None, C.byref(reserved), host.ctypes.data) == HR_ERR_INVALID
        assert r.L.hr_select_tiles_selected(r._h, None, C.byref(reserved), FLOOR, 0.05, C.byref(active)) == HR_ERR_INVALID
        untouched("reserved")
        # the floor and the threshold
        for bad in ({"floor": 0.0}, {"floor": -1.0}, {"floor": float("nan")}, {"floor": float("inf")}):
            for name in ("estimate", "image", "tiles"):
                assert _err(ha, calls[name], **bad) == HR_ERR_INVALID, (name, bad)
            untouched(bad)
        for name in ("estimate", "tiles"):
            assert _err(ha, calls[name], threshold=-0.5) == HR_ERR_INVALID and _err(ha, calls[name], threshold=float("nan")) == HR_ERR_INVALID, name
        untouched("threshold")
        # NULL = defaults, and a null output
        assert r.L.hr_read_selected_mse(r._h, None, None, host.ctypes.data) == 0 and same(host, r.selected_mse())
        assert r.L.hr_selected_noise_estimate(r._h, None, None, FLOOR, 0.05, None) == HR_ERR_INVALID
        assert r.L.hr_read_selected_mse(r._h, None, None, None) == HR_ERR_INVALID
        untouched("null")
        # a pixel with one sampling (writing the counts makes S stale; the refused calls leave the mask and the counts alone)
        low = counts.copy()
        low[7, 9] = 1
        r.write_sample_counts(low)
        for name, call in calls.items():
            assert _err(ha, call) == HR_ERR_INVALID, name
        assert np.array_equal(r.tile_mask()[0], planted) and np.array_equal(r.read_sample_counts(), low)
        r.write_sample_counts(counts)
        # moments and buckets that do not cover the same samplings
        mom, m_n = r.read_moments()
        r.write_moments(mom, m_n + 1)
        for name, call in calls.items():
            assert _err(ha, call) == HR_ERR_INVALID, name
        r.write_moments(mom, m_n)
        assert r.selected_mse().shape == (h, w)
        assert np.array_equal(r.tile_mask()[0], planted) and np.array_equal(r.read_sample_counts(), counts)
        # the tile call without sample_counts; the others work without them
        r.set_tile_mask(None)
        r.set_option("sample_counts", 0)
        r.clear()
        r.render(1, 12)
        assert _err(ha, calls["tiles"]) == HR_ERR_INVALID
        assert r.tile_mask()[1] == planted.size and r.selected_noise_estimate(FLOOR, 0.05)["samplings"] == 11
        # either option off
        r.set_option("moments", 0)
        for name, call in calls.items():
            assert _err(ha, call) == HR_ERR_INVALID, name
        r.set_option("moments", 1)
        r.set_option("robust_buckets", 0)
        for name, call in calls.items():
            assert _err(ha, call) == HR_ERR_INVALID, name


# ---------------------------------------------------------------------------------------------------------------- a rendered case

def test_rendered_case(ha, scenes):
    """rtcamp6_v3_1 at 96x54, K = 9, default parameters: the mean of M falls from 16 to 64 samplings.  The oracle's samplings through the host core
    say the same (tools/select_noise_quality.py: mean M 0.481 -> 0.120).  The second condition the feature was asked to meet — at 64 samplings the
    selection by e_S keeps no more tiles than the selection by the raw moments' e at the same floor and threshold — does NOT hold for the oracle's
    samplings with the default smooth (0.839 of the tiles against 0.726; with smooth 0: 0.723 against 0.726), so it is not asserted (DESIGN.md
    §4.17 says why); both counts are printed."""
    w, h, K, thr = 96, 54, 9, 0.05
    with renderer(ha, scenes("rtcamp6_v3_1")[0], None, None, (w, h), moments=True, counts=True, buckets=K) as r:
        r.render(1, 17)
        m16 = float(r.selected_mse().mean())
        r.render(17, 65)
        m64 = float(r.selected_mse().mean())
        by_s = r.select_tiles_selected(FLOOR, thr)
        r.set_tile_mask(None)
        by_raw = r.select_tiles(FLOOR, thr)
        print("rtcamp6_v3_1 on the device: mean M %.6g at 16 samplings, %.6g at 64; tiles kept at 64 samplings by e_S %d, by e %d of %d" % (m16, m64, by_s, by_raw, r.tile_mask()[0].size))
        assert 0.0 < m64 < m16


# ---------------------------------------------------------------------------------------------------------------- the CLI
BASE = ["--assets", ASSETS, "--scene", "simple", "-w", 32, "-h", 18, "-t", 1000, "-i", 1000, "--denoise-auto", 3, "--auto-noise", "--noise-check", 8, "--launch", 1]


def _noise_lines(text):
    return [(int(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4)))
            for m in re.finditer(r"^noise: samplings=(\d+) mean=(\S+) max=(\S+) above=(\d+)$", text, re.M)]


def _sampled(text):
    return int(re.search(r"^sampled: (\d+)x4 spp\.$", text, re.M).group(1))


def test_cli_noise_target_asks_the_selected_image(tmp_path, ha, scenes):
    """A trial run with the target 0 prints the estimate at every check; with a target between the first two the run passes the first check and
    stops at the second, where the library's own hr_selected_noise_estimate says the same, and writes the image and the noise map."""
    trial = run_cli(BASE + ["-s", 32, "--noise-target", 0], tmp_path / "trial", timeout=120)
    assert trial.returncode == 0, trial.stdout
    lines = _noise_lines(trial.stdout)
    print("trial:", lines)
    assert len(lines) >= 3 and lines[0][1] > lines[1][1] > 0, lines
    E = float("%.6g" % (0.5 * (lines[0][1] + lines[1][1])))
    run = run_cli(BASE + ["-s", 32, "--noise-target", E, "--noise-image", "noise.png"], tmp_path / "a", timeout=120)
    assert run.returncode == 0 and "reached noise target" in run.stdout, run.stdout
    got, done = _noise_lines(run.stdout), _sampled(run.stdout)
    assert done == lines[1][0] and got[0][:3] == lines[0][:3] and got[0][1] > E and got[-1][0] == done and got[-1][1] <= E, run.stdout
    with renderer(ha, scenes("simple")[0], None, None, (32, 18), moments=True, buckets=3) as r:
        for s in range(1, done + 1):                                                   # one sampling a launch, as --launch 1: the fp32 accumulator adds in that order
            r.render(s, s + 1)
        est = r.selected_noise_estimate(FLOOR, E)
        e_img = r.selected_noise_image(FLOOR)
        r.denoise_select()
        assert np.array_equal(ha.decode_image(str(tmp_path / "a" / "result.png"))[..., :3], r.resolve_selected())
        raw = r.noise_estimate(FLOOR, E)
    assert got[-1] == (done, float("%.9g" % est["mean_error"]), float("%.9g" % est["max_error"]), est["pixels_above"])
    assert raw["mean_error"] != est["mean_error"]                                       # (not the moments' estimate)
    grey = ha.decode_image(str(tmp_path / "a" / "noise.png"))
    assert np.array_equal(grey[..., 0], (np.minimum(1.0, e_img / E) * 255.0 + 0.5).astype(np.uint8))


def test_cli_adaptive_asks_the_selected_image(tmp_path, ha, scenes):
    w, h = 32, 18
    with renderer(ha, scenes("simple")[0], None, None, (w, h), moments=True, buckets=3) as r:
        for s in range(1, 9):                                                          # one sampling a launch, as --launch 1
            r.render(s, s + 1)
        img = r.selected_noise_image(FLOOR)
    ty, tx = (h + 3) // 4, (w + 3) // 4
    padded = np.zeros((ty * 4, tx * 4))
    padded[:h, :w] = img
    E = float("%.6g" % np.median(padded.reshape(ty, 4, tx, 4).max(axis=(1, 3))))    # some tiles stop at the first check, some go on
    run = run_cli(BASE + ["-s", 24, "--adaptive", E, "--sample-image", "samples.png"], tmp_path, timeout=120)
    assert run.returncode == 0, run.stdout
    checks = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"^adaptive: samplings=(\d+) active=(\d+) tiles=(\d+)$", run.stdout, re.M)]
    assert checks and checks[0][0] == 8 and 0 < checks[0][1] < checks[0][2] == tx * ty, run.stdout
    assert checks[0][1] == int(numpy_tile_rule(img, E).sum())                           # the first check is the library's rule on e_S
    assert all(b[1] <= a[1] for a, b in zip(checks, checks[1:]))
    assert (tmp_path / "result.png").exists() and "denoise-auto: buckets=3" in run.stdout, run.stdout
    grey = ha.decode_image(str(tmp_path / "samples.png"))                             # fewer paths than without a mask: some pixels stopped early
    assert grey.shape[:2] == (h, w) and grey[..., 0].max() == 255 and grey[..., 0].min() < 255
