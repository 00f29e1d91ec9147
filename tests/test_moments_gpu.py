"""Per-pixel sample moments and the noise estimate (option "moments") on the MI355X.  The definition is exact: x_s, a sampling's
contribution to a pixel, is what `clear; render(s, s + 1); read_accumulator` returns today, S1 / S2 are their sums in f64 in the order rendered —
so the moments are checked to the bit against the library's own per-sampling renders, whatever the launch cuts, shading mode and pipeline."""
import re

import numpy as np
import pytest

import ckpt
from cli import ASSETS, run_cli
from gpu_helpers import error_of, renderer, same
from post_numpy import noise_reference, ulp_distance

pytestmark = pytest.mark.gpu

W, H, S = 96, 54, 24
REGION = (29, 17, 40, 24)
SCENES = ["spheres", "rtcamp6_v3_1"]    # no meshes (precise shading in the megakernel by default) / a mesh scene
# (options, debug options) of the renders whose moments are checked
CONFIGS = {"default": ({}, {}), "fp32": ({"precise_shading": 0}, {}), "precise": ({"precise_shading": 1}, {}),
           "mega": ({}, {"trace_mode": 0}), "split": ({}, {"trace_mode": 1}),
           "fp32-split": ({"precise_shading": 0}, {"trace_mode": 1}), "precise-mega": ({"precise_shading": 1}, {"trace_mode": 0})}


def _make(ha, sc, opts=None, dbg=None, region=None, moments=True):
    return renderer(ha, sc, opts, dbg, (W, H), region, moments=moments)


def _err(ha, fn, *a):
    return error_of(ha, fn, *a)[0]


def _per_sampling(r, samplings):
    """x_s the parent's way: one sampling into a zeroed accumulator."""
    xs = []
    for s in samplings:
        r.clear()
        r.render(s, s + 1)
        xs.append(r.read_accumulator())
    return np.stack(xs)


def _moments_of(xs):
    """S1, S2 by a sequential f64 loop (cumsum: one value at a time, in order — np.sum adds pairwise, another order)."""
    x = xs.astype(np.float64)
    return np.concatenate([np.cumsum(x, axis=0)[-1], np.cumsum(x * x, axis=0)[-1]], axis=-1)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_moments_to_the_bit(ha, scenes, name, config):
    sc, _ = scenes(name)
    opts, dbg = CONFIGS[config]
    ref_r = _make(ha, sc, opts, dbg, moments=False)
    r = _make(ha, sc, opts, dbg)
    try:
        xs = _per_sampling(ref_r, range(1, S + 1))
        assert np.isfinite(xs).all() and xs.sum() > 0 and xs.std(axis=0).max() > 0
        ref = _moments_of(xs)
        for batch, cuts in [(0, [(1, S + 1)]), (1, [(1, S + 1)]), (5, [(1, S + 1)]), (0, [(1, 10), (10, S + 1)]), (5, [(1, 8), (8, S + 1)])]:
            r.set_option("batch", batch)
            r.clear()
            for a, b in cuts:
                r.render(a, b)
            mom, n = r.read_moments()
            assert n == S and mom.shape == (H, W, 6)
            assert same(mom, ref), (name, config, batch, cuts, float(np.abs(mom - ref).max()))
        # a stride-2 shard against its own samplings
        r.set_option("batch", 0)
        for first in (1, 2):
            r.clear()
            r.render(first, S + 1, 2)
            mom, n = r.read_moments()
            assert n == S // 2
            assert same(mom, _moments_of(xs[first - 1::2])), (name, config, "stride 2 from", first)
    finally:
        r.close()
        ref_r.close()


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("config", ["default", "fp32", "split"])
def test_the_accumulator_does_not_move(ha, scenes, name, config):
    sc, _ = scenes(name)
    opts, dbg = CONFIGS[config]
    accs = []
    for on in (False, True):
        with _make(ha, sc, opts, dbg, moments=on) as r:
            r.render(1, 8)
            r.set_option("batch", 3)
            r.render(8, S + 1)
            r.render(2, S + 1, 3)
            accs.append(r.read_accumulator())
            img = r.resolve(S)
        accs.append(img)
    assert np.array_equal(accs[0].view(np.uint32), accs[2].view(np.uint32)) and np.array_equal(accs[1], accs[3])


@pytest.mark.parametrize("name", SCENES)
def test_region_moments_are_the_frames_window(ha, scenes, name):
    sc, _ = scenes(name)
    full = _make(ha, sc)
    reg = _make(ha, sc, region=REGION)
    try:
        full.render(1, S + 1)
        reg.render(1, S + 1)
        mf, nf = full.read_moments()
        mr, nr = reg.read_moments()
        x0, y0, w, h = REGION
        assert nf == nr == S and mr.shape == (h, w, 6)
        assert same(mr, mf[y0:y0 + h, x0:x0 + w])
        # the region's noise image is the estimate of the same moments
        assert np.array_equal(reg.noise_image(0.01), full.noise_image(0.01)[y0:y0 + h, x0:x0 + w])
        assert reg.noise_estimate(0.01, 0.05)["pixels"] == w * h
    finally:
        full.close()
        reg.close()


def test_life_cycle(ha, scenes):
    HR_ERR_INVALID, HR_ERR_NO_TARGET, HR_ERR_UNSUPPORTED = -1, -4, -6
    sc, _ = scenes("rtcamp6_v3_1")
    r = ha.Renderer(0)
    r2 = None
    try:
        r.upload_scene(sc)
        assert _err(ha, r.set_option, "moments", 1) == HR_ERR_NO_TARGET      # before hr_set_resolution
        r.set_resolution(W, H)
        # off: the four functions refuse
        assert _err(ha, r.read_moments) == HR_ERR_INVALID and _err(ha, r.write_moments, np.zeros((H, W, 6)), 3) == HR_ERR_INVALID
        assert _err(ha, r.noise_estimate, 0.01, 0.05) == HR_ERR_INVALID and _err(ha, r.noise_image, 0.01) == HR_ERR_INVALID
        assert _err(ha, r.set_option, "moments", 2) == HR_ERR_INVALID
        r.render_debug(2)                                                       # allowed while off
        r.clear()
        r.set_option("moments", 1)
        mom, n = r.read_moments()
        assert n == 0 and not mom.any()
        assert _err(ha, r.render_debug, 2) == HR_ERR_UNSUPPORTED
        # n < 2: no variance
        assert _err(ha, r.noise_estimate, 0.01, 0.05) == HR_ERR_INVALID
        r.render(1, 2)
        assert r.read_moments()[1] == 1 and _err(ha, r.noise_estimate, 0.01, 0.05) == HR_ERR_INVALID and _err(ha, r.noise_image, 0.01) == HR_ERR_INVALID
        r.render(2, 3)
        assert r.noise_estimate(0.01, 0.05)["samplings"] == 2
        assert _err(ha, r.noise_estimate, 0.0, 0.05) == HR_ERR_INVALID and _err(ha, r.noise_estimate, -1.0, 0.05) == HR_ERR_INVALID
        assert _err(ha, r.noise_estimate, float("nan"), 0.05) == HR_ERR_INVALID
        # hr_clear, hr_set_region, hr_set_resolution zero moments and count (the last two at the new size)
        r.clear()
        mom, n = r.read_moments()
        assert n == 0 and not mom.any()
        r.render(1, 4)
        r.set_region(*REGION)
        mom, n = r.read_moments()
        assert n == 0 and mom.shape == (REGION[3], REGION[2], 6) and not mom.any()
        r.render(1, 4)
        assert r.read_moments()[1] == 3 and r.read_moments()[0].any()
        r.set_resolution(64, 32)
        mom, n = r.read_moments()
        assert n == 0 and mom.shape == (32, 64, 6) and not mom.any()
        # hr_write_accumulator does not touch them; write -> read is exact
        r.render(1, 4)
        before, n = r.read_moments()
        r.write_accumulator(np.ones((32, 64, 3), dtype=np.float32))
        after, n2 = r.read_moments()
        assert n == n2 == 3 and same(before, after)
        rng = np.random.default_rng(7)
        data = rng.standard_normal((32, 64, 6)) * 10.0 ** rng.integers(-300, 60, (32, 64, 6))
        r.write_moments(data, 123456789012)
        back, n = r.read_moments()
        assert n == 123456789012 and same(back, data)
        # off frees, on again starts from zero
        r.set_option("moments", 0)
        assert _err(ha, r.read_moments) == HR_ERR_INVALID
        r.set_option("moments", 1)
        mom, n = r.read_moments()
        assert n == 0 and not mom.any()
        # two shards: moments added on the host in rank order, written into one context -> the count S and the whole render's estimate
        r.set_resolution(W, H)
        r2 = _make(ha, sc)
        r.render(1, S + 1, 2)
        r2.render(2, S + 1, 2)
        (m0, n0), (m1, n1) = r.read_moments(), r2.read_moments()
        assert n0 == n1 == S // 2
        r2.write_moments(m0 + m1, n0 + n1)
        tot, n = r2.read_moments()
        assert n == S and same(tot, m0 + m1)
        est = r2.noise_estimate(0.01, 0.05)
        assert est["samplings"] == S and est["pixels"] == W * H and 0 < est["mean_error"] < est["max_error"]
        # the same samplings rendered by one context: the same sums up to the order of the additions
        r.clear()
        r.render(1, S + 1)
        one, _n = r.read_moments()
        assert np.allclose(one, tot, rtol=1e-12, atol=0)
    finally:
        r.close()
        if r2 is not None:
            r2.close()


@pytest.mark.parametrize("name", SCENES)
def test_noise_map_and_summary(ha, scenes, name):
    sc, _ = scenes(name)
    with _make(ha, sc) as r:
        r.render(1, S + 1)
        mom, n = r.read_moments()
        for floor, thr in [(0.01, 0.05), (0.5, 0.01), (1e-6, 1.0)]:
            img = r.noise_image(floor)
            ref = noise_reference(mom, n, floor)
            assert img.shape == (H, W) and np.isfinite(img).all() and (img >= 0).all() and img.max() > 0
            d = ulp_distance(img, ref)
            print("%s floor %g: worst %d ulp, mean e %.6f, max e %.6f" % (name, floor, int(d.max()), img.mean(), img.max()))
            assert d.max() <= 4
            est = r.noise_estimate(floor, thr)
            assert est["samplings"] == S and est["pixels"] == W * H
            assert est["max_error"] == img.max()
            assert est["pixels_above"] == int((img > thr).sum())
            assert abs(est["mean_error"] - img.mean()) <= 1e-9 * img.mean()
            again = r.noise_estimate(floor, thr)
            assert again == est and np.float64(again["mean_error"]).tobytes() == np.float64(est["mean_error"]).tobytes()
            assert np.array_equal(r.noise_image(floor), img)
        assert 0 < r.noise_estimate(0.01, 0.05)["pixels_above"] <= W * H


@pytest.mark.parametrize("name,oracle_rms", [("rtcamp6_v3_1", 1.0040), ("cornell_mini", 1.0143)])
def test_the_estimate_means_something(ha, scenes, name, oracle_rms):
    """Two disjoint sets of samplings (1..64 and 65..128) of one scene at 96x54: per pixel and channel z = (mu_A - mu_B) / sqrt(se_A^2 + se_B^2)
    over the pixels with se > 0 in both sets; the RMS of z is 1 for a correct standard error, and a forgotten / 4, / n or sqrt moves it by a
    factor of 2 or more: the gate is [0.6, 1.6].  Path-traced samples are heavy-tailed, so scene and size were fixed from the CPU oracle first
    (per-sampling accumulators of its render(), the same statistic in numpy, 96x54, 2 x 64 samplings): rtcamp6_v3_1 1.0040 (15,115 of
    15,552 channels), cornell_mini 1.0143 (12,727), simple 1.0116 (6,723) — all inside [0.8, 1.25].  "spheres" gives 0.38 in the oracle (7,561
    channels): there the per-sampling values of a pixel vary less between sets than within one, the estimate is conservative; it is not
    used as a gate."""
    assert 0.8 <= oracle_rms <= 1.25
    sc, _ = scenes(name)
    with _make(ha, sc) as r:
        stats = []
        for first in (1, 65):
            r.clear()
            r.render(first, first + 64)
            mom, n = r.read_moments()
            assert n == 64
            m = mom[..., :3] / n
            var = np.maximum(0.0, (mom[..., 3:] - mom[..., :3] * m) / (n - 1))
            stats.append((m / 4.0, np.sqrt(var / n) / 4.0))
    (ma, sa), (mb, sb) = stats
    k = (sa > 0) & (sb > 0)
    z = (ma - mb)[k] / np.sqrt(sa[k] ** 2 + sb[k] ** 2)
    rms = float(np.sqrt((z ** 2).mean()))
    print("%s: RMS of z %.4f over %d of %d channels (oracle %.4f)" % (name, rms, int(k.sum()), k.size, oracle_rms))
    assert k.sum() > 5000 and 0.6 <= rms <= 1.6, rms


def _noise_lines(text):
    return [(int(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4)))
            for m in re.finditer(r"^noise: samplings=(\d+) mean=(\S+) max=(\S+) above=(\d+)$", text, re.M)]


def test_cli_noise_target(tmp_path, ha, scenes):
    """rtcamp6_v3_1 at 96x54.  The target comes from a trial run the test makes itself (`-s 64 --noise-target 0`: its one `noise:` line is
    what 64 samplings reach; the moments do not depend on launch cuts, so the 256-sampling run meets the same value at its first check):
    E = 1.05 x that mean, so the run with `-s 256` has to stop at 64."""
    from PIL import Image
    base = ["--assets", ASSETS, "-w", W, "-h", H, "-t", 1000, "-i", 1000]
    d0 = tmp_path / "trial"
    d0.mkdir()
    p = run_cli(base + ["-s", 64, "--noise-target", 0], d0, timeout=300)
    assert p.returncode == 0, p.stdout
    trial = _noise_lines(p.stdout)
    print("trial:", trial)
    assert [l[0] for l in trial] == [64] and trial[0][1] > 0
    CLI_TARGET = float("%.6g" % (1.05 * trial[0][1]))
    d1 = tmp_path / "a"
    d1.mkdir()
    p = run_cli(base + ["-s", 256, "--noise-target", CLI_TARGET, "--noise-image", "noise.png"], d1, timeout=300)
    assert p.returncode == 0, p.stdout
    lines = _noise_lines(p.stdout)
    done = int(re.search(r"^sampled: (\d+)x4 spp\.$", p.stdout, re.M).group(1))
    assert lines and done == 64 and lines[-1][0] == done and lines[-1][1] <= CLI_TARGET, p.stdout
    assert lines[0][:3] == trial[0][:3]
    assert "reached noise target" in p.stdout
    assert p.stdout.index("rendering: %dx4 sampled" % lines[0][0]) < p.stdout.index("noise: samplings=%d " % lines[0][0])
    assert all(m > CLI_TARGET for _, m, _, _ in lines[:-2])             # it stopped at the first check that met the target
    result = open(d1 / "result.txt").read()
    assert _noise_lines(result) == [lines[-1]] and "sampled: %dx4 spp." % done in result
    assert np.asarray(Image.open(d1 / "result.png")).shape == (H, W, 3)
    # the final image is resolved with the samplings actually rendered
    sc, _ = scenes("rtcamp6_v3_1")
    with _make(ha, sc) as r:
        r.render(1, done + 1)
        exp = r.resolve(done)
        est = r.noise_estimate(0.01, CLI_TARGET)
        e_img = r.noise_image(0.01)
    assert np.array_equal(np.asarray(Image.open(d1 / "result.png")), exp)
    assert lines[-1] == (done, float("%.9g" % est["mean_error"]), float("%.9g" % est["max_error"]), est["pixels_above"])
    grey = np.asarray(Image.open(d1 / "noise.png"))
    assert grey.shape[:2] == (H, W)
    g = grey[..., 0] if grey.ndim == 3 else grey
    assert np.array_equal(g, (np.minimum(1.0, e_img / CLI_TARGET) * 255.0 + 0.5).astype(np.uint8))
    # a target of 0 is never reached: all 8 samplings, one estimate at the end
    d2 = tmp_path / "b"
    d2.mkdir()
    p = run_cli(base + ["-s", 8, "--noise-target", 0, "--checkpoint", "ck8"], d2, timeout=300)
    assert p.returncode == 0 and "sampled: 8x4 spp." in p.stdout and "reached max sampling" in p.stdout, p.stdout
    assert [l[0] for l in _noise_lines(p.stdout)] == [8]
    # checkpoint -> resume continues the count: 8 + 8 samplings leave the moments of a straight 16 (they do not depend on launch cuts)
    p = run_cli(base + ["-s", 16, "--noise-target", 0, "--resume", "ck8", "--checkpoint", "ck16"], d2, timeout=300)
    assert p.returncode == 0 and "resumed at 8x4 sampled" in p.stdout, p.stdout
    assert [l[0] for l in _noise_lines(p.stdout)] == [16]
    d3 = tmp_path / "c"
    d3.mkdir()
    p = run_cli(base + ["-s", 16, "--noise-target", 0, "--checkpoint", "ck16"], d3, timeout=300)
    assert p.returncode == 0, p.stdout
    acc_bytes = 20 + W * H * 12

    def trailer(path):
        c = ckpt.read(path)
        assert c.used == c.size == acc_bytes + 12 + W * H * 48 and c.has_moments and c.complete == ckpt.S_MOMENTS   # "HRMS" behind the accumulator, nothing else
        return c.moments_n, c.moments.tobytes()
    (n_a, mom_a), (n_b, mom_b) = trailer(d2 / "ck16"), trailer(d3 / "ck16")
    assert n_a == n_b == 16 and mom_a == mom_b
    assert trailer(d2 / "ck8")[0] == 8
    # a file written without moments keeps today's bytes, and cannot be resumed with a noise target
    p = run_cli(base + ["-s", 4, "--checkpoint", "plain"], d3, timeout=300)
    assert p.returncode == 0 and not _noise_lines(p.stdout), p.stdout
    assert len(open(d3 / "plain", "rb").read()) == acc_bytes
    p = run_cli(base + ["-s", 8, "--resume", "plain", "--noise-target", 0.05], d3, timeout=300)
    assert p.returncode == 1 and "--noise-target" in p.stdout and "moments" in p.stdout, p.stdout
    # only the image asked for: E = 0.05, no early stop
    p = run_cli(base + ["-s", 4, "--noise-image", "n.png"], d3, timeout=300)
    assert p.returncode == 0 and "sampled: 4x4 spp." in p.stdout and [l[0] for l in _noise_lines(p.stdout)] == [4], p.stdout
    assert np.asarray(Image.open(d3 / "n.png")).shape[:2] == (H, W)
