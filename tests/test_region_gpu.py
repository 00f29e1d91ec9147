"""Region rendering (hr_set_region, border / crop render) on the MI355X.  The contract: a path's seed and camera ray come from its pixel's
FRAME coordinates, so pixel (i, j) of a region accumulator is bit-identical to pixel (x0+i, y0+j) of the full-frame render with the same
hr_render calls and options — checked to the bit here for both shading modes, the split pipeline, the debug renderer, tiles stitched from
separate contexts, extreme frames and the CLI."""
import numpy as np
import pytest

import ckpt
from cli import ASSETS, run_cli
from gpu_helpers import renderer

pytestmark = pytest.mark.gpu

W, H = 480, 270
REGIONS = [(37, 21, 101, 63), (0, 0, 1, 1), (0, 100, 480, 5), (467, 263, 13, 7), (0, 0, 480, 270)]
SAMPLINGS = [(1, 9, 1), (3, 16, 3)]
# per scene: (precise_shading, debug options) of each pipeline; "spheres" takes precise shading by default
MODES = {"fp32": ({"precise_shading": 0}, {}), "precise": ({"precise_shading": 1}, {}), "split": ({}, {"trace_mode": 1})}
# the per-scene gates of tests/test_gpu_parity.py (fp32 shading / precise shading)
GATES = {"rtcamp6_v3_1": (0.9998, 0.9995)}
GATES_PRECISE = {"spheres": (0.9998, 0.9997)}


def _render(r, frame, region, s0, s1, stride=1):
    r.set_resolution(*frame)
    if region is not None:
        r.set_region(*region)
    r.render(s0, s1, stride)
    return r.read_accumulator()


def _crop(a, reg):
    x0, y0, w, h = reg
    return a[y0:y0 + h, x0:x0 + w]


@pytest.mark.parametrize("name", ["rtcamp6_v3_1", "spheres", "rtcamp5", "material_examples"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_region_is_a_bit_exact_crop(ha, scenes, name, mode):
    sc, _ = scenes(name)
    with renderer(ha, sc, *MODES[mode]) as r:
        for (s0, s1, st) in SAMPLINGS:
            full = _render(r, (W, H), None, s0, s1, st)
            assert np.isfinite(full).all() and full.sum() > 0
            for reg in REGIONS:
                acc = _render(r, (W, H), reg, s0, s1, st)
                assert acc.shape == (reg[3], reg[2], 3)
                assert np.array_equal(acc, _crop(full, reg)), (name, mode, reg, s0, s1, st)


@pytest.mark.parametrize("name,precise", [("rtcamp6_v3_1", 0), ("spheres", 1)])
def test_region_matches_oracle_region(ha, scenes, name, precise):
    sc, o = scenes(name)
    reg, s = (37, 21, 101, 63), 4
    with renderer(ha, sc, {"precise_shading": precise}) as r:
        acc = _render(r, (W, H), reg, 1, s + 1).astype(np.float64)
    ref = o.render_region(W, H, reg[0], reg[1], reg[2], reg[3], 1, s + 1, threads=0)
    rel = np.abs(acc - ref) / np.maximum(1.0, np.abs(ref))
    f2, f3 = float((rel <= 1e-2).mean()), float((rel <= 1e-3).mean())
    g2, g3 = (GATES_PRECISE if precise else GATES)[name]
    print("region parity %s %s: within 1e-2 %.5f (gate %.4f), within 1e-3 %.5f (gate %.4f)" % (name, reg, f2, g2, f3, g3))
    assert f2 >= g2 and f3 >= g3, (name, f2, f3)


def test_stitched_tiles_equal_the_frame(ha, scenes):
    """Four uneven tiles (split at x = 193, y = 101) rendered by four contexts stitch into the full-frame accumulator bit for bit; written into a
    full-frame context, that accumulator resolves to the full-frame image's bytes."""
    sc, _ = scenes("rtcamp6_v3_1")
    tiles = [(0, 0, 193, 101), (193, 0, W - 193, 101), (0, 101, 193, H - 101), (193, 101, W - 193, H - 101)]
    rs = [renderer(ha, sc) for _ in tiles]
    full_r = renderer(ha, sc)
    try:
        stitched = np.zeros((H, W, 3), dtype=np.float32)
        for r, t in zip(rs, tiles):
            stitched[t[1]:t[1] + t[3], t[0]:t[0] + t[2]] = _render(r, (W, H), t, 1, 5)
        full = _render(full_r, (W, H), None, 1, 5)
        assert np.array_equal(stitched, full)
        img = full_r.resolve(4)
        full_r.write_accumulator(stitched)
        assert np.array_equal(full_r.resolve(4), img)
    finally:
        for r in rs + [full_r]:
            r.close()


def test_region_resolve(ha, scenes, orc):
    """hr_resolve of a region is update_imgbuf of the region's accumulator as an image of its own (within 1 LSB of the oracle's post chain,
    > 99 % exact); one pixel in from its edges it is the full-frame image's bytes."""
    sc, _ = scenes("rtcamp6_v3_1")
    with renderer(ha, sc) as r:
        full = _render(r, (W, H), None, 1, 4)
        full_img = r.resolve(3)
        for reg in [(37, 21, 101, 63), (467, 263, 13, 7), (0, 100, 480, 5)]:
            acc = _render(r, (W, H), reg, 1, 4)
            assert np.array_equal(acc, _crop(full, reg))
            img = r.resolve(3)
            assert img.shape == (reg[3], reg[2], 3)
            exp = orc.resolve(acc.astype(np.float64), 3)
            d = np.abs(img.astype(int) - exp.astype(int))
            assert d.max() <= 1 and (d == 0).mean() > 0.99, (reg, d.max(), (d == 0).mean())
            assert np.array_equal(img[1:-1, 1:-1], _crop(full_img, reg)[1:-1, 1:-1]), reg


def test_region_debug_renderer(ha, scenes):
    sc, _ = scenes("rtcamp6_v3_1")
    r = renderer(ha, sc)
    reg = (37, 21, 101, 63)
    try:
        for mode in range(4):
            r.set_resolution(W, H)
            r.render_debug(mode)
            full = r.read_accumulator()
            r.set_region(*reg)
            r.render_debug(mode)
            acc = r.read_accumulator()
            assert full.sum() > 0 and np.array_equal(acc, _crop(full, reg)), mode
    finally:
        r.close()


@pytest.mark.parametrize("frame,regions,s", [((7680, 4320), [(7616, 4256, 64, 64)], (1, 2)),
                                             ((257, 3), [(0, 0, 5, 3), (250, 1, 7, 2)], (1, 5))])
def test_region_extreme_frames(ha, scenes, frame, regions, s):
    """The far corner of an 8K frame, and a 257 x 3 frame (aspect ratio beyond 4:1: the saturating seed word, isaac_core.h path_seed_words)."""
    sc, _ = scenes("rtcamp6_v3_1")
    with renderer(ha, sc) as r:
        full = _render(r, frame, None, *s)
        for reg in regions:
            acc = _render(r, frame, reg, *s)
            assert np.array_equal(acc, _crop(full, reg)), (frame, reg)


def test_region_lifecycle(ha, scenes):
    import torch
    sc, _ = scenes("cornell_mini")
    with ha.Renderer(0) as r:
        with pytest.raises(ha.HipError) as e:
            r.set_region(0, 0, 1, 1)
        assert e.value.code == -4                                       # HR_ERR_NO_TARGET: hr_set_resolution first
        r.upload_scene(sc)
        r.set_resolution(W, H)
        assert r.region() == (0, 0, W, H)
        reg = (37, 21, 101, 63)
        r.set_region(*reg)
        r.render(1, 4)
        before = r.read_accumulator()
        for bad in [(10, 10, 0, 5), (10, 10, 5, 0), (470, 0, 20, 5), (0, 0, 481, 1), (0, 0, 1, 271), (481, 0, 1, 1), (0, 266, 1, 5),
                    (0xFFFFFFFF, 0, 2, 1), (0, 0xFFFFFFFF, 1, 2), (2, 0, 0xFFFFFFFF, 1)]:
            with pytest.raises(ha.HipError) as e:
                r.set_region(*bad)
            assert e.value.code == -1, bad                              # HR_ERR_INVALID
            assert r.region() == reg
        assert np.array_equal(r.read_accumulator(), before)            # the accumulator stays in place
        st = r.stats()
        assert st["paths"] == 101 * 63 * 4 * 3
        with pytest.raises(ha.HipError) as e:
            r.debug_path_log(1)
        assert e.value.code == -6                                       # HR_ERR_UNSUPPORTED while a region is set
        # a caller-bound accumulator of the region's size is taken, a smaller one refused (32 bytes in one of torch's 2-MiB small-block
        # segments against the region's 600 x 600 x 3 floats), and the bound one receives what the internal one does
        r.set_resolution(1024, 1024)
        r.set_region(10, 10, 600, 600)
        r.render(1, 2)
        own = r.read_accumulator().copy()
        small = torch.zeros((8,), dtype=torch.float32, device="cuda:0")
        with pytest.raises(ha.HipError) as e:
            r.bind_accumulator(small.data_ptr())
        assert e.value.code == -1 and "too small" in str(e.value), str(e.value)
        good = torch.zeros((600, 600, 3), dtype=torch.float32, device="cuda:0")
        r.bind_accumulator(good.data_ptr())
        r.clear()
        r.render(1, 2)
        r.synchronize()
        assert np.array_equal(good.cpu().numpy(), own)
        r.bind_accumulator(None)
        # hr_set_resolution resets the region to the whole frame
        r.set_resolution(W, H)
        assert r.region() == (0, 0, W, H)
        assert r.read_accumulator().shape == (H, W, 3)
        r.set_region(0, 0, W, H)                                        # the whole frame as a region is no region
        r.debug_path_log(1)


def test_region_same_device_exchange(ha, scenes):
    """Two contexts on one region, samplings sharded with stride 2, summed by hr_allreduce_accumulators (same-device group): the total is the
    one-context region render (to the tolerance of test_same_device_group_sum)."""
    sc, _ = scenes("cornell_mini")
    reg = (37, 21, 101, 63)
    rs = [renderer(ha, sc) for _ in range(2)]
    one = renderer(ha, sc)
    try:
        for r in rs:
            r.set_resolution(W, H)
            r.set_region(*reg)
        ha.comm_init_local(rs)
        for k, r in enumerate(rs):
            r.render(1 + k, 9, 2)
        ha.allreduce_accumulators(rs)
        parts = np.sum([r.accumulator_sum(False) for r in rs], axis=0)
        assert (np.abs(parts - np.array(rs[0].accumulator_sum(True))) <= 1e-6 * parts).all()
        tot = rs[0].read_accumulator().astype(np.float64)
        assert tot.shape == (63, 101, 3) and np.array_equal(tot, rs[1].read_accumulator())
        ref = _render(one, (W, H), reg, 1, 9).astype(np.float64)
        assert np.abs(tot - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    finally:
        for r in rs + [one]:
            r.close()


def test_cli_region(tmp_path, ha, scenes):
    from PIL import Image
    reg = (37, 21, 101, 63)
    rarg = "%d,%d,%d,%d" % reg
    small = ["--assets", ASSETS, "-w", 96, "-h", 54, "-t", 1000, "-i", 1000]
    base = ["--assets", ASSETS, "-w", W, "-h", H, "-t", 1000, "-i", 1000, "--launch", 1]
    # the PNG of a region run: w x h, hr_resolve of a region context (one sampling per launch, as --launch 1 renders them)
    d1 = tmp_path / "a"
    d1.mkdir()
    p = run_cli(base + ["-s", 4, "--region", rarg, "--checkpoint", "ck"], d1, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "region: 37,21 101x63." in p.stdout
    img = np.asarray(Image.open(d1 / "result.png"))
    sc, _ = scenes("rtcamp6_v3_1")
    with renderer(ha, sc) as r:
        r.set_resolution(W, H)
        r.set_region(*reg)
        for s in range(1, 5):
            r.render(s, s + 1)
        exp = r.resolve(4)
    assert img.shape == (63, 101, 3) and np.array_equal(img, exp)
    c = ckpt.read(d1 / "ck")
    assert c.magic == ckpt.REGION and c.region == reg and c.complete == ckpt.S_ACCUMULATOR and c.used == c.size == 36 + 101 * 63 * 12
    # checkpoint / resume round trip: 2 + 2 samplings == the uninterrupted 4 (accumulator and image)
    d2 = tmp_path / "b"
    d2.mkdir()
    p = run_cli(base + ["-s", 2, "--region", rarg, "--checkpoint", "ck2"], d2, timeout=300)
    assert p.returncode == 0, p.stdout
    p = run_cli(base + ["-s", 4, "--region", rarg, "--resume", "ck2", "--checkpoint", "ck4"], d2, timeout=300)
    assert p.returncode == 0 and "resumed at 2x4 sampled" in p.stdout, p.stdout
    assert (d2 / "ck4").read_bytes() == (d1 / "ck").read_bytes()
    assert np.array_equal(np.asarray(Image.open(d2 / "result.png")), img)
    # a region checkpoint resumed with another region, or without one, is refused
    p = run_cli(base + ["-s", 4, "--region", "36,21,101,63", "--resume", "ck2"], d2, timeout=300)
    assert p.returncode != 0 and "region" in p.stdout, p.stdout
    p = run_cli(base + ["-s", 4, "--resume", "ck2"], d2, timeout=300)
    assert p.returncode != 0 and "region" in p.stdout, p.stdout
    # a full-frame checkpoint keeps its format ("HRA2", five words, W x H x 3 floats) and is refused under --region
    d3 = tmp_path / "c"
    d3.mkdir()
    p = run_cli(small + ["-s", 1, "--checkpoint", "ckf"], d3, timeout=300)
    assert p.returncode == 0, p.stdout
    c = ckpt.read(d3 / "ckf")
    assert c.magic == ckpt.FRAME and (c.width, c.height, c.samplings) == (96, 54, 1) and c.complete == ckpt.S_ACCUMULATOR and c.used == c.size == 20 + 96 * 54 * 12
    p = run_cli(small + ["-s", 2, "--region", "0,0,8,8", "--resume", "ckf"], d3, timeout=300)
    assert p.returncode != 0, p.stdout
