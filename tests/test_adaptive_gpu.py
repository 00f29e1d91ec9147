"""Adaptive sampling on the MI355X: per-pixel sample counts (option "sample_counts"), renders over an active-tile mask
(hr_set_tile_mask), the device-side choice of the tiles (hr_select_tiles) and the counted resolve.  The contract is exact — a masked render adds to
the pixels of its active tiles what an unmasked render adds and nothing anywhere else — so everything here is compared bit for bit, except the
noise image against its numpy restatement (4 ulp, the bar of §4.7)."""
import numpy as np
import pytest

import ckpt
from cli import ASSETS, run_cli
from gpu_helpers import error_of, renderer, retarget, same
from post_numpy import noise_reference as _noise_reference
from post_numpy import ulp_distance

pytestmark = pytest.mark.gpu

HR_ERR_INVALID, HR_ERR_NO_TARGET, HR_ERR_UNSUPPORTED = -1, -4, -6
SCENES = ["cornell_mini", "rtcamp6_v3_1"]            # no meshes / a mesh scene
# a frame whose right and bottom tiles overhang it, and the same window inside a larger frame
TARGETS = {"frame": ((37, 23), None), "region": ((64, 48), (5, 3, 37, 23))}
RW, RH = 37, 23
TX, TY = (RW + 3) // 4, (RH + 3) // 4                   # 10 x 6 tiles
# (options, debug options): shading x trace pipeline, and the fp32 node records
MODES = {"fp32-mega": ({"precise_shading": 0}, {"trace_mode": 0}), "fp32-split": ({"precise_shading": 0}, {"trace_mode": 1}),
         "precise-mega": ({"precise_shading": 1}, {"trace_mode": 0}), "precise-split": ({"precise_shading": 1}, {"trace_mode": 1}),
         "fp32-mega-fp32-nodes": ({"precise_shading": 0, "quant_nodes": 0}, {"trace_mode": 0})}


def _masks():
    """Single tiles (64 paths a sampling: fewer than the seed kernel's 80 columns per group; the last one's lanes overhang the frame), a
    checkerboard, 7 scattered tiles (448 paths: no multiple of 80), all, none."""
    first, last = np.zeros((TY, TX), np.uint8), np.zeros((TY, TX), np.uint8)
    first[0, 0] = 1
    last[TY - 1, TX - 1] = 1
    yy, xx = np.mgrid[0:TY, 0:TX]
    checker = ((xx + yy) & 1).astype(np.uint8)
    scattered = np.zeros((TY, TX), np.uint8)
    for y, x in [(0, 3), (1, 9), (2, 0), (3, 5), (4, 4), (5, 0), (5, 8)]:
        scattered[y, x] = 1
    return {"first": first, "last": last, "checker": checker, "scattered": scattered, "all": np.ones((TY, TX), np.uint8), "none": np.zeros((TY, TX), np.uint8)}


MASKS = _masks()


def _pixels(mask):
    """(RH, RW) bool: the in-region pixels of a tile mask."""
    return np.kron(np.asarray(mask) != 0, np.ones((4, 4), bool))[:RH, :RW]


def _make(ha, sc, opts=None, dbg=None, target="frame", moments=True, counts=True):
    return renderer(ha, sc, opts, dbg, *TARGETS[target], moments=moments, counts=counts)


def _aim(r, target, moments=True, counts=True):
    retarget(r, *TARGETS[target], moments=moments, counts=counts)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_masked_render_is_the_unmasked_render_on_its_tiles(ha, scenes, name, mode):
    sc, _ = scenes(name)
    opts, dbg = MODES[mode]
    full, masked = _make(ha, sc, opts, dbg, counts=False), _make(ha, sc, opts, dbg)
    try:
        for target in sorted(TARGETS):
            _aim(full, target, counts=False)    # (the reference runs the kernels without counts: the counting forms change neither buffer)
            _aim(masked, target)
            for batch in (1, 5, 0):
                full.set_option("batch", batch)
                masked.set_option("batch", batch)
                for args in [(1, 8, 1), (1, 9, 2)]:
                    full.clear()
                    full.render(*args)
                    acc, (mom, n) = full.read_accumulator(), full.read_moments()
                    assert np.isfinite(acc).all() and acc.sum() > 0 and n == len(range(*args))
                    for mname, mask in MASKS.items():
                        what = (name, mode, target, batch, args, mname)
                        pix = _pixels(mask)
                        masked.clear()
                        masked.set_tile_mask(mask)
                        masked.render(*args)
                        macc, (mmom, mn) = masked.read_accumulator(), masked.read_moments()
                        assert mn == n, what
                        assert same(mmom, np.where(pix[..., None], mom, 0.0)), what
                        if batch:    # (automatic: a sparse mask takes more samplings per launch, and the fp32 accumulator depends on the launch cuts)
                            assert same(macc, np.where(pix[..., None], acc, np.float32(0))), what
                        assert np.array_equal(masked.read_sample_counts(), np.where(pix, n, 0).astype(np.uint32)), what
                    # all tiles == no mask
                    masked.clear()
                    masked.set_tile_mask(None)
                    masked.render(*args)
                    assert same(masked.read_accumulator(), acc) and same(masked.read_moments()[0], mom), (name, mode, target, batch, args)
    finally:
        full.close()
        masked.close()


def test_none_active_leaves_the_accumulator(ha, scenes):
    sc, _ = scenes("cornell_mini")
    with _make(ha, sc) as r:
        r.render(1, 4)
        before, launches = r.read_accumulator(), r.stats()["trace_launches"]
        r.set_tile_mask(MASKS["none"])
        r.render(4, 9)                        # HR_OK, nothing enqueued
        assert same(r.read_accumulator(), before) and r.stats()["trace_launches"] == launches
        assert r.tile_mask()[1] == 0 and (r.read_sample_counts() == 3).all()


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_counts(ha, scenes, target):
    sc, _ = scenes("rtcamp6_v3_1")
    with _make(ha, sc, target=target) as r:
        assert not r.read_sample_counts().any()
        expect = np.zeros((RH, RW), np.int64)
        for mask, args in [(None, (1, 5, 1)), (MASKS["checker"], (5, 9, 1)), (MASKS["scattered"], (9, 20, 2)), (MASKS["none"], (20, 25, 1)), (MASKS["last"], (20, 23, 1))]:
            r.set_tile_mask(mask)
            r.render(*args)
            expect += len(range(*args)) * (_pixels(mask) if mask is not None else 1)
        counts = r.read_sample_counts()
        assert counts.dtype == np.uint32 and np.array_equal(counts, expect)
        assert (counts[_pixels(MASKS["checker"]) == 0] >= 4).all() and counts.min() == 4      # pixels no mask ever covered: the first phase only
        assert r.stats()["paths"] == 4 * int(expect.sum())
        # write / read
        rng = np.random.default_rng(3)
        data = rng.integers(0, 2 ** 32, (RH, RW), dtype=np.uint64).astype(np.uint32)
        acc = r.read_accumulator()
        r.write_sample_counts(data)
        assert np.array_equal(r.read_sample_counts(), data) and same(r.read_accumulator(), acc)
        r.write_accumulator(acc * 2)                                    # does not touch the counts
        assert np.array_equal(r.read_sample_counts(), data)
        # hr_clear zeroes the counts and keeps the mask
        r.set_tile_mask(MASKS["scattered"])
        r.clear()
        assert not r.read_sample_counts().any()
        mask, active = r.tile_mask()
        assert np.array_equal(mask, MASKS["scattered"]) and active == 7
        r.render(1, 3)
        assert np.array_equal(r.read_sample_counts(), 2 * _pixels(MASKS["scattered"]))
        # hr_set_region (and hr_set_resolution) remove the mask and zero the counts at the new size
        r.set_region(0, 0, 9, 6)
        mask, active = r.tile_mask()
        assert mask.shape == (2, 3) and mask.all() and active == 6
        assert r.read_sample_counts().shape == (6, 9) and not r.read_sample_counts().any()
        r.render(1, 2)
        assert (r.read_sample_counts() == 1).all()
        # switching the option off removes the mask as well
        r.set_tile_mask(np.eye(2, 3, dtype=np.uint8))
        assert r.tile_mask()[1] == 2
        r.set_option("sample_counts", 0)
        assert r.tile_mask()[1] == 6 and error_of(ha, r.read_sample_counts)[0] == HR_ERR_INVALID


@pytest.mark.parametrize("name", SCENES)
def test_resolve_counted(ha, scenes, name):
    sc, _ = scenes(name)
    with _make(ha, sc) as r:
        for S in (6, 24):     # 1 / 24 and 1 / 96: not powers of two
            r.clear()
            r.render(1, S + 1)
            ref = r.resolve(S)
            assert ref.any() and np.array_equal(r.resolve_counted(), ref)
            # doubled accumulator and doubled count on a checkerboard of tiles: both exact, 1 / (8 S) is half of 1 / (4 S)
            acc, counts = r.read_accumulator(), r.read_sample_counts()
            pix = _pixels(MASKS["checker"])
            r.write_accumulator(np.where(pix[..., None], acc * np.float32(2), acc))
            r.write_sample_counts(np.where(pix, counts * 2, counts))
            assert np.array_equal(r.resolve_counted(), ref), S
            # count 0 with accumulator 0 is a black pixel
            hole = _pixels(MASKS["scattered"])
            acc0 = np.where(hole[..., None], np.float32(0), acc)
            r.write_accumulator(acc0)
            r.write_sample_counts(np.where(hole, 0, S))
            got = r.resolve_counted()
            r.write_sample_counts(np.full((RH, RW), S))
            assert np.array_equal(got, r.resolve(S)) and np.array_equal(got, r.resolve_counted())


def _tile_max(img):
    pad = np.full((TY * 4, TX * 4), -np.inf)
    pad[:RH, :RW] = img
    return pad.reshape(TY, 4, TX, 4).max(axis=(1, 3))


@pytest.mark.parametrize("name", SCENES)
def test_estimate_with_per_pixel_counts(ha, scenes, name):
    sc, _ = scenes(name)
    with _make(ha, sc) as r:
        r.render(1, 2)
        assert error_of(ha, r.noise_image, 0.01)[0] == HR_ERR_INVALID            # every count is 1
        r.clear()
        r.set_tile_mask(MASKS["first"])
        r.render(1, 9)
        code, text = error_of(ha, r.noise_estimate, 0.01, 0.05)                  # 8 samplings issued, but most pixels have none
        assert code == HR_ERR_INVALID and "0 samplings" in text
        assert error_of(ha, r.select_tiles, 0.01, 0.05)[0] == HR_ERR_INVALID
        r.set_tile_mask(None)
        r.clear()
        r.render(1, 9)
        r.set_tile_mask(MASKS["checker"])
        r.render(9, 21)
        (mom, n), counts = r.read_moments(), r.read_sample_counts()
        assert n == 20 and set(np.unique(counts)) == {8, 20}
        for floor in (0.01, 0.5):
            img = r.noise_image(floor)
            d = ulp_distance(img, _noise_reference(mom, counts, floor))
            print("%s floor %g: worst %d ulp" % (name, floor, int(d.max())))
            assert d.max() <= 4
            est = r.noise_estimate(floor, 0.05)
            assert est["samplings"] == 20 and est["pixels"] == RW * RH and est["max_error"] == img.max() and est["pixels_above"] == int((img > 0.05).sum())


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("target", sorted(TARGETS))
def test_select_tiles(ha, scenes, name, target):
    sc, _ = scenes(name)
    with _make(ha, sc, target=target) as r:
        r.render(1, 17)
        floor = 0.01
        tmax = _tile_max(r.noise_image(floor))
        thr = float(np.median(tmax))
        active = r.select_tiles(floor, thr)
        mask, n = r.tile_mask()
        assert np.array_equal(mask != 0, tmax > thr) and n == active == int((tmax > thr).sum()) and 0 < active < TX * TY
        assert r.select_tiles(floor, thr) == active and np.array_equal(r.tile_mask()[0], mask)       # a second call: the identical mask
        # tiles a selection cleared stay cleared under a lower threshold
        low = float(np.sort(tmax.ravel())[TX * TY // 4])
        assert int((tmax > low).sum()) > active
        assert r.select_tiles(floor, low) == active and np.array_equal(r.tile_mask()[0], mask)
        # ... and a higher one clears more
        high = float(np.sort(tmax.ravel())[3 * TX * TY // 4])
        assert r.select_tiles(floor, high) == int((tmax > high).sum()) < active
        # the masked render goes where the mask says
        mask = r.tile_mask()[0]
        r.render(17, 21)
        assert np.array_equal(r.read_sample_counts(), 16 + 4 * _pixels(mask))
        # hr_set_tile_mask(NULL) starts over
        r.set_tile_mask(None)
        tmax2 = _tile_max(r.noise_image(floor))
        assert r.select_tiles(floor, thr) == int((tmax2 > thr).sum())


@pytest.mark.parametrize("name", SCENES)
def test_end_to_end_prefix_property(ha, scenes, name):
    """16 uniform samplings, then four rounds of select / 16 more: every pixel holds the moments of a uniform render of samplings 1 .. its count."""
    sc, _ = scenes(name)
    a, u = _make(ha, sc), _make(ha, sc, counts=False)
    try:
        snaps = {}
        for k in range(1, 6):
            u.render(16 * k - 15, 16 * k + 1)
            snaps[16 * k] = u.read_moments()[0]
        a.render(1, 17)
        thr = float(np.median(_tile_max(a.noise_image(0.01))))
        for k in range(2, 6):
            a.select_tiles(0.01, thr)
            a.render(16 * k - 15, 16 * k + 1)
        counts, (mom, n) = a.read_sample_counts(), a.read_moments()
        values = sorted(int(v) for v in np.unique(counts))
        print(name, "counts", values)
        assert n == 80 and len(values) >= 2 and set(values) <= set(snaps)
        for v in values:
            sel = counts == v
            assert same(mom[sel], snaps[v][sel]), (name, v)
        assert a.stats()["paths"] == 4 * int(counts.sum())
    finally:
        a.close()
        u.close()


def test_refusals(ha, scenes):
    sc, _ = scenes("cornell_mini")
    with ha.Renderer(0) as r:
        r.upload_scene(sc)
        assert error_of(ha, r.set_option, "sample_counts", 1)[0] == HR_ERR_NO_TARGET
        r.set_resolution(RW, RH)
        code, text = error_of(ha, r.set_tile_mask, MASKS["checker"])
        assert code == HR_ERR_INVALID and "sample_counts" in text
        assert error_of(ha, r.read_sample_counts)[0] == HR_ERR_INVALID and error_of(ha, r.resolve_counted)[0] == HR_ERR_INVALID
        assert error_of(ha, r.select_tiles, 0.01, 0.05)[0] == HR_ERR_INVALID
        assert error_of(ha, r.set_option, "sample_counts", 2)[0] == HR_ERR_INVALID
        r.render_debug(2)                                # allowed while the option is off
        r.clear()
        r.set_option("sample_counts", 1)
        assert error_of(ha, r.select_tiles, 0.01, 0.05)[0] == HR_ERR_INVALID     # needs the moments too
        assert error_of(ha, r.render_debug, 2)[0] == HR_ERR_UNSUPPORTED
        r.set_tile_mask(MASKS["checker"])
        code, text = error_of(ha, r.render_debug, 2)
        assert code == HR_ERR_UNSUPPORTED and "tile mask" in text
        rays = np.array([[0, 0, 5, 0, 0, -1]], dtype=np.float32)
        for fn, args in [(r.debug_intersect, (rays,)), (r.debug_trace, (rays,)), (r.debug_path_log, (1,)), (r.debug_draws, (1, 0, 64, 8)), (r.debug_wf_profile, (1, 1))]:
            code, text = error_of(ha, fn, *args)
            assert code == HR_ERR_UNSUPPORTED and "tile mask" in text, fn
        # option combinations that have no kernel over a tile list
        for setter, key, on, off, word in [(r.set_option, "counters", 1, 0, "counters"), (r.set_option, "russian_roulette", 3, 0, "russian_roulette"),
                                           (r.set_debug_option, "min_waves", 4, 5, "min_waves"), (r.set_debug_option, "seed_mode", 1, 2, "seed_mode"),
                                           (r.set_debug_option, "seed_prof", 1, 0, "seed_prof")]:
            setter(key, on)
            code, text = error_of(ha, r.render, 1, 3)
            assert code == HR_ERR_UNSUPPORTED and word in text and "tile mask" in text, key
            setter(key, off)
        assert not r.read_sample_counts().any()          # nothing of the refused renders arrived
        r.render(1, 3)
        assert np.array_equal(r.read_sample_counts(), 2 * _pixels(MASKS["checker"]))
        # without the mask the same options render as they always did
        r.set_tile_mask(None)
        r.set_option("counters", 1)
        r.render(3, 4)
        r.synchronize()


def test_options_start_each_other_over(ha, scenes):
    """Switching "moments" or "sample_counts" on zeroes the other one's buffer (the two cover the same samplings) and leaves the accumulator; set
    on again while on it keeps what has been gathered.  On the frame and on the region of the same size (sides that are no multiples of 4)."""
    sc, _ = scenes("cornell_mini")
    with ha.Renderer(0) as r:
        r.upload_scene(sc)
        for target in sorted(TARGETS):
            _aim(r, target, moments=True, counts=False)
            r.render(1, 3)
            acc, (mom, n) = r.read_accumulator(), r.read_moments()
            assert n == 2 and mom.shape == (RH, RW, 6) and mom.any() and acc.any(), target
            r.set_option("sample_counts", 1)
            mom, n = r.read_moments()
            assert n == 0 and not mom.any(), target
            assert same(r.read_accumulator(), acc), target
            counts = r.read_sample_counts()
            assert counts.shape == (RH, RW) and not counts.any(), target
            r.render(3, 5)
            acc, (mom, n), counts = r.read_accumulator(), r.read_moments(), r.read_sample_counts()
            assert (counts == 2).all() and n == 2 and mom.any(), target
            r.set_option("sample_counts", 1)                  # already on: nothing changes
            assert same(r.read_accumulator(), acc) and same(r.read_moments()[0], mom) and r.read_moments()[1] == 2, target
            assert np.array_equal(r.read_sample_counts(), counts), target
            r.set_option("moments", 0)
            r.set_option("moments", 1)
            assert not r.read_sample_counts().any() and same(r.read_accumulator(), acc), target
            mom, n = r.read_moments()
            assert n == 0 and not mom.any(), target


def test_debug_refusal_precedence(ha, scenes):
    """What a debug entry point refuses first: a region, then a tile mask, then a missing target, then a missing scene.  Nothing is rendered."""
    HR_ERR_NO_SCENE = -3
    rays = np.array([[0, 0, 5, 0, 0, -1]], dtype=np.float32)

    def path_draws(r):
        out = np.empty((max(r.height, 1), max(r.width, 1), 4, 20), dtype=np.float32)
        r._check(r.L.hr_debug_path_draws(r._h, 1, out.ctypes.data))

    def four(r):
        return [(r.debug_path_log, (1,)), (r.debug_wf_profile, (1, 1)), (r.debug_intersect, (rays,)), (r.debug_trace, (rays,))]

    (fw, fh), region = TARGETS["region"]
    with ha.Renderer(0) as r:                                      # a resolution and a region, no scene
        r.set_resolution(fw, fh)
        r.set_region(*region)
        for fn, args in four(r):
            code, text = error_of(ha, fn, *args)
            assert code == HR_ERR_UNSUPPORTED and "region" in text, fn
        r.set_resolution(fw, fh)                            # full frame again
        for fn, args in four(r):
            assert error_of(ha, fn, *args)[0] == HR_ERR_NO_SCENE, fn
    sc, _ = scenes("cornell_mini")
    with ha.Renderer(0) as r:                                      # a scene, no resolution
        r.upload_scene(sc)
        assert error_of(ha, r.debug_draws, 1, 0, 64, 8)[0] == HR_ERR_NO_TARGET
        assert error_of(ha, r.debug_path_log, 1)[0] == HR_ERR_NO_TARGET
    with ha.Renderer(0) as r:                                      # a region, counts and a mask: the region is what is named
        r.set_resolution(fw, fh)
        r.set_region(*region)
        r.set_option("sample_counts", 1)
        r.set_tile_mask(MASKS["checker"])
        for fn, args in four(r) + [(r.debug_draws, (1, 0, 64, 8)), (path_draws, (r,))]:
            code, text = error_of(ha, fn, *args)
            assert code == HR_ERR_UNSUPPORTED and "region" in text, fn


def _checkpoint_counts(path, w, h):
    """{"HRA2" header, accumulator, "HRMS" trailer, "HRSC" trailer}: the per-pixel counts of a checkpoint written with --adaptive."""
    c = ckpt.read(path)
    assert c.magic == ckpt.FRAME and c.has_moments and c.has_counts and c.complete == ckpt.S_COUNTS
    assert c.used == c.size == 5 * 4 + w * h * 3 * 4 + (4 + 8 + w * h * 6 * 8) + (4 + w * h * 4) and c.counts.shape == (h, w)
    return c.counts


def test_cli_adaptive(tmp_path, ha, scenes):
    import re
    w, h = 64, 48
    sc, _ = scenes("cornell_mini")
    # a threshold between the tile maxima after the first phase: some tiles stop at the first check, some go on
    with _make(ha, sc, counts=False) as r:
        r.set_resolution(w, h)
        r.set_option("moments", 1)
        r.render(1, 9)
        img = r.noise_image(0.01)
    thr = float(np.median(img.reshape(h // 4, 4, w // 4, 4).max(axis=(1, 3))))
    plain = ["--assets", ASSETS, "-w", str(w), "-h", str(h), "--scene", "cornell_mini", "-t", "600"]
    base = plain + ["--noise-check", "8", "--adaptive", repr(thr)]
    run = run_cli(base + ["-s", "24", "--sample-image", "samples.png", "--checkpoint", "a.ckpt"], tmp_path, timeout=120)
    assert run.returncode == 0, run.stdout
    checks = re.findall(r"adaptive: samplings=(\d+) active=(\d+) tiles=(\d+)", run.stdout)
    assert checks and checks[0][0] == "8" and 0 < int(checks[0][1]) < int(checks[0][2]) == (w // 4) * (h // 4)
    # one progress line per sampling issued, numbered 1 .. the last one, whether the render ran to -s or stopped with no tile left
    lines = [int(v) for v in re.findall(r"^rendering: (\d+)x4 sampled", run.stdout, flags=re.M)]
    issued = int(re.search(r"^sampled: (\d+)x4 spp", run.stdout, flags=re.M).group(1))
    assert lines == list(range(1, issued + 1)) and (issued == 24 or ("no tile is active" in run.stdout and issued == int(checks[-1][0])))
    assert (tmp_path / "samples.png").exists() and (tmp_path / "result.png").exists()
    grey = ha.decode_image(str(tmp_path / "samples.png"))
    assert grey.shape[:2] == (h, w) and grey[..., 0].max() == 255 and len(np.unique(grey[..., 0])) >= 2
    counts = _checkpoint_counts(str(tmp_path / "a.ckpt"), w, h)
    assert len(np.unique(counts)) >= 2 and counts.min() >= 8 and np.array_equal(grey[..., 0], np.floor(counts / counts.max() * 255.0 + 0.5).astype(np.uint8))
    # resume: the counts come back, the tiles are chosen again before anything is rendered, and every pixel only ever gains samplings
    again = run_cli(base + ["-s", "40", "--resume", "a.ckpt", "--checkpoint", "b.ckpt"], tmp_path, timeout=120)
    assert again.returncode == 0, again.stdout
    assert "holds no sample moments" not in again.stdout        # the moments were found and restored
    first = re.search(r"adaptive: samplings=(\d+) active=(\d+)", again.stdout)
    sampled = int(re.search(r"resumed at (\d+)x4 sampled", again.stdout).group(1))
    assert first and int(first.group(1)) == sampled
    after = _checkpoint_counts(str(tmp_path / "b.ckpt"), w, h)
    assert (after >= counts).all() and (after[counts < counts.max()] == counts[counts < counts.max()]).all()
    # resumed with nothing left to render: the counts round-trip unchanged
    same = run_cli(base + ["-s", str(sampled), "--resume", "a.ckpt", "--checkpoint", "c.ckpt"], tmp_path, timeout=120)
    assert same.returncode == 0 and np.array_equal(_checkpoint_counts(str(tmp_path / "c.ckpt"), w, h), counts)
    # without the new flags: a checkpoint with moments resumes silently, one without says that its samplings are not covered
    assert run_cli(plain + ["-s", "4", "--noise-image", "n.png", "--checkpoint", "m.ckpt"], tmp_path, timeout=120).returncode == 0
    assert run_cli(plain + ["-s", "4", "--checkpoint", "p.ckpt"], tmp_path, timeout=120).returncode == 0
    with_mom = run_cli(plain + ["-s", "6", "--noise-image", "n.png", "--resume", "m.ckpt"], tmp_path, timeout=120)
    without = run_cli(plain + ["-s", "6", "--noise-image", "n.png", "--sample-image", "s.png", "--resume", "p.ckpt"], tmp_path, timeout=120)
    assert with_mom.returncode == 0 and "holds no sample moments" not in with_mom.stdout
    assert without.returncode == 0 and "holds no sample moments" in without.stdout
    for args, word in [(["--gpus", "2"], "one device"), (["--noise-target", "0.1"], "two stop rules")]:
        bad = run_cli(base + ["-s", "8"] + args, tmp_path, timeout=120)
        assert bad.returncode == 1 and word in bad.stdout
