#!/usr/bin/env python3
"""tools/guide_lens_quality.py [--scenes a,b,..] [--bounces 0,2] [--window WxH] [--truth N] [--no-wide]: DESIGN.md §4.9's quality figure for the
lens-sampled guide planes (hr_render_guides_lens), on the HOST, no device.  The checker's f64 path tracer renders 16, 64 and N samplings (the
truth; the library's seeds, so its samplings); the guide planes are the HOST FORM of the device function (tests/guide_lens_harness.cpp over
csrc/pt_core.h: guide_lens_point's table, guide_lens_ray, guide_chain_link) for pinhole rays, 4 and 16 lens points; csrc/denoise_core.h
compiled by g++ — the filter the device runs, bit for bit — filters with the default parameters.

It runs the hand-built wide-aperture scene of the tests (96x54, the whole frame, truth 2,048 samplings) and, per named scene with an aperture, one
window of the 1920x1080 frame: the window, on a 4-pixel grid, in which the most pixels have lens (L = 16) and pinhole planes 0 .. 5 that differ
by more than 0.02 — looked for on every fourth pixel of every fourth row of the frame, then counted exactly inside the chosen window.  A window
without out-of-focus edges shows nothing.

Prints, per case, guide_bounces and sampling count, mean((x - t)^2 / (t^2 + 0.01^2)) of the denoised image over that of the raw mean — over the
window and over the pixels where the planes differ — for the three kinds of guide planes.  A ratio above 1 means the filter RAISED the error."""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hanamaru-renderer_amd", "python")]
import guide_chain as gc  # noqa: E402
import guide_lens as gl  # noqa: E402
import hanamaru_amd as ha  # noqa: E402
import oracle_py as orc  # noqa: E402
import post_cores as pc  # noqa: E402  (lib / core_denoise: the g++ build of denoise_core.h)

FW, FH, GRID = 1920, 1080, 4
KINDS = ((1, "pinhole"), (4, "4 lens points"), (16, "16 lens points"))


def best_window(hl, bounces, ww, wh):
    """the window (x0, y0, ww, wh) of the full frame, on the GRID, with the most differing pixels among the grid's samples"""
    gw, gh = FW // GRID, FH // GRID
    grid = (0, 0, gw, gh)
    lens = hl.lens(FW, FH, bounces, 16, window=grid, per_ray=False, step=GRID)[2]
    pin = hl.lens(FW, FH, bounces, 1, window=grid, per_ray=False, step=GRID)[2]
    m = gl.differ_mask(lens, pin).astype(np.int64)
    sat = np.zeros((gh + 1, gw + 1), np.int64)
    sat[1:, 1:] = m.cumsum(0).cumsum(1)
    cw, ch = ww // GRID, wh // GRID
    counts = sat[ch:, cw:] - sat[:-ch, cw:] - sat[ch:, :-cw] + sat[:-ch, :-cw]
    y, x = np.unravel_index(np.argmax(counts), counts.shape)
    return (int(x) * GRID, int(y) * GRID, ww, wh), int(m.sum())


def run_case(label, sc, hl, core, frame, window, bounces_list, truth_n):
    w, h = frame
    x0, y0, ww, wh = window
    osc = orc.OracleScene(sc.desc_ptr)
    acc = np.zeros((wh, ww, 3))
    s1, s2 = np.zeros((wh, ww, 3)), np.zeros((wh, ww, 3))
    short = {}
    for s in range(1, truth_n + 1):
        x = osc.render_region(w, h, x0, y0, ww, wh, s, s + 1)       # one sampling: the sum of the pixel's four sub-samples
        acc += x
        if s <= 64:
            s1 += x
            s2 += x * x
        if s in (16, 64):
            short[s] = (acc.astype(np.float32), np.concatenate([s1, s2], axis=-1))
    truth = acc / (4.0 * truth_n)
    for bounces in bounces_list:
        guides = {n: hl.lens(w, h, bounces, n, window=window, per_ray=False)[2] for n, _ in KINDS}
        mask = gl.differ_mask(guides[16], guides[1])
        for s in (16, 64):
            a, mom = short[s]
            raw = a / np.float32(4 * s)
            cells = []
            for n, _ in KINDS:
                d = pc.core_denoise(core, a, mom, s, guides[n])
                whole = gc.rel_sq_error(d, truth) / gc.rel_sq_error(raw, truth)
                masked = gc.rel_sq_error(d[mask], truth[mask]) / gc.rel_sq_error(raw[mask], truth[mask]) if mask.any() else float("nan")
                cells.append("%.3f / %.3f" % (whole, masked))
            print("| %s | %d | %d of %d | %d | " % (label, bounces, mask.sum(), mask.size, s) + " | ".join(cells) + " |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="rtcamp6_v3_1,tbf3,rtcamp6_v3,material_examples,rtcamp5,cornell_mini")
    ap.add_argument("--bounces", default="0,2")
    ap.add_argument("--window", default="192x108")
    ap.add_argument("--truth", type=int, default=1024)
    ap.add_argument("--no-wide", action="store_true")
    args = ap.parse_args()
    bounces = [int(k) for k in args.bounces.split(",")]
    ww, wh = (int(v) for v in args.window.split("x"))
    core = pc.lib()
    lib = gl.build_harness(tempfile.mkdtemp(prefix="guide_lens_"))
    print("| case | guide_bounces | pixels where the planes differ by > 0.02 | samplings | " + " | ".join("%s: whole / differing" % name for _, name in KINDS) + " |")
    print("|---|---|---|---|" + "---|" * len(KINDS))
    if not args.no_wide:
        sc = gl.wide_scene(ha)
        hl = gl.HostLens(lib, sc.desc_ptr)
        run_case("hand-built wide-aperture scene, 96x54, truth 2,048", sc, hl, core, (96, 54), (0, 0, 96, 54), bounces, 2048)
        hl.close()
    for name in [n for n in args.scenes.split(",") if n]:
        sc = ha.Scene(name)
        if sc.desc.camera.lens_radius == 0.0:
            print("| %s: no aperture, skipped |" % name)
            continue
        hl = gl.HostLens(lib, sc.desc_ptr)
        window, on_grid = best_window(hl, 0, ww, wh)
        label = "%s (aperture %.3g), window (%d, %d, %d, %d) of %dx%d, truth %d; %d of the frame's %d grid samples differ" % (
            name, 2 * sc.desc.camera.lens_radius, window[0], window[1], ww, wh, FW, FH, args.truth, on_grid, (FW // GRID) * (FH // GRID))
        run_case(label, sc, hl, core, (FW, FH), window, bounces, args.truth)
        hl.close()


if __name__ == "__main__":
    main()
