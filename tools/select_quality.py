#!/usr/bin/env python3
"""tools/select_quality.py [--scenes a,b,..] [--buckets K] [--truth N]: DESIGN.md §4.16's quality table for the denoiser that picks its level per
pixel, on the HOST, no device: the checker's f64 path tracer renders the 96x54 frame at 16 and 64 samplings (the library's seeds, so its
samplings) and the truth (2,048 samplings from 100001), the guide planes are the f64 chain of tests/guide_chain.py with 0 and 2 bounces, and
csrc/select_core.h and csrc/denoise_core.h compiled by g++ — the filters the device runs, bit for bit — filter with the default parameters.
Prints mean((x - t)^2 / (t^2 + 0.01^2)) over that of the raw mean: the whole-buffer filter at levels = 4 beside the selection with smooth 0 .. 3,
and the worst case of every smooth over the table: the default of hr_select_params.smooth is the value with the lowest worst case."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hanamaru-renderer_amd", "python")]
import guide_chain as gc  # noqa: E402
import hanamaru_amd as ha  # noqa: E402
import oracle_py as orc  # noqa: E402
import post_cores as pc  # noqa: E402  (lib / core_denoise / core_select: the g++ build of denoise_core.h and select_core.h)
from post_numpy import fill_buckets, rel_sq_error, sums_of  # noqa: E402

W, H = 96, 54
SMOOTH = (0, 1, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="rtcamp6_v3_1,cornell_mini,spheres")
    ap.add_argument("--buckets", type=int, default=9)
    ap.add_argument("--truth", type=int, default=2048)
    args = ap.parse_args()
    K = args.buckets
    worst = {s: 0.0 for s in SMOOTH}
    worst_fixed = 0.0
    core = pc.lib()
    print("| scene, guide_bounces | samplings | fixed 4 | " + " | ".join("select, smooth %d" % s for s in SMOOTH) + " |")
    print("|---|---|---|" + "---|" * len(SMOOTH))
    for name in args.scenes.split(","):
        sc = ha.Scene(name)
        osc = orc.OracleScene(sc.desc_ptr)
        x = np.stack([osc.render(W, H, s, s + 1)[0] for s in range(1, 65)]).astype(np.float32)   # x_s: one sampling's 2x2 sum per pixel
        truth = osc.render(W, H, 100001, 100001 + args.truth)[0].astype(np.float64) / (4.0 * args.truth)
        for bounces in (0, 2):
            guides = gc.planes_of(gc.oracle_chain(orc, osc, sc.desc, W, H, bounces)[0]).astype(np.float32)
            for n in (16, 64):
                acc, mom = sums_of(x[:n])
                B = fill_buckets(x[:n], K)
                e_raw = rel_sq_error(acc / np.float32(4 * n), truth)
                fixed = rel_sq_error(pc.core_denoise(core, acc, mom, n, guides), truth) / e_raw
                sel = {s: rel_sq_error(pc.core_select(core, B, acc, mom, n, guides, smooth=s)[0], truth) / e_raw for s in SMOOTH}
                worst_fixed = max(worst_fixed, fixed)
                for s in SMOOTH:
                    worst[s] = max(worst[s], sel[s])
                print("| %s, %d | %d | %.2f | " % (name, bounces, n, fixed) + " | ".join("%.2f" % sel[s] for s in SMOOTH) + " |", flush=True)
    print("| worst case | | %.4f | " % worst_fixed + " | ".join("%.4f" % worst[s] for s in SMOOTH) + " |")
    print("lowest worst case (a tie goes to the fewer passes): smooth %d" % min(SMOOTH, key=lambda s: (worst[s], s)))


if __name__ == "__main__":
    main()
