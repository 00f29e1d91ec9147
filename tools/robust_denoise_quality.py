#!/usr/bin/env python3
"""tools/robust_denoise_quality.py [--scenes a,b,..] [--truth N]: DESIGN.md §4.12's quality table for the robust denoiser (hr_denoise_robust), on the
HOST, no device: the checker's f64 path tracer renders the 96x54 frame one sampling at a time (the library's seeds, so its samplings) and the truth
from samplings 100001 .. 100000 + N, the guide planes are the f64 chain of tests/guide_chain.py, and csrc/robust_core.h and csrc/denoise_core.h
compiled by g++ — what the device runs, bit for bit — give R, today's denoised mean D and the denoised robust radiance DR with the default
parameters.  Prints mean((x - t)^2 / (t^2 + 0.01^2)) as ratios per scene, sampling count n, K and guide_bounces."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hanamaru-renderer_amd", "python")]
import guide_chain as gc  # noqa: E402
import hanamaru_amd as ha  # noqa: E402
import oracle_py as orc  # noqa: E402
import post_cores as pc  # noqa: E402  (the g++ build of robust_core.h and denoise_core.h: core_r, core_filter)
from post_numpy import fill_buckets  # noqa: E402
from post_quality import quality_figures  # noqa: E402

W, H = 96, 54
KS, NS, BOUNCES = (5, 9), (16, 64), (0, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_mini,rtcamp6_v3_1")
    ap.add_argument("--truth", type=int, default=1024)
    args = ap.parse_args()
    core = pc.lib()
    print("| scene | n | K | bounces | R / mean | D / mean | DR / R | DR / mean | sum DR / sum R |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in args.scenes.split(","):
        sc = ha.Scene(name)
        osc = orc.OracleScene(sc.desc_ptr)
        guides = {b: gc.planes_of(gc.oracle_chain(orc, osc, sc.desc, W, H, b)[0]).astype(np.float32) for b in BOUNCES}
        x = np.stack([osc.render(W, H, s, s + 1)[0] for s in range(1, max(NS) + 1)]).astype(np.float32)
        truth = osc.render(W, H, 100001, 100001 + args.truth)[0].astype(np.float64) / (4.0 * args.truth)
        for n in NS:
            acc = np.zeros((H, W, 3), dtype=np.float32)
            for s in range(n):
                acc = acc + x[s]
            xd = x[:n].astype(np.float64)
            mom = np.concatenate([xd.sum(axis=0), (xd * xd).sum(axis=0)], axis=-1)
            for K in KS:
                B = fill_buckets(x[:n], K)
                R = pc.core_r(core, B, n)[0].astype(np.float64)
                for b in BOUNCES:
                    r_mean, d_mean, dr_r, _ = quality_figures(core, x[:n], acc, mom, guides[b], truth, K)
                    DR = pc.core_filter(core, B, n, guides[b]).astype(np.float64)
                    print("| %s | %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.4f |" % (name, n, K, b, r_mean, d_mean, dr_r, dr_r * r_mean, DR.sum() / R.sum()), flush=True)


if __name__ == "__main__":
    main()
