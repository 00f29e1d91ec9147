#!/usr/bin/env python3
"""tools/restore_quality.py [--scenes a,b,..] [--truth N]: DESIGN.md §4.14's quality table for the restored robust resolve (hr_robust_restore), on the
HOST, no device: the checker's f64 path tracer renders the 96x54 frame one sampling at a time (the library's seeds, so its samplings) and the truth
from samplings 100001 .. 100000 + N, the guide planes are the f64 chain of tests/guide_chain.py, and csrc/restore_core.h, csrc/robust_core.h and
csrc/denoise_core.h compiled by g++ — what the device runs, bit for bit — give R, R' on R and R' on the denoised robust radiance DR with the default
parameters.  Prints mean((x - t)^2 / (t^2 + 0.01^2)) as ratios to the plain mean's, and the energy of R and R' against M, the plain mean of the bucket
means, per scene, sampling count n, K and guide_bounces."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hanamaru-renderer_amd", "python")]
import guide_chain as gc  # noqa: E402
import hanamaru_amd as ha  # noqa: E402
import oracle_py as orc  # noqa: E402
import post_cores as pc  # noqa: E402  (the g++ build of restore_core.h, robust_core.h and denoise_core.h)
from post_quality import restore_figures  # noqa: E402

W, H = 96, 54
KS, NS, BOUNCES = (5, 9), (16, 64), (0, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_mini,rtcamp6_v3_1")
    ap.add_argument("--truth", type=int, default=1024)
    args = ap.parse_args()
    core = pc.lib()
    print("| scene | n | K | bounces | R / mean | R' / mean | R' (base DR) / mean | sum R / sum M | sum R' / sum M |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in args.scenes.split(","):
        sc = ha.Scene(name)
        osc = orc.OracleScene(sc.desc_ptr)
        guides = {b: gc.planes_of(gc.oracle_chain(orc, osc, sc.desc, W, H, b)[0]).astype(np.float32) for b in BOUNCES}
        x = np.stack([osc.render(W, H, s, s + 1)[0] for s in range(1, max(NS) + 1)]).astype(np.float32)
        truth = osc.render(W, H, 100001, 100001 + args.truth)[0].astype(np.float64) / (4.0 * args.truth)
        for n in NS:
            for K in KS:
                for b in BOUNCES:
                    f = restore_figures(core, x[:n], guides[b], truth, K)
                    print("| %s | %d | %d | %d | %.3f | %.3f | %.3f | %.4f | %.4f |" % (name, n, K, b, f["R/mean"], f["R'/mean"], f["R'(DR)/mean"], f["sumR/sumM"], f["sumR'/sumM"]),
                          flush=True)


if __name__ == "__main__":
    main()
