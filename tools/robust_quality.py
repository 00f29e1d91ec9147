#!/usr/bin/env python3
"""tools/robust_quality.py [--scenes a,b,..] [--truth N]: DESIGN.md §4.10's quality table for the firefly-robust resolve (option "robust_buckets"),
on the HOST, no device: the checker's f64 path tracer renders the 48x27 frame one sampling at a time (samplings 1 .. 256: the library's seeds, so its
samplings) and the truth from samplings 100001 .. 100000 + N (default 4,096); the buckets are filled as bucket_kernel fills them and csrc/robust_core.h
compiled by g++ — the estimator the device runs, bit for bit — resolves them for K in {5, 9} at n in {16, 64, 256}.  Prints, per scene and n, the plain
mean's mean((x - t)^2 / (t^2 + 0.01^2)), the robust resolve's figure over it, the energy kept (sum R / sum mean) and the share of pixels trimmed."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hanamaru-renderer_amd", "python")]
import hanamaru_amd as ha  # noqa: E402
import oracle_py as orc  # noqa: E402
import post_cores as pc  # noqa: E402  (lib / core_robust: the g++ build of robust_core.h)
from post_numpy import fill_buckets, rel_sq_error  # noqa: E402

W, H = 48, 27
KS, NS = (5, 9), (16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="rtcamp6_v3_1,cornell_mini,spheres")
    ap.add_argument("--truth", type=int, default=4096)
    args = ap.parse_args()
    core = pc.lib()
    print("| scene | n | plain mean, relMSE | " + " | ".join("robust / mean, K = %d" % k for k in KS) + " | energy kept, K = %s | pixels trimmed, K = %s |"
          % (" / ".join(map(str, KS)), " / ".join(map(str, KS))))
    print("|---|---|---|" + "---|" * (len(KS) + 2))
    for name in args.scenes.split(","):
        sc = ha.Scene(name)
        osc = orc.OracleScene(sc.desc_ptr)
        truth = osc.render(W, H, 100001, 100001 + args.truth)[0].astype(np.float64) / (4.0 * args.truth)
        x = np.stack([osc.render(W, H, s, s + 1)[0] for s in range(1, max(NS) + 1)]).astype(np.float32)   # x_s: a sampling's 2x2 sum per pixel, fp32
        for n in NS:
            acc = np.zeros((H, W, 3), dtype=np.float32)
            for s in range(n):
                acc = acc + x[s]                                            # the fp32 accumulator, one sampling at a time
            mean = acc / np.float32(4 * n)
            e_mean = rel_sq_error(mean, truth)
            ratio, kept, trimmed = [], [], []
            for K in KS:
                R, trim = pc.core_robust(core, fill_buckets(x[:n], K), n)
                ratio.append("%.3f" % (rel_sq_error(R, truth) / e_mean))
                kept.append("%.3f" % (R.astype(np.float64).sum() / mean.astype(np.float64).sum()))
                trimmed.append("%.3f" % (trim > 0).mean())
            print("| %s | %d | %.3g | %s | %s | %s |" % (name, n, e_mean, " | ".join(ratio), " / ".join(kept), " / ".join(trimmed)), flush=True)


if __name__ == "__main__":
    main()
