#!/usr/bin/env python3
"""tools/robust_noise_quality.py [--scenes a,b,..]: DESIGN.md §4.11's calibration table for the robust noise estimate, on the HOST, no device: the
checker's f64 path tracer renders the 48x27 frame one sampling at a time (the library's seeds, so its samplings); for n in {16, 64, 256} set A is
samplings 1 .. n and set B samplings n + 1 .. 2 n; the buckets are filled as bucket_kernel fills them and robust_pixel_error of csrc/robust_core.h
compiled by g++ — the estimator the device runs — gives e_R for K in {5, 9, 15}.  Prints, per scene, n and K:
  RMS z        z = (Ry_A - Ry_B) / sqrt(se_A^2 + se_B^2) per pixel over the pixels with a non-zero denominator; 1 for a correct standard error
  mean e_R     of set A / set B (floor 0.01)
  mean raw e   §4.7's e of the same samplings' moments, set A / set B
  se = 0       the share of pixels whose winsorized spread is 0 (set A / set B): full trim, or exactly converged pixels"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hanamaru-renderer_amd", "python")]
import hanamaru_amd as ha  # noqa: E402
import oracle_py as orc  # noqa: E402
import post_cores as pc  # noqa: E402  (lib / core_error: the g++ build of robust_core.h)
from post_numpy import fill_buckets, numpy_error  # noqa: E402  (numpy_error for se and Ry)

W, H, FLOOR = 48, 27, 0.01
KS, NS = (5, 9, 15), (16, 64, 256)


def raw_error(x, floor=FLOOR):
    """§4.7's e of the per-sampling values x (n, h, w, 3)"""
    x = x.astype(np.float64)
    n = x.shape[0]
    s1, s2 = x.sum(axis=0), (x * x).sum(axis=0)
    m = s1 / n
    se = np.sqrt(np.maximum(0.0, (s2 - s1 * m) / (n - 1)) / n) / 4.0
    return se.sum(axis=-1) / ((m / 4.0).sum(axis=-1) + 3.0 * floor)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="rtcamp6_v3_1,cornell_mini,spheres")
    args = ap.parse_args()
    core = pc.lib()
    print("| scene | n | K | RMS z | mean e_R (A / B) | mean raw e (A / B) | se = 0 (A / B) |")
    print("|---|---|---|---|---|---|---|")
    for name in args.scenes.split(","):
        sc = ha.Scene(name)
        osc = orc.OracleScene(sc.desc_ptr)
        x = np.stack([osc.render(W, H, s, s + 1)[0] for s in range(1, 2 * max(NS) + 1)]).astype(np.float32)
        for n in NS:
            sets = (x[:n], x[n:2 * n])
            raw = [raw_error(s).mean() for s in sets]
            for K in KS:
                e, se, ry = [], [], []
                for s in sets:
                    B = fill_buckets(s, K)
                    e.append(pc.core_error(core, B, n, FLOOR)[0])
                    _, _, se_s, ry_s, _ = numpy_error(B, n, FLOOR, parts=True)
                    se.append(se_s)
                    ry.append(ry_s)
                den = np.sqrt(se[0] ** 2 + se[1] ** 2)
                ok = den > 0
                rms = np.sqrt(np.mean(((ry[0] - ry[1])[ok] / den[ok]) ** 2))
                print("| %s | %d | %d | %.2f | %.4f / %.4f | %.4f / %.4f | %.4f / %.4f |"
                      % (name, n, K, rms, e[0].mean(), e[1].mean(), raw[0], raw[1], (se[0] == 0).mean(), (se[1] == 0).mean()), flush=True)


if __name__ == "__main__":
    main()
