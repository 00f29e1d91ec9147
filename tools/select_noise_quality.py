#!/usr/bin/env python3
"""tools/select_noise_quality.py [--scenes a,b,..] [--buckets K] [--truth N]: DESIGN.md §4.17's calibration table for the error estimate of the
image hr_denoise_select makes, on the HOST, no device: the checker's f64 path tracer renders the 96x54 frame at 16 and 64 samplings (the library's
seeds, so its samplings) and the truth (2,048 samplings from 100001), the guide planes are the f64 chain of tests/guide_chain.py with 0 and 2
bounces, and csrc/select_noise_core.h compiled by g++ — what the device runs, bit for bit — gives S, L and M with the default parameters and
smooth 0 and 2.  Per row:
  (a) mean(M) / mean(sum_c (S_c - t_c)^2), the calibration ratio (1: the estimate's mean is the true mean squared error)
  (b) the same over the pixels with L > 0 only
  (c) the rank correlation (Spearman) of M with the true squared error, both summed over 4x4 tiles
  (d) the share of tiles --adaptive 0.05 would keep under e_S, beside the share under e of the raw moments (floor 0.01)
and mean(M) itself.  Nothing here is a gate: the table says what the estimate is worth."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hanamaru-renderer_amd", "python")]
import guide_chain as gc  # noqa: E402
import hanamaru_amd as ha  # noqa: E402
import oracle_py as orc  # noqa: E402
import select_noise_cores as snc  # noqa: E402  (the g++ build of select_noise_core.h)
from post_numpy import fill_buckets, noise_reference, sums_of  # noqa: E402
from select_noise_numpy import numpy_tile_rule  # noqa: E402

W, H = 96, 54
FLOOR, THRESHOLD = 0.01, 0.05


def tile_sums(a):
    ty, tx = (H + 3) // 4, (W + 3) // 4
    p = np.zeros((ty * 4, tx * 4))
    p[:H, :W] = a
    return p.reshape(ty, 4, tx, 4).sum(axis=(1, 3)).reshape(-1)


def ranks(v):
    """average ranks (ties share their mean rank)"""
    order = np.argsort(v, kind="stable")
    r = np.empty(v.size)
    r[order] = np.arange(v.size, dtype=np.float64)
    for val in np.unique(v):
        m = v == val
        if m.sum() > 1:
            r[m] = r[m].mean()
    return r


def spearman(a, b):
    ra, rb = ranks(a), ranks(b)
    return float(np.corrcoef(ra, rb)[0, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="rtcamp6_v3_1,cornell_mini,spheres")
    ap.add_argument("--buckets", type=int, default=9)
    ap.add_argument("--truth", type=int, default=2048)
    args = ap.parse_args()
    K = args.buckets
    core = snc.lib()
    print("| scene, guide_bounces | samplings | smooth | (a) mean M / true MSE | (b) the same, L > 0 | pixels with L > 0 | (c) rank correlation, 4x4 tiles | (d) tiles kept by e_S | by raw e | mean M |")
    print("|---|---|---|---|---|---|---|---|---|---|")
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
                raw_tiles = float(numpy_tile_rule(noise_reference(mom, n, FLOOR), THRESHOLD).mean())
                for smooth in (0, 2):
                    S, L, M = snc.core_select_noise(core, B, acc, mom, n, guides, smooth=smooth)
                    err = ((S.astype(np.float64) - truth) ** 2).sum(axis=-1)
                    up = L > 0
                    b = M[up].mean() / err[up].mean() if up.any() else float("nan")
                    e_s = snc.core_errors(core, M, S, FLOOR)
                    print("| %s, %d | %d | %d | %.2f | %.2f | %.3f | %.3f | %.3f | %.3f | %.4g |"
                          % (name, bounces, n, smooth, M.mean() / err.mean(), b, up.mean(), spearman(tile_sums(M), tile_sums(err)),
                             float(numpy_tile_rule(e_s, THRESHOLD).mean()), raw_tiles, M.mean()), flush=True)


if __name__ == "__main__":
    main()
