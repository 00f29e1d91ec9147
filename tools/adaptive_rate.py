#!/usr/bin/env python3
"""tools/adaptive_rate.py: what rendering over a tile mask is worth.  rtcamp6_v3_1 at 1920x1080, after a warm-up:
  (a) the feature-off rate (no option set), three runs — to be compared with the same lines of the parent build, runs interleaved;
  (b) Mpaths/s of masked launches at 100 / 50 / 25 / 10 % active tiles, random and blocky masks, against the unmasked rate of the same run
      (paths = 4 x the in-region pixels of the active tiles per sampling: hr_stats.paths).
Wall time with hr_synchronize included.  Not run by bench.py.  Not built yet: (c) the CLI's wall time to `--adaptive E` against rendering
uniformly to the same maximum e."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
import hanamaru_amd as ha  # noqa: E402


def timed(r, begin, end):
    r.clear()
    t0 = time.perf_counter()
    r.render(begin, end)
    r.synchronize()
    dt = time.perf_counter() - t0
    return r.stats()["paths"] / dt * 1e-6, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="rtcamp6_v3_1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samplings", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    W, H, S = a.width, a.height, a.samplings
    sc = ha.Scene(a.scene)
    r = ha.Renderer(0)
    r.upload_scene(sc)
    r.set_resolution(W, H)
    r.render(1, S + 1)
    r.synchronize()
    print("scene %s, %dx%d, %d samplings per case" % (a.scene, W, H, S))
    for k in range(a.rounds):
        print("(a) feature off, run %d: %9.1f Mpaths/s" % (k, timed(r, S + 1, 2 * S + 1)[0]))
    if not hasattr(r, "set_tile_mask"):
        return    # (the parent build: part (a) only)
    r.set_option("sample_counts", 1)
    base = timed(r, S + 1, 2 * S + 1)[0]
    print("(b) sample_counts on, no mask: %9.1f Mpaths/s" % base)
    ty, tx = (H + 3) // 4, (W + 3) // 4
    rng = np.random.default_rng(1)
    for pct in (100, 50, 25, 10):
        rand = rng.random((ty, tx)) < pct / 100.0
        blocky = np.zeros((ty, tx), bool)
        blocky[:, :max(1, tx * pct // 100)] = True          # a band of whole columns of tiles
        for kind, mask in (("random", rand), ("blocky", blocky)):
            r.set_tile_mask(mask)
            rate, dt = timed(r, S + 1, 2 * S + 1)
            print("(b) %3d %% %-6s: %7d active tiles, %9.1f Mpaths/s (%.2f of unmasked), %.3f s" % (pct, kind, r.tile_mask()[1], rate, rate / base, dt))
    r.close()


if __name__ == "__main__":
    main()
