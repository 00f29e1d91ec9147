#!/usr/bin/env python3
"""tools/region_rate.py: how region rendering (hr_set_region) fills the chip.  Renders rtcamp6_v3_1 at 1920x1080 on the whole frame and on
centred regions of 960x540, 256x256 and 64x64, 64 samplings each (after a warm-up of the same size), and prints Mpaths/s (camera paths of
the region per second of wall time, hr_synchronize included) and ms per launch (HIP events of the trace side: hr_stats.trace_kernel_ms /
trace_launches).  Not run by bench.py."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
import hanamaru_amd as ha  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="rtcamp6_v3_1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samplings", type=int, default=64)
    a = ap.parse_args()
    W, H, S = a.width, a.height, a.samplings
    sc = ha.Scene(a.scene)
    r = ha.Renderer(0)
    r.upload_scene(sc)
    print("scene %s, frame %dx%d, %d samplings per case (warm-up: the same once before)" % (a.scene, W, H, S))
    print("%-10s %-22s %10s %9s %12s %14s" % ("case", "region x0,y0 wxh", "Mpaths/s", "launches", "ms/launch", "trace ms/launch"))
    for (w, h) in [(W, H), (960, 540), (256, 256), (64, 64)]:
        x0, y0 = (W - w) // 2, (H - h) // 2
        r.set_resolution(W, H)
        if (w, h) != (W, H):
            r.set_region(x0, y0, w, h)
        r.render(1, S + 1)
        r.synchronize()
        r.clear()   # zero accumulator and stats: what follows is the timed run alone
        t0 = time.perf_counter()
        r.render(S + 1, 2 * S + 1)
        r.synchronize()
        dt = time.perf_counter() - t0
        st = r.stats()
        n = max(1, st["trace_launches"])
        print("%-10s %-22s %10.1f %9d %12.3f %14.3f" % ("full" if (w, h) == (W, H) else "%dx%d" % (w, h), "%d,%d %dx%d" % (x0, y0, w, h),
                                                     st["paths"] / dt * 1e-6, n, dt * 1e3 / n, st["trace_kernel_ms"] / n))
    r.close()


if __name__ == "__main__":
    main()
