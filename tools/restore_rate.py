#!/usr/bin/env python3
"""tools/restore_rate.py [--buckets K] [--repeat N]: what one hr_robust_restore costs.  Renders rtcamp6_v3_1 at 1920x1080 with
option robust_buckets K (default 9), 64 samplings, renders the guide planes, and then — after one warm-up call of each — times hr_robust_restore
with levels 0 (the init and final passes alone) and with levels 4 beside hr_denoise_robust with levels 4, N times alternating in one process, by
hr_stats.post_kernel_ms (the kernels' own event pair).  Prints every time and the medians.  Not run by bench.py."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="rtcamp6_v3_1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samplings", type=int, default=64)
    ap.add_argument("--buckets", type=int, default=9)
    ap.add_argument("--repeat", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
    import hanamaru_amd as ha
    W, H, K = a.width, a.height, a.buckets
    r = ha.Renderer(0)
    r.upload_scene(ha.Scene(a.scene, os.path.join(ROOT, "assets")))
    r.set_resolution(W, H)
    r.set_option("robust_buckets", K)
    r.render(1, a.samplings + 1)
    r.synchronize()
    r.render_guides()

    def timed(call):
        before = r.stats()["post_kernel_ms"]
        call()
        return r.stats()["post_kernel_ms"] - before

    cases = [("hr_robust_restore levels 0", lambda: r.robust_restore(levels=0)), ("hr_robust_restore levels 4", lambda: r.robust_restore(levels=4)),
             ("hr_denoise_robust levels 4", lambda: r.denoise_robust(levels=4))]
    for _, call in cases:
        timed(call)
    times = {name: [] for name, _ in cases}
    for _ in range(a.repeat):
        for name, call in cases:
            times[name].append(timed(call))
    print("library %s\nscene %s, %dx%d, K = %d, %d samplings" % (ha.HIP_LIB, a.scene, W, H, K, a.samplings))
    for name, _ in cases:
        print("%-27s ms: " % name + " ".join("%.3f" % t for t in times[name]) + "   median %.3f" % statistics.median(times[name]))
    r.close()


if __name__ == "__main__":
    main()
