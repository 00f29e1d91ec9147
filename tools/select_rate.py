#!/usr/bin/env python3
"""tools/select_rate.py [--buckets K] [--repeat N]: what one hr_denoise_select costs.  Renders rtcamp6_v3_1 at 1920x1080 with
options moments and robust_buckets K (default 9), 16 samplings, renders the guide planes, and then — after one warm-up call of each — times
hr_denoise_select (levels 4; smooth 0 and 2) beside hr_denoise with levels 4, N times alternating in one process, by hr_stats.post_kernel_ms (the
kernels' own event pair).  The yardstick is THREE hr_denoise calls: the selection filters three states, and its fused level kernel is there to beat
three single launches.  hr_denoise's kernels are the parent commit's to the byte (profiles/select_kernel_resources.txt), so its time here is the
parent's.  Prints every time, the medians and the ratio.  Not run by bench.py."""
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
    ap.add_argument("--samplings", type=int, default=16)
    ap.add_argument("--buckets", type=int, default=9)
    ap.add_argument("--repeat", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
    import hanamaru_amd as ha
    W, H, K = a.width, a.height, a.buckets
    r = ha.Renderer(0)
    r.upload_scene(ha.Scene(a.scene, os.path.join(ROOT, "assets")))
    r.set_resolution(W, H)
    r.set_option("moments", 1)
    r.set_option("robust_buckets", K)
    r.render(1, a.samplings + 1)
    r.synchronize()
    r.render_guides()

    def timed(call):
        before = r.stats()["post_kernel_ms"]
        call()
        return r.stats()["post_kernel_ms"] - before

    cases = [("hr_denoise levels 4", lambda: r.denoise(levels=4)), ("hr_denoise_select levels 4 smooth 0", lambda: r.denoise_select(levels=4, smooth=0)),
             ("hr_denoise_select levels 4 smooth 2", lambda: r.denoise_select(levels=4, smooth=2))]
    for _, call in cases:
        timed(call)
    times = {name: [] for name, _ in cases}
    for _ in range(a.repeat):
        for name, call in cases:
            times[name].append(timed(call))
    print("library %s\nscene %s, %dx%d, K = %d, %d samplings" % (os.path.relpath(ha.HIP_LIB, ROOT), a.scene, W, H, K, a.samplings))
    med = {}
    for name, _ in cases:
        med[name] = statistics.median(times[name])
        print("%-36s ms: " % name + " ".join("%.3f" % t for t in times[name]) + "   median %.3f" % med[name])
    three = 3.0 * med["hr_denoise levels 4"]
    print("three hr_denoise calls %.3f ms; hr_denoise_select (smooth 0) / that = %.3f" % (three, med["hr_denoise_select levels 4 smooth 0"] / three))
    r.close()


if __name__ == "__main__":
    main()
