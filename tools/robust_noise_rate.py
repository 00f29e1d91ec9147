#!/usr/bin/env python3
"""tools/robust_noise_rate.py [--buckets K] [--repeat N]: what one robust noise estimate costs.  Renders rtcamp6_v3_1 at 1920x1080
with option robust_buckets K (default 9), 64 samplings, and then — after one warm-up call of each — times hr_robust and hr_robust_noise_estimate N
times alternating, by hr_stats.post_kernel_ms (the kernel's own event pair).  Prints every time, the median of each, and for the estimate the bytes
it reads (24 K per pixel) over the median: the bandwidth it reaches.  Which fetch scheme robust_noise_kernel uses is the build's (kernel_variants.h:
ROBUST_NOISE_STAGED); the figures of the other come from a library built with the other setting — --package: the python directory of that build of
the package, with its libraries two levels above hanamaru_amd/, as tools/robust_rate.py takes it.  Not run by bench.py."""
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
    ap.add_argument("--package", default=os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    import hanamaru_amd as ha
    W, H, K = a.width, a.height, a.buckets
    r = ha.Renderer(0)
    r.upload_scene(ha.Scene(a.scene, os.path.join(ROOT, "assets")))
    r.set_resolution(W, H)
    r.set_option("robust_buckets", K)
    r.render(1, a.samplings + 1)
    r.synchronize()

    def timed(call):
        before = r.stats()["post_kernel_ms"]
        out = call()
        return r.stats()["post_kernel_ms"] - before, out

    timed(r.robust)
    timed(lambda: r.robust_noise_estimate(0.01, 0.08))
    t_rob, t_est, est = [], [], None
    for _ in range(a.repeat):
        t_rob.append(timed(r.robust)[0])
        ms, est = timed(lambda: r.robust_noise_estimate(0.01, 0.08))
        t_est.append(ms)
    mbytes = W * H * 24 * K / 1e6
    print("library %s\nscene %s, %dx%d, K = %d, %d samplings" % (ha.HIP_LIB, a.scene, W, H, K, a.samplings))
    print("hr_robust                ms: " + " ".join("%.3f" % t for t in t_rob) + "   median %.3f" % statistics.median(t_rob))
    print("hr_robust_noise_estimate ms: " + " ".join("%.3f" % t for t in t_est) + "   median %.3f" % statistics.median(t_est))
    print("the estimate reads %.0f MB: %.0f GB/s at the median" % (mbytes, mbytes / statistics.median(t_est)))
    print("estimate: mean e_R %.6f max %.4f above 0.08: %d of %d pixels" % (est["mean_error"], est["max_error"], est["pixels_above"], est["pixels"]))
    r.close()


if __name__ == "__main__":
    main()
