#!/usr/bin/env python3
"""tools/fold_rate.py [--contexts 2,8] [--buckets K] [--repeat N]: what one same-device hr_fold_statistics costs.  N contexts on
device 0 in one hr_comm_init_local group, 1920x1080, options moments + sample_counts + robust_buckets K (default 9) + bucket_by_sampling 1; every
context renders a few samplings of its shard, then — after one warm-up fold — the group is folded `repeat` times, each time behind one more
sampling per context (the planes' contents do not change what the kernel moves).  The time is rank 0's hr_stats.post_kernel_ms (one event pair
around all kernels of a fold).  Traffic model: per peer the planes' B bytes (accumulator 12, moments 48, counts 4, buckets 24 K per pixel) are read
twice (root and peer) and written twice (the sum and the zeros): 4 B.  Prints every time, the median and the bandwidth at the median.  Not run by
bench.py."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell_mini")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--contexts", default="2,8")
    ap.add_argument("--buckets", type=int, default=9)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--package", default=os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    import hanamaru_amd as ha
    W, H, K = a.width, a.height, a.buckets
    scene = ha.Scene(a.scene, os.path.join(ROOT, "assets"))
    mbytes = W * H * (12 + 48 + 4 + 24 * K) / 1e6
    print("library %s\nscene %s, %dx%d, K = %d: %.0f MB of planes per context" % (ha.HIP_LIB, a.scene, W, H, K, mbytes))
    for n in [int(x) for x in a.contexts.split(",")]:
        rs = [ha.Renderer(0) for _ in range(n)]
        try:
            for r in rs:
                r.upload_scene(scene)
                r.set_resolution(W, H)
                for key, value in (("moments", 1), ("sample_counts", 1), ("robust_buckets", K), ("bucket_by_sampling", 1)):
                    r.set_option(key, value)
            ha.comm_init_local(rs)
            times, s = [], 1
            for i in range(a.repeat + 1):
                for k, r in enumerate(rs):
                    r.render(s + k, s + n, n)
                s += n
                before = rs[0].stats()["post_kernel_ms"]
                ha.fold_statistics(rs)
                times.append(rs[0].stats()["post_kernel_ms"] - before)
            times = times[1:]
            med = statistics.median(times)
            moved = 4 * mbytes * (n - 1)
            counts = rs[0].read_sample_counts()
            assert counts.min() == counts.max() == s - 1 and rs[0].read_buckets()[1] == s - 1
            print("%d contexts: fold ms " % n + " ".join("%.3f" % t for t in times) + "   median %.3f   %.0f MB moved: %.2f TB/s" % (med, moved, moved / med / 1e3))
        finally:
            for r in rs:
                r.close()


if __name__ == "__main__":
    main()
