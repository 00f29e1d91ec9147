#!/usr/bin/env python3
"""tools/robust_rate.py [--package DIR]: what option "robust_buckets" costs.  Renders rtcamp6_v3_1 at 1920x1080, 128 samplings per case after
a warm-up of the same size, with robust_buckets 0 and K (default 9) alternating (three rounds), and prints Mpaths/s of wall time (hr_synchronize
included) per case, then hr_stats.post_kernel_ms of one hr_robust.  --package: the python directory of another build of the package with its
libraries two levels above hanamaru_amd/ (the parent commit's, to compare K = 0 against it from a job that alternates the two); a build without the
option measures K = 0 only.  Not run by bench.py."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="rtcamp6_v3_1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samplings", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--buckets", type=int, default=9)
    ap.add_argument("--package", default=os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    import hanamaru_amd as ha
    W, H, S = a.width, a.height, a.samplings
    sc = ha.Scene(a.scene, os.path.join(ROOT, "assets"))
    r = ha.Renderer(0)
    r.upload_scene(sc)
    r.set_resolution(W, H)
    cases = [0, a.buckets]
    try:
        r.set_option("robust_buckets", a.buckets)
        r.set_option("robust_buckets", 0)
    except ha.HipError:
        cases = [0]                                   # a build without the option
    r.render(1, S + 1)
    r.synchronize()
    print("library %s\nscene %s, %dx%d, %d samplings per case" % (ha.HIP_LIB, a.scene, W, H, S))
    rates = {k: [] for k in cases}
    for rnd in range(a.rounds):
        for k in cases:
            if len(cases) > 1:
                r.set_option("robust_buckets", k)
            r.clear()
            t0 = time.perf_counter()
            r.render(S + 1, 2 * S + 1)
            r.synchronize()
            dt = time.perf_counter() - t0
            rate = r.stats()["paths"] / dt * 1e-6
            rates[k].append(rate)
            print("round %d robust_buckets %d: %9.1f Mpaths/s" % (rnd, k, rate))
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    print("mean: " + ", ".join("robust_buckets %d %.1f Mpaths/s" % (k, m) for k, m in mean.items())
          + (" (%+.2f %%)" % ((mean[cases[1]] / mean[0] - 1.0) * 100.0) if len(cases) > 1 else ""))
    if len(cases) > 1:
        before = r.stats()["post_kernel_ms"]
        r.robust()
        print("hr_robust (K = %d): %.3f ms of post_kernel_ms, %.4f of the pixels trimmed" % (cases[1], r.stats()["post_kernel_ms"] - before, (r.read_robust_trim() > 0).mean()))
    r.close()


if __name__ == "__main__":
    main()
