#!/usr/bin/env python3
"""tools/moments_rate.py: what option "moments" costs.  Renders rtcamp6_v3_1 at 1920x1080, 64 samplings per case after a warm-up of the same
size, with moments 0 and 1 alternating (three rounds), and prints Mpaths/s of wall time (hr_synchronize included) per case, then the time of
one hr_noise_estimate.  Not run by bench.py."""
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
    rates = {0: [], 1: []}
    for k in range(a.rounds):
        for on in (0, 1):
            r.set_option("moments", on)
            r.clear()
            t0 = time.perf_counter()
            r.render(S + 1, 2 * S + 1)
            r.synchronize()
            dt = time.perf_counter() - t0
            rate = r.stats()["paths"] / dt * 1e-6
            rates[on].append(rate)
            print("round %d moments %d: %9.1f Mpaths/s" % (k, on, rate))
    m0, m1 = sum(rates[0]) / len(rates[0]), sum(rates[1]) / len(rates[1])
    print("mean: moments 0 %.1f, moments 1 %.1f Mpaths/s (%+.2f %%)" % (m0, m1, (m1 / m0 - 1.0) * 100.0))
    t0 = time.perf_counter()
    est = r.noise_estimate(0.01, 0.05)
    print("hr_noise_estimate: %.2f ms, %s" % ((time.perf_counter() - t0) * 1e3, est))
    r.close()


if __name__ == "__main__":
    main()
