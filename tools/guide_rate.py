#!/usr/bin/env python3
"""tools/guide_rate.py: what the guide pass costs by option "guide_bounces" (DESIGN.md §4.9).  hr_stats.debug_kernel_ms of ONE hr_render_guides of
rtcamp6_v3_1 at 1920x1080 for K = 0, 1, 4, 8, after a warm-up pass, three rounds with the values alternating.  Not run by bench.py."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
import hanamaru_amd as ha  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="rtcamp6_v3_1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", default="0,1,4,8")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    bounces = [int(k) for k in a.bounces.split(",")]
    r = ha.Renderer(0)
    r.upload_scene(ha.Scene(a.scene))
    r.set_resolution(a.width, a.height)
    for k in bounces:                                            # warm-up: every kernel once
        r.set_option("guide_bounces", k)
        r.render_guides()
    r.synchronize()
    print("scene %s, %dx%d, one hr_render_guides per case" % (a.scene, a.width, a.height))
    ms = {k: [] for k in bounces}
    for rnd in range(a.rounds):
        for k in bounces:
            r.set_option("guide_bounces", k)
            before = r.stats()["debug_kernel_ms"]
            r.render_guides()
            r.synchronize()
            ms[k].append(r.stats()["debug_kernel_ms"] - before)
            print("round %d guide_bounces %d: %8.3f ms" % (rnd, k, ms[k][-1]))
    print("median: " + ", ".join("K = %d %.3f ms" % (k, sorted(v)[len(v) // 2]) for k, v in ms.items()))
    r.close()


if __name__ == "__main__":
    main()
