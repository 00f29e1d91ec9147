#!/usr/bin/env python3
"""tools/guide_rate.py: what the guide pass costs by option "guide_bounces" and by the lens points of hr_render_guides_lens.
hr_stats.debug_kernel_ms of ONE hr_render_guides (lens 0) or ONE hr_render_guides_lens(L) at 1920x1080 for every pair of --bounces and --lens, after
a warm-up pass, three rounds with the cases alternating.  Defaults: rtcamp6_v3_1, K = 0, 1, 4, 8, pinhole only — the figures of the guide chain;
`--scenes rtcamp6_v3_1,tbf3 --bounces 0,4 --lens 0,4,16` are the figures of the lens-sampled planes.  Not run by bench.py."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
import hanamaru_amd as ha  # noqa: E402


def one_pass(r, lens):
    if lens:
        r.render_guides_lens(lens)
    else:
        r.render_guides()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="rtcamp6_v3_1")
    ap.add_argument("--scenes", default="", help="several scenes, comma-separated (overrides --scene)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", default="0,1,4,8")
    ap.add_argument("--lens", default="0", help="lens points per case: 0 (hr_render_guides), 4 or 16 (hr_render_guides_lens)")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    cases = [(int(k), int(n)) for n in a.lens.split(",") for k in a.bounces.split(",")]
    for scene in (a.scenes.split(",") if a.scenes else [a.scene]):
        r = ha.Renderer(0)
        r.upload_scene(ha.Scene(scene))
        r.set_resolution(a.width, a.height)
        for k, n in cases:                                           # warm-up: every kernel once
            r.set_option("guide_bounces", k)
            one_pass(r, n)
        r.synchronize()
        print("scene %s, %dx%d, one guide pass per case (lens 0: hr_render_guides)" % (scene, a.width, a.height))
        ms = {c: [] for c in cases}
        for rnd in range(a.rounds):
            for k, n in cases:
                r.set_option("guide_bounces", k)
                before = r.stats()["debug_kernel_ms"]
                one_pass(r, n)
                r.synchronize()
                ms[(k, n)].append(r.stats()["debug_kernel_ms"] - before)
                print("round %d guide_bounces %d lens %d: %8.3f ms" % (rnd, k, n, ms[(k, n)][-1]))
        print("median: " + ", ".join("K = %d L = %d %.3f ms" % (k, n, sorted(v)[len(v) // 2]) for (k, n), v in ms.items()))
        r.close()


if __name__ == "__main__":
    main()
