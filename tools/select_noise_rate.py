#!/usr/bin/env python3
"""tools/select_noise_rate.py --parent DIR [--buckets K] [--repeat N]: what one hr_selected_noise_estimate costs, against the
PARENT commit's hr_denoise_select on the same device.  DIR is the python directory of a build of the parent commit (its hanamaru-renderer_amd/python,
beside its own libhanamaru_hip.so).  Each build is measured in a child process of its own (one process loads one library): rtcamp6_v3_1 at 1920x1080
with options moments and robust_buckets K (default 9), 16 samplings, the guide planes rendered, then — after one warm-up call of each — N calls
alternating, timed by hr_stats.post_kernel_ms (the kernels' own event pair), levels 4, smooth 0 and 2.  Prints every time, the medians and the
ratio estimate / parent's select.  Not run by bench.py."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH = (0, 2)


def measure(a):
    """the child: one build, one JSON line"""
    sys.path.insert(0, os.path.abspath(a.package))
    import hanamaru_amd as ha
    r = ha.Renderer(0)
    r.upload_scene(ha.Scene(a.scene, os.path.join(ROOT, "assets")))
    r.set_resolution(a.width, a.height)
    r.set_option("moments", 1)
    r.set_option("robust_buckets", a.buckets)
    r.render(1, a.samplings + 1)
    r.synchronize()
    r.render_guides()

    def timed(call):
        before = r.stats()["post_kernel_ms"]
        call()
        return r.stats()["post_kernel_ms"] - before

    cases = [("select smooth %d" % s, lambda s=s: r.denoise_select(levels=4, smooth=s)) for s in SMOOTH]
    if hasattr(r, "selected_noise_estimate"):
        cases += [("estimate smooth %d" % s, lambda s=s: r.selected_noise_estimate(0.01, 0.05, levels=4, smooth=s)) for s in SMOOTH]
    for _, call in cases:
        timed(call)
    times = {name: [] for name, _ in cases}
    for _ in range(a.repeat):
        for name, call in cases:
            times[name].append(timed(call))
    r.close()
    print(json.dumps({"library": ha.HIP_LIB, "times": times}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="rtcamp6_v3_1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samplings", type=int, default=16)
    ap.add_argument("--buckets", type=int, default=9)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--parent", help="the python directory of a build of the parent commit")
    ap.add_argument("--package", help=argparse.SUPPRESS)          # the child's: the one build it measures
    a = ap.parse_args()
    if a.package:
        return measure(a)
    if not a.parent:
        ap.error("--parent DIR: the parent commit's hr_denoise_select is the yardstick")
    got = {}
    for who, package in (("parent", a.parent), ("this build", os.path.join(ROOT, "hanamaru-renderer_amd", "python"))):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--package", package, "--scene", a.scene, "--width", str(a.width), "--height", str(a.height),
                                "--samplings", str(a.samplings), "--buckets", str(a.buckets), "--repeat", str(a.repeat)], stdout=subprocess.PIPE, text=True, timeout=600)
        if child.returncode != 0:
            sys.exit("%s: the measuring process ended with %d" % (who, child.returncode))
        got[who] = json.loads(child.stdout.strip().splitlines()[-1])
    print("scene %s, %dx%d, K = %d, %d samplings, levels 4, hr_stats.post_kernel_ms of %d calls each" % (a.scene, a.width, a.height, a.buckets, a.samplings, a.repeat))
    med = {}
    for who in ("parent", "this build"):
        print("%s: %s" % (who, os.path.relpath(got[who]["library"], ROOT)))
        for name, t in got[who]["times"].items():
            med[who, name] = statistics.median(t)
            print("  %-18s ms: " % name + " ".join("%.3f" % v for v in t) + "   median %.3f" % med[who, name])
    for s in SMOOTH:
        est, sel = med["this build", "estimate smooth %d" % s], med["parent", "select smooth %d" % s]
        print("smooth %d: hr_selected_noise_estimate %.3f ms, the parent's hr_denoise_select %.3f ms, ratio %.3f (this build's hr_denoise_select: %.3f ms)"
              % (s, est, sel, est / sel, med["this build", "select smooth %d" % s]))


if __name__ == "__main__":
    main()
