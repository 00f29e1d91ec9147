#!/usr/bin/env python3
"""tools/guide_quality.py [--scenes a,b,..] [--bounces 0,1,2,4,8]: DESIGN.md §4.9's quality figure for the guide chain (option "guide_bounces"),
on the HOST, no device: the checker's f64 path tracer renders the 96x54 frame at 16, 64 and 2,048 samplings (the truth; the library's seeds, so
its samplings), the guide planes are the f64 chain over the oracle's intersect_material and material_sample(.., r0 = 1, r1 = 0, ..)
(tests/guide_chain.py oracle_chain), and csrc/denoise_core.h compiled by g++ — the filter the device runs, bit for bit — filters with the default
parameters.  Prints mean((x - t)^2 / (t^2 + 0.01^2)) of the denoised image over that of the raw mean per scene, K and sampling count."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hanamaru-renderer_amd", "python")]
import guide_chain as gc  # noqa: E402
import hanamaru_amd as ha  # noqa: E402
import oracle_py as orc  # noqa: E402
import post_cores as pc  # noqa: E402  (lib / core_denoise: the g++ build of denoise_core.h)

W, H, TRUTH = 96, 54, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="spheres,rtcamp6_v3_1,cornell_mini")
    ap.add_argument("--bounces", default="0,1,2,4,8")
    args = ap.parse_args()
    bounces = [int(k) for k in args.bounces.split(",")]
    core = pc.lib()
    print("| scene | samplings | " + " | ".join("K = %d" % k for k in bounces) + " |")
    print("|---|---|" + "---|" * len(bounces))
    for name in args.scenes.split(","):
        sc = ha.Scene(name)
        osc = orc.OracleScene(sc.desc_ptr)
        guides = {k: gc.planes_of(gc.oracle_chain(orc, osc, sc.desc, W, H, k)[0]).astype(np.float32) for k in bounces}
        acc = np.zeros((H, W, 3))
        s1, s2 = np.zeros((H, W, 3)), np.zeros((H, W, 3))
        short = {}
        for s in range(1, TRUTH + 1):
            x, _ = osc.render(W, H, s, s + 1)                       # one sampling: the sum of the pixel's four sub-samples
            acc += x
            if s <= 64:
                s1 += x
                s2 += x * x
            if s in (16, 64):
                short[s] = (acc.astype(np.float32), np.concatenate([s1, s2], axis=-1))
        truth = acc / (4.0 * TRUTH)
        for s in (16, 64):
            a, mom = short[s]
            e_raw = gc.rel_sq_error(a / np.float32(4 * s), truth)
            cells = ["%.2f" % (gc.rel_sq_error(pc.core_denoise(core, a, mom, s, guides[k]), truth) / e_raw) for k in bounces]
            print("| %s | %d | " % (name, s) + " | ".join(cells) + " |", flush=True)


if __name__ == "__main__":
    main()
