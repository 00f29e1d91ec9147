#!/usr/bin/env python3
"""tools/post_parent_diff.py --parent DIR: every post-processing call of DESIGN.md §4.7 to §4.17 in this build and in a build of the PARENT commit,
output by output, as raw bytes.  DIR is the python directory of a build of the parent commit (its hanamaru-renderer_amd/python, beside its own
libhanamaru_hip.so).  Each build runs in a child process of its own (one process loads one library) and leaves its outputs in an .npz file.  The
inputs are the planes of tests/select_noise_numpy.synthetic, written with the write_* calls — no scene, no render: frames 13x7 and 37x19 and a 37x19
region at (5, 3) of 64x48, K = 3 and 9, n uniform (2 K + 1) and mixed per pixel (K .. 64, option sample_counts).  Per case: the three noise images
with their hr_noise summaries, the robust noise trim, R and its trim, D of hr_denoise and of hr_denoise_robust, R' on base 0 and 1, S, L, M, e_S and
its summary with smooth 0 and 2 and levels 0 and 3, the resolves, and (sample_counts on) the three tile selections without and with a mask in
force.  Prints one line per case and ends with 1 when a pair of outputs differs.  Not run by bench.py."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 0.01
TARGETS = (((13, 7), None), ((37, 19), None), ((64, 48), (5, 3, 37, 19)))


def cases():
    for frame, region in TARGETS:
        for K in (3, 9):
            for mixed in (False, True):
                yield frame, region, K, mixed


def case_name(frame, region, K, mixed):
    return "%dx%d%s K=%d n %s" % (frame + ((" region %d,%d %dx%d" % region) if region else "",) + (K, "mixed" if mixed else "uniform"))


def outputs(r, K, mixed, w, h):
    """every call, in one order: (name, array) pairs"""
    out = []

    def keep(name, value):
        out.append((name, np.ascontiguousarray(value)))

    def summary(name, est):
        keep(name, np.array([est["mean_error"], est["max_error"], float(est["samplings"]), float(est["pixels"]), float(est["pixels_above"])]))

    img = r.noise_image(FLOOR)
    thr = float(np.median(img))
    keep("noise image", img)
    summary("noise summary", r.noise_estimate(FLOOR, thr))
    rimg = r.robust_noise_image(FLOOR)
    rthr = float(np.median(rimg))
    keep("robust noise image", rimg)
    keep("robust noise trim", r.robust_noise_trim(FLOOR))
    summary("robust noise summary", r.robust_noise_estimate(FLOOR, rthr))
    r.robust()
    keep("R", r.read_robust())
    keep("R trim", r.read_robust_trim())
    keep("resolve_robust", r.resolve_robust())
    r.denoise()
    keep("D of hr_denoise", r.read_denoised())
    keep("resolve_denoised", r.resolve_denoised())
    r.robust_restore(base=0)
    keep("R' base 0", r.read_restored())
    r.denoise_robust()
    keep("D of hr_denoise_robust", r.read_denoised())
    r.robust_restore(base=1)
    keep("R' base 1", r.read_restored())
    keep("resolve_restored", r.resolve_restored())
    sthr = None
    for smooth in (0, 2):
        for levels in (0, 3):
            tag = " smooth %d levels %d" % (smooth, levels)
            r.denoise_select(smooth=smooth, levels=levels)
            keep("S" + tag, r.read_selected())
            keep("L" + tag, r.read_selected_levels())
            keep("M" + tag, r.selected_mse(smooth=smooth, levels=levels))
            simg = r.selected_noise_image(FLOOR, smooth=smooth, levels=levels)
            sthr = float(np.median(simg))
            keep("selected noise image" + tag, simg)
            summary("selected noise summary" + tag, r.selected_noise_estimate(FLOOR, sthr, smooth=smooth, levels=levels))
    keep("resolve_selected", r.resolve_selected())
    keep("resolve", r.resolve(2 * K + 1))
    if mixed:
        keep("resolve_counted", r.resolve_counted())
        ty, tx = (h + 3) // 4, (w + 3) // 4
        yy, xx = np.mgrid[0:ty, 0:tx]
        checker = ((xx + yy) & 1).astype(np.uint8)
        selections = (("select_tiles", lambda: r.select_tiles(FLOOR, thr)), ("select_tiles_robust", lambda: r.select_tiles_robust(FLOOR, rthr)),
                      ("select_tiles_selected", lambda: r.select_tiles_selected(FLOOR, sthr, smooth=2, levels=3)))
        for name, call in selections:
            for mask in (None, checker):
                r.set_tile_mask(mask)
                active = call()
                keep("%s %s mask" % (name, "without a" if mask is None else "with a"), np.append(r.tile_mask()[0].reshape(-1).astype(np.uint32), active))
        r.set_tile_mask(None)
    return out


def run_build(a):
    """the child: one build, its outputs into a.out"""
    sys.path.insert(0, os.path.abspath(a.package))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hanamaru_amd as ha
    from select_noise_numpy import synthetic
    got = {}
    with ha.Renderer(0) as r:
        for frame, region, K, mixed in cases():
            w, h = region[2:] if region else frame
            r.set_resolution(*frame)
            if region:
                r.set_region(*region)
            r.set_option("moments", 1)
            r.set_option("sample_counts", 1 if mixed else 0)
            r.set_option("robust_buckets", K)
            n = 2 * K + 1
            if mixed:
                n = np.random.default_rng(w * h + K).integers(K, 65, size=(h, w)).astype(np.uint32)
                n.reshape(-1)[:2] = [K, 64]
            B, acc, mom, n, g = synthetic(400 + K, w, h, K, n)
            n_all = int(n.max()) if mixed else int(n)
            r.write_accumulator(acc)
            r.write_moments(mom, n_all)
            r.write_buckets(B, n_all)
            if mixed:
                r.write_sample_counts(n)
            r.write_guides(g)
            for name, value in outputs(r, K, mixed, w, h):
                got[case_name(frame, region, K, mixed) + " | " + name] = value
    np.savez(a.out, **got)
    print(ha.HIP_LIB)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the python directory of a build of the parent commit")
    ap.add_argument("--package", help=argparse.SUPPRESS)          # the child's: the one build it runs
    ap.add_argument("--out", help=argparse.SUPPRESS)              # the child's: where its outputs go
    a = ap.parse_args()
    if a.package:
        return run_build(a)
    if not a.parent:
        ap.error("--parent DIR: the parent commit's outputs are what this build's are held against")
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for who, package in (("parent", a.parent), ("this build", os.path.join(ROOT, "hanamaru-renderer_amd", "python"))):
            out = os.path.join(tmp, who.replace(" ", "_") + ".npz")
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--package", package, "--out", out], stdout=subprocess.PIPE, text=True, timeout=600)
            if child.returncode != 0:
                sys.exit("%s: the process ended with %d" % (who, child.returncode))
            print("%s: %s" % (who, os.path.relpath(child.stdout.strip().splitlines()[-1], ROOT)))
            with np.load(out) as z:
                got[who] = {k: z[k] for k in z.files}
    old, new = got["parent"], got["this build"]
    if sorted(old) != sorted(new):
        sys.exit("the two builds made different calls: %s" % sorted(set(old) ^ set(new)))
    differ = [k for k in new if old[k].dtype != new[k].dtype or old[k].shape != new[k].shape or old[k].tobytes() != new[k].tobytes()]
    for frame, region, K, mixed in cases():
        name = case_name(frame, region, K, mixed)
        keys = [k for k in new if k.startswith(name + " | ")]
        bad = [k.split(" | ")[1] for k in keys if k in differ]
        print("%-34s %3d outputs, %7d bytes: %s" % (name, len(keys), sum(new[k].nbytes for k in keys), "DIFFER: " + ", ".join(bad) if bad else "all equal"))
    print("%d outputs compared as raw bytes, %d differ" % (len(new), len(differ)))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
