"""The checker-side helpers of the post-processing quality figures, shared by the tests and by tools/*_quality.py: the
per-sampling renders of the oracle, cached per scene, and the figures taken from them through the host build of the core headers.

No GPU in this module."""
import numpy as np

import guide_chain as gc
from post_cores import core_denoise, core_error, core_filter, core_r, core_restore
from post_numpy import bits, fill_buckets, numpy_error, rel_sq_error, sums_of

# the robust resolve and its noise estimate: frame, samplings, buckets, truth samplings
QW, QH, QN, QK, QTRUTH = 48, 27, 64, 9, 2048
# the short render of the filters: frame, samplings, guide_bounces, truth samplings
SHORT_W, SHORT_H, SHORT_N, SHORT_BOUNCES, SHORT_TRUTH = 96, 54, 16, 2, 512
_sets, _short = {}, {}


def oracle_buckets_and_truth(osc, w, h, n, ks, truth_n, truth_begin=100001):
    """({K: buckets of samplings 1 .. n}, fp32 accumulator of them, truth radiance from truth_n samplings starting at truth_begin)."""
    x = np.stack([osc.render(w, h, s, s + 1)[0] for s in range(1, n + 1)]).astype(np.float32)    # x_s: one sampling's 2x2 sum per pixel
    truth, _ = osc.render(w, h, truth_begin, truth_begin + truth_n)
    return {K: fill_buckets(x, K) for K in ks}, sums_of(x)[0], truth.astype(np.float64) / (4.0 * truth_n)


def oracle_sets(scenes, name):
    """The buckets of samplings 1 .. 64 and of 65 .. 128, K = 9, rendered once per scene."""
    if name not in _sets:
        _, osc = scenes(name)
        x = np.stack([osc.render(QW, QH, s, s + 1)[0] for s in range(1, 2 * QN + 1)]).astype(np.float32)
        _sets[name] = (fill_buckets(x[:QN], QK), fill_buckets(x[QN:], QK))
    return _sets[name]


def oracle_short_render(orc, scenes, name):
    """(per-sampling values x (SHORT_N, h, w, 3) fp32, fp32 accumulator, moments, guide planes with SHORT_BOUNCES bounces, truth radiance), once
    per scene."""
    if name not in _short:
        sc, osc = scenes(name)
        x = np.stack([osc.render(SHORT_W, SHORT_H, s, s + 1)[0] for s in range(1, SHORT_N + 1)]).astype(np.float32)
        acc, mom = sums_of(x)
        guides = gc.planes_of(gc.oracle_chain(orc, osc, sc.desc, SHORT_W, SHORT_H, SHORT_BOUNCES)[0]).astype(np.float32)
        truth, _ = osc.render(SHORT_W, SHORT_H, 100001, 100001 + SHORT_TRUTH)
        _short[name] = (x, acc, mom, guides, truth.astype(np.float64) / (4.0 * SHORT_TRUTH))
    return _short[name]


def plain_spread_error(buckets, n, floor=0.01):
    """The untrimmed counterpart of the robust noise estimate: the standard error of the mean of the K bucket means of the channel sum, over that
    mean + 3 floor."""
    B = np.asarray(buckets, dtype=np.float64)
    K = B.shape[-2]
    nb = (np.uint64(n) - np.arange(K, dtype=np.uint64) + np.uint64(K - 1)) // np.uint64(K)
    y = (B / nb.astype(np.float64)[:, None] / 4.0).sum(axis=-1)
    se = y.std(axis=-1, ddof=1) / np.sqrt(K)
    den = y.mean(axis=-1) + 3.0 * floor
    return np.where(den > 0.0, se / np.where(den > 0.0, den, 1.0), 0.0)


def rms_z(core, A, B, n, floor=0.01):
    """z = (Ry_A - Ry_B) / sqrt(se_A^2 + se_B^2) per pixel: its RMS over the pixels with a non-zero denominator, and the share of those without."""
    eA, eB = core_error(core, A, n, floor)[0], core_error(core, B, n, floor)[0]
    _, _, seA, ryA, _ = numpy_error(A, n, floor, parts=True)
    _, _, seB, ryB, _ = numpy_error(B, n, floor, parts=True)
    assert np.array_equal(bits(eA), bits(numpy_error(A, n, floor)[0])) and np.array_equal(bits(eB), bits(numpy_error(B, n, floor)[0]))
    den = np.sqrt(seA ** 2 + seB ** 2)
    ok = den > 0
    z = (ryA[ok] - ryB[ok]) / den[ok]
    return float(np.sqrt(np.mean(z ** 2))), float(1.0 - ok.mean())


def quality_figures(core, x, acc, mom, guides, truth, K):
    """(R / mean, D / mean, DR / R, DR / D): relative squared errors of the robust radiance, hr_denoise and the robust denoiser."""
    n = x.shape[0]
    B = fill_buckets(x, K)
    e_mean = rel_sq_error(acc / np.float32(4 * n), truth)
    e_r = rel_sq_error(core_r(core, B, n)[0], truth)
    e_d = rel_sq_error(core_denoise(core, acc, mom, n, guides), truth)
    e_dr = rel_sq_error(core_filter(core, B, n, guides), truth)
    return e_r / e_mean, e_d / e_mean, e_dr / e_r, e_dr / e_d


def restore_figures(core, x, guides, truth, K):
    """{R / mean, R' / mean, R' (base DR) / mean, sum R / sum M, sum R' / sum M, R' / R} of the samplings x (n, h, w, 3): relative squared errors against
    the truth as ratios, and the energy against M, the plain mean of the bucket means."""
    n = x.shape[0]
    B = fill_buckets(x, K)
    acc = sums_of(x)[0]
    nb = (n - np.arange(K) + K - 1) // K
    M = (B / nb[:, None] / 4.0).mean(axis=-2)
    R = core_r(core, B, n)[0]
    Rp = core_restore(core, B, n, guides)
    DR = core_filter(core, B, n, guides)
    Rpd = core_restore(core, B, n, guides, D=DR, base=1)
    e_mean = rel_sq_error(acc / np.float32(4 * n), truth)
    e_r, e_rp, e_rpd = rel_sq_error(R, truth), rel_sq_error(Rp, truth), rel_sq_error(Rpd, truth)
    return {"R/mean": e_r / e_mean, "R'/mean": e_rp / e_mean, "R'(DR)/mean": e_rpd / e_mean, "sumR/sumM": float(R.astype(np.float64).sum() / M.sum()),
            "sumR'/sumM": float(Rp.astype(np.float64).sum() / M.sum()), "R'/R": e_rp / e_r}
