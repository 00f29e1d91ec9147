"""Which derived image survives which mutation, on the MI355X: a characterisation matrix.  Rows are the calls that change what
an image was made of, columns the derived images — the guide planes, D of hr_denoise, D of hr_denoise_robust, R, R' on R (base 0), R' on D (base 1).
A cell says whether the image, made on a fresh state, can still be read after the call: 1 = its read returns OK, 0 = HR_ERR_INVALID.  EXPECTED was
recorded from the library as it stood before the validity table replaced the per-image flags, and holds for the table unchanged.

The state of every cell: cornell_mini, a 20 x 12 frame (240 pixels: one partial span of 256, the makers' edge path), options moments and
sample_counts on, robust_buckets 3, samplings 1 .. 6 rendered; the denoisers and the restore run one level."""
import numpy as np
import pytest

from gpu_helpers import error_of

pytestmark = pytest.mark.gpu

HR_ERR_INVALID, HR_ERR_UNSUPPORTED = -1, -6
W, H, K, N = 20, 12, 3, 6
COLUMNS = ["guides", "D denoise", "D denoise_robust", "R", "R' base 0", "R' base 1"]


class Rig:
    """the renderer under test, a second one on the same device for the fold, a tensor to bind, and planes to write back"""

    def __init__(self, ha, sc):
        import torch
        self.ha, self.sc = ha, sc
        self.r, self.peer = ha.Renderer(0), ha.Renderer(0)
        for x in (self.r, self.peer):
            x.upload_scene(sc)
        self.tensor = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
        self.fresh()
        r = self.r
        r.render_guides()
        self.acc, (self.mom, _), self.cnt, (self.B, _), self.g = r.read_accumulator(), r.read_moments(), r.read_sample_counts(), r.read_buckets(), r.read_guides()
        assert (self.cnt == N).all() and self.B.shape == (H, W, K, 3) and self.B.any() and self.g.any()

    def close(self):
        self.r.close()
        self.peer.close()

    def planes(self, x, by_sampling=0):
        """a new target with the three plane options on: every plane zeroed, no derived image, no mask, no bound accumulator"""
        x.set_option("guide_bounces", 0)
        x.set_option("bucket_by_sampling", by_sampling)
        x.set_resolution(W, H)
        x.set_option("moments", 1)
        x.set_option("sample_counts", 1)
        x.set_option("robust_buckets", K)

    def fresh(self, by_sampling=0):
        self.planes(self.r, by_sampling)
        self.r.render(1, N + 1)

    def fold(self):
        ha, r, peer = self.ha, self.r, self.peer
        self.planes(peer, 1)
        ha.comm_init_local([r, peer])
        try:
            ha.fold_statistics([r, peer])
        finally:
            r.comm_destroy()


@pytest.fixture(scope="module")
def rig(ha, scenes):
    x = Rig(ha, scenes("cornell_mini")[0])
    yield x
    x.close()


def _restore_on_d(r):
    r.denoise_robust(levels=1)
    r.robust_restore(levels=1, base=1)


# column -> (how the image is made on the fresh state, the reads that must agree about it)
MAKERS = {
    "guides": (lambda r: r.render_guides(), ["read_guides"]),
    "D denoise": (lambda r: r.denoise(levels=1), ["read_denoised", "resolve_denoised"]),
    "D denoise_robust": (lambda r: r.denoise_robust(levels=1), ["read_denoised", "resolve_denoised"]),
    "R": (lambda r: r.robust(), ["read_robust", "read_robust_trim", "resolve_robust"]),
    "R' base 0": (lambda r: r.robust_restore(levels=1, base=0), ["read_restored", "resolve_restored"]),
    "R' base 1": (_restore_on_d, ["read_restored", "resolve_restored"]),
}


def _refused(x, code, fn, *a, **kw):
    assert error_of(x.ha, fn, *a, **kw)[0] == code


def _restore_base_1(x):
    """base 1 needs a D of hr_denoise_robust: where the cell's state has none the call is refused, and the cell says what a refusal leaves"""
    try:
        x.r.robust_restore(levels=1, base=1)
    except x.ha.HipError as e:
        assert e.code == HR_ERR_INVALID


def _options_off_render_debug(x):
    """hr_render_debug runs only with the three plane options off — and switching them off is a mutation of its own"""
    for key in ("moments", "sample_counts", "robust_buckets"):
        x.r.set_option(key, 0)
    x.r.render_debug(0)


def _off_on(key):
    def call(x):
        x.r.set_option(key, 0)
        x.r.set_option(key, 1)
    return call


CHECKER = (np.indices(((H + 3) // 4, (W + 3) // 4)).sum(axis=0) & 1).astype(np.uint8)

# row -> the mutation (of the rig).  "fold_statistics" starts from buckets indexed by the sampling: a fold refuses the others.
ROWS = {
    "render": lambda x: x.r.render(N + 1, N + 2),
    "render_debug refused": lambda x: _refused(x, HR_ERR_UNSUPPORTED, x.r.render_debug, 0),
    "options off, render_debug": _options_off_render_debug,
    "clear": lambda x: x.r.clear(),
    "write_accumulator": lambda x: x.r.write_accumulator(x.acc),
    "write_moments": lambda x: x.r.write_moments(x.mom, N),
    "write_sample_counts": lambda x: x.r.write_sample_counts(x.cnt),
    "write_buckets": lambda x: x.r.write_buckets(x.B, N),
    "write_guides": lambda x: x.r.write_guides(x.g),
    "render_guides": lambda x: x.r.render_guides(),
    "guide_bounces same": lambda x: x.r.set_option("guide_bounces", 0),
    "guide_bounces other": lambda x: x.r.set_option("guide_bounces", 2),
    "moments off": lambda x: x.r.set_option("moments", 0),
    "moments off, on": _off_on("moments"),
    "moments same": lambda x: x.r.set_option("moments", 1),
    "sample_counts off": lambda x: x.r.set_option("sample_counts", 0),
    "sample_counts off, on": _off_on("sample_counts"),
    "sample_counts same": lambda x: x.r.set_option("sample_counts", 1),
    "robust_buckets same": lambda x: x.r.set_option("robust_buckets", K),
    "robust_buckets other": lambda x: x.r.set_option("robust_buckets", 5),
    "robust_buckets off": lambda x: x.r.set_option("robust_buckets", 0),
    "bucket_by_sampling same": lambda x: x.r.set_option("bucket_by_sampling", 0),
    "bucket_by_sampling toggled": lambda x: x.r.set_option("bucket_by_sampling", 1),
    "set_region": lambda x: x.r.set_region(2, 1, 9, 6),
    "set_resolution": lambda x: x.r.set_resolution(W, H),
    "upload_scene": lambda x: x.r.upload_scene(x.sc),
    "bind_accumulator": lambda x: x.r.bind_accumulator(x.tensor.data_ptr()),
    "fold_statistics": lambda x: x.fold(),
    "set_tile_mask": lambda x: x.r.set_tile_mask(CHECKER),
    "robust": lambda x: x.r.robust(),
    "denoise": lambda x: x.r.denoise(levels=1),
    "denoise_robust": lambda x: x.r.denoise_robust(levels=1),
    "robust_restore base 0": lambda x: x.r.robust_restore(levels=1, base=0),
    "robust_restore base 1": _restore_base_1,
}

# one digit per column, in COLUMNS' order
EXPECTED = {
    "render":                     "100000",
    "render_debug refused":       "111111",
    "options off, render_debug":  "100000",
    "clear":                      "100000",
    "write_accumulator":          "100000",
    "write_moments":              "100000",   # R and its R' too: conservative, the buckets are not the moments'
    "write_sample_counts":        "100000",
    "write_buckets":              "100000",   # D of hr_denoise too: conservative
    "write_guides":               "100100",
    "render_guides":              "100100",
    "guide_bounces same":         "111111",
    "guide_bounces other":        "000100",
    "moments off":                "100000",
    "moments off, on":            "100000",
    "moments same":               "111111",
    "sample_counts off":          "100000",
    "sample_counts off, on":      "100000",
    "sample_counts same":         "111111",
    "robust_buckets same":        "111111",
    "robust_buckets other":       "100000",   # (the counts and the moments start over with the buckets: D of hr_denoise goes)
    "robust_buckets off":         "110000",   # (the counts stay: D of hr_denoise stays)
    "bucket_by_sampling same":    "111111",
    "bucket_by_sampling toggled": "100000",
    "set_region":                 "000000",
    "set_resolution":             "000000",
    "upload_scene":               "000100",   # R is not made of the scene's guides; its R' is
    "bind_accumulator":           "100000",
    "fold_statistics":            "100000",
    "set_tile_mask":              "111111",
    "robust":                     "111111",   # R' is not made of R
    "denoise":                    "111110",   # a new D: only the R' that was based on D
    "denoise_robust":             "111110",
    "robust_restore base 0":      "111111",
    "robust_restore base 1":      "111111",
}


def observe(x, row):
    """the row as the library has it: a digit per column"""
    out = ""
    for col in COLUMNS:
        make, reads = MAKERS[col]
        x.fresh(by_sampling=1 if row == "fold_statistics" else 0)
        make(x.r)
        for name in reads:
            getattr(x.r, name)()                                                       # readable before the call
        ROWS[row](x)
        codes = set()
        for name in reads:
            try:
                getattr(x.r, name)()
                codes.add(0)
            except x.ha.HipError as e:
                codes.add(e.code)
        assert len(codes) == 1 and codes <= {0, HR_ERR_INVALID}, (row, col, codes)     # every read of the image says the same, OK or HR_ERR_INVALID
        out += "1" if codes == {0} else "0"
    return out


@pytest.mark.parametrize("row", list(ROWS))
def test_matrix_row(rig, row):
    got = observe(rig, row)
    print("%-28s %s" % (row, got))
    assert got == EXPECTED[row], (row, dict(zip(COLUMNS, zip(got, EXPECTED[row]))))
