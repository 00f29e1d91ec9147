"""The checkpoint file of hanamaru-hip (hanamaru-renderer_amd/host/checkpoint.h states the format) read and packed in Python, with the fields
of the C++ struct.  Shared by the CLI tests and tests/test_checkpoint_cpu.py.  Not a test module."""
import struct
from types import SimpleNamespace

import numpy as np

FRAME, REGION, MOMENTS, COUNTS, BUCKETS = (struct.unpack("<I", m)[0] for m in (b"HRA2", b"HRR2", b"HRMS", b"HRSC", b"HRBK"))
S_NONE, S_HEADER, S_ACCUMULATOR, S_MOMENTS, S_COUNTS, S_BUCKETS = range(6)


def scene_hash(name):
    """FNV-1a of the scene name, the header's last word."""
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xffffffff
    return h


def new(width, height, samplings, scene, acc, region=None, moments=None, counts=None, buckets=None):
    """A checkpoint from its values: region (x0, y0, w, h) or None, acc [h, w, 3], moments (n, [h, w, 6]), counts [h, w], buckets (n, [h, w, K, 3])."""
    c = SimpleNamespace(magic=REGION if region else FRAME, width=width, height=height, samplings=samplings, scene_hash=scene_hash(scene),
                        region=tuple(region or (0, 0, width, height)), acc=np.asarray(acc, np.float32),
                        has_moments=moments is not None, moments_n=0, moments=None, has_counts=counts is not None, counts=None,
                        has_buckets=buckets is not None, buckets_head=buckets is not None, buckets_k=0, buckets_n=0, buckets=None)
    if moments is not None:
        c.moments_n, c.moments = moments[0], np.asarray(moments[1], np.float64)
    if counts is not None:
        c.counts = np.asarray(counts, np.uint32)
    if buckets is not None:
        c.buckets_n, c.buckets = buckets[0], np.asarray(buckets[1], np.float64)
        c.buckets_k = c.buckets.shape[2]
    return c


def pack(c):
    """The file's bytes."""
    raw = struct.pack("<5I", c.magic, c.width, c.height, c.samplings, c.scene_hash)
    if c.magic == REGION:
        raw += struct.pack("<4I", *c.region)
    raw += c.acc.astype("<f4").tobytes()
    if c.has_moments:
        raw += struct.pack("<IQ", MOMENTS, c.moments_n) + c.moments.astype("<f8").tobytes()
    if c.has_counts:
        raw += struct.pack("<I", COUNTS) + c.counts.astype("<u4").tobytes()
    if c.has_buckets:
        raw += struct.pack("<IIQ", BUCKETS, c.buckets_k, c.buckets_n) + c.buckets.astype("<f8").tobytes()
    return raw


def parse(raw):
    """The sections in order, each sized by the file's own header, up to the first that is absent or cut short — as ckpt::read.  On top of
    the struct's fields: size (the file's length) and used (the bytes of the sections read: used == size says that nothing else follows)."""
    c = SimpleNamespace(magic=0, width=0, height=0, samplings=0, scene_hash=0, region=(0, 0, 0, 0), acc=None, has_moments=False, moments_n=0, moments=None,
                        has_counts=False, counts=None, has_buckets=False, buckets_head=False, buckets_k=0, buckets_n=0, buckets=None,
                        complete=S_NONE, cut=S_HEADER, size=len(raw), used=0)
    pos = 0

    def take(fmt):
        nonlocal pos
        n = struct.calcsize(fmt)
        if pos + n > len(raw):
            return None
        pos += n
        return struct.unpack(fmt, raw[pos - n:pos])

    def array(dtype, shape):
        nonlocal pos
        n = int(np.prod(shape, dtype=object)) * np.dtype(dtype).itemsize
        if pos + n > len(raw):
            return None
        pos += n
        return np.frombuffer(raw, dtype=dtype, count=n // np.dtype(dtype).itemsize, offset=pos - n).reshape(shape)

    def done(section):
        c.complete, c.cut, c.used = section, S_NONE, pos
        return (take("<I") or (0,))[0]   # the magic of the trailer that follows, 0 at the end of the file

    hdr = take("<5I")
    if hdr is None:
        return c
    c.magic, c.width, c.height, c.samplings, c.scene_hash = hdr
    c.region = (0, 0, c.width, c.height)
    if c.magic not in (FRAME, REGION):
        return c
    if c.magic == REGION:
        c.region = take("<4I")
        if c.region is None:
            c.region = (0, 0, c.width, c.height)
            return c
    w, h = c.region[2:]
    c.complete, c.cut, c.used = S_HEADER, S_ACCUMULATOR, pos
    c.acc = array("<f4", (h, w, 3))
    if c.acc is None:
        return c
    magic = done(S_ACCUMULATOR)
    if magic == MOMENTS:
        c.cut = S_MOMENTS
        n = take("<Q")
        if n is None:
            return c
        c.moments_n = n[0]
        c.moments = array("<f8", (h, w, 6))
        if c.moments is None:
            return c
        c.has_moments = True
        magic = done(S_MOMENTS)
    if magic == COUNTS:
        c.cut = S_COUNTS
        c.counts = array("<u4", (h, w))
        if c.counts is None:
            return c
        c.has_counts = True
        magic = done(S_COUNTS)
    if magic == BUCKETS:
        c.cut = S_BUCKETS
        k, n = take("<I"), take("<Q")
        c.buckets_k = k[0] if k else 0
        if n is None:
            return c
        c.buckets_head, c.buckets_n = True, n[0]
        c.buckets = array("<f8", (h, w, c.buckets_k, 3))
        if c.buckets is None:
            return c
        c.has_buckets = True
        done(S_BUCKETS)
    return c


def read(path):
    with open(str(path), "rb") as f:
        return parse(f.read())
