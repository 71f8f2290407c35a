"""A plain-Python statement of what include/ditherpie_hip_png_file.h and dither_pie_amd/apng.py write: the chunk, the packed
assembly of a call, and the whole APNG file around given zlib streams.  struct and zlib.crc32 only; it shares no code with
the package."""
import struct
import zlib
from fractions import Fraction

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def crc(data):
    return zlib.crc32(data) & 0xFFFFFFFF


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc(kind + data))


def frame_chunk(stream, f, n_idat, seq0, seq_step):
    if f < n_idat:
        return chunk(b"IDAT", stream)
    return chunk(b"fdAT", struct.pack(">I", (seq0 + (f - n_idat) * seq_step) & 0xFFFFFFFF) + stream)


def assemble(streams, pre=None, post=None, n_idat=None, seq0=0, seq_step=2):
    """-> (bytes, offsets).  pre: None, bytes (shared) or a list of bytes (one per frame); post: None or bytes."""
    n_idat = len(streams) if n_idat is None else n_idat
    out, offsets = b"", [0]
    for f, s in enumerate(streams):
        p = b"" if pre is None else pre if isinstance(pre, bytes) else pre[f]
        out += p + frame_chunk(s, f, n_idat, seq0, seq_step) + (post or b"")
        offsets.append(len(out))
    return out, offsets


def png_depth(k):
    return 1 if k <= 2 else 2 if k <= 4 else 4 if k <= 16 else 8


def delay(fps):
    r = Fraction(fps).limit_denominator(65535)
    return r.denominator, r.numerator


def delta_planes(planes, transparent):
    """Frame 0 whole; every other frame holds `transparent` where it equals the original previous plane."""
    out = planes.copy()
    for f in range(1, len(planes)):
        out[f][planes[f] == planes[f - 1]] = transparent
    return out


def apng_plan(k, delta):
    """-> (entries in PLTE, transparent index or None, bit depth)"""
    keyed = delta and k <= 255
    return (k + 1 if keyed else k), (k if keyed else None), png_depth(k + 1 if keyed else k)


def apng_file(width, height, palette, delta, loop, fps, streams):
    """The file ApngWriter writes around the per-frame zlib streams (of delta_planes(...) at apng_plan's depth)."""
    pal = np.asarray(palette, np.uint8)
    k = len(pal)
    entries, transparent, depth = apng_plan(k, delta)
    num, den = delay(fps)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, 3, 0, 0, 0))
    out += chunk(b"acTL", struct.pack(">II", len(streams), loop))
    out += chunk(b"PLTE", pal.tobytes() + bytes(3 * (entries - k)))
    if transparent is not None:
        out += chunk(b"tRNS", b"\xff" * k + b"\x00")
    for i, s in enumerate(streams):
        blend = 1 if (transparent is not None and i > 0) else 0
        out += chunk(b"fcTL", struct.pack(">IIIIIHHBB", 0 if i == 0 else 2 * i - 1, width, height, 0, 0, num, den, 0, blend))
        out += chunk(b"IDAT", s) if i == 0 else chunk(b"fdAT", struct.pack(">I", 2 * i) + s)
    return out + chunk(b"IEND", b"")


def clip(rs, n, h, w, k, repeat=0.6):
    """n planes of k colours of which about `repeat` of the pixels repeat the frame before."""
    planes = rs.randint(0, k, (n, h, w)).astype(np.uint8)
    for f in range(1, n):
        keep = rs.rand(h, w) < repeat
        planes[f][keep] = planes[f - 1][keep]
    return planes
