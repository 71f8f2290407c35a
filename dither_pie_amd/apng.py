"""Animated PNG output: ApngWriter wraps the device's zlib streams (backend.png_deflate), inter-frame deltas
(backend.DeltaStream) and finished chunks (backend.png_file_assemble: CRC-32 and chunk framing on the device) in an APNG
container.  The pixels never leave the GPU uncompressed, and what comes back per add() is exactly the bytes that go into the
file, in one copy.

    with ApngWriter(open("clip.png", "w+b"), width, height, fps) as a:
        a.add(planes, palette)            # planes: uint8 CUDA [N,H,W] palette indices, palette: [K,3] uint8, K <= 256

What GIF cannot do and this can: all 256 colours together with deltas' savings up to 255, and an exact frame rate -- the
delay is a fraction of two 16-bit numbers (delay(fps)), so 30 fps is 1/30 s and 30000/1001 fps is 1001/30000 s.

Layout of the file: signature, IHDR (colour type 3, no interlace), acTL (frame count, loop count), PLTE, tRNS when deltas are
on, then per frame i an fcTL chunk (sequence number 0 for i = 0, else 2 i - 1; the whole canvas at offset 0, 0; the delay;
dispose_op 0 -- leave in place; blend_op 1 -- over -- for a delta frame, else 0 -- source) and ONE data chunk: IDAT for
i = 0, fdAT with sequence number 2 i for the others.  IEND.  A decoder that knows no APNG shows frame 0.

One palette per file: an APNG has a single PLTE.  The palette of the first add() is the file's; a later add() with other
colours raises ValueError.

Deltas (delta=True, the default) and the palette: with K <= 255 colours PLTE gets K + 1 entries, entry K = (0, 0, 0), and
tRNS makes exactly that entry transparent (K bytes of 255 and one 0); the bit depth is png_depth(K + 1).  So deltas cost
a depth step at K = 2, 4 and 16 (1 -> 2, 2 -> 4, 4 -> 8 bits per pixel), as GIF's extra table bit does; pass delta=False
where that matters more than the repeats.  At K = 256 no index is left: K entries, no tRNS, every frame whole -- as with
delta=False at any K.  `delta` and `blocks` are fixed at construction: `delta` decides IHDR, PLTE and tRNS.

Delta rule (the one GifWriter uses): the first frame of the file goes out whole; every other frame holds index K where it
equals the ORIGINAL previous plane.  The result does not depend on how the stream was cut into add() calls.

The file object must be seekable: acTL holds the frame count, which is known at close(); it is written with a placeholder
and patched there, with its CRC.  A writer that never got a frame writes nothing.

encoder="host" produces the same file through the library's host statements (backend.png_deflate_host,
backend.png_file_assemble_host) on host arrays, with no GPU involved.

Not built: cropping delta frames to their dirty rectangle, a palette per frame or scene, several devices.
"""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

from .png import PNG_SIGNATURE, chunk

APNG_MAX_COLOURS = 256
FCTL_BYTES = 38


def delay(fps):
    """The frame delay as APNG stores it: (numerator, denominator) of 1 / fps in seconds, from the closest fraction to fps with
    a denominator of at most 65535.  ValueError unless both numbers fit 1 ... 65535."""
    try:
        rate = Fraction(fps)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f"fps must be a positive number, not {fps!r}") from None
    if rate <= 0:
        raise ValueError(f"fps must be positive, not {fps!r}")
    rate = rate.limit_denominator(65535)
    num, den = rate.denominator, rate.numerator
    if not (1 <= num <= 65535 and 1 <= den <= 65535):
        raise ValueError(f"a frame delay of 1 / {fps!r} s does not fit two numbers of 1 ... 65535")
    return num, den


def _palette(palette):
    pal = np.asarray(palette)
    if pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
        raise ValueError("palette must be [K,3] with K >= 1")
    if pal.shape[0] > APNG_MAX_COLOURS:
        raise ValueError(f"a PNG palette holds {APNG_MAX_COLOURS} colours, not {pal.shape[0]}")
    if pal.min() < 0 or pal.max() > 255:
        raise ValueError("palette entries must be in 0 ... 255")
    return np.ascontiguousarray(pal.astype(np.uint8))


def fctl(seq, width, height, delay_num, delay_den, blend):
    """One fcTL chunk (38 bytes): the whole canvas, dispose_op 0."""
    return chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, width, height, 0, 0, delay_num, delay_den, 0, blend))


class _DeviceEncoder:
    """Deltas, streams, CRCs and chunks on the GPU; what ApngWriter uses unless told otherwise."""

    def __init__(self, seg_bytes, blocks):
        self.seg_bytes, self.blocks, self.stream = seg_bytes, blocks, None

    def check(self, planes):
        import torch
        if not (isinstance(planes, torch.Tensor) and planes.is_cuda):
            raise ValueError("planes must be a CUDA tensor (encoder='host' takes host arrays)")
        if planes.dtype != torch.uint8:
            raise ValueError(f"planes must be one-byte indices (torch.uint8), not {planes.dtype}: a PNG palette holds 256 colours")
        return planes if planes.dim() == 3 else planes.unsqueeze(0)

    def encode(self, planes, depth, transparent, prefixes, n_idat, seq0):
        from . import backend
        todo = planes
        if transparent is not None:
            if self.stream is None or self.stream.device != planes.device:
                self.stream = backend.DeltaStream(planes.device)
            todo, _ = self.stream.add(planes, transparent)
        parts = []
        for a in range(0, todo.shape[0], backend.PNG_MAX_FRAMES):
            b = min(todo.shape[0], a + backend.PNG_MAX_FRAMES)
            payload, sizes = backend.png_deflate(todo[a:b], depth, self.seg_bytes, self.blocks)
            idat = max(0, n_idat - a)
            out, offsets = backend.png_file_assemble(payload, sizes, pre=prefixes[a:b], n_idat=idat, seq0=seq0 + 2 * (a - n_idat + idat), seq_step=2)
            parts.append(memoryview(out[:int(offsets[-1].item())].cpu().numpy()))   # exactly the chunks' bytes, one copy
        return parts[0] if len(parts) == 1 else b"".join(parts)


class _HostEncoder:
    """The same on the host (the library's host statements and a numpy comparison): no device involved."""

    def __init__(self, seg_bytes, blocks):
        self.seg_bytes, self.blocks, self.prev = seg_bytes, blocks, None

    def check(self, planes):
        if hasattr(planes, "detach"):
            if planes.is_cuda:
                raise ValueError("encoder='host' takes host arrays, not CUDA tensors")
            planes = planes.detach().numpy()
        planes = np.asarray(planes)
        if planes.dtype != np.uint8:
            raise ValueError(f"planes must be one-byte indices (uint8), not {planes.dtype}: a PNG palette holds 256 colours")
        return planes if planes.ndim == 3 else planes[None]

    def encode(self, planes, depth, transparent, prefixes, n_idat, seq0):
        from . import backend
        todo = planes
        if transparent is not None:
            todo = planes.copy()
            before = np.concatenate([planes[:1] if self.prev is None else self.prev[None], planes[:-1]])
            same = planes == before
            if self.prev is None:
                same[0] = False
            todo[same] = transparent
            self.prev = planes[-1].copy()
        streams = backend.png_deflate_host(todo, depth, self.seg_bytes, self.blocks)
        return backend.png_file_assemble_host(streams, pre=prefixes, n_idat=n_idat, seq0=seq0, seq_step=2)[0]


class ApngWriter:
    """ApngWriter(fileobj, width, height, fps, loop=0, delta=True): an animated PNG written frame batch by frame batch.
    fileobj: a seekable binary file object (it is not closed by close()).  loop: repetitions, 0 = forever.  delta: write
    frames as differences from their predecessor where the palette leaves an index free (the module's text: a depth step at
    K = 2, 4 and 16).  seg_bytes, blocks: passed to the deflate encoder.  encoder: "device" (the GPU; a missing kernel is an
    error, nothing falls back) or "host" (the library's host statements of the same bytes, for machines without a GPU)."""

    def __init__(self, fileobj, width, height, fps, loop=0, delta=True, seg_bytes=None, encoder="device", blocks="fixed"):
        self.width, self.height = int(width), int(height)
        if not (1 <= self.width < 2 ** 31 and 1 <= self.height < 2 ** 31):
            raise ValueError("a PNG is 1 ... 2^31 - 1 pixels wide and high")
        if not 0 <= int(loop) < 2 ** 31:
            raise ValueError("loop must be in 0 ... 2^31 - 1")
        if encoder not in ("device", "host"):
            raise ValueError(f"encoder must be 'device' or 'host', not {encoder!r}")
        if blocks not in ("fixed", "dynamic"):
            raise ValueError(f"blocks must be 'fixed' or 'dynamic', not {blocks!r}")
        if seg_bytes is not None and not 256 <= int(seg_bytes) <= 32768:
            raise ValueError(f"seg_bytes must be in 256 ... 32768, not {seg_bytes!r}")
        try:
            seekable = bool(fileobj.seekable())
        except AttributeError:
            seekable = False
        if not seekable:
            raise ValueError("fileobj must be seekable: the frame count in acTL is patched at close()")
        self.delay, self.loop, self.delta = delay(fps), int(loop), bool(delta)
        self.f = fileobj
        self.enc = (_DeviceEncoder if encoder == "device" else _HostEncoder)(seg_bytes, blocks)
        self.palette = None
        self.depth = None
        self.transparent = None
        self.actl_at = None
        self.n_frames = 0
        self.closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _actl(self):
        return chunk(b"acTL", struct.pack(">II", self.n_frames, self.loop))

    def _header(self, pal):
        from . import backend
        k = pal.shape[0]
        keyed = self.delta and k <= 255
        self.transparent = k if keyed else None
        self.depth = backend.png_depth(k + 1 if keyed else k)
        self.f.write(PNG_SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", self.width, self.height, self.depth, 3, 0, 0, 0)))
        self.actl_at = self.f.tell()
        tail = chunk(b"PLTE", pal.tobytes() + (b"\x00\x00\x00" if keyed else b""))
        if keyed:
            tail += chunk(b"tRNS", b"\xff" * k + b"\x00")
        self.f.write(self._actl() + tail)
        self.palette = pal

    def add(self, planes, palette):
        """Append the frames planes [N,H,W] (or one plane [H,W]) of palette indices of the file's palette [K,3] uint8 -> the
        number of frames written.  ValueError: two-byte planes or K > 256, a geometry other than the writer's, colours other
        than those of the first add(), planes that are not on a GPU (or are, for the host encoder)."""
        if self.closed:
            raise ValueError("the writer is closed")
        pal = _palette(palette)
        p = self.enc.check(planes)
        if len(p.shape) != 3 or tuple(p.shape[1:]) != (self.height, self.width):
            raise ValueError(f"planes of shape {tuple(p.shape)} do not fit a {self.height} x {self.width} writer ([N,H,W])")
        if self.palette is not None and not (self.palette.shape == pal.shape and np.array_equal(self.palette, pal)):
            raise ValueError("an APNG has one palette: this add() brings other colours than the first one did")
        n = int(p.shape[0])
        if n == 0:
            return 0
        if self.palette is None:
            self._header(pal)
        i0 = self.n_frames
        num, den = self.delay
        prefixes = np.frombuffer(b"".join(fctl(0 if i == 0 else 2 * i - 1, self.width, self.height, num, den,
                                               1 if (self.transparent is not None and i > 0) else 0) for i in range(i0, i0 + n)),
                                 np.uint8).reshape(n, FCTL_BYTES)
        self.f.write(self.enc.encode(p, self.depth, self.transparent, prefixes, 1 if i0 == 0 else 0, 2 if i0 == 0 else 2 * i0))
        self.n_frames += n
        return n

    def close(self):
        """Write IEND and the frame count.  A writer that never got a frame writes nothing: there is no PNG without pixels."""
        if not self.closed:
            self.closed = True
            if self.palette is not None:
                self.f.write(chunk(b"IEND", b""))
                end = self.f.tell()
                self.f.seek(self.actl_at)
                self.f.write(self._actl())
                self.f.seek(end)


def write_apng(path, planes, palette, fps, loop=0, delta=True, seg_bytes=None, encoder="device", blocks="fixed"):
    """An in-memory clip planes [N,H,W] of one palette -> the file `path`.  Returns the number of frames written."""
    shape = tuple(planes.shape)
    if len(shape) != 3 or shape[0] < 1:
        raise ValueError("planes must be [N,H,W] with N >= 1")
    with open(path, "w+b") as f, ApngWriter(f, shape[2], shape[1], fps, loop, delta, seg_bytes, encoder, blocks) as a:
        return a.add(planes, palette)
