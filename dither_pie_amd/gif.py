"""Animated GIF output: GifWriter wraps the device's LZW image data (backend.gif_lzw) and inter-frame deltas
(backend.DeltaStream) in a GIF89a container.  The container is a few bytes per frame and is written here in plain Python; the
pixels never leave the GPU uncompressed.

    with GifWriter(open("clip.gif", "wb"), width, height, fps) as g:
        g.add(planes, palette)            # planes: uint8 CUDA [N,H,W] palette indices, palette: [K,3] uint8, K <= 256

Layout of the file: header, logical screen descriptor with the FIRST palette as the global colour table, the NETSCAPE2.0
loop block, then per frame a graphic control extension (disposal 1 -- leave in place --, the delay, the transparent index
when the frame is a delta), an image descriptor covering the whole screen, a local colour table only when the frame's palette
is not the global one, and the encoder's bytes verbatim.

Colour tables hold a power of two of entries, padded with zeros.  A palette of K <= 255 colours is given a table of K + 1
entries' size: index K is the transparent index of delta frames, and the table (hence min_code_size = max(2, bits)) must be
the same for every frame of that palette, delta or whole.  At K = 256 no index is left and every frame goes out whole.

Delta rules: the very first frame goes out whole; a frame whose palette differs from the frame before goes out whole (the
indices mean other colours); every other frame holds the transparent index where it equals the frame before.  The comparison
is always with the ORIGINAL previous plane.  A frame that repeats its predecessor is written all the same (all transparent:
a few dozen bytes), so frame numbers and timing stay those of the source.

Delay: GIF counts in centiseconds and viewers clamp delays below 2 to 10, so every frame lasts max(2, round(100 / fps)) cs.
That drifts against the source rate: 30 fps plays at 100 / 3 = 33.3 fps (3 cs), 24 fps at 25 fps (4 cs), 60 fps at 50 fps;
25 and 50 fps are exact.  The file is a silent loop; nothing downstream depends on the wall clock.

One device-to-host copy of payload bytes per add(): the frame sizes are read first (a synchronisation), then the block
payload[:, :max(sizes)] in one copy -- a strided gather on the device and one transfer, instead of a transfer per frame.
"""
from __future__ import annotations

import struct

import numpy as np

GIF_MAX_COLOURS = 256


def table_bits(n_entries):
    """Bits of the smallest GIF colour table that holds n_entries (a table has 2 ... 256 entries)."""
    bits = 1
    while (1 << bits) < n_entries:
        bits += 1
    return bits


def delay_cs(fps):
    """The frame delay in centiseconds: max(2, round(100 / fps))."""
    if not fps > 0:
        raise ValueError(f"fps must be positive, not {fps!r}")
    return max(2, int(round(100.0 / float(fps))))


def _palette(palette):
    pal = np.asarray(palette)
    if pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
        raise ValueError("palette must be [K,3] with K >= 1")
    if pal.shape[0] > GIF_MAX_COLOURS:
        raise ValueError(f"a GIF colour table holds {GIF_MAX_COLOURS} colours, not {pal.shape[0]}")
    if pal.min() < 0 or pal.max() > 255:
        raise ValueError("palette entries must be in 0 ... 255")
    return np.ascontiguousarray(pal.astype(np.uint8))


class _DeviceEncoder:
    """Deltas and image data on the GPU; what GifWriter uses unless told otherwise."""

    def __init__(self, chunk_px):
        self.chunk_px, self.stream = chunk_px, None

    def check(self, planes):
        import torch
        if not (isinstance(planes, torch.Tensor) and planes.is_cuda):
            raise ValueError("planes must be a CUDA tensor (encoder='host' takes host arrays)")
        if planes.dtype != torch.uint8:
            raise ValueError(f"planes must be one-byte indices (torch.uint8), not {planes.dtype}: a GIF table holds 256 colours")
        return planes if planes.dim() == 3 else planes.unsqueeze(0)

    def encode(self, planes, min_code_size, transparent, first_whole):
        from . import backend
        if self.stream is None or self.stream.device != planes.device:
            self.stream = backend.DeltaStream(planes.device)
        todo = planes
        if transparent is not None:
            if first_whole:
                self.stream.reset()
            todo, _ = self.stream.add(planes, transparent)
        elif planes.shape[0]:
            self.stream.carry(planes[-1])
        payload, sizes = backend.gif_lzw(todo, min_code_size, self.chunk_px)
        sizes = sizes.cpu().tolist()
        block = payload[:, :max(sizes)].cpu().numpy() if sizes else None
        return [block[f, :n].tobytes() for f, n in enumerate(sizes)]


class _HostEncoder:
    """The same on the host (dp_gif_lzw_host_u8 and a numpy comparison): no device involved."""

    def __init__(self, chunk_px):
        self.chunk_px, self.prev = chunk_px, None

    def check(self, planes):
        if hasattr(planes, "detach"):
            if planes.is_cuda:
                raise ValueError("encoder='host' takes host arrays, not CUDA tensors")
            planes = planes.detach().numpy()
        planes = np.asarray(planes)
        if planes.dtype != np.uint8:
            raise ValueError(f"planes must be one-byte indices (uint8), not {planes.dtype}: a GIF table holds 256 colours")
        return planes if planes.ndim == 3 else planes[None]

    def encode(self, planes, min_code_size, transparent, first_whole):
        from . import backend
        todo = planes
        if transparent is not None and planes.shape[0]:
            todo = planes.copy()
            before = np.concatenate([planes[:1] if (first_whole or self.prev is None) else self.prev[None], planes[:-1]])
            same = planes == before
            if first_whole or self.prev is None:
                same[0] = False
            todo[same] = transparent
        if planes.shape[0]:
            self.prev = planes[-1].copy()
        return backend.gif_lzw_host(todo, min_code_size, self.chunk_px)


class GifWriter:
    """GifWriter(fileobj, width, height, fps, loop=0): an animated GIF written frame batch by frame batch.  fileobj: a
    binary file object (it is not closed by close()).  loop: repetitions, 0 = forever.  chunk_px: passed to the encoder.
    encoder: "device" (the GPU encoder; a missing kernel is an error, nothing falls back) or "host" (the library's host
    statement of the same stream, for machines without a GPU)."""

    def __init__(self, fileobj, width, height, fps, loop=0, chunk_px=None, encoder="device"):
        self.width, self.height = int(width), int(height)
        if not (1 <= self.width <= 65535 and 1 <= self.height <= 65535):
            raise ValueError("a GIF screen is 1 ... 65535 pixels wide and high")
        if not 0 <= int(loop) <= 65535:
            raise ValueError("loop must be in 0 ... 65535")
        if encoder not in ("device", "host"):
            raise ValueError(f"encoder must be 'device' or 'host', not {encoder!r}")
        self.delay, self.loop = delay_cs(fps), int(loop)
        self.f = fileobj
        self.enc = (_DeviceEncoder if encoder == "device" else _HostEncoder)(chunk_px)
        self.global_palette = None
        self.last_palette = None
        self.n_frames = 0
        self.closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @staticmethod
    def _bits(pal):
        k = pal.shape[0]
        return table_bits(k + 1 if k <= 255 else k)

    @staticmethod
    def _table(pal, bits):
        return pal.tobytes() + bytes(3 * ((1 << bits) - pal.shape[0]))

    def _header(self, pal):
        bits = self._bits(pal)
        self.f.write(b"GIF89a" + struct.pack("<HHBBB", self.width, self.height, 0x80 | ((bits - 1) << 4) | (bits - 1), 0, 0))
        self.f.write(self._table(pal, bits))
        self.f.write(b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", self.loop) + b"\x00")
        self.global_palette = pal

    def add(self, planes, palette, delta=True):
        """Append the frames planes [N,H,W] (or one plane [H,W]) of palette indices, all of one palette [K,3] uint8.
        ValueError: two-byte planes or K > 256, a geometry other than the writer's, planes that are not on a GPU."""
        if self.closed:
            raise ValueError("the writer is closed")
        pal = _palette(palette)
        p = self.enc.check(planes)
        if len(p.shape) != 3 or tuple(p.shape[1:]) != (self.height, self.width):
            raise ValueError(f"planes of shape {tuple(p.shape)} do not fit a {self.height} x {self.width} writer ([N,H,W])")
        if p.shape[0] == 0:
            return 0
        if self.global_palette is None:
            self._header(pal)
        k = pal.shape[0]
        bits = self._bits(pal)
        same_palette = self.last_palette is not None and self.last_palette.shape == pal.shape and np.array_equal(self.last_palette, pal)
        transparent = k if (delta and k <= 255) else None
        blobs = self.enc.encode(p, max(2, bits), transparent, first_whole=not same_palette)
        local = not (self.global_palette.shape == pal.shape and np.array_equal(self.global_palette, pal))
        out = []
        for i, blob in enumerate(blobs):
            keyed = transparent is not None and (same_palette or i > 0)
            out.append(b"\x21\xf9\x04" + struct.pack("<BHB", (1 << 2) | (1 if keyed else 0), self.delay, transparent if keyed else 0) + b"\x00")
            out.append(b"\x2c" + struct.pack("<HHHHB", 0, 0, self.width, self.height, (0x80 | (bits - 1)) if local else 0))
            if local:
                out.append(self._table(pal, bits))
            out.append(blob)
        self.f.write(b"".join(out))
        self.last_palette = pal
        self.n_frames += len(blobs)
        return len(blobs)

    def close(self):
        """Write the trailer.  A writer that never got a frame writes nothing: there is no GIF without a screen's palette."""
        if not self.closed:
            self.closed = True
            if self.global_palette is not None:
                self.f.write(b"\x3b")


def write_gif(path, planes, palette, fps, loop=0, delta=True, chunk_px=None, encoder="device"):
    """An in-memory clip planes [N,H,W] of one palette -> the file `path`.  Returns the number of frames written."""
    shape = tuple(planes.shape)
    if len(shape) != 3 or shape[0] < 1:
        raise ValueError("planes must be [N,H,W] with N >= 1")
    with open(path, "wb") as f, GifWriter(f, shape[2], shape[1], fps, loop, chunk_px, encoder) as g:
        return g.add(planes, palette, delta)
