"""PNG-8 output: encode_png wraps the device's zlib stream of palette-index planes (backend.png_deflate) in a PNG container.
The container is a few dozen bytes per file and is written here in plain Python; the compressed bytes never exist
uncompressed on the host, and the planes never leave the GPU.

    files = encode_png(planes, palette)              # planes: CUDA uint8 [N,H,W] (or [H,W]); palette: [K,3], K <= 256
    write_png("still.png", plane, palette)
    write_png_sequence("frame_%05d.png", planes, palette, start=1)

What a file is: the signature, IHDR (colour type 3, bit depth backend.png_depth(K): 1, 2, 4 or 8, no interlace), PLTE with
exactly K entries, the stream in IDAT chunks of at most IDAT_BYTES, IEND.  Every row has filter 0.  No ancillary chunk: no
gamma, no text, and no tRNS unless it is asked for.  Decoding gives palette[plane], exactly.
transparent=T (keyword only, default None): palette entry T is fully transparent -- a tRNS chunk of T bytes of 255 and one 0
follows PLTE (the entries behind T are opaque by the format's default); the palette must have more than T entries.  Without the
keyword the files are what they were, byte for byte.

Chunk CRCs are zlib.crc32 on the host, over the compressed bytes: a fraction of the plane (tools/bench_scripts/png_encode.py
times it beside the kernels).  One size read-back and one block copy per call, as gif.GifWriter does.
encoder="host" runs the normative host statement (backend.png_deflate_host) on host arrays: the same bytes without a GPU.
blocks="dynamic" (default "fixed") lets the encoder write dynamic-Huffman blocks as well: the same pixels in fewer bytes.
assemble="device" (default "host") builds the files on the GPU as well (backend.png_file_assemble): the chunk CRCs are
computed there, the finished files are packed back to back and come over in one copy of exactly their size.  Each stream
is then ONE IDAT chunk (a chunk may hold 2^31 - 1 bytes), so a file whose stream is longer than IDAT_BYTES differs from the
host-assembled one in its chunking: it equals container(..., idat_bytes=2**31 - 1) of the same stream, byte for byte.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

PNG_MAX_COLOURS = 256
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
IDAT_BYTES = 1 << 20      # a stream longer than this is cut into several IDAT chunks (a decoder concatenates them)


def _palette(palette):
    pal = np.asarray(palette)
    if pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
        raise ValueError("palette must be [K,3] with K >= 1")
    if pal.shape[0] > PNG_MAX_COLOURS:
        raise ValueError(f"a PNG palette holds {PNG_MAX_COLOURS} colours, not {pal.shape[0]}")
    if pal.min() < 0 or pal.max() > 255:
        raise ValueError("palette entries must be in 0 ... 255")
    return np.ascontiguousarray(pal.astype(np.uint8))


def chunk(kind, data):
    """One PNG chunk: length, type, data, CRC-32 of type and data."""
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)) & 0xFFFFFFFF)


def _transparent(transparent, n_colours):
    """The tRNS chunk of a key index (b"" for None); ValueError unless the palette has the entry."""
    if transparent is None:
        return b""
    if isinstance(transparent, bool) or not isinstance(transparent, (int, np.integer)) or not 0 <= transparent < n_colours:
        raise ValueError(f"transparent must be None or the index of a palette entry (0 ... {n_colours - 1}), not {transparent!r}")
    return chunk(b"tRNS", b"\xff" * int(transparent) + b"\x00")


def container(width, height, depth, palette, stream, idat_bytes=IDAT_BYTES, *, transparent=None):
    """The file around one zlib stream: signature, IHDR, PLTE, (tRNS,) IDAT ..., IEND."""
    pal = _palette(palette)
    if not (1 <= int(width) < 2 ** 31 and 1 <= int(height) < 2 ** 31):
        raise ValueError("a PNG is 1 ... 2^31 - 1 pixels wide and high")
    if depth not in (1, 2, 4, 8) or pal.shape[0] > (1 << depth):
        raise ValueError(f"bit depth {depth!r} does not hold a palette of {pal.shape[0]}")
    parts = [PNG_SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", int(width), int(height), depth, 3, 0, 0, 0)), chunk(b"PLTE", pal.tobytes())]
    if transparent is not None:
        parts.append(_transparent(transparent, pal.shape[0]))
    for a in range(0, max(len(stream), 1), int(idat_bytes)):
        parts.append(chunk(b"IDAT", stream[a:a + int(idat_bytes)]))
    parts.append(chunk(b"IEND", b""))
    return b"".join(parts)


def _device_planes(planes):
    import torch
    if not (isinstance(planes, torch.Tensor) and planes.is_cuda):
        raise ValueError("planes must be a CUDA tensor (encoder='host' takes host arrays)")
    if planes.dtype != torch.uint8:
        raise ValueError(f"planes must be one-byte indices (torch.uint8), not {planes.dtype}: a PNG palette holds 256 colours")
    if planes.dim() not in (2, 3):
        raise ValueError("planes must be [N,H,W] or [H,W]")
    return planes if planes.dim() == 3 else planes.unsqueeze(0)


def _streams(planes, depth, seg_bytes, encoder, blocks):
    from . import backend
    if blocks not in backend.PNG_BLOCKS:
        raise ValueError(f"blocks must be one of {backend.PNG_BLOCKS}, not {blocks!r}")
    if encoder == "device":
        p = _device_planes(planes)
        if p.shape[0] == 0:
            return [], p.shape
        payload, sizes = backend.png_deflate(p, depth, seg_bytes, blocks)
        sizes = sizes.cpu().tolist()
        block = payload[:, :max(sizes)].cpu().numpy()
        return [block[f, :n].tobytes() for f, n in enumerate(sizes)], p.shape
    if encoder != "host":
        raise ValueError(f"encoder must be 'device' or 'host', not {encoder!r}")
    if hasattr(planes, "detach"):
        if planes.is_cuda:
            raise ValueError("encoder='host' takes host arrays, not CUDA tensors")
        planes = planes.detach().numpy()
    p = np.asarray(planes)
    if p.dtype != np.uint8:
        raise ValueError(f"planes must be one-byte indices (uint8), not {p.dtype}: a PNG palette holds 256 colours")
    if p.ndim not in (2, 3):
        raise ValueError("planes must be [N,H,W] or [H,W]")
    p = p if p.ndim == 3 else p[None]
    return backend.png_deflate_host(p, depth, seg_bytes, blocks), p.shape


ASSEMBLE = ("host", "device")


def _check_assemble(assemble, encoder):
    if assemble not in ASSEMBLE:
        raise ValueError(f"assemble must be one of {ASSEMBLE}, not {assemble!r}")
    if assemble == "device" and encoder != "device":
        raise ValueError("assemble='device' builds the files on the GPU: it needs encoder='device'")


def _files_on_device(planes, pal, depth, seg_bytes, blocks, transparent=None):
    """The files of encode_png, assembled on the GPU: prefix = signature, IHDR, PLTE (, tRNS); one IDAT chunk; suffix = IEND."""
    from . import backend
    if blocks not in backend.PNG_BLOCKS:
        raise ValueError(f"blocks must be one of {backend.PNG_BLOCKS}, not {blocks!r}")
    p = _device_planes(planes)
    head = container(p.shape[2], p.shape[1], depth, pal, b"", transparent=transparent)   # (checks the geometry as the host path does)
    pre = head[:len(head) - 24]                                        # without the empty IDAT (12 bytes) and IEND (12)
    files = []
    for a in range(0, p.shape[0], backend.PNG_MAX_FRAMES):
        payload, sizes = backend.png_deflate(p[a:a + backend.PNG_MAX_FRAMES], depth, seg_bytes, blocks)
        out, offsets = backend.png_file_assemble(payload, sizes, pre=pre, post=chunk(b"IEND", b""))
        offsets = offsets.cpu().tolist()
        block = out[:offsets[-1]].cpu().numpy()                       # exactly the files' bytes, one copy
        files += [block[offsets[f]:offsets[f + 1]].tobytes() for f in range(len(offsets) - 1)]
    return files


def encode_png(planes, palette, seg_bytes=None, encoder="device", blocks="fixed", assemble="host", *, transparent=None):
    """Index planes [N,H,W] (or [H,W]) and their palette [K,3] -> [the bytes of a PNG file per plane].  ValueError: more than
    256 colours, planes that are not one-byte indices, planes that are not on the GPU for the device encoder (or are, for
    the host encoder), a `blocks` outside backend.PNG_BLOCKS.  An index >= K is the caller's error (a decoder will show
    whatever entry its low bits name, or refuse the file).  blocks="dynamic" adds dynamic-Huffman blocks: smaller files that
    decode to the same pixels (include/ditherpie_hip_png_dyn.h).  assemble="device": chunk CRCs and the files themselves on
    the GPU (include/ditherpie_hip_png_file.h), one IDAT chunk per file; refused with encoder="host".  transparent=T: a tRNS
    chunk that makes palette entry T transparent (ValueError unless the palette has more than T entries)."""
    from . import backend
    _check_assemble(assemble, encoder)
    pal = _palette(palette)
    _transparent(transparent, pal.shape[0])
    depth = backend.png_depth(pal.shape[0])
    if assemble == "device":
        return _files_on_device(planes, pal, depth, seg_bytes, blocks, transparent)
    streams, shape = _streams(planes, depth, seg_bytes, encoder, blocks)
    return [container(shape[2], shape[1], depth, pal, s, transparent=transparent) for s in streams]


def write_png(path, plane, palette, seg_bytes=None, encoder="device", blocks="fixed", assemble="host", *, transparent=None):
    """One plane [H,W] (or [1,H,W]) as a PNG file -> the number of bytes written."""
    files = encode_png(plane, palette, seg_bytes, encoder, blocks, assemble, transparent=transparent)
    if len(files) != 1:
        raise ValueError(f"write_png takes one plane, not {len(files)}: write_png_sequence writes several")
    with open(path, "wb") as f:
        f.write(files[0])
    return len(files[0])


def write_png_sequence(pattern, planes, palette, start=1, seg_bytes=None, encoder="device", blocks="fixed", assemble="host", *, transparent=None):
    """Planes [N,H,W] as the files pattern % start, pattern % (start + 1), ... (the 'frame_%05d.png' of a frame
    directory) -> the list of paths written."""
    paths = []
    for k, data in enumerate(encode_png(planes, palette, seg_bytes, encoder, blocks, assemble, transparent=transparent)):
        path = str(pattern) % (int(start) + k)
        with open(path, "wb") as f:
            f.write(data)
        paths.append(path)
    return paths
