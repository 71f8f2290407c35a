"""A plain-Python statement of the GIF output (include/ditherpie_hip_gif.h, dither_pie_amd/gif.py): the chunked LZW stream,
its sub-block framing, the inter-frame delta and the GIF89a container.  Written from the rules of the header, slow on purpose,
and judged by Pillow's decoder (tests/test_gif_cpu.py); the host statement of the library (host_logic.h: gif_lzw_encode) and
the device encoder must produce these bytes."""
import struct

import numpy as np


# ---------------------------------------------------------------------------------------------------- the LZW stream
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc |= code << self.n                                      # LSB first
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def done(self):
        if self.n:
            self.out.append(self.acc & 0xFF)
        return bytes(self.out)


def lzw_codes(pixels, min_code_size, chunk_px):
    """-> [(code, width)...] of one frame: every chunk opens with a Clear at the width in force, EOI closes the frame."""
    clear, eoi = 1 << min_code_size, (1 << min_code_size) + 1
    mask = clear - 1                                                    # an index past the table is reduced to its low bits
    px = [int(v) & mask for v in pixels]
    codes = []
    width = min_code_size + 1
    for at in range(0, len(px), chunk_px):
        chunk = px[at:at + chunk_px]
        codes.append((clear, width))
        width, nxt, table = min_code_size + 1, clear + 2, {}
        cur = chunk[0]
        for c in chunk[1:]:
            hit = table.get((cur, c))
            if hit is not None:
                cur = hit
                continue
            codes.append((cur, width))
            if nxt < 4096:
                table[(cur, c)] = nxt
                if nxt == 1 << width and width < 12:
                    width += 1
                nxt += 1
            else:                                                       # no code is free: Clear at 12 bits, start over
                codes.append((clear, 12))
                width, nxt, table = min_code_size + 1, clear + 2, {}
            cur = c
        codes.append((cur, width))
        if nxt < 4096 and nxt == 1 << width and width < 12:             # the decoder adds its lagging entry on this code
            width += 1
    codes.append((eoi, width))
    return codes


def lzw_data(pixels, min_code_size, chunk_px):
    """The packed code stream of one frame, before sub-blocks."""
    b = _Bits()
    for code, width in lzw_codes(pixels, min_code_size, chunk_px):
        b.put(code, width)
    return b.done()


def image_data(pixels, min_code_size, chunk_px):
    """What follows the image descriptor / local table: the min_code_size byte, sub-blocks of <= 255 bytes, a zero."""
    data = lzw_data(pixels, min_code_size, chunk_px)
    out = bytearray([min_code_size])
    for a in range(0, len(data), 255):
        blk = data[a:a + 255]
        out.append(len(blk))
        out += blk
    out.append(0)
    return bytes(out)


def bound_bytes(h, w, chunk_px):
    """The header's worst case: a 12-bit code per pixel, a Clear per 3839 codes, a Clear per chunk, EOI; sub-block framing."""
    n_px = h * w
    chunk = min(chunk_px, n_px)
    codes = n_px + n_px // 3839 + (n_px + chunk - 1) // chunk + 1
    d = (12 * codes + 7) // 8
    return 1 + d + (d + 254) // 255 + 1


# ---------------------------------------------------------------------------------------------------- delta
def index_delta(planes, transparent, prev=None):
    """-> (out planes, changed-pixel count per frame); frame 0 against prev when given, else whole."""
    planes = np.asarray(planes, np.uint8)
    out = planes.copy()
    counts = np.zeros(len(planes), np.int64)
    for f in range(len(planes)):
        before = planes[f - 1] if f else prev
        if before is None:
            counts[f] = planes[f].size
            continue
        same = planes[f] == before
        out[f][same] = transparent
        counts[f] = int((~same).sum())
    return out, counts


# ---------------------------------------------------------------------------------------------------- the container
def table_bits(n_colours):
    bits = 1
    while (1 << bits) < n_colours:
        bits += 1
    return bits


def delay_cs(fps):
    return max(2, int(round(100.0 / fps)))


def _table(palette, bits):
    raw = bytes(np.asarray(palette, np.uint8).reshape(-1, 3).tobytes())
    return raw + bytes(3 * (1 << bits) - len(raw))


def container(frames, width, height, fps, loop=0, chunk_px=None):
    """frames: [(plane [h, w] uint8, palette [K, 3] uint8, transparent index or None)...] -> the bytes of a GIF89a file.  The
    first palette is the global table (padded for a transparent slot when the first frame of that palette needs none but a
    later one does: the table's size is that of K + 1 entries whenever K <= 255)."""
    chunk_px = chunk_px or width * height
    first = np.asarray(frames[0][1], np.uint8).reshape(-1, 3)

    def bits_of(pal):
        k = len(pal)
        return table_bits(k + 1 if k <= 255 else k)

    gbits = bits_of(first)
    out = bytearray(b"GIF89a")
    out += struct.pack("<HHBBB", width, height, 0x80 | ((gbits - 1) << 4) | (gbits - 1), 0, 0)
    out += _table(first, gbits)
    out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    for plane, palette, transparent in frames:
        pal = np.asarray(palette, np.uint8).reshape(-1, 3)
        plane = np.asarray(plane, np.uint8)
        assert plane.shape == (height, width)
        flags = (1 << 2) | (1 if transparent is not None else 0)       # disposal 1: leave in place
        out += b"\x21\xf9\x04" + struct.pack("<BHB", flags, delay_cs(fps), transparent if transparent is not None else 0) + b"\x00"
        local = not (pal.shape == first.shape and np.array_equal(pal, first))
        bits = bits_of(pal)
        out += b"\x2c" + struct.pack("<HHHHB", 0, 0, width, height, (0x80 | (bits - 1)) if local else 0)
        if local:
            out += _table(pal, bits)
        out += image_data(plane.reshape(-1), max(2, bits), chunk_px)
    out += b"\x3b"
    return bytes(out)


def clip_frames(planes, palettes, delta=True):
    """The writer's delta rules on a clip: planes [N, h, w], palettes one per frame -> the frame list container() takes."""
    frames, prev, prev_pal = [], None, None
    for plane, pal in zip(planes, palettes):
        pal = np.asarray(pal, np.uint8).reshape(-1, 3)
        k = len(pal)
        whole = (not delta) or prev is None or k > 255 or not (prev_pal.shape == pal.shape and np.array_equal(prev_pal, pal))
        if whole:
            frames.append((plane, pal, None))
        else:
            frames.append((index_delta(plane[None], k, prev)[0][0], pal, k))
        prev, prev_pal = plane, pal
    return frames


# ---------------------------------------------------------------------------------------------------- contents for the tests
def content(kind, rs, n, h, w, k):
    if kind == "noise":
        return rs.randint(0, k, (n, h, w)).astype(np.uint8)
    if kind == "flat":
        return np.full((n, h, w), rs.randint(0, k), np.uint8)
    tile = rs.randint(0, k, (n, 4, 4)).astype(np.uint8)               # dither-like: a 4x4 tile repeated, a few pixels disturbed
    out = np.tile(tile, (1, (h + 3) // 4, (w + 3) // 4))[:, :h, :w].copy()
    hits = rs.randint(0, max(1, h * w), max(1, h * w // 16))
    out.reshape(n, -1)[:, hits] = rs.randint(0, k, (n, len(hits))).astype(np.uint8)
    return out


def random_case(seed):
    """The seeded random cases of the CPU and GPU tiers: -> (planes [n, h, w], min_code_size, chunk_px)."""
    rs = np.random.RandomState(7000 + seed)
    k = int(rs.randint(2, 257))
    h, w = int(rs.randint(1, 65)), int(rs.randint(1, 65))
    chunk = int(rs.randint(1, 5001)) if rs.randint(0, 3) else int(rs.randint(1, 40))
    kind = ("noise", "tile", "flat")[seed % 3]
    n = 1 + seed % 3
    return content(kind, rs, n, h, w, k), max(2, table_bits(k)), chunk


def named_cases():
    """The hand-picked cases of both tiers: [(name, planes [n, h, w], min_code_size, chunk_px)], planes as the encoder gets
    them (deltas already applied where the case is about them)."""
    rs = np.random.RandomState(11)
    out = []

    def add(name, k, h, w, chunk, kind, n=2, planes=None, slots=None):
        p = content(kind, rs, n, h, w, k) if planes is None else planes
        out.append((name, p, max(2, table_bits(slots or k)), chunk or h * w))

    add("width_crosses_at_chunk_end", 2, 5, 7, 3, "noise")
    add("chunk_of_one", 16, 37, 53, 1, "tile")
    add("chunk_64", 16, 37, 53, 64, "tile")
    add("chunk_1000_k256", 256, 64, 70, 1000, "noise")
    clip = content("tile", rs, 3, 33, 129, 255)
    clip[2] = clip[1]                                                   # the third frame repeats the second: all transparent
    add("delta_transparent_255", 255, 33, 129, 4096, None, planes=index_delta(clip, 255)[0], slots=256)
    add("whole_frame_k3", 3, 200, 200, None, "noise", n=1)
    add("dictionary_fills", 256, 96, 96, None, "noise", n=1)            # > 3838 codes in one chunk: a 12-bit Clear inside it
    add("one_pixel", 4, 1, 1, 5, "noise", n=3)
    add("one_left_over", 16, 5, 5, 8, "noise")                          # 25 = 3 * 8 + 1
    add("flat", 16, 40, 40, 512, "flat")
    add("flat_whole", 7, 64, 64, None, "flat", n=1)
    return out


def subblock_edge_cases(wanted=(254, 255, 256, 509, 510, 511)):
    """One-row planes at 256 colours whose code stream has exactly the wanted numbers of data bytes: {length: (plane
    [1, 1, w], chunk_px)}.  Prefixes of a noise row, where a pixel costs nine or ten bits, so the length grows by one or two
    bytes a pixel.  As ONE chunk a row of noise has 2314 + 10 (codes - 255) bits, which is never in (4064, 4072]: 509 bytes
    need the extra Clear of a second chunk, so every width is tried whole and in chunks of 100 and of 37."""
    found = {}
    for seed in range(8):
        row = np.random.RandomState(500 + seed).randint(0, 256, 460).astype(np.uint8)
        for w in list(range(200, 232)) + list(range(405, 440)):
            for chunk in (w, 100, 37):
                d = len(lzw_data(row[:w], 8, chunk))
                if d in wanted and d not in found:
                    found[d] = (row[:w].reshape(1, 1, w).copy(), chunk)
        if len(found) == len(wanted):
            break
    return found
