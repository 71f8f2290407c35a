"""Plain numpy / Python reference for the PNG-8 output (include/ditherpie_hip_png.h, dither_pie_amd/png.py), written from
the rules of the header and of RFC 1950 / 1951, not from the code under test:

  filtered(plane, depth)        the filtered bytes of a plane (filter 0 on every row, leftmost pixel in the high bits)
  container(...)                the file around a zlib stream
  content(kind, ...)            planes of noise, tiles, one colour, or the photo-like field of the size tests
  walk(stream)                  a small inflate: every block's type, bit span, output span, tokens and the farthest position
                                a match reaches back to; checks LEN/NLEN, code lengths and the Adler-32
  segment_sizes / smallest_type the bytes a segment takes as stored and as fixed Huffman, recomputed from decoded tokens
  named_cases(), random_cases() the inputs of tests/test_png_cpu.py and tests/test_gpu_png.py

The judges of correctness are zlib.decompress and Pillow; the walker adds what they do not tell (block types, match reach).
"""
import struct
import zlib

import numpy as np

SEG_DEFAULT = 8192
DEPTHS = (1, 2, 4, 8)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
STORED, FIXED, DYNAMIC = 0, 1, 2


def depth_of(k):
    return 1 if k <= 2 else 2 if k <= 4 else 4 if k <= 16 else 8


def row_bytes(w, depth):
    return 1 + (w * depth + 7) // 8


def filtered_size(h, w, depth):
    return h * row_bytes(w, depth)


def n_segments(F, seg):
    s = min(seg, F)
    return (F + s - 1) // s


def bound_bytes(h, w, depth, seg):
    F = filtered_size(h, w, depth)
    return 2 + F + 10 * n_segments(F, seg) + 4


def filtered(plane, depth):
    plane = np.asarray(plane, np.uint8)
    h, w = plane.shape
    ppb, rb = 8 // depth, (w * depth + 7) // 8
    pad = np.zeros((h, rb * ppb), np.uint8)
    pad[:, :w] = plane & ((1 << depth) - 1)
    v = np.zeros((h, rb), np.uint32)
    for k in range(ppb):
        v |= pad[:, k::ppb].astype(np.uint32) << (8 - depth * (k + 1))
    return np.concatenate([np.zeros((h, 1), np.uint8), v.astype(np.uint8)], axis=1).tobytes()


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def container(w, h, depth, palette, stream, idat_bytes=1 << 20):
    pal = np.asarray(palette, np.uint8)
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, 3, 0, 0, 0)), chunk(b"PLTE", pal.tobytes())]
    for a in range(0, max(len(stream), 1), idat_bytes):
        out.append(chunk(b"IDAT", stream[a:a + idat_bytes]))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def chunks_of(data):
    """[(type, payload)] of a PNG file; checks the signature and every CRC."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        out.append((kind, body))
        at += 12 + n
    assert at == len(data)
    return out


# ------------------------------------------------------------------------------------------------------------ content
B4 = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]])


def photo_plane(k, h=512, w=768):
    """The photo-like plane of the size tests: a smooth field and a little noise, Bayer 4x4 to k colours."""
    y, x = np.mgrid[0:h, 0:w]
    v = np.clip(0.5 + 0.4 * np.sin(x / 37.0) * np.cos(y / 53.0) + np.random.RandomState(1).normal(0, 0.02, (h, w)), 0, 1)
    return np.clip(np.floor(v * (k - 1) + (B4[y % 4, x % 4] + 0.5) / 16.0), 0, k - 1).astype(np.uint8)


def content(kind, rs, n, h, w, k):
    if kind == "noise":
        return rs.randint(0, k, (n, h, w)).astype(np.uint8)
    if kind == "flat":
        return np.stack([np.full((h, w), rs.randint(0, k), np.uint8) for _ in range(n)])
    if kind == "tile":
        out = []
        for _ in range(n):
            th, tw = rs.randint(1, 6), rs.randint(2, 12)
            t = rs.randint(0, k, (th, tw)).astype(np.uint8)
            out.append(np.tile(t, (h // th + 1, w // tw + 1))[:h, :w])
        return np.stack(out)
    if kind == "photo":
        y, x = np.mgrid[0:h, 0:w]
        out = []
        for _ in range(n):
            a, b = rs.uniform(5, 40, 2)
            v = np.clip(0.5 + 0.4 * np.sin(x / a) * np.cos(y / b) + rs.normal(0, 0.02, (h, w)), 0, 1)
            out.append(np.clip(np.floor(v * (k - 1) + (B4[y % 4, x % 4] + 0.5) / 16.0), 0, k - 1).astype(np.uint8))
        return np.stack(out)
    raise ValueError(kind)


def _plane_of_filtered(data, w):
    """A depth-8 plane of width w whose filtered bytes are filter byte 0 + the given bytes per row (len(data) % w == 0)."""
    return np.frombuffer(bytes(data), np.uint8).reshape(-1, w)[None].copy()


# Literal alphabets for the code-length code of a dynamic block (RFC 1951 3.2.7: 16 repeats a length 3 ... 6 times, 17 writes
# 3 ... 10 zeros, 18 writes 11 ... 138): runs of absent symbols ('a') of 3, 6, 7, 10, 11, 138 and 139 -- each side of every
# limit -- and runs of present symbols ('p') of the same lengths, every present byte exactly once (equal counts, hence equal
# code lengths, and no trigram twice, hence no match).  Symbol 0 is present in every segment: it is the filter byte.  One
# segment cannot hold them all (the runs alone are 314 symbols), so they are spread over four; the runs are listed from
# symbol 0 to 255.  The encoder writes stored and fixed blocks today; the cases are stream cases until it writes dynamic ones.
CODE_LENGTH_RUNS = {
    "code-length runs: zeros 3 6 7 10 11 138": [("p", 1), ("a", 3), ("p", 3), ("a", 6), ("p", 6), ("a", 7), ("p", 7), ("a", 10), ("p", 10),
                                                ("a", 11), ("p", 11), ("a", 138), ("p", 43)],
    "code-length runs: zeros 139": [("p", 1), ("a", 139), ("p", 116)],
    "code-length runs: repeats 138": [("p", 138), ("a", 3), ("p", 115)],
    "code-length runs: repeats 139": [("p", 139), ("a", 3), ("p", 114)],
}


def symbols_of_runs(runs):
    assert sum(n for _, n in runs) == 256 and runs[0][0] == "p"
    out, at = [], 0
    for kind, n in runs:
        if kind == "p":
            out += list(range(at, at + n))
        at += n
    return out


def runs_of_symbols(symbols):
    """The inverse: [("p" | "a", length)] over 0 ... 255 for a set of byte values."""
    have, runs = set(symbols), []
    for v in range(256):
        kind = "p" if v in have else "a"
        if runs and runs[-1][0] == kind:
            runs[-1] = (kind, runs[-1][1] + 1)
        else:
            runs.append((kind, 1))
    return runs


def named_cases():
    """[(name, planes [n,h,w] uint8, depth, seg_bytes)]."""
    rs = np.random.RandomState(7)
    cases = []
    for d in DEPTHS:                                                    # widths with w * d % 8 != 0, every depth
        for w in (1, 3, 5, 7, 9):
            for h in (1, 2, 5):
                cases.append((f"odd d{d} {h}x{w}", rs.randint(0, 1 << d, (1, h, w)).astype(np.uint8), d, 256))
    cases.append(("boundary in mid-row", content("tile", rs, 1, 40, 99, 16), 4, 300))          # rows of 51 bytes, segments of 300
    cases.append(("seg == F", content("tile", rs, 1, 16, 31, 256), 8, 512))                     # F = 16 * 32
    cases.append(("last segment of 1 byte", content("noise", rs, 1, 1, 256, 4), 8, 256))        # F = 257
    cases.append(("last segment of 2 bytes", content("noise", rs, 1, 2, 128, 4), 8, 256))       # F = 258
    cases.append(("seg 256", content("photo", rs, 1, 48, 70, 16), 4, 256))
    cases.append(("seg 32768", content("photo", rs, 1, 200, 400, 16), 8, 32768))                # F = 80200: 3 segments
    cases.append(("flat", np.zeros((1, 64, 127), np.uint8), 8, 8192))                           # 8192 zeros: runs > 258, distance 1
    cases.append(("flat rows", np.full((2, 64, 127), 5, np.uint8), 8, 1000))                    # a filter byte breaks every run
    cases.append(("flat to the segment end", np.zeros((1, 8, 63), np.uint8), 8, 512))           # all zero: a match ends at every end
    far = np.zeros((32, 63), np.uint8)                                  # rows of 64: a row of 1 ... 143, zeros, the row again
    far[0] = far[31] = rs.randint(1, 144, 63)
    cases.append(("distance close to the segment", far[None], 8, 2048))                        # F = 2048, distance 31 * 64 = 1984
    far = np.zeros((256, 127), np.uint8)                                # rows of 128: two rows, zeros, the two rows again
    far[0:2] = far[254:256] = rs.randint(1, 144, (2, 127))
    cases.append(("distance close to 32768", far[None], 8, 32768))                             # F = 32768, distance 254 * 128 = 32512
    t = rs.randint(1, 256, 4000).astype(np.uint8)
    cases.append(("period of half a 8 KiB segment", _plane_of_filtered(np.tile(t, 3)[:8160], 255), 8, 8192))
    cases.append(("noise 256", content("noise", rs, 1, 64, 127, 256), 8, 4096))                 # the stored fallback
    cases.append(("20-byte segment", np.array([[[1, 2, 3, 1, 2, 3, 1, 2, 3, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]]], np.uint8), 8, 256))
    cases.append(("all literals", (1 + rs.permutation(255))[None, None].astype(np.uint8), 8, 1024))   # no byte twice: no trigram twice
    one = rs.randint(0, 256, 300).astype(np.uint8)
    one[200:260] = one[10:70]                                           # one repeat: one distance code
    cases.append(("one distance", one[None, None], 8, 512))
    cases.append(("one distinct literal", np.zeros((1, 1, 700), np.uint8), 8, 1024))            # (the filter byte is a zero too)
    fib, vals = [1, 1], rs.permutation(256)[:26]
    while len(fib) < 26:
        fib.append(fib[-1] + fib[-2])
    bag = np.repeat(vals, np.maximum(1, np.array(fib, np.int64) * 32512 // sum(fib))).astype(np.uint8)[:32512]
    bag = np.concatenate([bag, np.full(32512 - len(bag), vals[-1], np.uint8)])
    cases.append(("fibonacci counts", _plane_of_filtered(rs.permutation(bag), 127), 8, 32768))  # 256 rows of 128: one segment
    for name, runs in CODE_LENGTH_RUNS.items():                         # literal alphabets for the code-length code, see there
        present = [v for v in symbols_of_runs(runs) if v != 0]
        cases.append((name, np.array(rs.permutation(present), np.uint8)[None, None], 8, 1024))
    cases.append(("adler of 255s", np.full((1, 128, 128), 255, np.uint8), 8, 32768))
    return cases


KINDS = ("noise", "tile", "flat", "photo")


def random_cases(count, seed=11):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(count):
        d = DEPTHS[rs.randint(4)]
        n, h, w = rs.randint(1, 4), rs.randint(1, 97), rs.randint(1, 97)
        seg = int(rs.choice([256, 257, 300, 512, 1000, 4096, 8192, 32768]))
        kind = KINDS[rs.randint(4)]
        k = rs.randint(2, (1 << d) + 1)
        out.append((f"random {i} {kind} n{n} {h}x{w} d{d} seg{seg}", content(kind, rs, n, h, w, k), d, seg))
    return out


# ------------------------------------------------------------------------------------------------------------ inflate
class _Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _canonical(lengths):
    """RFC 1951 3.2.2: {(length, code): symbol}."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for sym, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = sym
            nxt[n] += 1
    return table


def _symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (n, code) in table:
            return table[(n, code)]
    raise AssertionError("no such code")


_FIXED_LIT = _canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = _canonical([5] * 30)


def walk(stream):
    """-> (output bytes, blocks); a block: dict(type, final, bit0, bit1 (one past its last bit), out0, out1, tokens,
    reach (the smallest output position a match of the block copies from, or None), maxlen (the longest literal/length or
    distance code of a dynamic block), maxcl (its longest code-length code)).  A token is a byte value or (length, distance).
    Raises on anything RFC 1950 / 1951 forbid."""
    assert stream[0] == 0x78 and stream[1] == 0x01 and (stream[0] * 256 + stream[1]) % 31 == 0
    bits = _Bits(stream)
    bits.pos = 16
    out, blocks = bytearray(), []
    while True:
        blk = dict(bit0=bits.pos, out0=len(out), tokens=[], reach=None, maxlen=0, maxcl=0)
        blk["final"], blk["type"] = bits.take(1), bits.take(2)
        assert blk["type"] in (STORED, FIXED, DYNAMIC)
        if blk["type"] == STORED:
            bits.pos = (bits.pos + 7) & ~7
            n, inv = bits.take(16), bits.take(16)
            assert n ^ inv == 0xFFFF, "LEN / NLEN"
            at = bits.pos >> 3
            assert at + n <= len(stream) - 4
            out += stream[at:at + n]
            blk["tokens"] = list(stream[at:at + n])
            bits.pos += 8 * n
        else:
            lit, dist = _FIXED_LIT, _FIXED_DIST
            if blk["type"] == DYNAMIC:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = bits.take(3)
                blk["maxcl"] = max(cl)
                clt, lens = _canonical(cl), []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        assert lens
                        lens += [lens[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.take(3))
                    else:
                        lens += [0] * (11 + bits.take(7))
                assert len(lens) == hlit + hdist and lens[256] > 0
                blk["maxlen"] = max(lens)
                lit, dist = _canonical(lens[:hlit]), _canonical(lens[hlit:])
            while True:
                s = _symbol(bits, lit)
                if s == 256:
                    break
                if s < 256:
                    out.append(s)
                    blk["tokens"].append(s)
                    continue
                assert s <= 285
                length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                dc = _symbol(bits, dist)
                assert dc < 30
                d = DIST_BASE[dc] + bits.take(DIST_EXTRA[dc])
                src = len(out) - d
                assert src >= 0 and 3 <= length <= 258 and d <= 32768
                blk["reach"] = src if blk["reach"] is None else min(blk["reach"], src)
                for i in range(length):
                    out.append(out[src + i])
                blk["tokens"].append((length, d))
        blk["bit1"], blk["out1"] = bits.pos, len(out)
        blocks.append(blk)
        if blk["final"]:
            break
    at = (bits.pos + 7) >> 3
    assert at + 4 == len(stream), "bytes behind the trailer"
    assert struct.unpack(">I", stream[at:at + 4])[0] == zlib.adler32(bytes(out)) & 0xFFFFFFFF, "Adler-32"
    return bytes(out), blocks


def segments_of(blocks):
    """Groups a walk's blocks by segment: [(data block, realigning block or None)]; checks the framing of the header: a data
    block starts on a byte boundary, an empty stored block without BFINAL follows every segment but the last."""
    segs, i = [], 0
    while i < len(blocks):
        b = blocks[i]
        assert b["bit0"] % 8 == 0 and b["out1"] > b["out0"], "a data block starts on a byte boundary and is not empty"
        if b["final"]:
            assert i == len(blocks) - 1
            segs.append((b, None))
            break
        e = blocks[i + 1]
        assert e["type"] == STORED and e["out1"] == e["out0"] and not e["final"], "the realigning block"
        segs.append((b, e))
        i += 2
    assert segs and segs[-1][1] is None
    return segs


def _fixed_bits(tokens):
    bits = 3 + 7
    for t in tokens:
        if isinstance(t, tuple):
            length, d = t
            li = max(i for i in range(29) if LEN_BASE[i] <= length)
            di = max(i for i in range(30) if DIST_BASE[i] <= d)
            bits += (7 if 257 + li < 280 else 8) + LEN_EXTRA[li] + 5 + DIST_EXTRA[di]
        else:
            bits += 8 if t < 144 else 9
    return bits


def segment_sizes(tokens, n, last):
    """The bytes of a segment of n filtered bytes by block type, [stored, fixed], for the tokens decoded from it, the
    realigning block included: the rule of the header."""
    fb = _fixed_bits(tokens)
    return [5 + n + (0 if last else 5), (fb + 7) // 8 if last else (fb + 3 + 7) // 8 + 4]


def smallest_type(sizes):
    return sizes.index(min(sizes))                                      # ties: the earlier type


def hash3(b0, b1, b2):
    return (((b0 | (b1 << 8) | (b2 << 16)) * 0x9E3779B1) & 0xFFFFFFFF) >> 20


def greedy_tokens(s):
    """The tokens the header's matcher gives for one segment's bytes: one candidate per position (the last earlier position
    of the segment with the same trigram hash), length by comparison up to min(258, n - p), a length >= 3 always taken."""
    n, heads, cand = len(s), {}, [None] * len(s)
    for p in range(n - 2):
        k = hash3(s[p], s[p + 1], s[p + 2])
        cand[p] = heads.get(k)
        heads[k] = p
    tokens, p = [], 0
    while p < n:
        q, length = cand[p], 0
        if q is not None:
            top = min(258, n - p)
            while length < top and s[q + length] == s[p + length]:
                length += 1
        if length >= 3:
            tokens.append((length, p - q))
            p += length
        else:
            tokens.append(s[p])
            p += 1
    return tokens
