"""Plain Python restatement of the dynamic-Huffman rule of include/ditherpie_hip_png_dyn.h, written from the header's text and
RFC 1951, not from the code under test:

  code_lengths(counts, L)       rule (a)-(f): padding, sort, two-queue merge, the limit through num[], lengths in sorted order
  canonical_codes(lengths)      RFC 1951 3.2.2
  run_length(lengths)           the greedy code-length coding of the concatenated length lists: [(symbol, extra bits, value)]
  dynamic_plan(tokens)          histograms -> the three codes, HLIT / HDIST / HCLEN, the bits of the block
  deflate(plane, depth, seg, blocks)   the whole stream, matcher and framing of tests/png_ref.py, the third candidate added
  walk(stream)                  png_ref.walk with each dynamic block's length lists and code-length symbol sequence
  new_cases()                   the inputs the dynamic blocks were added for

The judges of correctness are zlib.decompress and Pillow; this file says which bytes the project writes."""
import heapq
import struct
import zlib

import numpy as np

import png_ref as pr

LIMITS = (15, 15, 7)                                                    # literal/length, distance, code-length alphabet
N_LIT, N_DIST, N_CL = 286, 30, 19
MAX_COUNT = 1 << 20


# ------------------------------------------------------------------------------------------------------------ the codes
def code_lengths(counts, L, info=None):
    """-> [length per symbol].  info (a dict) receives 'over' (leaves deeper than L) and 'rounds' (fix-up rounds)."""
    c = list(counts)
    while sum(1 for x in c if x) < 2:                                   # (a)
        c[c.index(0)] = 1
    used = sorted((c[s], s) for s in range(len(c)) if c[s])             # (b)
    n = len(used)
    weight, parent_of_leaf, parent_of_node = [], [None] * n, []         # (c)
    li = ni = 0
    for k in range(n - 1):
        w = 0
        for _ in range(2):
            if li < n and (ni >= len(weight) or used[li][0] <= weight[ni]):
                parent_of_leaf[li] = k
                w += used[li][0]
                li += 1
            else:
                parent_of_node[ni] = k
                w += weight[ni]
                ni += 1
        weight.append(w)
        parent_of_node.append(None)
    depth_of_node = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth_of_node[k] = depth_of_node[parent_of_node[k]] + 1
    num = [0] * (L + 1)                                                 # (d)
    over = 0
    for i in range(n):
        d = depth_of_node[parent_of_leaf[i]] + 1
        over += d > L
        num[min(d, L)] += 1
    total = sum(num[i] << (L - i) for i in range(1, L + 1))
    rounds = 0
    while total > 1 << L:
        num[L] -= 1
        i = max(i for i in range(1, L) if num[i] > 0)
        num[i] -= 1
        num[i + 1] += 2
        total -= 1
        rounds += 1
    assert rounds <= n
    lengths, at = [0] * len(c), 0                                       # (e)
    for d in range(L, 0, -1):
        for _ in range(num[d]):
            lengths[used[at][1]] = d
            at += 1
    assert at == n
    if info is not None:
        info.update(over=over, rounds=rounds)
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> [code per symbol] (meaningful where the length is not 0)."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            out[s] = nxt[n]
            nxt[n] += 1
    return out


def kraft(lengths):
    return sum(2.0 ** -n for n in lengths if n)


def heap_huffman_cost(counts):
    """Σ count * length of an optimal prefix code, by the textbook heap: the sum of all merged weights."""
    h = [c for c in counts if c]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


def run_length(lengths):
    """The concatenated length lists -> [(symbol 0 ... 18, extra bits, their value)], greedy."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, r = lengths[i], 1
        while i + r < n and lengths[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            k = min(r, 138)
            out.append((18, 7, k - 11))
            i += k
        elif v == 0 and r >= 3:
            out.append((17, 3, r - 3))
            i += r
        elif v == 0:
            out.append((0, 0, 0))
            i += 1
        else:
            out.append((v, 0, 0))
            i += 1
            rest = r - 1
            while rest >= 3:
                k = min(rest, 6)
                out.append((16, 2, k - 3))
                i += k
                rest -= k
    return out


def _token_symbols(t):
    """a token -> (literal/length symbol, extra bits, value, distance symbol or None, extra bits, value)"""
    if not isinstance(t, tuple):
        return t, 0, 0, None, 0, 0
    length, d = t
    li = max(i for i in range(29) if pr.LEN_BASE[i] <= length)
    di = max(i for i in range(30) if pr.DIST_BASE[i] <= d)
    return 257 + li, pr.LEN_EXTRA[li], length - pr.LEN_BASE[li], di, pr.DIST_EXTRA[di], d - pr.DIST_BASE[di]


def dynamic_plan(tokens):
    """-> dict(lit, dist, cl (length lists), hlit, hdist, hclen, seq, bits): everything the block's header says, and the bits of
    the block from its three header bits through end-of-block, from the histograms, the extra-bit total and the lengths."""
    lit_n, dist_n, extra = [0] * N_LIT, [0] * N_DIST, 0
    for t in tokens:
        ls, le, _, ds, de, _ = _token_symbols(t)
        lit_n[ls] += 1
        extra += le
        if ds is not None:
            dist_n[ds] += 1
            extra += de
    lit_n[256] = 1
    lit, dist = code_lengths(lit_n, LIMITS[0]), code_lengths(dist_n, LIMITS[1])
    hlit = max(257, max(s for s in range(N_LIT) if lit[s]) + 1)
    hdist = max(s for s in range(N_DIST) if dist[s]) + 1
    seq = run_length(lit[:hlit] + dist[:hdist])
    cl_n = [0] * N_CL
    for s, _, _ in seq:
        cl_n[s] += 1
    cl = code_lengths(cl_n, LIMITS[2])
    hclen = max(4, 1 + max(i for i in range(N_CL) if cl[pr.CL_ORDER[i]]))
    bits = 3 + 5 + 5 + 4 + 3 * hclen + sum(cl[s] + e for s, e, _ in seq)
    bits += sum(lit_n[s] * lit[s] for s in range(N_LIT)) + sum(dist_n[s] * dist[s] for s in range(N_DIST)) + extra
    return dict(lit=lit, dist=dist, cl=cl, hlit=hlit, hdist=hdist, hclen=hclen, seq=seq, bits=bits)


# ------------------------------------------------------------------------------------------------------------ the stream
class _Out:
    def __init__(self):
        self.bytes, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, v, nb):                                               # LSB first
        self.acc |= v << self.n
        self.n += nb
        self.total += nb
        while self.n >= 8:
            self.bytes.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nb):                                           # a Huffman code: most significant bit first
        self.put(int(format(code, f"0{nb}b")[::-1], 2) if nb else 0, nb)

    def flush(self):
        if self.n:
            self.bytes.append(self.acc & 0xFF)
        self.acc = self.n = 0


def _fixed_lengths():
    return [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30


def _write_tokens(o, tokens, lit, dist):
    lc, dc = canonical_codes(lit), canonical_codes(dist)
    for t in tokens:
        ls, le, lv, ds, de, dv = _token_symbols(t)
        o.code(lc[ls], lit[ls])
        o.put(lv, le)
        if ds is not None:
            o.code(dc[ds], dist[ds])
            o.put(dv, de)
    o.code(lc[256], lit[256])


def segment_sizes(tokens, n, last):
    """[stored, fixed, dynamic] bytes of a segment, the realigning block included."""
    def huff(bits):
        return (bits + 7) // 8 if last else (bits + 3 + 7) // 8 + 4
    return pr.segment_sizes(tokens, n, last) + [huff(dynamic_plan(tokens)["bits"])]


def segment_bytes(s, last, blocks="dynamic"):
    """One segment's filtered bytes -> (its bytes in the stream, the type written)."""
    n, tokens = len(s), pr.greedy_tokens(s)
    sizes = segment_sizes(tokens, n, last) if blocks == "dynamic" else pr.segment_sizes(tokens, n, last)
    kind = sizes.index(min(sizes))
    if kind == pr.STORED:
        out = bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(s)
        return out + (b"" if last else b"\x00\x00\x00\xff\xff"), kind
    o = _Out()
    o.put((1 if last else 0) | (kind << 1), 3)
    if kind == pr.FIXED:
        _write_tokens(o, tokens, *_fixed_lengths())
    else:
        p = dynamic_plan(tokens)
        o.put(p["hlit"] - 257, 5)
        o.put(p["hdist"] - 1, 5)
        o.put(p["hclen"] - 4, 4)
        for i in range(p["hclen"]):
            o.put(p["cl"][pr.CL_ORDER[i]], 3)
        cc = canonical_codes(p["cl"])
        for sym, e, v in p["seq"]:
            o.code(cc[sym], p["cl"][sym])
            o.put(v, e)
        _write_tokens(o, tokens, p["lit"], p["dist"])
        assert o.total == p["bits"]
    if not last:
        o.put(0, 3)
    o.flush()
    out = bytes(o.bytes) + (b"" if last else b"\x00\x00\xff\xff")
    assert len(out) == sizes[kind]
    return out, kind


def deflate(plane, depth, seg, blocks="dynamic"):
    """-> (the zlib stream of one plane, [type per segment])"""
    raw = pr.filtered(plane, depth)
    F = len(raw)
    s = min(seg, F)
    out, kinds = bytearray(b"\x78\x01"), []
    for at in range(0, F, s):
        b, kind = segment_bytes(raw[at:at + s], at + s >= F, blocks)
        out += b
        kinds.append(kind)
    return bytes(out + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)), kinds


# ------------------------------------------------------------------------------------------------------------ the walker
def walk(stream):
    """png_ref.walk, and for a dynamic block also lit / dist (its length lists as sent: HLIT and HDIST entries), cl (the 19
    code-length code lengths), hclen and seq ([(code-length symbol, number of lengths it stands for)])."""
    assert stream[0] == 0x78 and stream[1] == 0x01
    bits = pr._Bits(stream)
    bits.pos = 16
    out, blocks = bytearray(), []
    while True:
        blk = dict(bit0=bits.pos, out0=len(out), tokens=[], reach=None, maxlen=0, maxcl=0)
        blk["final"], blk["type"] = bits.take(1), bits.take(2)
        assert blk["type"] in (pr.STORED, pr.FIXED, pr.DYNAMIC)
        if blk["type"] == pr.STORED:
            bits.pos = (bits.pos + 7) & ~7
            n, inv = bits.take(16), bits.take(16)
            assert n ^ inv == 0xFFFF, "LEN / NLEN"
            at = bits.pos >> 3
            assert at + n <= len(stream) - 4
            out += stream[at:at + n]
            blk["tokens"] = list(stream[at:at + n])
            bits.pos += 8 * n
        else:
            lit, dist = pr._FIXED_LIT, pr._FIXED_DIST
            if blk["type"] == pr.DYNAMIC:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                assert hlit <= 286 and hdist <= 30
                cl = [0] * 19
                for i in range(hclen):
                    cl[pr.CL_ORDER[i]] = bits.take(3)
                clt, lens, seq = pr._canonical(cl), [], []
                assert abs(kraft(cl) - 1.0) < 1e-12, "the code-length code is complete"
                while len(lens) < hlit + hdist:
                    s = pr._symbol(bits, clt)
                    if s < 16:
                        k, v = 1, s
                    elif s == 16:
                        assert lens
                        k, v = 3 + bits.take(2), lens[-1]
                    elif s == 17:
                        k, v = 3 + bits.take(3), 0
                    else:
                        k, v = 11 + bits.take(7), 0
                    lens += [v] * k
                    seq.append((s, k))
                assert len(lens) == hlit + hdist and lens[256] > 0
                blk.update(maxcl=max(cl), maxlen=max(lens), lit=lens[:hlit], dist=lens[hlit:], cl=cl, hclen=hclen, seq=seq)
                assert abs(kraft(blk["lit"]) - 1.0) < 1e-12 and abs(kraft(blk["dist"]) - 1.0) < 1e-12, "complete codes"
                lit, dist = pr._canonical(blk["lit"]), pr._canonical(blk["dist"])
            while True:
                s = pr._symbol(bits, lit)
                if s == 256:
                    break
                if s < 256:
                    out.append(s)
                    blk["tokens"].append(s)
                    continue
                assert s <= 285
                length = pr.LEN_BASE[s - 257] + bits.take(pr.LEN_EXTRA[s - 257])
                dc = pr._symbol(bits, dist)
                assert dc < 30
                d = pr.DIST_BASE[dc] + bits.take(pr.DIST_EXTRA[dc])
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


# ------------------------------------------------------------------------------------------------------------ the inputs
def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def builder_inputs():
    """[(name, counts, L)] of the code construction on its own (dp_png_code_lengths_*)."""
    one, two = [0] * 40, [0] * 286
    one[17] = 5
    two[3], two[285] = 9, 2
    return [("fibonacci 21 at 15", fibonacci(21), 15), ("fibonacci 19 at 7", fibonacci(19), 7), ("286 equal", [7] * 286, 15),
            ("1 ... 286", list(range(1, 287)), 15), ("all zero", [0] * 30, 15), ("one used", one, 15), ("two used", two, 15),
            ("19 equal at 7", [3] * 19, 7), ("top count", [MAX_COUNT] * 5 + [1, 0, 2], 15)]


def random_histograms(L, count=64, seed=21):
    rs = np.random.RandomState(seed + L)
    out = []
    for i in range(count):
        m = int(rs.randint(2, min(286, 1 << L) + 1))
        kind = i % 4
        if kind == 0:
            c = rs.randint(0, 50, m)
        elif kind == 1:
            c = (rs.exponential(1.0, m) ** 4 * 40).astype(np.int64)
        elif kind == 2:
            c = np.array(sorted(fibonacci(min(m, 29))) + [0] * (m - min(m, 29)))[rs.permutation(m)]
        else:
            c = rs.randint(0, 2, m) * rs.randint(1, MAX_COUNT + 1, m)
        out.append((f"random L{L} {i}", [int(min(x, MAX_COUNT)) for x in c], L))
    return out


EQUAL_GROUPS = [(g, g) for g in range(1, 14)]                           # (present values, absent values behind them), then 36 present


def equal_group_values():
    vals, at = [], 1
    for g, gap in EQUAL_GROUPS:
        vals += list(range(at, at + g))
        at += g + gap
    vals += list(range(at, at + 36))
    assert len(vals) == 127 and vals[-1] < 256
    return vals


def _no_match(row):
    return all(not isinstance(t, tuple) for t in pr.greedy_tokens(bytes([0]) + bytes(row)))


def _permutations(vals, times, seed):
    """`times` random permutations of vals on one row, the first seed from `seed` on for which the matcher finds no match."""
    for s in range(seed, seed + 200):
        rs = np.random.RandomState(s)
        row = np.concatenate([rs.permutation(vals) for _ in range(times)]).astype(np.uint8)
        if _no_match(row):
            return row
    raise AssertionError("no seed without a match")


def new_cases():
    """[(name, planes [1,h,w] uint8, depth 8, seg_bytes)], each one segment."""
    cases = [("equal-length groups", _permutations(equal_group_values(), 4, 100)[None, None], 8, 1024)]
    for name in ("code-length runs: zeros 3 6 7 10 11 138", "code-length runs: zeros 139"):
        present = [v for v in pr.symbols_of_runs(pr.CODE_LENGTH_RUNS[name]) if v != 0]
        for times in (4, 16):
            cases.append((f"{name} x{times}", _permutations(present, times, 200)[None, None], 8, 4096))
    cases.append(("code-length code at 7 bits", _cl7_case()[None, None], 8, 4096))
    cases.append(("no match, dynamic", _skewed_no_match(32), 8, 2048))
    cases.append(("one distance code, dynamic", _skewed_one_distance(33), 8, 2048))
    return cases


def _skewed_row(rs, n=200, k=24):
    """n draws from k byte values: short codes in a dynamic block, and few enough trigrams twice that a seed without one exists."""
    return (1 + rs.permutation(255)[:k])[rs.randint(0, k, n)].astype(np.uint8)


def _skewed_no_match(seed):
    for s in range(seed, seed + 400):
        row = _skewed_row(np.random.RandomState(s))
        if _no_match(row):
            return row[None, None]
    raise AssertionError("no seed without a match")


def _skewed_one_distance(seed):
    for s in range(seed, seed + 400):
        row = _skewed_row(np.random.RandomState(s))
        row = np.concatenate([row, row[10:16]])                         # one repeat of six bytes: one match
        toks = pr.greedy_tokens(bytes([0]) + bytes(row))
        if sum(isinstance(t, tuple) for t in toks) == 1:
            return row[None, None]
    raise AssertionError("no seed with exactly one match")


def _cl7_case():
    """A random row whose code-length code reaches the limit of 7 bits: literal counts spread over many magnitudes give many
    distinct lengths with Fibonacci-like frequencies."""
    for s in range(300, 2000):
        rs = np.random.RandomState(s)
        vals = rs.permutation(255)[:40] + 1
        reps = np.maximum(1, (2.0 ** rs.uniform(0, 9, 40)).astype(np.int64))
        row = rs.permutation(np.repeat(vals, reps)).astype(np.uint8)[:4000]
        toks = pr.greedy_tokens(bytes([0]) + bytes(row))
        p = dynamic_plan(toks)
        if max(p["cl"]) == 7:
            return row
    raise AssertionError("no seed whose code-length code reaches 7 bits")
