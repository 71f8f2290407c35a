"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_png_file.h on the guarded arena
(tests/arena.py), as tests/test_gpu_png_memory.py is for the PNG header: every pointer the library sees lies inside one arena;
the runs / streams, prefixes and the suffix have exactly their size and sit at odd addresses; the output is exactly
n * dp_png_file_bound_bytes, the workspace exactly what the helper says and 16- but not 32-byte aligned, sizes and offsets 8-
but not 16-byte aligned, the CRC words 4- but not 8-byte aligned; whatever the outputs and the workspace held before -- zeros,
0xFF, noise -- the results are those of zlib.crc32 and of the host statement; no byte of the output at or after
offsets[n] changes; guards of >= 1 MiB stay intact; inputs are unchanged; a call with a workspace or an output one byte
short is refused and nothing is launched.  tests/test_png_file_cpu.py checks COVERAGE against the header.  No test here is
meant to fault."""
import zlib

import numpy as np
import pytest

import arena as ar
import png_file_ref as fr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_png_crc32_u8": ["test_crc32"],
    "dp_png_file_assemble_u8": ["test_file_assemble"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EWORKSPACE = 0, 1, 5
FILLS = ("zeros", "ones", ar.noise(93))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _lengths(be, case, stride):
    P, S = be.PNG_CRC_PIECE_BYTES, be.PNG_CRC_SPAN_BYTES
    return [[0, 1, 2, 3, 4, 5, stride], [P - 1, P, P + 1, 0, stride], [S + 1, S, S - 1, 3, stride, 0], [stride]][case]


@pytest.mark.parametrize("case", range(4))
def test_crc32(gpu, case):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    S = be.PNG_CRC_SPAN_BYTES
    stride = (9, 131, 2 * S + 7, 3 * S + 1)[case]                       # odd: the runs start at every residue mod 4
    sizes = _lengths(be, case, stride)
    n = len(sizes)
    residue = (1, 3, 6, 15)[case]
    rs = np.random.RandomState(70 + case)
    data = rs.randint(0, 256, (n, stride)).astype(np.uint8)
    want = [zlib.crc32(data[r, :k].tobytes()) for r, k in enumerate(sizes)]
    need = L.dp_png_crc32_workspace_bytes(n, stride)
    assert need > 0
    A = ar.Arena(ar.capacity_for([(n * stride, g), (8 * n, g), (4 * n, g), (need, g)]), "cuda", 40 + case)
    A.carve("data", n * stride, residue, g)                             # exactly the runs, at an odd address
    A.put("data", data)
    A.carve("sizes", 8 * n, 8, g)                                       # 8-byte aligned and no better
    A.put("sizes", np.array(sizes, np.int64))
    A.carve("crc", 4 * n, 4, g)                                         # 4-byte aligned and no better
    A.carve("ws", need, 0, g)                                           # exactly the workspace, 16- but not 32-byte aligned
    assert A.ptr("ws") % 32 == 16 and A.ptr("sizes") % 16 == 8 and A.ptr("crc") % 8 == 4 and A.ptr("data") % 16 == residue
    st = be._stream()
    for i, fill in enumerate(FILLS):
        A.reseed(700 + 10 * case + i)
        A.fill("crc", fill)
        A.fill("ws", FILLS[(i + 1) % 3])                                # stale scratch of any kind
        rc = L.dp_png_crc32_u8(A.ptr("data"), stride, A.ptr("sizes"), n, A.ptr("crc"), A.ptr("ws"), need, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert A.get("crc", np.uint32).tolist() == want, (case, fill)
        A.check()
        A.unchanged("data")
        A.unchanged("sizes")

    for name in ("crc", "ws"):                                          # refusals launch nothing: every buffer keeps what it holds
        A.put(name, A.get(name).copy())
    ok = [A.ptr("data"), stride, A.ptr("sizes"), n, A.ptr("crc"), A.ptr("ws"), need]

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[dict(stride=1, sizes=2, n=3, crc=4, ws=5, need=6)[key]] = v
        rc = L.dp_png_crc32_u8(*a, st)
        torch.cuda.synchronize()
        assert b"dp_png_crc32_u8" in L.dp_last_error(), L.dp_last_error()
        return rc
    assert call(need=need - 1) == DP_EWORKSPACE and call(need=0) == DP_EWORKSPACE
    for bad in (dict(ws=A.ptr("ws") + 8), dict(ws=None), dict(sizes=A.ptr("sizes") + 4), dict(crc=A.ptr("crc") + 2), dict(crc=None), dict(stride=-1), dict(n=-1)):
        assert call(**bad) == DP_EINVAL, bad
    assert L.dp_png_crc32_u8(A.ptr("data"), stride, A.ptr("sizes"), 0, A.ptr("crc"), A.ptr("ws"), need, st) == DP_OK
    torch.cuda.synchronize()
    for name in ("data", "sizes", "crc", "ws"):
        A.unchanged(name)
    A.check()
    del A


# (frames, stream stride, pre_bytes, per-frame prefixes, post_bytes, n_idat of 0 / 1 / n)
FILE_CASES = [(4, 131, 38, True, 0, 1), (3, 9, 0, False, 12, 3), (5, 2 * 16384 + 7, 41, False, 1, 0), (1, 3 * 16384 + 1, 4096, True, 64, 1), (6, 64, 3, True, 5, 0)]


@pytest.mark.parametrize("case", range(len(FILE_CASES)))
def test_file_assemble(gpu, case):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    n, stride, pre_bytes, per_frame, post_bytes, n_idat = FILE_CASES[case]
    P, S = be.PNG_CRC_PIECE_BYTES, be.PNG_CRC_SPAN_BYTES
    sizes = ([stride, 0, P + 1, 5], [0, 9, 4], [S + 1, stride, 0, S - 1, 3], [stride], [64, 63, 1, 0, 2, 64])[case]
    assert len(sizes) == n
    residue = (1, 3, 7, 15, 5)[case]
    seq0, step = (2, 2) if n_idat == 1 else (2 * 7, 2) if n_idat == 0 else (0, 2)
    rs = np.random.RandomState(80 + case)
    streams = rs.randint(0, 256, (n, stride)).astype(np.uint8)
    pre = rs.randint(0, 256, (n if per_frame else 1, pre_bytes)).astype(np.uint8)
    post = rs.randint(0, 256, post_bytes).astype(np.uint8)
    runs = [streams[f, :k].tobytes() for f, k in enumerate(sizes)]
    want, woffs = fr.assemble(runs, None if not pre_bytes else [p.tobytes() for p in pre] if per_frame else pre[0].tobytes(), post.tobytes(), n_idat, seq0, step)
    assert (want, woffs) == be.png_file_assemble_host(runs, (pre if per_frame else pre[0]) if pre_bytes else None, post.tobytes() or None, n_idat, seq0, step)
    bound = L.dp_png_file_bound_bytes(stride, pre_bytes, post_bytes)
    need = L.dp_png_file_workspace_bytes(n, stride)
    assert bound == pre_bytes + 16 + stride + post_bytes and need > 0
    specs = [(n * stride, g), (8 * n, g), (max(pre.size, 1), g), (max(post.size, 1), g), (n * bound, g), (8 * (n + 1), g), (need, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 50 + case)
    A.carve("streams", n * stride, residue, g)                          # exactly n strides, at an odd address
    A.put("streams", streams)
    A.carve("sizes", 8 * n, 8, g)                                       # 8-byte aligned and no better
    A.put("sizes", np.array(sizes, np.int64))
    A.carve("pre", max(pre.size, 1), (residue + 6) % 16 | 1, g)
    A.carve("post", max(post.size, 1), (residue + 2) % 16 | 1, g)
    if pre.size:
        A.put("pre", pre)
    if post.size:
        A.put("post", post)
    A.carve("out", n * bound, (residue + 3) % 16, g)                    # exactly n bounds
    A.carve("offsets", 8 * (n + 1), 8, g)
    A.carve("ws", need, 0, g)                                           # exactly the workspace, 16- but not 32-byte aligned
    assert A.ptr("ws") % 32 == 16 and A.ptr("sizes") % 16 == 8 and A.ptr("offsets") % 16 == 8 and A.ptr("streams") % 2 == 1
    st = be._stream()
    ok = [A.ptr("streams"), stride, A.ptr("sizes"), n, n_idat, seq0, step, A.ptr("pre") if pre_bytes else None, pre_bytes if per_frame else 0, pre_bytes,
          A.ptr("post") if post_bytes else None, post_bytes, A.ptr("out"), n * bound, A.ptr("offsets"), A.ptr("ws"), need]
    for i, fill in enumerate(FILLS):
        A.reseed(800 + 10 * case + i)
        A.fill("out", fill)
        A.fill("offsets", FILLS[(i + 1) % 3])
        A.fill("ws", FILLS[(i + 2) % 3])                                # stale scratch of any kind
        before = A.get("out").copy()
        rc = L.dp_png_file_assemble_u8(*ok, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert A.get("offsets", np.int64).tolist() == woffs, (case, fill)
        out = A.get("out")
        assert out[:len(want)].tobytes() == want, (case, fill)
        assert np.array_equal(out[len(want):], before[len(want):]), (case, fill)   # nothing at or after offsets[n]
        A.check()
        for name in ("streams", "sizes", "pre", "post"):
            A.unchanged(name)

    for name in ("out", "offsets", "ws"):                               # refusals launch nothing: every buffer keeps what it holds
        A.put(name, A.get(name).copy())
    names = dict(stride=1, sizes=2, n=3, n_idat=4, pre_stride=8, pre_bytes=9, post_bytes=11, out=12, out_bytes=13, offsets=14, ws=15, need=16)

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[names[key]] = v
        rc = L.dp_png_file_assemble_u8(*a, st)
        torch.cuda.synchronize()
        assert b"dp_png_file_assemble_u8" in L.dp_last_error(), L.dp_last_error()
        return rc
    assert call(need=need - 1) == DP_EWORKSPACE and call(need=0) == DP_EWORKSPACE
    assert call(out_bytes=n * bound - 1) == DP_EINVAL
    for bad in (dict(ws=A.ptr("ws") + 8), dict(ws=None), dict(sizes=A.ptr("sizes") + 4), dict(offsets=A.ptr("offsets") + 4), dict(out=None), dict(n_idat=n + 1),
                dict(n_idat=-1), dict(pre_bytes=4097), dict(post_bytes=65), dict(stride=(1 << 31) - 16)):
        assert call(**bad) == DP_EINVAL, bad
    empty = list(ok)
    empty[3] = empty[4] = 0
    assert L.dp_png_file_assemble_u8(*empty, st) == DP_OK               # n == 0: a no-op
    torch.cuda.synchronize()
    for name in ("streams", "sizes", "pre", "post", "out", "offsets", "ws"):
        A.unchanged(name)
    A.check()
    del A
