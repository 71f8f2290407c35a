"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_png_dyn.h on the guarded arena
(tests/arena.py), as tests/test_gpu_png_memory.py is for ditherpie_hip_png.h: every pointer the library sees lies inside one
arena; the planes and the histograms have exactly their size and sit at odd (the histograms: 4-byte and no better)
addresses; the encoder's output is exactly n * stride bytes with stride = dp_png_deflate_bound_bytes, its workspace exactly
dp_png_deflate_dyn_workspace_bytes and 16- but not 32-byte aligned, the sizes 8- but not 16-byte aligned; whatever the
outputs and the workspace held before -- zeros, 0xFF, noise -- the streams are those of the host statement and inflate
(zlib) to tests/png_ref.py's filtered bytes; guards of >= 1 MiB stay intact; inputs are unchanged; a call with a workspace
or a stride one byte short is refused and nothing is launched.  tests/test_png_dyn_cpu.py checks COVERAGE against the
header.  No test here is meant to fault."""
import zlib

import numpy as np
import pytest

import arena as ar
import png_dyn_ref as dr
import png_ref as pr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_png_deflate_dyn_encode_u8": ["test_deflate_dyn_encode"],
    "dp_png_code_lengths_u8": ["test_code_lengths"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EWORKSPACE = 0, 1, 5
FILLS = ("zeros", "ones", ar.noise(93))
SHAPES = [(3, 17, 33), (4, 64, 64), (2, 37, 53), (1, 1, 1), (3, 3, 5)]
KINDS = ("tile", "noise", "photo", "noise", "flat")
SEGS = (256, 300, 8192, 32768)


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("depth", pr.DEPTHS)
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_deflate_dyn_encode(gpu, case, depth):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    n, h, w = SHAPES[case]
    n_px = h * w
    residue = (1, 3, 7, 15, 9)[case]
    seg = SEGS[(case + pr.DEPTHS.index(depth)) % len(SEGS)]
    rs = np.random.RandomState(60 + 10 * case + depth)
    planes = pr.content(KINDS[case], rs, n, h, w, 1 << depth)
    want = be.png_deflate_host(planes, depth, seg, blocks="dynamic")
    for f in range(n):
        assert zlib.decompress(want[f]) == pr.filtered(planes[f], depth)
    stride = L.dp_png_deflate_bound_bytes(h, w, depth, seg)
    need = L.dp_png_deflate_dyn_workspace_bytes(n, h, w, depth, seg)
    assert stride == pr.bound_bytes(h, w, depth, seg) and need > L.dp_png_deflate_workspace_bytes(n, h, w, depth, seg)
    specs = [(n * n_px, g), (n * stride, g), (8 * n, g), (need, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 90 + case)
    A.carve("planes", n * n_px, residue, g)                             # exactly n h w bytes, at an odd address
    A.put("planes", planes)
    A.carve("out", n * stride, (residue + 3) % 16, g)                   # exactly n * stride bytes, stride = the bound
    A.carve("sizes", 8 * n, 8, g)                                       # 8-byte aligned and no better
    A.carve("ws", need, 0, g)                                           # exactly the workspace, 16- but not 32-byte aligned
    assert A.ptr("ws") % 32 == 16 and A.ptr("sizes") % 16 == 8 and A.ptr("planes") % 2 == 1
    st = be._stream()
    for i, fill in enumerate(FILLS):
        A.reseed(600 + 10 * case + i)
        A.fill("out", fill)
        A.fill("sizes", FILLS[(i + 1) % 3])
        A.fill("ws", FILLS[(i + 2) % 3])                                # stale scratch of any kind
        rc = L.dp_png_deflate_dyn_encode_u8(A.ptr("planes"), n, h, w, depth, seg, A.ptr("out"), stride, A.ptr("sizes"), A.ptr("ws"), need, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        sizes = A.get("sizes", np.int64).tolist()
        assert sizes == [len(b) for b in want], (case, depth, fill)
        out = A.get("out").reshape(n, stride)
        for f in range(n):
            assert out[f, :sizes[f]].tobytes() == want[f], (case, depth, fill, f)
        A.check()
        A.unchanged("planes")

    # refusals launch nothing: every buffer keeps what it holds
    for name in ("out", "sizes", "ws"):
        A.put(name, A.get(name).copy())
    ok = [A.ptr("planes"), n, h, w, depth, seg, A.ptr("out"), stride, A.ptr("sizes"), A.ptr("ws"), need]

    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[dict(depth=4, seg=5, out=6, stride=7, sizes=8, ws=9, need=10)[key]] = v
        rc = L.dp_png_deflate_dyn_encode_u8(*a, st)
        torch.cuda.synchronize()
        assert b"dp_png_deflate_dyn_encode_u8" in L.dp_last_error(), L.dp_last_error()
        return rc
    assert call(need=need - 1) == DP_EWORKSPACE and call(need=0) == DP_EWORKSPACE
    assert call(need=L.dp_png_deflate_workspace_bytes(n, h, w, depth, seg)) == DP_EWORKSPACE   # the fixed-mode workspace is too small
    assert call(stride=stride - 1) == DP_EINVAL
    for bad in (dict(ws=A.ptr("ws") + 8), dict(ws=None), dict(sizes=A.ptr("sizes") + 4), dict(depth=3), dict(depth=16), dict(seg=255), dict(seg=32769),
                dict(out=None)):
        assert call(**bad) == DP_EINVAL, bad
    assert L.dp_png_deflate_dyn_encode_u8(A.ptr("planes"), 0, h, w, depth, seg, A.ptr("out"), stride, A.ptr("sizes"), A.ptr("ws"), need, st) == DP_OK
    torch.cuda.synchronize()
    for name in ("planes", "out", "sizes", "ws"):
        A.unchanged(name)
    A.check()
    del A


@pytest.mark.parametrize("m, L, a", [(286, 15, 7), (30, 15, 3), (19, 7, 5), (2, 1, 1), (133, 9, 2)])
def test_code_lengths(gpu, m, L, a):
    import torch
    lib, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(70 + m)
    counts = np.zeros((a, m), np.uint32)
    for i in range(a):
        kind = i % 3
        counts[i] = (rs.randint(0, 40, m) if kind == 0 else np.array((dr.fibonacci(min(m, 29)) + [0] * m)[:m])[rs.permutation(m)] if kind == 1 else
                     rs.randint(0, 2, m) * rs.randint(1, dr.MAX_COUNT + 1, m))
    want = be.png_code_lengths_host(counts, L)
    for i in range(a):
        assert want[i].tolist() == dr.code_lengths(counts[i].tolist(), L)
    A = ar.Arena(ar.capacity_for([(4 * a * m, g), (a * m, g)]), "cuda", 95)
    A.carve("counts", 4 * a * m, 4, g)                                  # exactly a * m counts, 4-byte aligned and no better
    A.put("counts", counts.view(np.uint8).reshape(-1))
    A.carve("lengths", a * m, 5, g)                                     # exactly a * m bytes, at an odd address
    assert A.ptr("counts") % 8 == 4 and A.ptr("lengths") % 2 == 1
    st = be._stream()
    for i, fill in enumerate(FILLS):
        A.reseed(700 + i)
        A.fill("lengths", fill)
        rc = lib.dp_png_code_lengths_u8(A.ptr("counts"), a, m, L, A.ptr("lengths"), st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, lib.dp_last_error())
        assert A.get("lengths").reshape(a, m).tolist() == want.tolist(), fill
        A.check()
        A.unchanged("counts")
    A.put("lengths", A.get("lengths").copy())
    for bad in ((None, a, m, L, A.ptr("lengths")), (A.ptr("counts"), a, m, L, None), (A.ptr("counts") + 2, a, m, L, A.ptr("lengths")),
                (A.ptr("counts"), -1, m, L, A.ptr("lengths")), (A.ptr("counts"), a, 1, L, A.ptr("lengths")), (A.ptr("counts"), a, 287, 15, A.ptr("lengths")),
                (A.ptr("counts"), a, m, 0, A.ptr("lengths")), (A.ptr("counts"), a, m, 16, A.ptr("lengths")), (A.ptr("counts"), a, 9, 3, A.ptr("lengths"))):
        assert lib.dp_png_code_lengths_u8(*bad, st) == DP_EINVAL and b"dp_png_code_lengths_u8" in lib.dp_last_error(), bad
    assert lib.dp_png_code_lengths_u8(A.ptr("counts"), 0, m, L, A.ptr("lengths"), st) == DP_OK
    torch.cuda.synchronize()
    A.unchanged("counts")
    A.unchanged("lengths")
    A.check()
    del A
