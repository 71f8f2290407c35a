"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_gif.h on the guarded arena
(tests/arena.py), as tests/test_gpu_scene_memory.py is for the scene header: every pointer the library sees lies inside one
arena; the planes, the carried plane and the delta output have exactly their size and sit at odd addresses; the encoder's
output is exactly n * stride bytes with stride = dp_gif_lzw_bound_bytes, its workspace exactly dp_gif_lzw_workspace_bytes and
16- but not 32-byte aligned, the sizes 8- but not 16-byte aligned; whatever the outputs and the workspace held before --
zeros, 0xFF, noise -- the results are those of tests/gif_ref.py; guards of >= 1 MiB stay intact; inputs are unchanged; a call
with a workspace or a stride one byte short is refused and nothing is launched.
tests/test_gif_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import gif_ref as gr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_index_delta_u8": ["test_index_delta"],
    "dp_gif_lzw_encode_u8": ["test_lzw_encode"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EWORKSPACE = 0, 1, 5
FILLS = ("zeros", "ones", ar.noise(91))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case, n, h, w, residue", [(0, 3, 17, 33, 1), (1, 4, 64, 64, 0), (2, 2, 37, 53, 7), (3, 1, 1, 1, 3), (4, 3, 3, 5, 4)])
def test_index_delta(gpu, case, n, h, w, residue):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    n_px = h * w
    rs = np.random.RandomState(40 + case)
    planes = rs.randint(0, 6, (n, h, w)).astype(np.uint8)               # few colours: many pixels repeat
    if n > 2:
        planes[2] = planes[1]                                           # a frame that repeats its predecessor: count 0
    before = rs.randint(0, 6, (h, w)).astype(np.uint8)
    specs = [(n * n_px, g), (n_px, g), (n * n_px, g), (8 * n, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 70 + case)
    A.carve("planes", n * n_px, residue, g)
    A.put("planes", planes)
    A.carve("prev", n_px, (residue + 5) % 16, g)
    A.carve("out", n * n_px, (residue + 10) % 16, g)
    A.carve("changed", 8 * n, 8, g)                                     # 8-byte aligned and no better
    assert A.ptr("changed") % 16 == 8 and A.ptr("planes") % 16 == (residue or 16) % 16
    st = be._stream()
    for k, fill in enumerate(FILLS):
        for has_prev in (0, 1):
            A.reseed(300 + 10 * case + 2 * k + has_prev)
            A.fill("out", fill)
            A.fill("changed", FILLS[(k + 1) % 3])
            if has_prev:
                A.put("prev", before)
            else:
                A.fill("prev", FILLS[(k + 2) % 3])                      # not read: whatever it holds
            rc = L.dp_index_delta_u8(A.ptr("planes"), n, n_px, A.ptr("prev"), has_prev, 200 + case, A.ptr("out"), A.ptr("changed"), st)
            torch.cuda.synchronize()
            assert rc == DP_OK, (rc, L.dp_last_error())
            want, counts = gr.index_delta(planes, 200 + case, before if has_prev else None)
            assert np.array_equal(A.get("out").reshape(n, h, w), want), (case, fill, has_prev)
            assert np.array_equal(A.get("changed", np.int64), counts), (case, fill, has_prev)
            assert np.array_equal(A.get("prev").reshape(h, w), planes[-1])                # the last INPUT plane is carried
            A.check()
            A.unchanged("planes")

    # refusals launch nothing: every buffer keeps what it holds
    for name in ("prev", "out", "changed"):
        A.put(name, A.get(name).copy())
    for args in ((A.ptr("planes"), n, n_px, A.ptr("prev"), 1, 256, A.ptr("out"), A.ptr("changed")),
                 (A.ptr("planes"), n, n_px, A.ptr("prev"), 1, -1, A.ptr("out"), A.ptr("changed")),
                 (A.ptr("planes"), n, n_px, A.ptr("prev"), 1, 3, A.ptr("planes"), A.ptr("changed")),                 # in place
                 (A.ptr("planes"), n, n_px, A.ptr("prev"), 1, 3, A.ptr("planes") + n * n_px - 1, A.ptr("changed")),   # the last byte shared
                 (A.ptr("planes"), n, n_px, A.ptr("prev"), 1, 3, A.ptr("prev"), A.ptr("changed")),
                 (A.ptr("planes"), n, n_px, A.ptr("prev"), 1, 3, A.ptr("out"), A.ptr("changed") + 4),
                 (A.ptr("planes"), n, n_px, None, 0, 3, A.ptr("out"), A.ptr("changed"))):
        rc = L.dp_index_delta_u8(*args, st)
        torch.cuda.synchronize()
        assert rc == DP_EINVAL and b"dp_index_delta_u8" in L.dp_last_error(), (rc, L.dp_last_error())
    assert L.dp_index_delta_u8(A.ptr("planes"), 0, n_px, A.ptr("prev"), 1, 3, A.ptr("out"), A.ptr("changed"), st) == DP_OK   # a no-op
    torch.cuda.synchronize()
    for name in ("planes", "prev", "out", "changed"):
        A.unchanged(name)
    A.check()
    del A


@pytest.mark.parametrize("case, n, h, w, k, chunk, residue, kind", [
    (0, 3, 17, 33, 16, 64, 1, "tile"), (1, 2, 64, 70, 256, 1000, 3, "noise"), (2, 2, 37, 53, 16, 1, 7, "tile"), (3, 3, 1, 1, 4, 5, 15, "noise"),
    (4, 1, 96, 96, 256, 96 * 96, 0, "noise"), (5, 2, 5, 7, 2, 3, 9, "noise"), (6, 4, 40, 40, 7, 512, 2, "flat")])
def test_lzw_encode(gpu, case, n, h, w, k, chunk, residue, kind):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    n_px = h * w
    rs = np.random.RandomState(50 + case)
    planes = gr.content(kind, rs, n, h, w, k)
    mcs = max(2, gr.table_bits(k))
    want = [gr.image_data(f.reshape(-1), mcs, chunk) for f in planes]
    stride = L.dp_gif_lzw_bound_bytes(h, w, chunk)
    need = L.dp_gif_lzw_workspace_bytes(n, h, w, chunk)
    assert stride == gr.bound_bytes(h, w, chunk) and need > 0
    specs = [(n * n_px, g), (n * stride, g), (8 * n, g), (need, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 80 + case)
    A.carve("planes", n * n_px, residue, g)                             # exactly n h w bytes, at any address
    A.put("planes", planes)
    A.carve("out", n * stride, (residue + 3) % 16, g)                   # exactly n * stride bytes, stride = the bound
    A.carve("sizes", 8 * n, 8, g)                                       # 8-byte aligned and no better
    A.carve("ws", need, 0, g)                                           # exactly the workspace, 16- but not 32-byte aligned
    assert A.ptr("ws") % 32 == 16 and A.ptr("sizes") % 16 == 8
    st = be._stream()
    first = None
    for i, fill in enumerate(FILLS):
        A.reseed(500 + 10 * case + i)
        A.fill("out", fill)
        A.fill("sizes", FILLS[(i + 1) % 3])
        A.fill("ws", FILLS[(i + 2) % 3])                                # stale scratch of any kind
        rc = L.dp_gif_lzw_encode_u8(A.ptr("planes"), n, h, w, mcs, chunk, A.ptr("out"), stride, A.ptr("sizes"), A.ptr("ws"), need, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        sizes = A.get("sizes", np.int64).tolist()
        assert sizes == [len(b) for b in want], (case, fill)
        out = A.get("out").reshape(n, stride)
        for f in range(n):
            assert out[f, :sizes[f]].tobytes() == want[f], (case, fill, f)
        A.check()
        A.unchanged("planes")
        if first is None:
            first = sizes

    # refusals launch nothing: every buffer keeps what it holds
    for name in ("out", "sizes", "ws"):
        A.put(name, A.get(name).copy())
    ok = [A.ptr("planes"), n, h, w, mcs, chunk, A.ptr("out"), stride, A.ptr("sizes"), A.ptr("ws"), need]
    def call(**kw):
        a = list(ok)
        for key, v in kw.items():
            a[dict(mcs=4, chunk=5, out=6, stride=7, sizes=8, ws=9, need=10)[key]] = v
        rc = L.dp_gif_lzw_encode_u8(*a, st)
        torch.cuda.synchronize()
        assert b"dp_gif_lzw_encode_u8" in L.dp_last_error(), L.dp_last_error()
        return rc
    assert call(need=need - 1) == DP_EWORKSPACE and call(need=0) == DP_EWORKSPACE
    assert call(stride=stride - 1) == DP_EINVAL
    for bad in (dict(ws=A.ptr("ws") + 8), dict(ws=None), dict(sizes=A.ptr("sizes") + 4), dict(mcs=1), dict(mcs=9), dict(chunk=0), dict(out=None)):
        assert call(**bad) == DP_EINVAL, bad
    assert L.dp_gif_lzw_encode_u8(A.ptr("planes"), 0, h, w, mcs, chunk, A.ptr("out"), stride, A.ptr("sizes"), A.ptr("ws"), need, st) == DP_OK
    torch.cuda.synchronize()
    for name in ("planes", "out", "sizes", "ws"):
        A.unchanged(name)
    A.check()
    del A
