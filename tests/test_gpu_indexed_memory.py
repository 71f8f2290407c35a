"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_indexed.h, built on the guarded arena
(tests/arena.py) as tests/test_gpu_memory_discipline.py is for the main header: every pointer the library sees lies inside
one arena, buffers have exactly the documented size and sit at odd addresses (two-byte planes at even ones that are not
4-byte aligned; the aligned residues too, which is where the four-pixel kernels run), outputs are pre-filled with zeros,
0xFF and noise, guards of >= 1 MiB are seeded, the counters start from a different value each time and must have been ADDED
to, inputs must be unchanged.  tests/test_indexed_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import indexed_ref as ir

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_index_from_rgb_u8": ["test_index_from_rgb"],
    "dp_rgb_from_index_u8": ["test_rgb_from_index"],
    "dp_resize_nearest_plane_u8": ["test_plane_resize"],
}
EXCLUDED = {}   # (dp_index_map_create / _info / _destroy take no *_dev pointer)

DP_OK = 0
FILLS = ("zeros", "ones", ar.noise(77))
CNT_FILLS = (ar.noise(5), "zeros", "ones")          # the counter before the call: noise, 0, 2^64 - 1 (the sum wraps)


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _run(L, fn, inputs, outputs, counted, call, verify, seed):
    """inputs: name -> (array, residue mod 16); outputs: name -> (nbytes, residue); counted: what the call must add to the
    counter, or None when the entry point has none; call(p) -> rc with p: name -> address; verify(o): o name -> bytes."""
    import torch
    g = ar.MIN_GUARD
    specs = [(np.asarray(v[0]).nbytes, g) for v in inputs.values()] + [(v[0], g) for v in outputs.values()] + [(8, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", seed)
    for name, v in inputs.items():
        A.carve(name, np.asarray(v[0]).nbytes, v[1], g)
        A.put(name, v[0])
        assert A.ptr(name) % 16 == v[1]
    for name, v in outputs.items():
        A.carve(name, v[0], v[1], g)
        assert A.ptr(name) % 16 == v[1] and A.view(name).numel() == v[0]
    A.carve("cnt", 8, 8, g)                                         # 8-byte aligned and no better
    p = {name: A.ptr(name) for name in list(inputs) + list(outputs) + ["cnt"]}
    kept = []
    for i, fill in enumerate(FILLS):
        A.reseed(seed * 1000 + 17 * i + 1)
        for name in outputs:
            A.fill(name, fill)
        A.fill("cnt", CNT_FILLS[i])
        before = int(A.get("cnt", np.uint64)[0])
        rc = call(p)
        torch.cuda.synchronize()
        assert rc == DP_OK, (fn, fill, rc, L.dp_last_error())
        o = {name: A.get(name).copy() for name in outputs}
        verify(o)
        after = int(A.get("cnt", np.uint64)[0])
        if counted is None:
            A.unchanged("cnt")
        else:
            assert after == (before + counted) % (1 << 64), (fn, "the counter was not added to", before, after, counted)
        A.check()
        for name in inputs:
            A.unchanged(name)
        kept.append(o)
    for k in kept[1:]:
        for name in kept[0]:
            assert np.array_equal(kept[0][name], k[name]), f"{fn}: '{name}' depends on what the buffer held before the call"
    del A


def _colours(rs, K):
    code = np.zeros(0, np.int64)
    while len(code) < K + 1:
        code = np.unique(np.concatenate([code, rs.randint(0, 1 << 24, 2 * K + 8)]))
    code = rs.permutation(code)[:K + 1]
    c = np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=1).astype(np.uint8)
    return c[:K], c[K]


# (K, index bytes, rgb residue, plane residue): odd addresses; two-byte planes at even, non-4-aligned ones; then the residues
# the four-pixel kernels need (rgb 4-byte, plane 4- / 8-byte aligned and no better), and mixed ones that must fall back
LAYOUTS = [(16, 1, 1, 3), (16, 1, 3, 1), (256, 1, 15, 7), (16, 1, 4, 12), (256, 1, 12, 4), (16, 1, 4, 1), (16, 1, 2, 4),
           (16, 2, 1, 2), (300, 2, 3, 6), (1024, 2, 5, 10), (1024, 2, 9, 14), (16, 2, 4, 8), (1024, 2, 12, 8), (257, 2, 4, 4),
           (257, 2, 4, 12)]
N_PX = [1, 2, 3, 4, 5, 7, 21, 105, 1003, 8174]


def _cases():
    i = 0
    for K, nb, r_rgb, r_idx in LAYOUTS:
        for n in (N_PX if (r_rgb, r_idx) in ((1, 3), (4, 12), (1, 2), (4, 8)) else [5, 1003]):
            yield i, K, nb, r_rgb, r_idx, n
            i += 1


def test_index_from_rgb(gpu):
    L, be = gpu
    for i, K, nb, r_rgb, r_idx, n in _cases():
        rs = np.random.RandomState(100 + i)
        colours, foreign = _colours(rs, K)
        colours[K // 2] = colours[0]                                 # a duplicate: the lowest index wins
        imap = be.IndexMap(colours)
        rgb = colours[rs.randint(0, K, n)]
        rgb[rs.randint(0, 5, n) == 0] = foreign
        want, _, n_missing = ir.to_indices(rgb, colours)
        want = want.astype(np.uint8 if nb == 1 else np.uint16)

        def call(p):
            assert p["rgb"] % 16 == r_rgb and p["idx"] % 16 == r_idx
            return L.dp_index_from_rgb_u8(p["rgb"], p["idx"], n, imap._h, nb, p["cnt"], be._stream())

        def verify(o):
            assert np.array_equal(o["idx"].view(want.dtype), want), (K, nb, r_rgb, r_idx, n)

        _run(L, "dp_index_from_rgb_u8", {"rgb": (rgb, r_rgb)}, {"idx": (n * nb, r_idx)}, n_missing, call, verify, 100 + i)


def test_rgb_from_index(gpu):
    L, be = gpu
    for i, K, nb, r_rgb, r_idx, n in _cases():
        rs = np.random.RandomState(300 + i)
        colours, _ = _colours(rs, K)
        imap = be.IndexMap(colours)
        idx = rs.randint(0, K, n)
        bad = rs.randint(0, 5, n) == 0
        idx[bad] = rs.randint(K, 256 if nb == 1 else 65536, int(bad.sum())) if K < (256 if nb == 1 else 65536) else idx[bad]
        idx = idx.astype(np.uint8 if nb == 1 else np.uint16)
        want, _, n_bad = ir.from_indices(idx, colours)

        def call(p):
            assert p["rgb"] % 16 == r_rgb and p["idx"] % 16 == r_idx
            return L.dp_rgb_from_index_u8(p["idx"], p["rgb"], n, imap._h, nb, p["cnt"], be._stream())

        def verify(o):
            assert np.array_equal(o["rgb"].reshape(-1, 3), want), (K, nb, r_rgb, r_idx, n)

        _run(L, "dp_rgb_from_index_u8", {"idx": (idx, r_idx)}, {"rgb": (3 * n, r_rgb)}, n_bad, call, verify, 300 + i)


def test_plane_resize(gpu):
    L, be = gpu
    i = 0
    for (n, h, w) in [(1, 1, 1), (1, 7, 1), (1, 5, 7), (3, 5, 7), (3, 31, 47)]:
        for (oh, ow) in ((1, 1), (h * 3 + 1, w * 2 + 1), (max(1, h // 2), max(1, w // 3)), (7, 5)):
            for eb, (r_in, r_out) in ((1, [(1, 3), (3, 1), (0, 9), (15, 7)][i % 4]), (2, [(2, 6), (6, 2), (10, 14), (14, 0)][i % 4])):
                rs = np.random.RandomState(500 + i)
                plane = rs.randint(0, 256 if eb == 1 else 65536, (n, h, w)).astype(np.uint8 if eb == 1 else np.uint16)
                want = ir.resize_nearest_plane(plane, oh, ow)

                def call(p):
                    return L.dp_resize_nearest_plane_u8(p["in"], p["out"], n, h, w, oh, ow, eb, be._stream())

                def verify(o):
                    assert np.array_equal(o["out"].view(want.dtype).reshape(want.shape), want), (n, h, w, oh, ow, eb)

                _run(L, "dp_resize_nearest_plane_u8", {"in": (plane, r_in)}, {"out": (n * oh * ow * eb, r_out)}, None, call, verify, 500 + i)
            i += 1
