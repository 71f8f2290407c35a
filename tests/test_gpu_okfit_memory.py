"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_okfit.h on the guarded arena
(tests/arena.py), as tests/test_gpu_metric_memory.py is for the metric header: the buffers the library sees lie inside one
arena, have exactly their size and sit at addresses that are as aligned as the header asks and no better (the palette at odd
ones); whatever outputs and workspace held before -- zeros, 0xFF, noise -- the result is that of tests/okfit_ref.py, so no call
depends on stale scratch; guards of >= 1 MiB stay intact; inputs are unchanged; a refused call launches nothing and leaves every
buffer as it was.  tests/test_okfit_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import ctypes as C

import numpy as np
import pytest

import arena as ar
import okfit_ref as ok

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_okfit_hist_count": ["test_hist_points_on_the_arena"],
    "dp_okfit_hist_points": ["test_hist_points_on_the_arena"],
    "dp_okfit_points_u32": ["test_points_and_fit_on_the_arena"],
    "dp_okfit_fit": ["test_points_and_fit_on_the_arena"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
FILLS = ("zeros", "ones", ar.noise(57))
REC = np.dtype([("code", "<u4"), ("count", "<u4"), ("lab", "<i2", (3,)), ("zero", "<i2")])


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def records(codes, counts):
    import metric_ref as mr
    rec = np.zeros(len(codes), REC)
    rec["code"], rec["count"], rec["lab"] = codes, counts, mr.lab(ok.colours_of(codes))
    return rec


def test_hist_points_on_the_arena(gpu):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(31)
    px = rs.randint(0, 256, (3000, 3)).astype(np.uint8)
    px[:900] = px[900:1800] // 64 * 64                                   # repeats, and cells with many colours beside empty ones
    codes, counts = ok.points_of(px)
    n = len(codes)
    want = records(codes, counts)
    hist = be.ColourHistogram(torch.from_numpy(px).cuda())
    hist_bytes, need = hist.buf.numel(), L.dp_okfit_hist_workspace_bytes()
    for case, cap in enumerate((n, n - 1, 7, n + 5)):
        A = ar.Arena(ar.capacity_for([(hist_bytes, g), (16 * cap, g), (8, g), (need, g)]), "cuda", 40 + case)
        A.carve("hist", hist_bytes, 0, g)
        A.view("hist").copy_(hist.buf)
        A.expected["hist"] = ("data", A.view("hist").clone())
        A.carve("pts", 16 * cap, 0, g)                                  # exactly `capacity` records, 16-byte aligned and no better
        A.carve("n", 8, 8, g)
        A.carve("ws", need, 0, g)
        assert A.ptr("pts") % 32 == 16 and A.ptr("n") % 16 == 8 and A.ptr("ws") % 32 == 16 and A.ptr("hist") % 32 == 16
        st = be._stream()
        for i, fill in enumerate(FILLS):
            A.reseed(300 + 10 * case + i)
            for name in ("pts", "n", "ws"):
                A.fill(name, fill)
            rc = L.dp_okfit_hist_count(A.ptr("hist"), A.ptr("n"), A.ptr("ws"), need, st)
            torch.cuda.synchronize()
            assert rc == DP_OK, (rc, L.dp_last_error())
            assert int(A.get("n", np.int64)[0]) == n
            A.unchanged("pts")                                          # the count writes no record
            A.fill("n", fill)
            A.fill("ws", FILLS[(i + 1) % 3])
            rc = L.dp_okfit_hist_points(A.ptr("hist"), A.ptr("pts"), cap, A.ptr("n"), A.ptr("ws"), need, st)
            torch.cuda.synchronize()
            assert rc == DP_OK, (rc, L.dp_last_error())                 # also with a capacity below n: the caller compares
            assert int(A.get("n", np.int64)[0]) == n, (case, fill)       # the true n
            got = A.get("pts").view(REC)
            m = min(n, cap)
            assert np.array_equal(got[:m], want[:m]), (case, fill)
            A.check()
            A.unchanged("hist")
        if cap > n:
            A.fill("pts", ar.noise(5))
            assert L.dp_okfit_hist_points(A.ptr("hist"), A.ptr("pts"), cap, A.ptr("n"), A.ptr("ws"), need, st) == DP_OK
            torch.cuda.synchronize()
            keep = A.get("pts").copy()
            A.fill("pts", ar.noise(5))
            assert np.array_equal(A.get("pts")[16 * n:], keep[16 * n:])  # the records past n are not touched
        # refusals launch nothing
        for name in ("pts", "n", "ws"):
            A.put(name, A.get(name).copy())
        for kw in (dict(h=None), dict(h=A.ptr("hist") + 8), dict(p=None), dict(p=A.ptr("pts") + 8), dict(cap=-1), dict(cap=(1 << 24) + 1), dict(n=None),
                   dict(n=A.ptr("n") + 4), dict(ws=None), dict(ws=A.ptr("ws") + 8), dict(wsb=need - 1)):
            v = dict(dict(h=A.ptr("hist"), p=A.ptr("pts"), cap=cap, n=A.ptr("n"), ws=A.ptr("ws"), wsb=need), **kw)
            rc = L.dp_okfit_hist_points(v["h"], v["p"], v["cap"], v["n"], v["ws"], v["wsb"], st)
            assert rc == DP_EINVAL and b"dp_okfit_hist_points" in L.dp_last_error(), (kw, rc, L.dp_last_error())
            if "p" not in kw and "cap" not in kw:
                rc = L.dp_okfit_hist_count(v["h"], v["n"], v["ws"], v["wsb"], st)
                assert rc == DP_EINVAL and b"dp_okfit_hist_count" in L.dp_last_error(), (kw, rc, L.dp_last_error())
        torch.cuda.synchronize()
        for name in ("pts", "n", "ws", "hist"):
            A.unchanged(name)
        A.check()
        del A


# case, points, colours, max_iter, residue of the palette (odd)
@pytest.mark.parametrize("case, n, K, max_iter, r_pal", [(0, 1, 1, 100, 1), (1, 257, 16, 100, 3), (2, 1000, 256, 3, 7), (3, 65, 17, 2, 15), (4, 5, 16, 100, 5)])
def test_points_and_fit_on_the_arena(gpu, case, n, K, max_iter, r_pal):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    codes, counts = ok.random_points(n, 80 + case)
    want_rec = records(codes, counts)
    want = ok.fit_points(codes, counts, K, max_iter)
    need = L.dp_okfit_workspace_bytes(n, K)
    assert need > 0
    A = ar.Arena(ar.capacity_for([(4 * n, g), (4 * n, g), (16 * n, g), (3 * K, g), (12 * K, g), (8, g), (need, g)]), "cuda", 60 + case)
    A.carve("codes", 4 * n, 4, g)                                       # 4-byte aligned and no better
    A.put("codes", codes.astype(np.uint32))
    A.carve("counts", 4 * n, 12, g)
    A.put("counts", counts.astype(np.uint32))
    A.carve("pts", 16 * n, 0, g)
    A.carve("pal", 3 * K, r_pal, g)                                     # exactly 3 K bytes at an odd address
    A.carve("centres", 12 * K, 4, g)
    A.carve("dist", 8, 8, g)
    A.carve("ws", need, 0, g)                                           # exactly the declared workspace
    assert A.ptr("pts") % 32 == 16 and A.ptr("pal") % 2 == 1 and A.ptr("centres") % 8 == 4 and A.ptr("dist") % 16 == 8 and A.ptr("ws") % 32 == 16
    st = be._stream()
    n_iter = C.c_int(-1)
    for i, fill in enumerate(FILLS):
        A.reseed(500 + 10 * case + i)
        for name in ("pts", "pal", "centres", "dist", "ws"):
            A.fill(name, fill)
        rc = L.dp_okfit_points_u32(A.ptr("codes"), A.ptr("counts"), n, A.ptr("pts"), st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert np.array_equal(A.get("pts").view(REC), want_rec), (case, fill)
        for name in ("pal", "centres", "dist", "ws"):
            A.unchanged(name)
        A.put("pts", A.get("pts").copy())
        rc = L.dp_okfit_fit(A.ptr("pts"), n, K, max_iter, A.ptr("pal"), A.ptr("centres"), A.ptr("dist"), C.byref(n_iter), A.ptr("ws"), need, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        got = (A.get("pal").reshape(K, 3), A.get("centres", np.int32).reshape(K, 3), n_iter.value, int(A.get("dist", np.uint64)[0]))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:], (case, fill, got[2:], want[2:])
        A.check()
        for name in ("codes", "counts", "pts"):
            A.unchanged(name)

    # refusals launch nothing: every buffer keeps what it holds
    for name in ("pal", "centres", "dist", "ws"):
        A.put(name, A.get(name).copy())
    n_iter.value = -5
    ok_args = dict(p=A.ptr("pts"), n=n, K=K, it=max_iter, pal=A.ptr("pal"), cen=A.ptr("centres"), dist=A.ptr("dist"), out=C.byref(n_iter), ws=A.ptr("ws"), wsb=need)
    for kw, code in ((dict(p=None), DP_EINVAL), (dict(p=A.ptr("pts") + 8), DP_EINVAL), (dict(n=0), DP_EINVAL), (dict(n=-1), DP_EINVAL), (dict(K=0), DP_EINVAL),
                     (dict(K=257), DP_EUNSUPPORTED), (dict(it=0), DP_EINVAL), (dict(it=10001), DP_EINVAL), (dict(pal=None), DP_EINVAL),
                     (dict(cen=None), DP_EINVAL), (dict(cen=A.ptr("centres") + 2), DP_EINVAL), (dict(dist=None), DP_EINVAL),
                     (dict(dist=A.ptr("dist") + 4), DP_EINVAL), (dict(out=None), DP_EINVAL), (dict(ws=None), DP_EINVAL), (dict(ws=A.ptr("ws") + 8), DP_EINVAL),
                     (dict(wsb=need - 1), DP_EINVAL)):
        v = dict(ok_args, **kw)
        rc = L.dp_okfit_fit(v["p"], v["n"], v["K"], v["it"], v["pal"], v["cen"], v["dist"], v["out"], v["ws"], v["wsb"], st)
        assert rc == code and b"dp_okfit_fit" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    for kw in (dict(c=None), dict(k=None), dict(p=None), dict(c=A.ptr("codes") + 2), dict(k=A.ptr("counts") + 1), dict(p=A.ptr("pts") + 8), dict(n=-1),
               dict(n=(1 << 24) + 1)):
        v = dict(dict(c=A.ptr("codes"), k=A.ptr("counts"), n=n, p=A.ptr("pts")), **kw)
        rc = L.dp_okfit_points_u32(v["c"], v["k"], v["n"], v["p"], st)
        assert rc == DP_EINVAL and b"dp_okfit_points_u32" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert L.dp_okfit_points_u32(A.ptr("codes"), A.ptr("counts"), 0, A.ptr("pts"), st) == DP_OK   # n = 0: a no-op
    torch.cuda.synchronize()
    assert n_iter.value == -5
    for name in ("codes", "counts", "pts", "pal", "centres", "dist", "ws"):
        A.unchanged(name)
    A.check()
    del A
