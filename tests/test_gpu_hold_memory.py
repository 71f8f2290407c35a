"""GPU tier: memory discipline of dp_hold_u8 (include/ditherpie_hip_hold.h) on the guarded arena (tests/arena.py), as
tests/test_gpu_resample_memory.py is for its header: every buffer the library sees lies inside one arena, has exactly its size and
sits at the residue asked for -- odd ones for the byte instance of the kernel, multiples of 4 (and no better than 16) for the dword
instance; whatever out, refreshed and -- without state -- the two state buffers held before (zeros, 0xFF, noise), the results are
those of tests/hold_ref.py; guards of >= 1 MiB stay intact; src and planes are unchanged; a refused call launches nothing and leaves
every buffer as it was.  The shapes put clipped cells, a last run of 1, 2 and 3 pixels, w < one run and the last row of a tile
against the guards.  No test here is meant to fault."""
import ctypes as C

import numpy as np
import pytest

import arena as ar
import hold_ref as hr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_hold_u8": ["test_hold_on_the_arena"],
}

DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2
FILLS = ("zeros", "ones", ar.noise(57))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend, _lib
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# case, (n, h, w, cell, tol, share256), residues of src / planes / anchor / held / out
@pytest.mark.parametrize("case, geom, res", [
    (0, (5, 17, 19, 16, 3, 0), (1, 3, 5, 7, 9)),            # clipped cells of 16, a last run of 3 pixels; every base odd
    (1, (4, 1, 1, 1, 0, 0), (15, 1, 3, 13, 11)),            # one pixel
    (2, (6, 9, 67, 4, 2, 64), (2, 6, 10, 14, 1)),           # two tiles across, a last run of 3; bases even and odd
    (3, (5, 33, 5, 8, 0, 256), (3, 2, 1, 0, 5)),            # three tiles down, a row of one whole run and one pixel
    (4, (4, 7, 10, 2, 5, 128), (7, 7, 7, 7, 7)),            # cells of 2, a last run of 2
    (5, (3, 3, 3, 16, 1, 1), (9, 5, 1, 13, 3)),             # w < one run
    (6, (4, 20, 68, 8, 6, 128), (0, 4, 8, 12, 0)),          # the dword instance: w % 4 == 0, every base 4-byte aligned and no better
    (7, (3, 33, 128, 16, 2, 32), (4, 4, 0, 8, 12)),         # the dword instance over 2 x 3 tiles, cells of 16 clipped at the bottom
    (8, (3, 18, 64, 1, 0, 0), (8, 0, 4, 0, 4)),             # the dword instance, cells of 1
    (9, (3, 18, 64, 16, 2, 0), (8, 1, 4, 0, 4)),            # ... and the same geometry on the byte instance: ONE odd base
])
def test_hold_on_the_arena(gpu, case, geom, res):
    import torch
    L, be, _lib = gpu
    g = ar.MIN_GUARD
    n, h, w, cell, tol, share256 = geom
    px = h * w
    src, planes = hr.clip(n, h, w, cell, tol, 300 + case)
    want_out, want_refreshed, want_state = hr.hold(src, planes, None, cell, tol, share256)
    more_src, more_planes = np.ascontiguousarray(src[::-1]), np.ascontiguousarray(planes[::-1])          # the stream goes on
    more_out, more_refreshed, more_state = hr.hold(more_src, more_planes, want_state, cell, tol, share256)
    sizes = dict(src=n * px * 3, planes=n * px, anchor=px * 3, held=px, out=n * px, refreshed=8 * n)
    A = ar.Arena(ar.capacity_for([(b, g) for b in sizes.values()]), "cuda", 40 + case)
    for name, r in zip(("src", "planes", "anchor", "held", "out"), res):
        A.carve(name, sizes[name], r, g)
        assert A.ptr(name) % 16 == r and (r or A.ptr(name) % 32 == 16)
    A.carve("refreshed", sizes["refreshed"], 8, g)                                                       # 8-byte aligned and no better
    assert A.ptr("refreshed") % 16 == 8
    vec = w % 4 == 0 and all(r % 4 == 0 for r in res)
    assert vec == (case in (6, 7, 8))
    st = be._stream().value
    ok = dict(struct_size=C.sizeof(_lib.HoldArgs), src_dev=A.ptr("src"), planes_dev=A.ptr("planes"), n_frames=n, h=h, w=w, cell=cell, tol=tol,
              share256=share256, anchor_dev=A.ptr("anchor"), held_dev=A.ptr("held"), has_state=0, out_dev=A.ptr("out"),
              refreshed_dev=A.ptr("refreshed"), stream=st)

    def call(**kw):
        a = _lib.HoldArgs(**dict(ok, **kw))
        return L.dp_hold_u8(C.byref(a))

    def same(out, refreshed, state, what):
        got = A.get("out").reshape(n, h, w)
        bad = np.argwhere(got != out)
        assert not len(bad), (what, len(bad), bad[:4].tolist())
        assert A.get("refreshed", np.int64).tolist() == refreshed.tolist(), what
        assert np.array_equal(A.get("anchor").reshape(h, w, 3), state[0]) and np.array_equal(A.get("held").reshape(h, w), state[1]), what

    for i, fill in enumerate(FILLS):
        A.reseed(700 + 10 * case + i)
        A.put("src", src)
        A.put("planes", planes)
        for j, name in enumerate(("out", "refreshed", "anchor", "held")):        # stale contents of everything the call writes
            A.fill(name, FILLS[(i + j) % 3])
        rc = call()
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        same(want_out, want_refreshed, want_state, (case, fill, "first"))
        A.check()
        A.unchanged("src")
        A.unchanged("planes")
        # ... and with the state the call left, over stale out and refreshed again
        A.put("src", more_src)
        A.put("planes", more_planes)
        A.fill("out", FILLS[(i + 1) % 3])
        A.fill("refreshed", FILLS[(i + 2) % 3])
        rc = call(has_state=1)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        same(more_out, more_refreshed, more_state, (case, fill, "second"))
        A.check()
        A.unchanged("src")
        A.unchanged("planes")

    # refusals launch nothing: every buffer keeps what it holds
    for name in ("out", "refreshed", "anchor", "held"):
        A.put(name, A.get(name).copy())
    size = ok["struct_size"]
    refusals = [(dict(src_dev=None), DP_EINVAL), (dict(planes_dev=None), DP_EINVAL), (dict(anchor_dev=None), DP_EINVAL), (dict(held_dev=None), DP_EINVAL),
                (dict(out_dev=None), DP_EINVAL), (dict(refreshed_dev=None), DP_EINVAL), (dict(n_frames=-1), DP_EINVAL),
                (dict(struct_size=size - 8), DP_EINVAL), (dict(struct_size=size + 8), DP_EINVAL), (dict(struct_size=0), DP_EINVAL),
                (dict(h=0), DP_EINVAL), (dict(w=-1), DP_EINVAL), (dict(cell=3), DP_EINVAL), (dict(cell=32), DP_EINVAL), (dict(tol=256), DP_EINVAL),
                (dict(share256=257), DP_EINVAL), (dict(refreshed_dev=A.ptr("refreshed") + 4), DP_EINVAL),
                (dict(out_dev=A.ptr("planes")), DP_EINVAL), (dict(out_dev=A.ptr("src") + 1), DP_EINVAL), (dict(out_dev=A.ptr("held")), DP_EINVAL),
                (dict(out_dev=A.ptr("anchor") + 3 * px - 1), DP_EINVAL), (dict(anchor_dev=A.ptr("src")), DP_EINVAL),
                (dict(held_dev=A.ptr("planes") + px * (n - 1)), DP_EINVAL), (dict(n_frames=65536), DP_EUNSUPPORTED)]
    for kw, code in refusals:
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == code and b"dp_hold_u8" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert call(n_frames=0) == DP_OK                                    # n_frames = 0: a no-op
    assert call(n_frames=0, src_dev=None, planes_dev=None, anchor_dev=None, held_dev=None, out_dev=None, refreshed_dev=None) == DP_OK
    torch.cuda.synchronize()
    for name in sizes:
        A.unchanged(name)
    A.check()
    del A
