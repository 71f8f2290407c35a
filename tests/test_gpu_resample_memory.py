"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_resample.h on the guarded arena
(tests/arena.py), as tests/test_gpu_idiff_memory.py is for its header: the frames the library sees lie inside one arena, have
exactly their size and sit at odd addresses; the workspace has exactly dp_resample_workspace_bytes bytes, 16-byte aligned and no
better, and holds noise; whatever the output held before -- zeros, 0xFF, noise -- the pixels are those of tests/resample_ref.py;
guards of >= 1 MiB stay intact; the input is unchanged; a refused call launches nothing and leaves every buffer as it was.
The shapes put the byte tail of a row (ow = 7: 21 bytes), the unaligned first and last dwords of a frame, the last narrower
column group and the last shorter row block of the staged horizontal kernel (16 columns x 64 rows) against guards.
tests/test_resample_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import ctypes as C

import numpy as np
import pytest

import arena as ar
import resample_ref as rr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_resample_u8": ["test_resample_on_the_arena"],
}
EXCLUDED = {
    "dp_resample_plan_create": "writes only the tables it allocates itself; every case here runs on the tables it uploaded",
}

DP_OK, DP_EINVAL, DP_EWORKSPACE = 0, 1, 5
FILLS = ("zeros", "ones", ar.noise(93))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend, _lib
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# case, frames, h, w, oh, ow, filter, residues of in / out
@pytest.mark.parametrize("case, n, h, w, oh, ow, name, r_in, r_out", [
    (0, 2, 37, 53, 8, 7, "lanczos", 1, 7),          # both passes; a 21-byte output row
    (1, 3, 17, 23, 40, 50, "box", 3, 5),            # an upscale, both passes, the naive horizontal kernel
    (2, 2, 130, 70, 66, 35, "bicubic", 15, 9),      # three row blocks and three column groups of the staged kernel
    (3, 2, 29, 18, 7, 18, "hamming", 5, 11),        # vertical only: rows of 54 bytes, a 2-byte tail
    (4, 2, 24, 31, 24, 9, "bilinear", 13, 3),       # horizontal only: no workspace
    (5, 1, 3, 400, 3, 2, "lanczos", 9, 1),          # a window wider than a staged row: the naive horizontal kernel
    (6, 2, 21, 19, 21, 19, "lanczos", 7, 13),       # equal sizes: the copy
])
def test_resample_on_the_arena(gpu, case, n, h, w, oh, ow, name, r_in, r_out):
    import torch
    L, be, _lib = gpu
    g = ar.MIN_GUARD
    frames = rr.content("noise", n, h, w, 60 + case)
    want = rr.resample(frames, oh, ow, name)
    plan = be.ResamplePlan(name, h, w, oh, ow)
    need = L.dp_resample_workspace_bytes(plan._h, n)
    assert need == rr.workspace_bytes(name, n, h, w, oh, ow) and need % 16 == 0
    assert (need > 0) == (oh != h and ow != w)
    nout = n * oh * ow * 3
    A = ar.Arena(ar.capacity_for([(frames.nbytes, g), (nout, g), (max(need, 16), g)]), "cuda", 80 + case)
    A.carve("in", frames.nbytes, r_in, g)                               # exactly 3 n h w bytes at an odd address
    A.put("in", frames)
    A.carve("out", nout, r_out, g)
    A.carve("ws", max(need, 16), 0, g)                                  # exactly the bytes asked for, 16-byte aligned and no better
    assert A.ptr("in") % 2 == 1 and A.ptr("out") % 2 == 1 and A.ptr("in") % 16 != A.ptr("out") % 16 and A.ptr("ws") % 32 == 16
    st = be._stream().value
    ok = dict(struct_size=C.sizeof(_lib.ResampleArgs), in_dev=A.ptr("in"), out_dev=A.ptr("out"), n_frames=n, plan=plan._h.value,
              workspace_dev=A.ptr("ws") if need else None, workspace_bytes=need, stream=st)

    def call(**kw):
        a = _lib.ResampleArgs(**dict(ok, **kw))
        return L.dp_resample_u8(C.byref(a))

    for i, fill in enumerate(FILLS):
        A.reseed(900 + 10 * case + i)
        A.fill("out", fill)
        A.fill("ws", FILLS[(i + 1) % 3])                                # whatever the workspace held
        rc = call()
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        got = A.get("out").reshape(n, oh, ow, 3)
        bad = np.argwhere((got != want).any(axis=-1))
        assert not len(bad), (case, fill, len(bad), bad[:4].tolist())
        A.check()
        A.unchanged("in")
        if not need:
            A.unchanged("ws")                                           # one pass: the workspace is not touched

    # refusals launch nothing: every buffer keeps what it holds
    A.put("out", A.get("out").copy())
    A.put("ws", A.get("ws").copy())
    size = ok["struct_size"]
    refusals = [(dict(in_dev=None), DP_EINVAL), (dict(out_dev=None), DP_EINVAL), (dict(plan=None), DP_EINVAL), (dict(n_frames=-1), DP_EINVAL),
                (dict(struct_size=size - 8), DP_EINVAL), (dict(struct_size=size + 8), DP_EINVAL), (dict(struct_size=0), DP_EINVAL),
                (dict(out_dev=A.ptr("in")), DP_EINVAL), (dict(workspace_dev=A.ptr("ws") + 8), DP_EINVAL), (dict(workspace_dev=A.ptr("ws") + 1), DP_EINVAL)]
    if need:
        refusals += [(dict(workspace_dev=None), DP_EINVAL), (dict(workspace_bytes=need - 1), DP_EWORKSPACE), (dict(workspace_bytes=0), DP_EWORKSPACE),
                     (dict(n_frames=n + 1), DP_EWORKSPACE)]              # (one frame more needs more workspace: refused before a launch)
    for kw, code in refusals:
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == code and b"dp_resample_u8" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert call(n_frames=0) == DP_OK                                    # n_frames = 0: a no-op
    assert call(n_frames=0, in_dev=None, out_dev=None, workspace_dev=None, workspace_bytes=0) == DP_OK
    torch.cuda.synchronize()
    A.unchanged("in")
    A.unchanged("out")
    A.unchanged("ws")
    A.check()
    del A
