"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_scene.h on the guarded arena
(tests/arena.py), as tests/test_gpu_clip_memory.py is for the clip header: every pointer the library sees lies inside one
arena; the frames have exactly their size and sit at odd addresses; the signature, carried-signature and distance buffers are
exactly as long and as aligned as the header asks and no better (16- but not 32-byte, 8- but not 16-byte); whatever the
outputs held before -- zeros, 0xFF, noise -- the values are those of tests/scene_ref.py; guards of >= 1 MiB stay intact;
inputs are unchanged; a misaligned buffer is refused with DP_EINVAL and nothing is launched.
tests/test_scenes_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import scene_ref as sr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_frame_signatures_u8": ["test_signatures_and_distances"],
    "dp_signature_distances": ["test_signatures_and_distances"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL = 0, 1
FILLS = ("zeros", "ones", ar.noise(78))
ROW = 4096 * 4


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case, n, h, w, residue", [(0, 3, 17, 33, 1), (1, 5, 129, 257, 3), (2, 2, 300, 400, 7), (3, 1, 1, 7, 15)])
def test_signatures_and_distances(gpu, case, n, h, w, residue):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(30 + case)
    frames = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    frames[0, :, : w // 2] = (15, 16, 240)                              # a flat half: many lanes on one bin
    other = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)              # the frame "before" the batch
    sig_want = sr.signatures(frames)
    prev_want = sr.signatures(other)[0]
    specs = [(frames.nbytes, g), (n * ROW, g), (ROW, g), (8 * n, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 60 + case)
    A.carve("frames", frames.nbytes, residue, g)                        # exactly 3 n h w bytes at an odd address
    A.put("frames", frames)
    A.carve("sig", n * ROW, 0, g)                                       # 16- but not 32-byte aligned
    A.carve("prev", ROW, 0, g)
    A.carve("dist", 8 * n, 8, g)                                        # 8-byte aligned and no better
    assert A.ptr("frames") % 2 == 1 and A.ptr("sig") % 32 == 16 and A.ptr("prev") % 32 == 16 and A.ptr("dist") % 16 == 8
    st = be._stream()
    for k, fill in enumerate(FILLS):
        A.reseed(900 + 10 * case + k)
        A.fill("sig", fill)                                             # the zeroing is part of the call
        A.fill("dist", FILLS[(k + 1) % 3])
        rc = L.dp_frame_signatures_u8(A.ptr("frames"), n, h, w, A.ptr("sig"), st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert np.array_equal(A.get("sig", np.uint32).reshape(n, 4096), sig_want), (case, fill)
        A.check()
        A.unchanged("frames")
        A.put("sig", A.get("sig").copy())                               # from here on the signatures are an input
        for has_prev in (0, 1):
            if has_prev:
                A.put("prev", prev_want.astype(np.uint32))
            else:
                A.fill("prev", FILLS[(k + 2) % 3])                      # not read: whatever it holds
            rc = L.dp_signature_distances(A.ptr("sig"), n, A.ptr("prev"), has_prev, A.ptr("dist"), st)
            torch.cuda.synchronize()
            assert rc == DP_OK, (rc, L.dp_last_error())
            want = sr.distances(sig_want, prev_want if has_prev else None)
            assert np.array_equal(A.get("dist", np.int64), want), (case, fill, has_prev)
            assert np.array_equal(A.get("prev", np.uint32), sig_want[-1])   # the last signature is carried
            A.check()
            A.unchanged("sig")
            A.unchanged("frames")

    # refusals launch nothing: every buffer keeps what it holds
    for name in ("sig", "prev", "dist"):
        A.put(name, A.get(name).copy())
    for ptr in (A.ptr("sig") + 8, A.ptr("sig") + 4, None):
        rc = L.dp_frame_signatures_u8(A.ptr("frames"), n, h, w, ptr, st)
        torch.cuda.synchronize()
        assert rc == DP_EINVAL and b"dp_frame_signatures_u8" in L.dp_last_error(), (rc, L.dp_last_error())
    for sig, prev, dist in ((A.ptr("sig") + 8, A.ptr("prev"), A.ptr("dist")), (A.ptr("sig"), A.ptr("prev") + 8, A.ptr("dist")),
                            (A.ptr("sig"), A.ptr("prev"), A.ptr("dist") + 4), (A.ptr("sig"), None, A.ptr("dist"))):
        rc = L.dp_signature_distances(sig, n, prev, 1, dist, st)
        torch.cuda.synchronize()
        assert rc == DP_EINVAL and b"dp_signature_distances" in L.dp_last_error(), (rc, L.dp_last_error())
    assert L.dp_frame_signatures_u8(A.ptr("frames"), 0, h, w, A.ptr("sig"), st) == DP_OK      # n_frames = 0: a no-op
    assert L.dp_signature_distances(A.ptr("sig"), 0, A.ptr("prev"), 1, A.ptr("dist"), st) == DP_OK
    torch.cuda.synchronize()
    for name in ("sig", "prev", "dist", "frames"):
        A.unchanged(name)
    A.check()
    del A
