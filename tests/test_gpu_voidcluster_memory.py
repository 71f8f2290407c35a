"""GPU tier: memory discipline of the device entry point of include/ditherpie_hip_voidcluster.h on the guarded arena
(tests/arena.py), as tests/test_gpu_dotdiff_memory.py is for the dot-diffusion header: the rank buffer the library sees lies
inside the arena, has exactly its size and sits at an odd multiple of 2 bytes; whatever it held before -- zeros, 0xFF, noise --
the ranks are those of tests/vac_ref.py; guards of >= 1 MiB stay intact; a refused call launches nothing and leaves every
byte as it was.  dp_thresholds_void_cluster takes no *_dev pointer (it allocates its own memory); its refusals are in
tests/test_voidcluster_cpu.py, which also checks COVERAGE against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import vac_ref as vr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_void_cluster_u16": ["test_void_cluster_on_the_arena"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL = 0, 1
FILLS = ("zeros", "ones", ar.noise(57))


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# case, matrices, h, w, sigma256, residue of ranks_dev mod 16
@pytest.mark.parametrize("case, n, h, w, s256, residue", [
    (0, 3, 13, 9, 384, 2),
    (1, 1, 128, 128, 384, 6),
    (2, 2, 8, 8, 768, 14),
])
def test_void_cluster_on_the_arena(gpu, case, n, h, w, s256, residue):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    seeds = np.array([11 + 7 * case + i for i in range(n)], np.uint32)
    want = np.stack([vr.ranks(h, w, int(s), s256) for s in seeds]).astype(np.uint16)
    nbytes = want.nbytes
    A = ar.Arena(ar.capacity_for([(nbytes, g)]), "cuda", 40 + case)
    A.carve("ranks", nbytes, residue, g)                                # exactly 2 n h w bytes at an odd multiple of 2
    assert A.ptr("ranks") % 4 == 2
    st = be._stream()
    for i, fill in enumerate(FILLS):
        A.reseed(500 + 10 * case + i)
        A.fill("ranks", fill)
        rc = L.dp_void_cluster_u16(A.ptr("ranks"), n, seeds.ctypes.data, h, w, s256, st)
        torch.cuda.synchronize()
        assert rc == DP_OK, (rc, L.dp_last_error())
        assert np.array_equal(A.get("ranks", np.uint16).reshape(n, h, w), want), (case, fill)
        A.check()

    # refusals launch nothing: the buffer keeps what it holds
    A.put("ranks", A.get("ranks").copy())
    for kw in (dict(r=None), dict(sd=None), dict(n=-1), dict(h=7), dict(h=129), dict(w=0), dict(w=129), dict(s=255), dict(s=769)):
        v = dict(r=A.ptr("ranks"), n=n, sd=seeds.ctypes.data, h=h, w=w, s=s256)
        v.update(kw)
        rc = L.dp_void_cluster_u16(v["r"], v["n"], v["sd"], v["h"], v["w"], v["s"], st)
        torch.cuda.synchronize()
        assert rc == DP_EINVAL and b"dp_void_cluster_u16" in L.dp_last_error(), (kw, rc, L.dp_last_error())
    assert L.dp_void_cluster_u16(A.ptr("ranks"), 0, seeds.ctypes.data, h, w, s256, st) == DP_OK   # n_matrices = 0: a no-op
    torch.cuda.synchronize()
    A.unchanged("ranks")
    A.check()
    del A
