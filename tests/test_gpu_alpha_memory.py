"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_alpha.h on the guarded arena (tests/arena.py), as
tests/test_gpu_hold_memory.py is for its header: every buffer the library sees lies inside one arena, has exactly its size and sits
at the residue asked for -- odd ones for the byte instances and the unaligned prefetches, multiples of 4 (and no better than 16) for
the dword instances; whatever the outputs (and the diffusion's workspace) held before (zeros, 0xFF, noise), the results are those of
tests/alpha_ref.py; guards of >= 1 MiB stay intact; the inputs are unchanged; a refused call launches nothing.  The shapes put a last
run of 1, 2 and 3 pixels, a frame smaller than a run, the last rows of a band and of a tile against the guards.  No test here is meant
to fault."""
import ctypes as C

import numpy as np
import pytest

import alpha_ref as ar
import arena as an
import dotdiff_ref as dr
import idiff_ref as ir

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_alpha_split_u8": ["test_split_key_join_on_the_arena"],
    "dp_alpha_key_u8": ["test_split_key_join_on_the_arena"],
    "dp_alpha_join_u8": ["test_split_key_join_on_the_arena"],
    "dp_alpha_idiff_u8": ["test_masked_idiff_on_the_arena"],
    "dp_alpha_dotdiff_u8": ["test_masked_dotdiff_on_the_arena"],
}

DP_OK, DP_EINVAL = 0, 1
FILLS = ("zeros", "ones", an.noise(91))
BLACK_WHITE = [(0, 0, 0), (255, 255, 255)]
FILL = (200, 3, 77)


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend, dithering_lib
    yield _lib.load(), backend, _lib, dithering_lib
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_the_coverage_table_names_every_device_entry_point():
    from dither_pie_amd import _lib
    assert set(COVERAGE) == {n for n in _lib.EXPORTS_ALPHA if "_host_" not in n}
    assert all(callable(globals().get(t)) for tests in COVERAGE.values() for t in tests)


def rgba_frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, h, w, 4)).astype(np.uint8)
    f[..., 3][rng.integers(0, 3, (n, h, w)) == 0] = 0
    f[..., 3][rng.integers(0, 3, (n, h, w)) == 0] = 255
    return f


# case, (n, h, w), residues of rgba / rgb / mask / planes / out / joined
@pytest.mark.parametrize("case, geom, res", [
    (0, (3, 17, 19), (1, 3, 5, 7, 9, 11)),              # a last run of 3 pixels; every base odd
    (1, (4, 1, 1), (15, 1, 3, 13, 11, 5)),              # one pixel
    (2, (2, 9, 67), (2, 6, 10, 14, 1, 3)),              # bases even and odd
    (3, (3, 33, 5), (3, 2, 1, 0, 5, 7)),                # a last run of 1
    (4, (2, 7, 10), (7, 7, 7, 7, 7, 7)),                # a last run of 2
    (5, (3, 1, 3), (9, 5, 1, 13, 3, 7)),                # a frame smaller than one run
    (6, (3, 20, 68), (0, 4, 8, 12, 0, 4)),              # the dword instances: h * w % 4 == 0, every base 4-byte aligned and no better
    (7, (2, 33, 128), (4, 4, 0, 8, 12, 8)),             # ... over several workgroups
    (8, (2, 33, 128), (4, 4, 1, 8, 12, 8)),             # ... and the same geometry on the byte instances: ONE odd base (the mask)
])
def test_split_key_join_on_the_arena(gpu, case, geom, res):
    import torch
    L, be, _lib, _ = gpu
    g = an.MIN_GUARD
    n, h, w = geom
    px = n * h * w
    src = rgba_frames(n, h, w, 300 + case)
    planes = np.random.default_rng(case).integers(0, 250, (n, h, w)).astype(np.uint8)
    kw = dict(mode=1, threshold=0, m=(2, 4, 8)[case % 3], y0=3 + case, x0=11) if case % 2 else dict(mode=0, threshold=128, m=0, y0=0, x0=0)
    matte = (250, 10, 128) if case % 3 == 0 else None
    rgb, mask, masked = ar.split(src, ar.MODES[kw["mode"]], kw["threshold"], kw["m"] or 4, matte, kw["y0"], kw["x0"])
    sizes = dict(rgba=4 * px, rgb=3 * px, mask=px, planes=px, out=px, joined=4 * px, masked=8 * n)
    A = an.Arena(an.capacity_for([(b, g) for b in sizes.values()]), "cuda", 60 + case)
    for name, r in zip(("rgba", "rgb", "mask", "planes", "out", "joined"), res):
        A.carve(name, sizes[name], r, g)
        assert A.ptr(name) % 16 == r and (r or A.ptr(name) % 32 == 16)
    A.carve("masked", sizes["masked"], 8, g)
    st = be._stream().value

    def split(**over):
        a = dict(struct_size=C.sizeof(_lib.AlphaSplitArgs), rgba_dev=A.ptr("rgba"), n_frames=n, h=h, w=w, has_matte=int(matte is not None),
                 matte=_lib._rgb3(*(matte or (0, 0, 0))), rgb_dev=A.ptr("rgb"), mask_dev=A.ptr("mask"), masked_dev=A.ptr("masked"), stream=st, **kw)
        return L.dp_alpha_split_u8(C.byref(_lib.AlphaSplitArgs(**dict(a, **over))))

    def key(**over):
        a = dict(struct_size=C.sizeof(_lib.AlphaKeyArgs), planes_dev=A.ptr("planes"), mask_dev=A.ptr("mask"), n_frames=n, h=h, w=w, key=251,
                 out_dev=A.ptr("out"), stream=st)
        return L.dp_alpha_key_u8(C.byref(_lib.AlphaKeyArgs(**dict(a, **over))))

    def join(**over):
        a = dict(struct_size=C.sizeof(_lib.AlphaJoinArgs), rgb_dev=A.ptr("rgb"), mask_dev=A.ptr("mask"), n_frames=n, h=h, w=w, fill=_lib._rgb3(*FILL),
                 rgba_dev=A.ptr("joined"), stream=st)
        return L.dp_alpha_join_u8(C.byref(_lib.AlphaJoinArgs(**dict(a, **over))))

    for i, fill in enumerate(FILLS):
        A.reseed(700 + 10 * case + i)
        A.put("rgba", src)
        A.put("planes", planes)
        for j, name in enumerate(("rgb", "mask", "masked", "out", "joined")):       # stale contents of everything the calls write
            A.fill(name, FILLS[(i + j) % 3])
        assert split() == DP_OK, L.dp_last_error()
        assert key() == DP_OK, L.dp_last_error()
        assert join() == DP_OK, L.dp_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(A.get("rgb").reshape(rgb.shape), rgb) and np.array_equal(A.get("mask").reshape(mask.shape), mask), (case, fill)
        assert A.get("masked", np.int64).tolist() == masked.tolist()
        assert np.array_equal(A.get("out").reshape(mask.shape), ar.key(planes, mask, 251)), (case, fill)
        assert np.array_equal(A.get("joined").reshape(n, h, w, 4), ar.join(rgb, mask, FILL)), (case, fill)
        A.check()
        A.unchanged("rgba")
        A.unchanged("planes")
    # the key in place
    assert key(out_dev=A.ptr("planes")) == DP_OK, L.dp_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(A.get("planes").reshape(mask.shape), ar.key(planes, mask, 251))
    A.check()
    # refusals launch nothing: every buffer keeps what it holds
    for name in sizes:
        A.put(name, A.get(name).copy())
    for rc in (split(rgb_dev=None), split(mode=2), split(masked_dev=A.ptr("masked") + 4), split(rgb_dev=A.ptr("rgba") + 1), split(n_frames=65536),
               key(key=256), key(out_dev=A.ptr("mask")), key(out_dev=A.ptr("planes") + 1), join(rgba_dev=A.ptr("rgb")), join(mask_dev=None),
               join(struct_size=8)):
        assert rc != DP_OK
    assert split(n_frames=0) == DP_OK and key(n_frames=0) == DP_OK and join(n_frames=0) == DP_OK
    torch.cuda.synchronize()
    for name in sizes:
        A.unchanged(name)
    A.check()
    del A


def grey_frames(n, h, w):
    rs = np.random.RandomState(7300 + 10 * h + w)
    v = rs.randint(0, 128, (n, h, w)) + (np.arange(w) * 127 // max(w - 1, 1))[None, None, :]
    return np.ascontiguousarray(np.repeat(v.astype(np.uint8)[..., None], 3, axis=-1))


def masks_for(n, h, w, seed):
    return np.stack([ar.mask_family(("half", "sixteenth", "checker")[f % 3], h, w, seed + f) for f in range(n)])


# case, (n, h, w), tap set, residues of in / mask / out
@pytest.mark.parametrize("case, geom, tapname, res", [
    (0, (2, 67, 21), "floyd_steinberg", (1, 3, 5)),     # two bands, the last of three rows; every base odd
    (1, (1, 1, 1), "jjn", (15, 1, 3)),                  # one pixel: every prefetch is the bytewise one
    (2, (1, 130, 9), "jjn", (2, 7, 9)),                 # three bands, a row of one period and one pixel
    (3, (2, 3, 40), "atkinson", (0, 0, 0)),             # five periods a row, aligned bases
    (4, (1, 64, 8), "floyd_steinberg", (3, 3, 3)),      # exactly a band of exactly a period
])
def test_masked_idiff_on_the_arena(gpu, orc, case, geom, tapname, res):
    import torch
    L, be, _lib, dl = gpu
    n, h, w = geom
    px = n * h * w
    taps, div = ir.KERNELS[tapname]
    spec = dl.prepare_palette(BLACK_WHITE, False)
    P = be.Palette(*spec)
    frames, masks = grey_frames(n, h, w), masks_for(n, h, w, 40 + case)
    want = np.stack([ar.idiff_masked_u8(orc, f, k, *spec, taps, div, 256, FILL) for f, k in zip(frames, masks)])
    ws_bytes = int(L.dp_idiff_workspace_bytes(n, h, w))
    g = an.MIN_GUARD
    sizes = dict(src=3 * px, mask=px, out=3 * px, ws=ws_bytes)
    A = an.Arena(an.capacity_for([(b, g) for b in sizes.values()]), "cuda", 80 + case)
    for name, r in zip(("src", "mask", "out"), res):
        A.carve(name, sizes[name], r, g)
    A.carve("ws", ws_bytes, 0, g)
    dx, dy, wt = (np.array([t[i] for t in taps], np.int32) for i in range(3))
    st = be._stream().value

    def call(**over):
        a = dict(struct_size=C.sizeof(_lib.AlphaIdiffArgs), in_dev=A.ptr("src"), mask_dev=A.ptr("mask"), out_dev=A.ptr("out"), n_frames=n, h=h, w=w,
                 pal=P._h, dx=dx.ctypes.data, dy=dy.ctypes.data, weight=wt.ctypes.data, n_taps=len(taps), divisor=div, strength256=256,
                 fill=_lib._rgb3(*FILL), workspace_dev=A.ptr("ws"), workspace_bytes=ws_bytes, stream=st)
        return L.dp_alpha_idiff_u8(C.byref(_lib.AlphaIdiffArgs(**dict(a, **over))))

    for i, fill in enumerate(FILLS):
        A.reseed(900 + 10 * case + i)
        A.put("src", frames)
        A.put("mask", masks)
        A.fill("out", FILLS[(i + 1) % 3])
        A.fill("ws", fill)                                                # a poisoned workspace: the library writes what it reads from it
        assert call() == DP_OK, L.dp_last_error()
        torch.cuda.synchronize()
        bad = np.argwhere(A.get("out").reshape(want.shape) != want)
        assert not len(bad), (case, fill, len(bad), bad[:4].tolist())
        A.check()
        A.unchanged("src")
        A.unchanged("mask")
    A.put("out", A.get("out").copy())
    for rc in (call(mask_dev=None), call(out_dev=A.ptr("src")), call(out_dev=A.ptr("mask")), call(workspace_bytes=ws_bytes - 1), call(n_taps=0),
               call(struct_size=16)):
        assert rc != DP_OK and b"dp_alpha_idiff_u8" in L.dp_last_error()
    assert call(n_frames=0) == DP_OK
    torch.cuda.synchronize()
    A.unchanged("out")
    A.check()
    del A


# case, (n, h, w), matrix, residues of in / mask / out
@pytest.mark.parametrize("case, geom, mname, res", [
    (0, (2, 15, 17), "knuth", (1, 3, 5)),               # less than a tile; every base odd
    (1, (1, 1, 1), "bayer2", (15, 1, 3)),
    (2, (1, 65, 81), "knuth", (2, 7, 9)),               # 2 x 2 tiles, the second ones a row and 17 columns
    (3, (2, 64, 64), "bayer4", (0, 0, 0)),              # exactly a tile, aligned bases
])
def test_masked_dotdiff_on_the_arena(gpu, orc, case, geom, mname, res):
    import torch
    L, be, _lib, dl = gpu
    n, h, w = geom
    px = n * h * w
    classes = np.ascontiguousarray({"knuth": dr.KNUTH, "bayer2": ar.bayer_rank(2), "bayer4": ar.bayer_rank(4)}[mname].astype(np.uint8))
    spec = dl.prepare_palette(BLACK_WHITE, False)
    P = be.Palette(*spec)
    frames, masks = grey_frames(n, h, w), masks_for(n, h, w, 70 + case)
    want = np.stack([ar.dotdiff_masked_u8(orc, f, k, *spec, classes, 256, FILL) for f, k in zip(frames, masks)])
    g = an.MIN_GUARD
    sizes = dict(src=3 * px, mask=px, out=3 * px)
    A = an.Arena(an.capacity_for([(b, g) for b in sizes.values()]), "cuda", 120 + case)
    for name, r in zip(("src", "mask", "out"), res):
        A.carve(name, sizes[name], r, g)
    st = be._stream().value

    def call(**over):
        a = dict(struct_size=C.sizeof(_lib.AlphaDotdiffArgs), in_dev=A.ptr("src"), mask_dev=A.ptr("mask"), out_dev=A.ptr("out"), n_frames=n, h=h, w=w,
                 pal=P._h, classes_host=classes.ctypes.data, m=classes.shape[0], strength256=256, fill=_lib._rgb3(*FILL), stream=st)
        return L.dp_alpha_dotdiff_u8(C.byref(_lib.AlphaDotdiffArgs(**dict(a, **over))))

    for i, fill in enumerate(FILLS):
        A.reseed(1100 + 10 * case + i)
        A.put("src", frames)
        A.put("mask", masks)
        A.fill("out", fill)
        assert call() == DP_OK, L.dp_last_error()
        torch.cuda.synchronize()
        bad = np.argwhere(A.get("out").reshape(want.shape) != want)
        assert not len(bad), (case, fill, len(bad), bad[:4].tolist())
        A.check()
        A.unchanged("src")
        A.unchanged("mask")
    A.put("out", A.get("out").copy())
    for rc in (call(mask_dev=None), call(out_dev=A.ptr("src")), call(out_dev=A.ptr("mask")), call(m=3), call(struct_size=16)):
        assert rc != DP_OK and b"dp_alpha_dotdiff_u8" in L.dp_last_error()
    assert call(n_frames=0) == DP_OK
    torch.cuda.synchronize()
    A.unchanged("out")
    A.check()
    del A
