"""GPU tier of cell-palette dithering: exact equality -- pixels and the per-cell masks -- of dp_cells_u8 (through
backend.cells, CellPaletteDitherStrategy and the instance hook of ImageDitherer) with the numpy statement tests/cells_ref.py,
which tries every combination per cell and knows nothing of ranks, rows or lanes.  The shapes cut cells on both edges and
have several cells each way; one case has all 7280 candidates; the `sets` output is what holds the kernel's rank-to-mask
function to the statement.  Then the tie cases, the equivalences and a first-ever call inside a graph capture."""
import io

import numpy as np
import pytest

import cells_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend, dithering_lib
    yield backend, dithering_lib
    dithering_lib.drop_device_caches()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def u16_zeros(shape):
    import torch
    return torch.zeros(tuple(shape), dtype=torch.int16, device="cuda").view(torch.uint16)


def palette_of(k):
    """k distinct colours; the first two differ so that ties between entries are rare but (grey axis) not absent."""
    rs = np.random.RandomState(500 + k)
    pal = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (127, 127, 127)][:k]
    while len(pal) < k:
        c = tuple(int(v) for v in rs.randint(0, 256, 3))
        if c not in pal:
            pal.append(c)
    return pal


def groups_of(kind, K):
    full = (1 << K) - 1
    if kind == "one":
        return [full]
    if kind == "zx":                                                    # two halves that share entry 0
        half = (K + 1) // 2
        return [(1 << half) - 1, (full & ~((1 << half) - 1)) | 1]
    if kind == "four":                                                  # four overlapping windows, the last wraps round
        q = max(K // 4, 1)
        win = [full & (((1 << (2 * q + 1)) - 1) << (i * q)) for i in range(3)]
        return win + [(full & ~((1 << (3 * q)) - 1)) | ((1 << (q + 1)) - 1)]
    if kind == "same4":                                                 # the whole palette four times: 4 C(K, k) candidates
        return [full] * 4
    raise ValueError(kind)


def frames_of(orc, content, n, h, w, seed):
    if content == "noise":
        return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    return np.stack([orc.imgl(h, w, seed + i, "smooth" if i % 2 == 0 else "dark") for i in range(n)])


# h, w, cw, ch, frames, K, k, fixed, groups, m, spread, gamma, content
GRID = [
    (13, 21, 4, 4, 2, 16, 2, 0, "one", 4, 64, False, "noise"),
    (13, 21, 4, 4, 3, 5, 3, 0b00001, "one", 2, 255, True, "imgl"),
    (13, 21, 4, 4, 2, 15, 1, 0b00110, "four", 8, 0, False, "imgl"),
    (13, 21, 4, 4, 3, 2, 1, 0, "zx", 4, 255, True, "noise"),
    (37, 53, 8, 8, 2, 16, 4, 0, "one", 8, 64, False, "imgl"),          # 1820 candidates
    (37, 53, 8, 8, 3, 15, 2, 0, "zx", 4, 64, True, "imgl"),            # the ZX Spectrum's shape of rule
    (37, 53, 8, 8, 2, 16, 2, 0, "one", 4, 64, True, "noise"),          # C64 hires
    (37, 53, 8, 8, 2, 5, 4, 0, "one", 2, 255, False, "noise"),
    (37, 53, 8, 8, 3, 1, 1, 0, "one", 8, 64, False, "imgl"),
    (37, 53, 4, 8, 2, 16, 3, 0b1, "one", 4, 64, False, "imgl"),        # C64 multicolour
    (37, 53, 4, 8, 3, 15, 4, 0, "four", 2, 0, True, "noise"),
    (37, 53, 4, 8, 2, 2, 2, 0, "one", 8, 255, False, "imgl"),
    (37, 53, 16, 16, 2, 16, 2, 0b1000000000000010, "four", 8, 255, True, "noise"),
    (37, 53, 16, 16, 3, 5, 4, 0, "one", 2, 0, False, "imgl"),
    (37, 53, 16, 16, 2, 15, 3, 0b100, "zx", 4, 64, False, "noise"),
    (37, 53, 16, 4, 2, 16, 1, 0b11, "four", 4, 64, True, "imgl"),
    (37, 53, 8, 16, 3, 5, 2, 0b10000, "four", 8, 64, False, "noise"),
    (1, 1, 8, 8, 2, 16, 2, 0, "one", 4, 64, False, "noise"),
    (1, 1, 4, 16, 3, 1, 1, 0, "one", 2, 255, True, "noise"),
    (1, 1, 16, 16, 2, 15, 4, 0b1, "zx", 8, 0, False, "imgl"),
    (3, 70, 8, 8, 2, 16, 3, 0, "four", 8, 255, False, "imgl"),
    (3, 70, 16, 4, 3, 2, 1, 0b01, "one", 4, 64, True, "noise"),
    (3, 70, 4, 16, 2, 5, 2, 0, "zx", 2, 64, False, "noise"),
    (16, 16, 16, 16, 2, 16, 4, 0, "same4", 4, 64, False, "noise"),     # all 7280 candidates
]


def test_the_grid_covers_what_it_promises():
    col = list(zip(*GRID))
    assert {(h, w) for h, w in zip(col[0], col[1])} == {(13, 21), (37, 53), (1, 1), (3, 70), (16, 16)}
    assert {(37, 53, c, r) for c, r in ((8, 8), (4, 8), (16, 16))} <= set(zip(col[0], col[1], col[2], col[3]))
    assert set(col[4]) == {2, 3} and set(col[5]) == {1, 2, 5, 15, 16} and set(col[6]) == {1, 2, 3, 4}
    assert 0 in col[7] and any(col[7]) and {"one", "zx", "four"} <= set(col[8])
    assert set(col[9]) == {2, 4, 8} and set(col[10]) == {0, 64, 255} and set(col[11]) == {False, True}
    assert set(col[12]) == {"noise", "imgl"}
    assert len(cr.candidates(16, 4, 0, groups_of("same4", 16))) == 7280
    for h, w, cw, ch, n, K, k, fixed, kind, m, spread, gamma, content in GRID:
        cr.candidates(K, k, fixed, groups_of(kind, K))                 # every row is a valid setting


@pytest.mark.parametrize("case", range(len(GRID)))
def test_matches_the_statement(gpu, orc, case):
    import torch
    be, dl = gpu
    h, w, cw, ch, n, K, k, fixed, kind, m, spread, gamma, content = GRID[case]
    groups = groups_of(kind, K)
    pal_f32, outc, lut = dl.prepare_palette(palette_of(K), gamma)
    assert pal_f32.shape == (K, 3)
    frames = frames_of(orc, content, n, h, w, 40 + case)
    want, want_sets = cr.cells_frames(frames, pal_f32, outc, lut, cw, ch, k, fixed, groups, m, spread)
    P = be.Palette(pal_f32, outc, lut)
    got, sets = be.cells(torch.from_numpy(frames).cuda(), P, (cw, ch), k, m, spread, fixed_mask=fixed, groups=groups, sets=True)
    assert sets.dtype == torch.uint16 and tuple(sets.shape) == want_sets.shape
    got, sets = got.cpu().numpy(), sets.cpu().numpy()
    bad_sets = np.argwhere(sets != want_sets)
    assert not len(bad_sets), (GRID[case], len(bad_sets), bad_sets[:4].tolist())
    bad = np.argwhere((got != want).any(axis=-1))
    assert not len(bad), (GRID[case], len(bad), bad[:4].tolist())
    del P


@pytest.mark.parametrize("gx", [1, 3])
def test_workgroups_walk_several_cells(gpu, orc, switches, gx):
    """The experiments library with a small grid: every workgroup takes many of the 35 (8 x 8) or 98 (4 x 8) cells in turn,
    which in the product a frame of more cells than workgroups does."""
    import torch
    be, dl = gpu
    switches.setenv("DP_CELLS_GRID_X", str(gx))
    pal_f32, outc, lut = dl.prepare_palette(palette_of(16), True)
    P = be.Palette(pal_f32, outc, lut)
    frames = frames_of(orc, "imgl", 2, 37, 53, 7)
    for (cw, ch), k, fixed in (((8, 8), 2, 0), ((4, 8), 3, 1)):
        want, want_sets = cr.cells_frames(frames, pal_f32, outc, lut, cw, ch, k, fixed, [0xFFFF], 4, 64)
        got, sets = be.cells(torch.from_numpy(frames).cuda(), P, (cw, ch), k, 4, 64, fixed_mask=fixed, sets=True)
        assert np.array_equal(sets.cpu().numpy(), want_sets) and np.array_equal(got.cpu().numpy(), want), (gx, cw, ch)
    del P


# ---------------------------------------------------------------------------------------------------- ties
def _run(be, P, frames, cell, k, fixed=0, groups=None, m=4, spread=0):
    import torch
    got, sets = be.cells(torch.from_numpy(frames).cuda(), P, cell, k, m, spread, fixed_mask=fixed, groups=groups, sets=True)
    return got.cpu().numpy(), sets.cpu().numpy()


def test_tie_cases(gpu):
    be, dl = gpu
    pal = palette_of(16)
    pal_f32, outc, lut = dl.prepare_palette(pal, False)
    P = be.Palette(pal_f32, outc, lut)
    rs = np.random.RandomState(9)
    # all-zero frames: entry 0 is black, every candidate that holds it costs 0
    zero = np.zeros((2, 13, 21, 3), np.uint8)
    # a frame flat in a palette colour
    flat = np.broadcast_to(np.array(pal[9], np.uint8), (2, 13, 21, 3)).copy()
    # every 8 x 8 cell holds exactly two palette colours
    two = np.empty((2, 24, 40, 3), np.uint8)
    for f in range(2):
        for cy in range(3):
            for cx in range(5):
                a, b = rs.choice(16, 2, replace=False)
                pick = rs.randint(0, 2, (8, 8))
                pick[0, 0], pick[0, 1] = 0, 1                           # both occur
                two[f, cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = outc[np.where(pick, a, b)]
    for name, frames, cell, k, fixed, groups in (("zero", zero, (4, 4), 2, 0, None), ("zero", zero, (8, 8), 3, 0b10, [0xFF0F, 0x0FFF]),
                                                 ("flat", flat, (4, 4), 2, 0, None), ("flat", flat, (16, 8), 4, 0, [0xFF00, 0xFFFF]),
                                                 ("two", two, (8, 8), 2, 0, None), ("two", two, (8, 8), 3, 0, None),
                                                 ("two", two, (8, 8), 3, 0, [0x0FFF, 0xFFF0, 0xFFFF])):
        for m, spread in ((4, 0), (8, 255)):
            want, want_sets = cr.cells_frames(frames, pal_f32, outc, lut, cell[0], cell[1], k, fixed, groups or [0xFFFF], m, spread)
            got, sets = _run(be, P, frames, cell, k, fixed, groups, m, spread)
            assert np.array_equal(sets, want_sets) and np.array_equal(got, want), (name, cell, k, fixed, groups, m, spread)
    # with k = 2 and no spread the cost is 0 for exactly one candidate, the cell's pair; the image comes back
    got, sets = _run(be, P, two, (8, 8), 2)
    assert np.array_equal(got, two)
    assert all(bin(int(s)).count("1") == 2 for s in sets.reshape(-1))
    # with k = 3 many candidates cost 0: the first enumerated one holds the pair and the LOWEST third entry
    got3, sets3 = _run(be, P, two, (8, 8), 3)
    assert np.array_equal(got3, two)
    for s2, s3 in zip(sets.reshape(-1).tolist(), sets3.reshape(-1).tolist()):
        third = s3 & ~s2
        assert s3 & s2 == s2 and bin(third).count("1") == 1
        assert third == min(1 << j for j in range(16) if not (s2 >> j) & 1)
    del P


def test_duplicate_palette_entries_tie_to_the_lowest_index(gpu):
    be, dl = gpu
    pal = [(10, 20, 30), (200, 100, 50), (10, 20, 30), (200, 100, 50), (90, 90, 90)]
    pal_f32 = np.array(pal, np.float32)
    outc = np.array([[1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [5, 0, 0]], np.uint8)   # an output pixel names its entry
    P = be.Palette(pal_f32, outc, None)
    frames = np.random.RandomState(4).randint(0, 256, (2, 13, 21, 3)).astype(np.uint8)
    for k, groups in ((2, [0b11111]), (4, [0b01111]), (2, [0b01100, 0b11111])):
        want, want_sets = cr.cells_frames(frames, pal_f32, outc, None, 4, 4, k, 0, groups, 4, 64)
        got, sets = _run(be, P, frames, (4, 4), k, 0, groups, 4, 64)
        assert np.array_equal(sets, want_sets) and np.array_equal(got, want), (k, groups)
    del P


# ---------------------------------------------------------------------------------------------------- equivalences
def test_in_place_sets_batches_and_the_strategy(gpu, orc):
    import torch
    be, dl = gpu
    pal = palette_of(16)
    pal_f32, outc, lut = dl.prepare_palette(pal, False)
    P = be.Palette(pal_f32, outc, lut)
    frames = torch.from_numpy(frames_of(orc, "imgl", 2, 37, 53, 21)).cuda()
    want, want_sets = be.cells(frames, P, (8, 8), 2, 4, 64, sets=True)
    assert torch.equal(be.cells(frames, P, (8, 8), 2, 4, 64), want)      # without sets
    assert not torch.equal(want[0], want[1])
    for i in range(2):                                                   # a batch equals its frames one by one
        one, s1 = be.cells(frames[i], P, (8, 8), 2, 4, 64, sets=True)
        assert one.shape == frames[i].shape and torch.equal(one, want[i]) and s1.shape == want_sets.shape[1:]
        assert torch.equal(s1.view(torch.int16), want_sets[i].view(torch.int16))
    buf = torch.full_like(frames, 0xAB)
    sbuf = u16_zeros(want_sets.shape)
    got, gs = be.cells(frames, P, (8, 8), 2, 4, 64, out=buf, sets=sbuf)
    assert got.data_ptr() == buf.data_ptr() and gs.data_ptr() == sbuf.data_ptr()
    assert torch.equal(buf, want) and torch.equal(sbuf.view(torch.int16), want_sets.view(torch.int16))
    inplace = frames.clone()                                             # in place
    got = be.cells(inplace, P, (8, 8), 2, 4, 64, out=inplace)
    assert got.data_ptr() == inplace.data_ptr() and torch.equal(inplace, want)
    with pytest.raises(ValueError):
        be.cells(frames, P, (8, 8), 2, 4, 64, out=torch.zeros(5, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        be.cells(frames, P, (8, 8), 2, 4, 64, sets=u16_zeros((5,)))
    with pytest.raises(TypeError):
        be.cells(frames, P, (8, 8), 2, 4, 64, sets=torch.zeros(want_sets.shape, dtype=torch.int32, device="cuda"))
    s = dl.CellPaletteDitherStrategy()                                   # the defaults are the call above
    assert torch.equal(s.dither_frames(frames, pal), want)
    got, gs = s.dither_frames(frames, pal, return_sets=True)
    assert torch.equal(got, want) and torch.equal(gs.view(torch.int16), want_sets.view(torch.int16))
    planes, colours = s.dither_frames_indexed(frames, pal)
    assert planes.dtype == torch.uint8 and planes.shape == frames.shape[:3]
    assert np.array_equal(colours[planes.cpu().numpy()], want.cpu().numpy())
    with pytest.raises(ValueError, match="tiled"):
        s._run(frames, P, y0=8)
    # the strategy contract of the reference: float pixels and palette in, float palette rows out
    px = frames[0].cpu().numpy().reshape(-1, 3).astype(np.float32)
    back = s.dither(px, np.array(pal, np.float32), (37, 53))
    assert back.shape == px.shape and np.array_equal(back.astype(np.uint8).reshape(37, 53, 3), want[0].cpu().numpy())
    del P


def test_image_ditherer_paths_with_the_instance(gpu, orc):
    import torch
    from PIL import Image
    be, dl = gpu
    from dither_pie_amd import video_processor as vp
    S = dl.CellPaletteDitherStrategy
    arr = orc.imgl(37, 53, 5)                                            # a 53 x 37 image
    img = Image.fromarray(arr, "RGB")
    for gamma in (False, True):
        for s, pal, ref_args in ((S.zx_spectrum(), S.ZX_SPECTRUM_PALETTE, (8, 8, 2, 0, [0x00FF, 0x7F01], 4, 64)),
                                 (S(cell="4x8", colours=3, shared=(0,), matrix="8x8", spread=128), palette_of(16), (4, 8, 3, 1, [0xFFFF], 8, 128))):
            d = dl.ImageDitherer(num_colors=len(pal), dither_mode=s, palette=pal, use_gamma=gamma)
            pal_f32, outc, lut = dl.prepare_palette(pal, gamma)
            want = cr.cells_u8(arr, pal_f32, outc, lut, *ref_args)[0]
            got = d.apply_dithering(img)
            assert got.mode == "RGB" and got.size == (53, 37) and np.array_equal(np.asarray(got), want), gamma
            p_img = d.apply_dithering_indexed(img)
            assert p_img.mode == "P" and np.array_equal(np.asarray(p_img.convert("RGB")), want), gamma
            png = d.apply_dithering_png(img)
            dec = Image.open(io.BytesIO(png))
            assert dec.mode == "P" and np.array_equal(np.asarray(dec.convert("RGB")), want), gamma
            stack = np.stack([arr, arr[::-1].copy(), 255 - arr])
            frames = torch.from_numpy(stack).cuda()
            rgb = vp.process_frames(frames, d)
            assert np.array_equal(rgb.cpu().numpy(), cr.cells_frames(stack, pal_f32, outc, lut, *ref_args)[0]), gamma
            planes, colours = vp.process_frames_indexed(frames, d)
            assert planes.shape == (3, 37, 53) and np.array_equal(colours[planes.cpu().numpy()], rgb.cpu().numpy()), gamma
            assert d.dither_mode is s                                    # the hook stores nothing and replaces nothing
    from dither_pie_amd import sharding
    with pytest.raises(ValueError):                                      # a band edge would split cells: no row-band sharding
        sharding.dither_band(d, frames[0, :8].contiguous(), 8)


# ---------------------------------------------------------------------------------------------------- capture
def test_first_call_with_a_palette_inside_a_graph_capture(gpu, orc):
    """The call is launches only: the FIRST call with a fresh palette is captured into a graph (one stream, no parallel
    branches) and the replay gives the bytes of the statement."""
    import torch
    be, dl = gpu
    pal_f32, outc, lut = dl.prepare_palette(palette_of(15), True)
    frames = frames_of(orc, "imgl", 2, 37, 53, 33)
    groups = groups_of("zx", 15)
    want, want_sets = cr.cells_frames(frames, pal_f32, outc, lut, 8, 8, 2, 0, groups, 4, 64)
    P = be.Palette(pal_f32, outc, lut)                                   # never used before the capture
    dev = torch.from_numpy(frames).cuda()
    out = torch.zeros_like(dev)
    sets = u16_zeros(want_sets.shape)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        be.cells(dev, P, (8, 8), 2, 4, 64, groups=groups, out=out, sets=sets)
    torch.cuda.synchronize()
    assert not bool(out.any())                                           # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(sets.cpu().numpy(), want_sets)
    dev.copy_(torch.from_numpy(frames[::-1].copy()).cuda())              # new input, the same graph
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[::-1]) and np.array_equal(sets.cpu().numpy(), want_sets[::-1])
    del g, P
