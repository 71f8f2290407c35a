"""GPU tier of the void-and-cluster generator: equality of dp_void_cluster_u16 (through backend.void_cluster_ranks) with the
numpy statement tests/vac_ref.py -- the smallest size, a window wider than the matrix, odd sizes, a strip, the default and
the full 128 x 128 footprint with 16 cells per lane -- in a batch and under graph capture; Thresholds.void_cluster; and the
matrix through the ordered kernels, the strategy, bands and indexed output against the oracle given the statement's
thresholds."""
import numpy as np
import pytest

import vac_ref as vr

pytestmark = pytest.mark.gpu

# h, w, seed, sigma
RANK_CASES = [(8, 8, 1, 1.5), (8, 8, 1, 3.0), (13, 9, 3, 1.5), (16, 24, 5, 1.0), (128, 8, 2, 1.5), (64, 64, 42, 1.5), (128, 128, 3, 1.5)]


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


@pytest.fixture(scope="module")
def default64():
    """The statement's 64 x 64 matrix of seed 42 and its thresholds, shared by the tests below."""
    r = vr.ranks(64, 64, 42, 384)
    return r, vr.thresholds(r)


@pytest.mark.parametrize("h, w, seed, sigma", RANK_CASES)
def test_ranks_equal_the_statement(gpu, default64, h, w, seed, sigma):
    be, _ = gpu
    got = be.void_cluster_ranks(h, w, [seed], sigma)
    import torch
    assert got.dtype == torch.int16 and got.is_cuda and tuple(got.shape) == (1, h, w)
    want = default64[0] if (h, w, seed, sigma) == (64, 64, 42, 1.5) else vr.ranks(h, w, seed, int(round(sigma * 256)))
    assert np.array_equal(got[0].cpu().numpy().astype(np.int64), want)


def test_batch_equals_single_calls(gpu):
    be, _ = gpu
    seeds = [0, 1, 0xFFFFFFFF, 77, 1 << 31]
    both = be.void_cluster_ranks(16, 24, seeds, 1.25).cpu().numpy()
    assert both.shape == (5, 16, 24)
    for i, s in enumerate(seeds):
        assert np.array_equal(both[i], be.void_cluster_ranks(16, 24, s, 1.25)[0].cpu().numpy()), s
    assert len({both[i].tobytes() for i in range(5)}) == 5              # the seed matters
    assert np.array_equal(both[2].astype(np.int64), vr.ranks(16, 24, 0xFFFFFFFF, 320))
    assert tuple(be.void_cluster_ranks(16, 24, [], 1.25).shape) == (0, 16, 24)
    # more matrices than one launch carries seeds for
    many = be.void_cluster_ranks(8, 8, list(range(70)), 1.5).cpu().numpy()
    assert np.array_equal(many[69].astype(np.int64), vr.ranks(8, 8, 69, 384)) and np.array_equal(many[1].astype(np.int64), vr.ranks(8, 8, 1, 384))


def test_captured_call_replays(gpu):
    """Launches only: the very first call with these arguments may sit inside a capture."""
    import torch
    be, _ = gpu
    out = torch.zeros((2, 24, 40), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        be.void_cluster_ranks(24, 40, [9, 10], 1.75, out=out)
    torch.cuda.synchronize()
    assert not bool(out.any())                                          # captured, not run
    eager = be.void_cluster_ranks(24, 40, [9, 10], 1.75)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert np.array_equal(eager[1].cpu().numpy().astype(np.int64), vr.ranks(24, 40, 10, 448))
    with pytest.raises(ValueError, match="out must be"):
        be.void_cluster_ranks(24, 40, [9], 1.75, out=out)


def test_thresholds_object(gpu, default64):
    be, dl = gpu
    t = be.Thresholds.void_cluster(64, 64, 42)
    assert t.shape == (64, 64) and t.integer_form and t.numpy().tobytes() == default64[1].tobytes()
    odd = be.Thresholds.void_cluster(13, 9, 3, 300 / 256)
    assert odd.shape == (13, 9) and odd.numpy().tobytes() == vr.thresholds(vr.ranks(13, 9, 3, 300)).tobytes()
    for size in (16, 32):                                               # (128 x 128 is a multiple of 2^-13 as well: CPU tier)
        assert be.Thresholds.void_cluster(size, size, 1).integer_form, size
    # the device path and the host path of the generator give the same bytes
    dev = dl.generate_void_and_cluster(64, 42, 1.5)
    host = be.void_cluster_thresholds(be.void_cluster_ranks_host(64, 64, 42, 1.5))
    assert dev.dtype == host.dtype == np.float32 and dev.tobytes() == host.tobytes() == default64[1].tobytes()
    assert dl.generate_void_and_cluster((13, 9), 3, 300 / 256).tobytes() == odd.numpy().tobytes()


def _palette(dl, k, gamma, seed):
    rs = np.random.RandomState(seed)
    return [tuple(c) for c in rs.randint(0, 256, (k, 3)).tolist()], gamma


@pytest.mark.parametrize("h, w, k, gamma", [(37, 53, 16, False), (70, 45, 256, True)])
def test_ordered_output_equals_the_oracle_with_the_statements_matrix(gpu, orc, default64, h, w, k, gamma):
    import torch
    from PIL import Image
    be, dl = gpu
    rs = np.random.RandomState(h)
    arr = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    arr[:, :, 0] = np.linspace(0, 255, w).astype(np.uint8)[None, :]
    pal, _ = _palette(dl, k, gamma, 5 + k)
    pal_f32, outc, lut = dl.prepare_palette(pal, gamma)
    want = orc.ordered_u8(arr, pal_f32, outc, lut, "matrix", thr=default64[1])
    frames = torch.from_numpy(arr[None]).cuda()
    thr = be.Thresholds.void_cluster(64, 64, 42)
    got = be.ordered(frames, be.Palette(pal_f32, outc, lut), be.MODE_MATRIX, thr=thr)
    assert np.array_equal(got[0].cpu().numpy(), want)

    s = dl.VoidAndClusterDitherStrategy()
    d = dl.ImageDitherer(num_colors=k, dither_mode=s, palette=pal, use_gamma=gamma)
    img = d.apply_dithering(Image.fromarray(arr, "RGB"))
    assert img.mode == "RGB" and np.array_equal(np.asarray(img), want)
    assert d.dither_mode is s and s.threshold_matrix.tobytes() == default64[1].tobytes()

    # a two-band (y0, x0) split equals the whole image: the mode is position-only
    from dither_pie_amd import sharding
    cut = h // 2 + 1
    top = sharding.dither_band(d, frames[0, :cut].contiguous(), 0)
    low = sharding.dither_band(d, frames[0, cut:].contiguous(), cut)
    assert np.array_equal(torch.cat([top, low]).cpu().numpy(), want)
    right = d.apply_dithering_frames(frames[:, :, 20:].contiguous(), y0=0, x0=20)
    assert np.array_equal(right[0].cpu().numpy(), want[:, 20:])

    planes, colours = d.apply_dithering_frames_indexed(frames)
    assert tuple(planes.shape) == (1, h, w) and np.array_equal(colours[planes.cpu().numpy().astype(np.int64) & 0xFFFF][0], want)
