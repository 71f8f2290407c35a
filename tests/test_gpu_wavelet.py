"""GPU tier of wavelet dithering (wavelet.hip on the product library): bit equality with the reference's recorded outputs
(tests/golden/wavelet.*, 1x1 up to 4K), a seeded fuzz against the CPU restatement (tests/wavelet_ref.py), batches, the
device-batch entry, the stream cache and the refusal of tiles and of a short stream."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import wavelet_ref as wr

pytestmark = pytest.mark.gpu


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


with open(os.path.join(GOLDEN, "wavelet.json")) as _fh:
    WL = json.load(_fh)
WL_NPZ = np.load(os.path.join(GOLDEN, "wavelet.npz"))


@pytest.fixture(scope="module")
def dl():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import dithering_lib
    return dithering_lib


@pytest.mark.parametrize("name", [c["name"] for c in WL["cases"]])
def test_matches_reference_fixture(dl, name):
    """dither_frames with the palette the reference used (median cut included) is ImageDitherer.apply_dithering's output."""
    import torch
    case = next(c for c in WL["cases"] if c["name"] == name)
    arr = wr.make_input(case["input"])
    assert sha(arr) == case["input_sha256"]
    s = dl.WaveletDitherStrategy(**case["params"])
    got = s.dither_frames(torch.from_numpy(arr).cuda(), [tuple(c) for c in case["palette"]], case["use_gamma"]).cpu().numpy()
    if case.get("full"):
        assert np.array_equal(got, WL_NPZ["out_" + name])
    assert sha(got) == case["output_sha256"]


@pytest.mark.parametrize("name", [e["name"] for e in WL["strategy"]])
def test_strategy_dither_matches_reference(dl, name):
    ent = next(e for e in WL["strategy"] if e["name"] == name)
    pal = WL_NPZ["st_pal_" + name]
    arr = wr.make_input(ent["input"])
    h, w, _ = arr.shape
    got = dl.WaveletDitherStrategy(**ent["params"]).dither(arr.reshape(-1, 3).astype(np.float32), pal, (h, w))
    assert got.dtype == np.float32 and np.array_equal(got, WL_NPZ["st_out_" + name])


def _fuzz_cases():
    rs = np.random.RandomState(846)
    shapes = [(1, 1), (1, 97), (97, 1), (2, 3), (3, 2), (5, 3), (64, 65), (130, 70)]
    while len(shapes) < 40:
        shapes.append((int(rs.randint(1, 160)), int(rs.randint(1, 160))))
    cases = []
    for i, (h, w) in enumerate(shapes):
        K = int(rs.choice([1, 2, 3, 10, 11, 16, 64, 200, 256, 600, 1024]))
        params = dict(wavelet=str(rs.choice(wr.WAVELETS)), subband_quant=int(rs.choice([1, 2, 3, 8, 16, 32, 33, 100, 65536])),
                      seed=int(rs.choice([0, 42, 9999, rs.randint(1 << 31)])))
        cases.append((i, h, w, K, bool(i % 3 == 1), int(rs.randint(1 << 30)), params))
    return cases


@pytest.mark.parametrize("i,h,w,K,gamma,seed,params", _fuzz_cases())
def test_fuzz_against_cpu_restatement(dl, i, h, w, K, gamma, seed, params):
    import torch
    from oracle import oracle as orc
    arr = orc.rnd(h, w, seed % 100000) if i % 2 else orc.imgl(h, w, seed % 1000)
    if i % 4 == 3:   # a flat channel: its four subbands are constant and draw nothing
        arr = arr.copy()
        arr[..., i % 3] = seed % 256
    if i % 7 == 6:   # a flat image
        arr = np.ascontiguousarray(np.broadcast_to(arr[:1, :1], arr.shape))
    pal = orc.palr(K, seed % 1000)
    if i % 5 == 0 and K > 4:   # duplicated entries: exact ties
        pal = pal[:K // 2] + pal[:K - K // 2]
    want = wr.apply(arr, pal, gamma, WL["taps"], **params)
    got = dl.WaveletDitherStrategy(**params).dither_frames(torch.from_numpy(arr).cuda(), pal, gamma).cpu().numpy()
    assert np.array_equal(got, want), (h, w, K, gamma, params)


def test_batch_equals_single_frames(dl):
    import torch
    from oracle import oracle as orc
    frames = np.stack([orc.rnd(97, 131, s) for s in range(5)] + [orc.imgl(97, 131, 3)])
    frames[2, ..., 1] = 77   # a frame with a flat channel: its stream offsets differ from its neighbours'
    for pal, gamma, params in ((orc.palr(16), False, {}), (orc.palr(300, 5), True, {"wavelet": "sym4", "subband_quant": 5})):
        s = dl.WaveletDitherStrategy(**params)
        batch = s.dither_frames(torch.from_numpy(frames).cuda(), pal, gamma).cpu().numpy()
        for k in range(len(frames)):
            one = s.dither_frames(torch.from_numpy(frames[k]).cuda(), pal, gamma).cpu().numpy()
            assert one.shape == frames[k].shape and np.array_equal(batch[k], one), k
            assert np.array_equal(one, wr.apply(frames[k], pal, gamma, WL["taps"], **params)), k
        out = torch.empty_like(torch.from_numpy(frames)).cuda()
        res = s.dither_frames(torch.from_numpy(frames).cuda(), pal, gamma, out=out)
        assert res.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), batch)


def test_dither_frames_equals_dither(dl):
    import torch
    from oracle import oracle as orc
    arr = orc.imgl(90, 150, 9)
    pal = orc.palr(32, 4)
    s = dl.WaveletDitherStrategy(wavelet="coif1", subband_quant=6, seed=3)
    flat = s.dither(arr.reshape(-1, 3).astype(np.float32), np.array(pal, np.float32), (90, 150))
    dev = s.dither_frames(torch.from_numpy(arr).cuda(), pal).cpu().numpy()
    assert np.array_equal(flat.reshape(90, 150, 3).astype(np.uint8), dev)


def test_stream_cache_reuse_and_eviction(dl, monkeypatch):
    import torch
    from dither_pie_amd import backend
    from oracle import oracle as orc
    backend._WL_STREAMS.clear()
    arr = torch.from_numpy(orc.imgl(40, 60, 2)).cuda()
    pal = orc.palr(16)
    s = dl.WaveletDitherStrategy(wavelet="db2", seed=5)
    first = s.dither_frames(arr, pal).cpu().numpy()
    assert len(backend._WL_STREAMS) == 1
    u = next(iter(backend._WL_STREAMS.values()))
    need = 12 * ((40 + 3) // 2) * ((60 + 3) // 2) + 40 * 60
    assert u.dtype == torch.float64 and u.numel() == need
    assert np.array_equal(u.cpu().numpy(), np.random.RandomState(5).random_sample(need))
    again = s.dither_frames(arr, pal).cpu().numpy()
    assert np.array_equal(first, again) and len(backend._WL_STREAMS) == 1
    assert next(iter(backend._WL_STREAMS.values())) is u   # reused, not regenerated
    # a byte budget of two small streams: the oldest goes first, the newest always stays
    monkeypatch.setattr(backend, "_WL_STREAMS_BYTES", 2 * need * 8)
    for seed in (6, 7, 8):
        dl.WaveletDitherStrategy(wavelet="db2", seed=seed).dither_frames(arr, pal)
    assert [k[1] for k in backend._WL_STREAMS] == [7, 8]
    monkeypatch.setattr(backend, "_WL_STREAMS_BYTES", 1)
    big = dl.WaveletDitherStrategy(wavelet="db2", seed=9).dither_frames(arr, pal).cpu().numpy()
    assert [k[1] for k in backend._WL_STREAMS] == [9]
    assert np.array_equal(big, wr.apply(orc.imgl(40, 60, 2), pal, False, WL["taps"], wavelet="db2", seed=9))


def test_tiles_short_stream_and_image_ditherer_refused(dl):
    import torch
    from dither_pie_amd import _lib, backend
    from dither_pie_amd._lib import DP_EINVAL
    from oracle import oracle as orc
    s = dl.WaveletDitherStrategy()
    arr = torch.from_numpy(orc.imgl(16, 16, 1)).cuda()
    pal = dl._device_palette(*dl.prepare_palette(orc.palr(8), False))
    with pytest.raises(ValueError):
        s._run(arr, pal, y0=8)
    with pytest.raises(ValueError):
        s._run(arr, pal, x0=3)
    with pytest.raises(NotImplementedError):
        dl.ImageDitherer()._get_dither_strategy(dl.DitherMode.WAVELET)
    # the library refuses a stream one value short, before any launch; the output stays untouched
    L = _lib.load()
    need = L.dp_wavelet_uniforms_needed(16, 16, 0)
    u = torch.rand(need, dtype=torch.float64, device="cuda")
    out = torch.full_like(arr, 7)
    P = backend.WaveletParams(0, 8, u.data_ptr(), need - 1)
    ws = torch.empty(L.dp_wavelet_workspace_bytes(1, 16, 16, C.byref(P)), dtype=torch.uint8, device="cuda")
    rc = L.dp_wavelet_u8(arr.data_ptr(), out.data_ptr(), 1, 16, 16, pal._h, C.byref(P), ws.data_ptr(), ws.numel(), None)
    assert rc == DP_EINVAL and b"stream" in L.dp_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all())
