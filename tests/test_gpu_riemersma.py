"""GPU tier of the Riemersma mode (riemersma.hip on the product library): bit equality with the reference's recorded outputs
(tests/golden/riemersma.*), a seeded fuzz against the CPU restatement (tests/riemersma_ref.py), batches, the video path
and the refusals."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import riemersma_ref
from test_riemersma_cpu import rm_input

pytestmark = pytest.mark.gpu


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


with open(os.path.join(GOLDEN, "riemersma.json")) as _fh:
    RM = json.load(_fh)
RM_NPZ = np.load(os.path.join(GOLDEN, "riemersma.npz"))


@pytest.fixture(scope="module")
def dl():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import dithering_lib
    return dithering_lib


@pytest.mark.parametrize("name", [c["name"] for c in RM["cases"]])
def test_matches_reference_fixture(dl, name):
    from PIL import Image
    case = next(c for c in RM["cases"] if c["name"] == name)
    arr = rm_input(case["input"])
    assert sha(arr) == case["input_sha256"]
    pal = None if case["palette_spec"][0] == "none" else [tuple(c) for c in case["palette"]]
    it = dl.ImageDitherer(case["num_colors"], dl.DitherMode.RIEMERSMA, pal, case["use_gamma"])
    got = np.array(it.apply_dithering(Image.fromarray(arr)))
    if pal is None:   # median cut of the image, as the reference chose it
        assert [list(c) for c in it.palette] == case["palette"]
    if case.get("full"):
        assert np.array_equal(got, RM_NPZ["out_" + name])
    assert sha(got) == case["output_sha256"]


def _fuzz_cases():
    rs = np.random.RandomState(2024)
    shapes = [(1, 1), (1, 2), (2, 1), (1, 257), (256, 1), (3, 200), (200, 3), (256, 256), (255, 129), (65, 64)]
    while len(shapes) < 40:
        h, w = int(rs.randint(1, 257)), int(rs.randint(1, 257))
        if h * w > 40000:
            continue
        shapes.append((h, w))
    cases = []
    for i, (h, w) in enumerate(shapes):
        K = int(rs.choice([1, 2, 3, 8, 16, 17, 63, 64, 65, 200, 256, 257, 600, 1024])) if i % 3 else int(rs.randint(1, 1025))
        cases.append((i, h, w, K, bool(i % 2), int(rs.randint(1 << 30))))
    return cases


@pytest.mark.parametrize("i,h,w,K,gamma,seed", _fuzz_cases())
def test_fuzz_against_cpu_restatement(dl, i, h, w, K, gamma, seed):
    import torch
    from oracle import oracle as orc
    arr = orc.rnd(h, w, seed % 100000) if i % 4 else orc.imgl(h, w, seed % 1000)
    pal = orc.palr(K, seed % 1000)
    if i % 5 == 0 and K > 4:   # duplicated entries: exact ties everywhere
        pal = pal[:K // 2] + pal[:K - K // 2]
    want = riemersma_ref.apply(arr, pal, gamma)
    it = dl.ImageDitherer(K, dl.DitherMode.RIEMERSMA, pal, gamma)
    got = it.apply_dithering_frames(torch.from_numpy(arr).cuda()).cpu().numpy()
    assert np.array_equal(got, want), (h, w, K, gamma)


def test_batch_equals_single_frames(dl):
    import torch
    from oracle import oracle as orc
    frames = np.stack([orc.rnd(97, 131, s) for s in range(5)] + [orc.imgl(97, 131, 3)])
    for pal, gamma in ((orc.palr(16), False), (orc.palr(300, 5), True)):
        it = dl.ImageDitherer(len(pal), dl.DitherMode.RIEMERSMA, pal, gamma)
        batch = it.apply_dithering_frames(torch.from_numpy(frames).cuda()).cpu().numpy()
        for k in range(len(frames)):
            one = it.apply_dithering_frames(torch.from_numpy(frames[k]).cuda()).cpu().numpy()
            assert np.array_equal(batch[k], one), k
        out = torch.empty_like(torch.from_numpy(frames)).cuda()
        res = it.apply_dithering_frames(torch.from_numpy(frames).cuda(), out=out)
        assert res.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), batch)


def test_video_path_equals_per_frame(dl):
    import torch
    from dither_pie_amd import video_processor as vp
    from oracle import oracle as orc
    frames = np.stack([orc.imgl(72, 120, s) for s in range(4)])
    it = dl.ImageDitherer(32, dl.DitherMode.RIEMERSMA, orc.palr(32))
    got = vp.process_frames(torch.from_numpy(frames).cuda(), it).cpu().numpy()
    for k in range(len(frames)):
        assert np.array_equal(got[k], riemersma_ref.apply(frames[k], orc.palr(32)))


def test_tiles_and_bands_are_refused(dl):
    import torch
    from dither_pie_amd import sharding
    from oracle import oracle as orc
    it = dl.ImageDitherer(16, dl.DitherMode.RIEMERSMA, orc.palr(16))
    x = torch.from_numpy(orc.rnd(32, 48, 1)).cuda()
    with pytest.raises(ValueError):
        it.apply_dithering_frames(x.unsqueeze(0), y0=4)
    with pytest.raises(ValueError):
        sharding.dither_band(it, x[8:16], 8)
