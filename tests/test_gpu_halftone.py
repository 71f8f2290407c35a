"""GPU tier of halftone dithering (halftone.hip on the product library): bit equality with the reference's recorded
outputs (tests/golden/halftone.*), a seeded fuzz against the CPU restatement (tests/halftone_ref.py), batches, the
device-batch entry, the pow class's host fix-up, the geometry cache and the refusal of tiles."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import halftone_ref
from test_halftone_cpu import ht_input

pytestmark = pytest.mark.gpu


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


with open(os.path.join(GOLDEN, "halftone.json")) as _fh:
    HT = json.load(_fh)
HT_NPZ = np.load(os.path.join(GOLDEN, "halftone.npz"))


@pytest.fixture(scope="module")
def dl():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import dithering_lib
    return dithering_lib


@pytest.mark.parametrize("name", [c["name"] for c in HT["cases"]])
def test_matches_reference_fixture(dl, name):
    """dither_frames with the palette the reference used (median cut included) is ImageDitherer.apply_dithering's output."""
    import torch
    case = next(c for c in HT["cases"] if c["name"] == name)
    arr = ht_input(case["input"])
    assert sha(arr) == case["input_sha256"]
    s = dl.HalftoneDitherStrategy(**dict(halftone_ref.DEFAULTS, **case["params"]))
    got = s.dither_frames(torch.from_numpy(arr).cuda(), [tuple(c) for c in case["palette"]], case["use_gamma"]).cpu().numpy()
    if case.get("full"):
        assert np.array_equal(got, HT_NPZ["out_" + name])
    assert sha(got) == case["output_sha256"]


@pytest.mark.parametrize("name", [e["name"] for e in HT["strategy"]])
def test_strategy_dither_matches_reference(dl, name):
    ent = next(e for e in HT["strategy"] if e["name"] == name)
    pal = HT_NPZ["st_pal_" + name]
    arr = ht_input(ent["input"])
    h, w, _ = arr.shape
    got = dl.HalftoneDitherStrategy(**ent["params"]).dither(arr.reshape(-1, 3).astype(np.float32), pal, (h, w))
    assert got.dtype == np.float32 and np.array_equal(got, HT_NPZ["st_out_" + name])


def _fuzz_cases():
    rs = np.random.RandomState(1498)
    shapes = [(1, 1), (1, 97), (97, 1), (2, 3), (64, 65), (130, 70)]
    while len(shapes) < 40:
        shapes.append((int(rs.randint(1, 200)), int(rs.randint(1, 200))))
    cases = []
    for i, (h, w) in enumerate(shapes):
        K = int(rs.choice([1, 2, 3, 10, 11, 16, 64, 200, 256, 600, 1024]))
        params = dict(cell_size=float(rs.choice([1, 2, 2.5, 3, 5, 7.5, 8, 13, 32, 50])),
                      angle=float(rs.choice([0.0, 15.0, 30.0, 45.0, 60.0, 90.0, 135.0, -30.0, 200.0, rs.uniform(-90, 360)])),
                      dot_gain=float(rs.choice([0.5, 1.0, 2.0, 1.5, 3.0, rs.uniform(0.5, 3.0)])),
                      min_dot_size=float(rs.choice([0.0, 0.0, 0.1, 0.3])), max_dot_size=float(rs.choice([1.0, 1.0, 0.8, 0.6])),
                      shape=str(rs.choice(["circle", "square", "diamond", "hexagon"])),
                      sharpness=float(rs.choice([1.0, 1.5, 0.5, 4.0, rs.uniform(0.5, 4.0)])))
        cases.append((i, h, w, K, bool(i % 3 == 1), int(rs.randint(1 << 30)), params))
    return cases


@pytest.mark.parametrize("i,h,w,K,gamma,seed,params", _fuzz_cases())
def test_fuzz_against_cpu_restatement(dl, i, h, w, K, gamma, seed, params):
    import torch
    from oracle import oracle as orc
    arr = orc.rnd(h, w, seed % 100000) if i % 2 else orc.imgl(h, w, seed % 1000)
    pal = orc.palr(K, seed % 1000)
    if i % 5 == 0 and K > 4:   # duplicated entries: exact ties
        pal = pal[:K // 2] + pal[:K - K // 2]
    want = halftone_ref.apply(arr, pal, gamma, **params)
    got = dl.HalftoneDitherStrategy(**params).dither_frames(torch.from_numpy(arr).cuda(), pal, gamma).cpu().numpy()
    assert np.array_equal(got, want), (h, w, K, gamma, params)


def test_batch_equals_single_frames(dl):
    import torch
    from oracle import oracle as orc
    frames = np.stack([orc.rnd(97, 131, s) for s in range(5)] + [orc.imgl(97, 131, 3)])
    for pal, gamma, params in ((orc.palr(16), False, {}), (orc.palr(300, 5), True, {"cell_size": 3, "dot_gain": 1.5})):
        s = dl.HalftoneDitherStrategy(**params)
        batch = s.dither_frames(torch.from_numpy(frames).cuda(), pal, gamma).cpu().numpy()
        for k in range(len(frames)):
            one = s.dither_frames(torch.from_numpy(frames[k]).cuda(), pal, gamma).cpu().numpy()
            assert one.shape == frames[k].shape and np.array_equal(batch[k], one), k
            assert np.array_equal(one, halftone_ref.apply(frames[k], pal, gamma, **params)), k
        out = torch.empty_like(torch.from_numpy(frames)).cuda()
        res = s.dither_frames(torch.from_numpy(frames).cuda(), pal, gamma, out=out)
        assert res.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), batch)


def test_dither_frames_equals_dither(dl):
    import torch
    from oracle import oracle as orc
    arr = orc.imgl(90, 150, 9)
    pal = orc.palr(32, 4)
    s = dl.HalftoneDitherStrategy(cell_size=6, angle=30.0, dot_gain=1.5, shape="square")
    flat = s.dither(arr.reshape(-1, 3).astype(np.float32), np.array(pal, np.float32), (90, 150))
    dev = s.dither_frames(torch.from_numpy(arr).cuda(), pal).cpu().numpy()
    assert np.array_equal(flat.reshape(90, 150, 3).astype(np.uint8), dev)


POW_PARAMS = dict(cell_size=8, angle=45.0, dot_gain=2.5, min_dot_size=0.0, max_dot_size=1.0, shape="circle", sharpness=4.0)
POW_H, POW_W, POW_PIXEL = 200, 256, 47940


def _chain32(p, params):
    t = params["min_dot_size"] + p * (params["max_dot_size"] - params["min_dot_size"])
    t = 0.5 + (t - 0.5) * params["sharpness"]
    return np.clip(t, 0.0, 1.0).astype(np.float32)


def test_pow_class_host_fixup_is_exact(dl):
    """A geometry whose pow thresholds need the host: pixel 47940 of 200 x 256 (cell 8, 45 deg, dot_gain 2.5, sharpness 4).
    Its np.power value lies within 8 float64 ulps of a float32 rounding boundary of the chain after pow (checked below on the
    host), so the device, which flags a pixel when the chain rounds differently 64 ulps below and above its own pow, must
    list it; the list's thresholds are np.power's, and the whole output equals the restatement."""
    import torch
    from dither_pie_amd import backend
    from oracle import oracle as orc
    params = POW_PARAMS
    y, x = divmod(POW_PIXEL, POW_W)
    a = np.radians(params["angle"])
    xr, yr = x * np.cos(a) - y * np.sin(a), x * np.sin(a) + y * np.cos(a)
    dx, dy = (xr % 8) / 8 - 0.5, (yr % 8) / 8 - 0.5
    p = np.power(np.clip(np.sqrt(dx ** 2 + dy ** 2) / 0.5, 0.0, 1.0), 1.0 / params["dot_gain"])
    b = np.array([p]).view(np.int64)[0]
    ends = np.array([b - 8, b + 8], np.int64).view(np.float64)
    assert _chain32(ends[0], params) != _chain32(ends[1], params)   # the premise: a boundary within 8 ulps
    P = backend.halftone_params(np.zeros((2, 3), np.float32), **params)
    assert P.exp_class == backend.HT_EXP_POW
    idx, thr = backend.halftone_fixups(torch.device("cuda", torch.cuda.current_device()), POW_H, POW_W, P)
    ids = idx.cpu().numpy()
    assert POW_PIXEL in ids and np.all(np.diff(ids) > 0)
    scr, _ = halftone_ref.screen_with_cells(POW_H, POW_W, **params)
    assert np.array_equal(thr.cpu().numpy().view(np.uint32), scr.ravel()[ids].view(np.uint32))
    arr = orc.imgl(POW_H, POW_W, 5)
    pal = orc.palr(16, 2)
    got = dl.HalftoneDitherStrategy(**params).dither_frames(torch.from_numpy(arr).cuda(), pal).cpu().numpy()
    assert np.array_equal(got, halftone_ref.apply(arr, pal, **params))


def test_ink_pass_takes_thresholds_from_the_fixup_list(dl):
    """The ink kernel reads the caller's list for exactly the pixels it flags.  A black frame and a black / white palette:
    every pixel whose threshold is below 1 is inked black, the rest stay paper white.  A forged list that gives every
    flagged pixel the threshold 1.0 must turn exactly those pixels white; an unflagged pixel on the same list keeps the
    device's own threshold (the list only settles what the device cannot decide)."""
    import ctypes as C
    import torch
    from dither_pie_amd import _lib, backend
    params = POW_PARAMS
    pal = dl._device_palette(*dl.prepare_palette([(0, 0, 0), (255, 255, 255)], False))
    P = backend.halftone_params(pal.pal_f32, **params)
    assert P.paper_idx == 1
    dev = torch.device("cuda", torch.cuda.current_device())
    flagged = backend.halftone_fixups(dev, POW_H, POW_W, P)[0].cpu().numpy()
    assert POW_PIXEL in flagged
    x = torch.zeros((1, POW_H, POW_W, 3), dtype=torch.uint8, device=dev)
    normal = backend.halftone(x, pal, params).cpu().numpy().reshape(-1, 3)
    scr, _ = halftone_ref.screen_with_cells(POW_H, POW_W, **params)
    assert np.array_equal(normal[:, 0] == 0, scr.ravel() < 1.0)
    inked = np.nonzero(normal[:, 0] == 0)[0]
    extra = int(next(i for i in inked if i not in set(flagged.tolist())))   # inked, not flagged
    forged_ids = np.sort(np.append(flagged, extra)).astype(np.int32)
    fi = torch.from_numpy(forged_ids).to(dev)
    ft = torch.ones(len(forged_ids), dtype=torch.float32, device=dev)
    P.fix_idx_dev, P.fix_thr_dev, P.n_fix = fi.data_ptr(), ft.data_ptr(), len(forged_ids)
    L = _lib.load()
    ws = torch.empty(L.dp_halftone_workspace_bytes(1, POW_H, POW_W, C.byref(P)), dtype=torch.uint8, device=dev)
    y = torch.empty_like(x)
    _lib.check(L.dp_halftone_u8(x.data_ptr(), y.data_ptr(), 1, POW_H, POW_W, pal._h, C.byref(P), ws.data_ptr(), ws.numel(),
                                backend._stream()))
    forged = y.cpu().numpy().reshape(-1, 3)
    changed = np.nonzero(np.any(forged != normal, axis=1))[0]
    assert POW_PIXEL in changed and np.array_equal(forged[changed], np.full((len(changed), 3), 255, np.uint8))
    assert np.array_equal(changed, np.intersect1d(flagged, inked))
    assert extra not in changed


def test_cached_geometry_second_call_equals_first(dl):
    import torch
    from oracle import oracle as orc
    arr = torch.from_numpy(np.stack([orc.imgl(150, 210, 7), orc.rnd(150, 210, 8)])).cuda()
    pal = orc.palr(64, 6)
    for params in ({}, {"dot_gain": 1.7, "sharpness": 3.0, "angle": 22.0}):
        s = dl.HalftoneDitherStrategy(**params)
        first = s.dither_frames(arr, pal).cpu().numpy()
        second = s.dither_frames(arr, pal).cpu().numpy()
        assert np.array_equal(first, second)
        assert np.array_equal(first[1], halftone_ref.apply(arr[1].cpu().numpy(), pal, **params))


def test_tiles_are_refused_and_image_ditherer_still_refuses(dl):
    import torch
    from PIL import Image
    from oracle import oracle as orc
    x = torch.from_numpy(orc.rnd(32, 48, 1)).cuda()
    s = dl.HalftoneDitherStrategy()
    pal = dl._device_palette(*dl.prepare_palette(orc.palr(16), False))
    with pytest.raises(ValueError):
        s._run(x.unsqueeze(0), pal, y0=4)
    with pytest.raises(NotImplementedError):
        dl.ImageDitherer(16, dl.DitherMode.HALFTONE, orc.palr(16)).apply_dithering(Image.fromarray(orc.rnd(8, 8, 1)))
