"""GPU tier: the filtered resize on the device (include/ditherpie_hip_resample.h, backend.resample) against the numpy statement
(tests/resample_ref.py, which tests/test_resample_cpu.py holds against Pillow), byte for byte, for every filter: both passes,
one pass, the copy, upscales, windows that cover the whole row, a batch of different frames, both horizontal kernels and the
32-bit-multiply instance; the video pipeline with a downscale filter against the pipeline assembled by hand from Pillow's resize;
"nearest" against today's output; one graph capture and replay.

The staged horizontal kernel works on blocks of STAGE_ROWS source rows x STAGE_COLS output columns (csrc/host_logic.h:
kResampleStageRows, kResampleStageCols); 130 x 70 -> 66 x 35 has three row blocks (64 + 64 + 2 rows of the intermediate's 130)
and three column groups (16 + 16 + 3).  The planner gives the staged kernel to BICUBIC and LANCZOS plans; BOX, BILINEAR and HAMMING,
and a window wider than a staged row (STAGE_BYTES source bytes: 3 x 400 -> 3 x 2 with LANCZOS), go to the naive kernel.  No real
geometry was found whose coefficients need the 32-bit-multiply instance (max |k| >= 2^23 implies a sum the planner refuses in
all but a sliver of cases), so that instance is reached through the
experiments library's switch DP_RESAMPLE_MUL32=1, and each horizontal kernel on the other's plans through DP_RESAMPLE_H=naive /
staged."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

import resample_ref as rr

pytestmark = pytest.mark.gpu

STAGE_ROWS, STAGE_COLS, STAGE_BYTES = 64, 16, 956

# (h, w, oh, ow, frames)
SHAPES = [
    (37, 53, 8, 10, 1),        # both passes, downscale
    (17, 23, 40, 50, 1),       # both passes, upscale
    (24, 31, 24, 9, 1),        # horizontal only
    (29, 18, 7, 18, 1),        # vertical only
    (21, 19, 21, 19, 2),       # identity: a copy
    (37, 53, 8, 7, 2),         # ow = 7: rows of 21 bytes, two frames
    (8, 8, 1, 1, 1),
    (5, 300, 5, 7, 1),
    (1, 300, 1, 2, 1),         # LANCZOS: the window is the whole row
    (33, 2, 3, 5, 1),
    (130, 70, 66, 35, 1),      # crosses the staged block's row and column boundaries (see the module docstring)
    (3, 400, 3, 2, 1),         # wider than a staged row: the naive horizontal kernel
    (12, 9, 5, 14, 3),         # a three-frame batch whose frames differ
]
PIL_FILTER = {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend
    yield backend
    torch.cuda.synchronize()
    backend.drop_resample_plans()
    torch.cuda.empty_cache()


_REF = {}


def _case(shape, name, kind="noise"):
    """(frames, the statement's output), computed once per (shape, filter, content) and never changed."""
    key = (shape, name, kind)
    if key not in _REF:
        h, w, oh, ow, n = shape
        frames = rr.content(kind, n, h, w, 131 * h + 17 * w + 7 * oh + ow + 1000 * rr.FILTERS.index(name))
        want = rr.resample(frames, oh, ow, name)
        frames.setflags(write=False)
        want.setflags(write=False)
        _REF[key] = (frames, want)
    return _REF[key]


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _check(got, want, label):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert not len(bad), (label, len(bad), bad[:4].tolist())


def test_the_shapes_straddle_the_staged_blocks():
    h, w, oh, ow, _ = SHAPES[10]
    assert (h, w, oh, ow) == (130, 70, 66, 35)
    p = rr.plan("box", h, w, oh, ow)
    rows = p["y1"] - p["y0"]
    assert rows > 2 * STAGE_ROWS and rows % STAGE_ROWS and ow > 2 * STAGE_COLS and ow % STAGE_COLS
    b = rr.coeffs(400, 2, "lanczos")[1]
    assert int(b[-1, 0] + b[-1, 1] - b[0, 0]) * 3 + 3 > STAGE_BYTES        # the naive plan
    b = rr.coeffs(300, 2, "lanczos")[1]
    assert tuple(b[0]) == (0, 300) and int(b[-1, 0] + b[-1, 1] - b[0, 0]) * 3 + 3 <= STAGE_BYTES   # the whole row, staged


@pytest.mark.parametrize("name", rr.FILTERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}x{s[3]}x{s[4]}")
def test_device_equals_the_statement(gpu, shape, name):
    import torch
    be = gpu
    frames, want = _case(shape, name)
    got = be.resample(torch.from_numpy(frames.copy()).cuda(), shape[2], shape[3], name)
    _check(got, want, (shape, name))
    if shape[4] == 3:
        assert (want[0] != want[1]).any() and (want[1] != want[2]).any()
    one = be.resample(torch.from_numpy(frames[0].copy()).cuda(), shape[2], shape[3], name)   # [H, W, 3] in, [H', W', 3] out
    assert one.dim() == 3
    _check(one, want[0], (shape, name, "single"))


@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
def test_overshoot_is_clamped_at_both_ends(gpu, name):
    import torch
    be = gpu
    # pure 0 / 255 through an upscale, a vertical-only and a horizontal-only pass, the staged blocks and a batch (a strong
    # downscale such as 37 x 53 -> 8 x 10 averages the overshoot away: it is not among them)
    for shape in (SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[10], SHAPES[12]):
        frames, want = _case(shape, name, "extremes")
        assert want.min() == 0 and want.max() == 255 and (want == 0).sum() >= 5 and (want == 255).sum() >= 5
        _check(be.resample(torch.from_numpy(frames.copy()).cuda(), shape[2], shape[3], name), want, (shape, name))


@pytest.mark.parametrize("name", rr.FILTERS)
def test_device_equals_pillow_itself(gpu, name):
    import torch
    be = gpu
    frames, _ = _case(SHAPES[0], name)
    got = be.resample(torch.from_numpy(frames.copy()).cuda(), 8, 10, name).cpu().numpy()
    assert np.array_equal(got[0], np.asarray(Image.fromarray(frames[0], "RGB").resize((10, 8), PIL_FILTER[name])))


@pytest.mark.parametrize("env", [{"DP_RESAMPLE_MUL32": "1"}, {"DP_RESAMPLE_H": "naive"}, {"DP_RESAMPLE_H": "staged"},
                                 {"DP_RESAMPLE_MUL32": "1", "DP_RESAMPLE_H": "naive"}, {"DP_RESAMPLE_MUL32": "1", "DP_RESAMPLE_H": "staged"}],
                         ids=["mul32", "naive", "staged", "mul32-naive", "mul32-staged"])
@pytest.mark.parametrize("name", ["box", "lanczos"])
def test_the_other_instances_through_the_switches(gpu, switches, env, name):
    """The 32-bit-multiply instance of every kernel, the naive horizontal kernel on plans that take the staged one (LANCZOS) and
    the staged one on plans that take the naive one (BOX): reached through the experiments library's switches (no real geometry
    asks for the first), same bytes."""
    import torch
    be = gpu
    for k, v in env.items():
        switches.setenv(k, v)
    for shape in (SHAPES[0], SHAPES[1], SHAPES[3], SHAPES[5], SHAPES[10], SHAPES[11], SHAPES[12]):
        frames, want = _case(shape, name)
        _check(be.resample(torch.from_numpy(frames.copy()).cuda(), shape[2], shape[3], name), want, (shape, name, env))
    be.drop_resample_plans()


def test_out_plan_and_refusals_on_the_device(gpu):
    import torch
    be = gpu
    frames, want = _case(SHAPES[0], "hamming")
    dev = torch.from_numpy(frames.copy()).cuda()
    plan = be.ResamplePlan("hamming", 37, 53, 8, 10)
    assert plan.workspace_bytes(1) == rr.workspace_bytes("hamming", 1, 37, 53, 8, 10) and plan.workspace_bytes(0) == 0
    out = torch.zeros((1, 8, 10, 3), dtype=torch.uint8, device="cuda")
    assert be.resample(dev, 8, 10, "hamming", out=out, plan=plan).data_ptr() == out.data_ptr()
    _check(out, want, "out=")
    with pytest.raises(ValueError, match="another filter"):
        be.resample(dev, 8, 10, "box", plan=plan)
    with pytest.raises(ValueError, match="another filter"):
        be.resample(dev, 8, 11, "hamming", plan=plan)
    with pytest.raises(ValueError):
        be.resample(dev, 8, 10, "hamming", out=torch.zeros((1, 8, 11, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        be.resample(dev, 8, 10, "hamming", out=torch.zeros((1, 8, 10, 3), dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError, match="16384"):
        be.resample(dev, 0, 10, "hamming")
    same = torch.from_numpy(_case(SHAPES[4], "box")[0].copy()).cuda()
    with pytest.raises(ValueError, match="in place"):
        be.resample(same, 21, 19, "box", out=same)
    with pytest.raises(ValueError, match="neither out nor plan"):
        be.resample(dev, 8, 10, "nearest", out=out)
    empty = be.resample(torch.zeros((0, 37, 53, 3), dtype=torch.uint8, device="cuda"), 8, 10, "hamming")
    assert tuple(empty.shape) == (0, 8, 10, 3)
    a = be._resample_plan(dev.device, "box", 37, 53, 8, 10)
    assert be._resample_plan(dev.device, "box", 37, 53, 8, 10) is a and be._resample_plan(dev.device, "box", 37, 53, 8, 11) is not a   # the cache


def test_nearest_is_todays_resize(gpu):
    import torch
    be = gpu
    frames, _ = _case(SHAPES[12], "box")
    dev = torch.from_numpy(frames.copy()).cuda()
    want = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((14, 5), Image.NEAREST)) for f in frames])
    assert np.array_equal(be.resample(dev, 5, 14, "nearest").cpu().numpy(), want)
    assert torch.equal(be.resample(dev, 5, 14, "nearest"), be.resize_nearest(dev, 5, 14))
    assert torch.equal(be.resample(dev[0], 5, 14, "nearest"), be.resize_nearest(dev[0], 5, 14))


# ---------------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("name", rr.FILTERS)
def test_process_frames_equals_the_pipeline_assembled_by_hand(gpu, orc, name):
    """process_frames(..., downscale_filter=f) = Pillow's resize of every frame with that filter to the pixelization geometry, then
    apply_dithering_frames, then the NEAREST enlargement; the indexed and the PNG variants give the same pixels."""
    import io
    import torch
    from dither_pie_amd import dithering_lib as d, video_processor as vp
    be = gpu
    frames = np.stack([orc.rnd(101, 67, 40 + i) for i in range(3)])
    dev = torch.from_numpy(frames).cuda()
    dith = d.ImageDitherer(16, d.DitherMode.BAYER, orc.generate_uniform_palette(16), False, {"size": "4x4"})
    tw, th = vp._even_dimensions(67, 101, 17)
    assert (th, tw) == (24, 16)
    small = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((tw, th), PIL_FILTER[name])) for f in frames])
    dithered = dith.apply_dithering_frames(torch.from_numpy(small).cuda())
    want = be.resize_nearest(dithered, 2 * th, 2 * tw).cpu().numpy()
    got = vp.process_frames(dev, dith, "regular", 17, 2, downscale_filter=name)
    assert tuple(got.shape) == (3,) + vp.output_size(101, 67, "regular", 17, 2) + (3,)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(vp.process_frames(dev, dith, "regular", 17, None, downscale_filter=name).cpu().numpy(), dithered.cpu().numpy())
    planes, colours = vp.process_frames_indexed(dev, dith, "regular", 17, 2, downscale_filter=name)
    assert np.array_equal(_np(colours)[_np(planes).astype(np.int64)], want)
    files = vp.process_frames_png(dev, dith, "regular", 17, 2, downscale_filter=name)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[1])).convert("RGB")), want[1])
    img = vp.pixelize_regular(Image.fromarray(frames[0], "RGB"), 17, resample=name)
    assert np.array_equal(np.asarray(img), small[0])
    # without pixelization the filter has nothing to do
    assert torch.equal(vp.process_frames(dev, dith, None, 17, None, downscale_filter=name), vp.process_frames(dev, dith))


def test_nearest_keeps_every_output_byte(gpu, orc):
    import torch
    from dither_pie_amd import dithering_lib as d, video_processor as vp
    be = gpu
    frames = np.stack([orc.rnd(101, 67, 50 + i) for i in range(2)])
    dev = torch.from_numpy(frames).cuda()
    dith = d.ImageDitherer(16, d.DitherMode.BAYER, orc.generate_uniform_palette(16), False, {"size": "4x4"})
    small = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((16, 24), Image.NEAREST)) for f in frames])
    want = be.resize_nearest(dith.apply_dithering_frames(torch.from_numpy(small).cuda()), 48, 32)
    for kw in ({}, {"downscale_filter": "nearest"}):
        assert torch.equal(vp.process_frames(dev, dith, "regular", 17, 2, **kw), want)
        planes, colours = vp.process_frames_indexed(dev, dith, "regular", 17, 2, **kw)
        assert np.array_equal(_np(colours)[_np(planes).astype(np.int64)], want.cpu().numpy())
    for kw in ({}, {"resample": "nearest"}):
        assert np.array_equal(np.asarray(vp.pixelize_regular(Image.fromarray(frames[0], "RGB"), 17, **kw)), small[0])
    assert (vp.process_frames(dev, dith, "regular", 17, 2, downscale_filter="box") != want).any()    # ... and the filter is not a no-op


# ---------------------------------------------------------------------------------------------------- capture
def test_capture_and_replay(gpu):
    """dp_resample_u8 only launches: with the plan and the workspace made beforehand, a call is captured into a graph -- a linear
    graph of two launches, horizontal then vertical, on one stream -- and the replay gives the statement's bytes, also for new
    input."""
    import torch
    from dither_pie_amd import _lib
    be = gpu
    shape = (37, 53, 8, 7, 2)
    frames, want = _case(shape, "lanczos")
    plan = be.ResamplePlan("lanczos", 37, 53, 8, 7)                       # the blocking upload happens here, not in the capture
    need = plan.workspace_bytes(2)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    dev = torch.from_numpy(frames.copy()).cuda()
    out = torch.zeros((2, 8, 7, 3), dtype=torch.uint8, device="cuda")
    L = _lib.load()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a = _lib.ResampleArgs(C.sizeof(_lib.ResampleArgs), dev.data_ptr(), out.data_ptr(), 2, plan._h.value, ws.data_ptr(), need,
                              torch.cuda.current_stream().cuda_stream)
        rc = L.dp_resample_u8(C.byref(a))
    assert rc == 0, L.dp_last_error()
    torch.cuda.synchronize()
    assert not bool(out.any())                                           # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    dev.copy_(torch.from_numpy(frames[::-1].copy()).cuda())              # new input, the same graph
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[::-1])
    del g
