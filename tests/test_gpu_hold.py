"""GPU tier of the temporal hold (include/ditherpie_hip_hold.h, csrc/hold.hip): the kernel against the numpy statement
(tests/hold_ref.py), bit for bit in out, refreshed and the state, on the cases of the CPU tier, on widths and heights around a
lane's run and a tile's edges for every cell size, on buffers at byte offsets 1, 2 and 3, for one frame and for none; HoldStream
makes batching invisible and reset() starts over; and end to end: files written by process_video_gif and process_video_apng with
`hold` decode to the statement applied to process_frames_indexed's planes, keep their static half and are no larger than the files
without it."""
import io

import numpy as np
import pytest

import hold_ref as hr
import scene_ref as sr
from conftest import fake_ffmpeg_tools

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    return torch


@pytest.fixture(scope="module")
def be(T):
    from dither_pie_amd import backend
    return backend


def _at_offset(T, a, off):
    """The array on the device at a base address = off (mod 4): a view into a larger byte buffer."""
    a = np.ascontiguousarray(a, np.uint8)
    buf = T.empty(a.size + 8, dtype=T.uint8, device="cuda")
    start = (off - buf.data_ptr()) % 4
    view = buf[start:start + a.size].view(a.shape)
    view.copy_(T.from_numpy(a))
    assert view.data_ptr() % 4 == off
    return view


def _run(T, be, src, planes, state, cell, tol, share256, off=0):
    """be.hold on device copies at base addresses = off (mod 4) -> numpy (out, refreshed, state)"""
    n, h, w = planes.shape
    st = None if state is None else (_at_offset(T, state[0], off), _at_offset(T, state[1], off))
    room = T.full((n * h * w + 8,), 0xA5, dtype=T.uint8, device="cuda")
    start = (off - room.data_ptr()) % 4
    out = room[start:start + n * h * w]
    got, refreshed, st2 = be.hold(_at_offset(T, src, off), _at_offset(T, planes, off), st, cell, tol, share256, out=out)
    assert got.data_ptr() == out.data_ptr() and refreshed.dtype == T.int64 and refreshed.is_cuda
    if st is not None:
        assert st2[0].data_ptr() == st[0].data_ptr() and st2[1].data_ptr() == st[1].data_ptr()      # updated in place
    T.cuda.synchronize()
    assert (room[:start] == 0xA5).all() and (room[start + n * h * w:] == 0xA5).all()
    return got.cpu().numpy(), refreshed.cpu().numpy(), (st2[0].cpu().numpy(), st2[1].cpu().numpy())


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:4].tolist())
    assert got[1].tolist() == want[1].tolist(), what
    assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[2][1], want[2][1]), what


@pytest.mark.parametrize("case", hr.CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_equals_the_statement_on_the_cases(T, be, case):
    n, h, w, cell, tol, share256 = case
    src, planes = hr.clip(n, h, w, cell, tol, 100 + hr.CASES.index(case))
    want = hr.hold(src, planes, None, cell, tol, share256)
    for off in (0, 1, 2, 3):
        _same(_run(T, be, src, planes, None, cell, tol, share256, off), want, (case, off))
    more = (np.ascontiguousarray(src[::-1]), np.ascontiguousarray(planes[::-1]))         # and on from the state it left
    want2 = hr.hold(*more, want[2], cell, tol, share256)
    for off in (0, 3):
        _same(_run(T, be, *more, want[2], cell, tol, share256, off), want2, (case, "state", off))


@pytest.mark.parametrize("h", [1, 15, 17])
@pytest.mark.parametrize("w", [1, 3, 5, 63, 65, 4, 64, 68])            # around a run and a tile; the last three take the dword instance
def test_kernel_on_widths_and_heights_around_runs_and_tiles(T, be, h, w):
    for cell in hr.CELLS:
        tol, share256 = (0, 0) if cell == 1 else (3, (0, 64, 128, 256)[(cell + h) % 4])
        src, planes = hr.clip(3, h, w, cell, tol, 7 * h + w + cell)
        want = hr.hold(src, planes, None, cell, tol, share256)
        _same(_run(T, be, src, planes, None, cell, tol, share256), want, (h, w, cell))
        _same(_run(T, be, src[:1], planes[:1], want[2], cell, tol, share256, 1 if w % 2 else 0),      # N = 1, with state
              hr.hold(src[:1], planes[:1], want[2], cell, tol, share256), (h, w, cell, "one"))


def test_one_frame_and_no_frame(T, be):
    src, planes = hr.clip(2, 19, 36, 8, 4, 12)
    _same(_run(T, be, src[:1], planes[:1], None, 8, 4, 16), hr.hold(src[:1], planes[:1], None, 8, 4, 16), "N = 1")
    # N = 0 touches nothing: neither a given state nor a given out, and there is no state to return without one
    anchor, held = T.full((19, 36, 3), 7, dtype=T.uint8, device="cuda"), T.full((19, 36), 9, dtype=T.uint8, device="cuda")
    empty_src, empty_planes = T.from_numpy(src[:0]).cuda(), T.from_numpy(planes[:0]).cuda()
    out, refreshed, state = be.hold(empty_src, empty_planes, (anchor, held), 8, 4, 16)
    T.cuda.synchronize()
    assert tuple(out.shape) == (0, 19, 36) and tuple(refreshed.shape) == (0,) and refreshed.dtype == T.int64
    assert state[0] is anchor and state[1] is held and (anchor == 7).all() and (held == 9).all()
    assert be.hold(empty_src, empty_planes, None, 8, 4, 16)[2] is None
    from dither_pie_amd import _lib
    import ctypes as C
    a = _lib.HoldArgs(C.sizeof(_lib.HoldArgs), None, None, 0, 19, 36, 8, 4, 16, anchor.data_ptr(), held.data_ptr(), 1, None, None, be._stream().value)
    assert _lib.load().dp_hold_u8(C.byref(a)) == 0
    T.cuda.synchronize()
    assert (anchor == 7).all() and (held == 9).all()


def test_wrapper_checks(T, be):
    src, planes = (T.from_numpy(a).cuda() for a in hr.clip(2, 8, 12, 8, 4, 3))
    with pytest.raises(ValueError, match="256 colours"):
        be.hold(src, planes.to(T.int16), None, 8, 4, 16)
    with pytest.raises(ValueError, match="in place"):
        be.hold(src, planes, None, 8, 4, 16, out=planes)
    with pytest.raises(ValueError):
        be.hold(src, planes[:1], None, 8, 4, 16)
    with pytest.raises(ValueError):
        be.hold(src, planes, None, 3, 4, 16)
    with pytest.raises(TypeError):
        be.hold(src.cpu(), planes, None, 8, 4, 16)
    with pytest.raises(ValueError):
        be.hold(src, planes, (T.zeros((8, 12, 3), dtype=T.uint8, device="cuda"), T.zeros((8, 11), dtype=T.uint8, device="cuda")), 8, 4, 16)


def test_hold_stream_makes_batching_invisible(T, be):
    cell, tol, share = 8, 4, 1 / 16
    src, planes = hr.clip(6, 21, 70, cell, tol, 31)
    want = hr.hold(src, planes, None, cell, tol, 16)
    dsrc, dplanes = T.from_numpy(src).cuda(), T.from_numpy(planes).cuda()
    one = be.HoldStream(cell=cell, tol=tol, share=share)
    assert one.settings == (8, 4, 16) and be.HoldStream().settings == (8, 4, 16)              # the defaults
    assert be.HoldStream(cell=2, tol=0, share=0.3).settings == (2, 0, 77) and be.HoldStream(share=7).settings[2] == 256
    out, refreshed = one.add(dsrc, dplanes)
    _same((out.cpu().numpy(), refreshed.cpu().numpy(), (one.anchor.cpu().numpy(), one.held.cpu().numpy())), want, "one call")
    cut = be.HoldStream(cell=cell, tol=tol, share=share)
    parts = [cut.add(dsrc[a:b], dplanes[a:b]) for a, b in ((0, 1), (1, 3), (3, 6))]             # 1 + 2 + 3
    got = (T.cat([p[0] for p in parts]).cpu().numpy(), T.cat([p[1] for p in parts]).cpu().numpy(), (cut.anchor.cpu().numpy(), cut.held.cpu().numpy()))
    _same(got, want, "1 + 2 + 3")
    # an empty batch: empty tensors, the state untouched
    out, refreshed = cut.add(dsrc[:0], dplanes[:0])
    assert tuple(out.shape) == (0, 21, 70) and tuple(refreshed.shape) == (0,) and refreshed.dtype == T.int64
    assert np.array_equal(cut.held.cpu().numpy(), want[2][1])
    # another geometry without reset() is refused; two-byte planes name the limit
    with pytest.raises(ValueError, match="reset"):
        cut.add(dsrc[:, :20], dplanes[:, :20])
    with pytest.raises(ValueError, match="256 colours"):
        cut.add(dsrc, dplanes.to(T.int16))
    # reset() mid-stream: the next frame refreshes everywhere, as the first of a stream does
    cut.reset()
    out, refreshed = cut.add(dsrc[2:5, :20].contiguous(), dplanes[2:5, :20].contiguous())      # (and the geometry may change now)
    want = hr.hold(src[2:5, :20], planes[2:5, :20], None, cell, tol, 16)
    _same((out.cpu().numpy(), refreshed.cpu().numpy(), (cut.anchor.cpu().numpy(), cut.held.cpu().numpy())), want, "after reset")
    assert int(refreshed[0]) == 20 * 70


# ---------------------------------------------------------------------------------------------------- end to end
H, W, N, BATCH = 48, 64, 12, 5
PALETTE = [(0, 0, 0), (255, 255, 255), (200, 30, 30), (30, 200, 30), (30, 30, 200), (220, 220, 40), (40, 220, 220), (220, 40, 220), (128, 128, 128),
           (64, 64, 64), (192, 192, 192), (128, 64, 0), (0, 128, 64), (64, 0, 128), (250, 150, 100), (100, 150, 250)]
HOLD = (8, 4, 1 / 16)                                                   # cell, tol, share: the defaults


def _clip():
    """12 frames of 48 x 64: a fixed smooth image plus noise of at most 2 per channel (half of tol), and a block of 12 x 12 that
    moves through the right half and changes its content every frame.  The left half is static up to the noise."""
    rs = np.random.RandomState(17)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([40 + x * 3, 30 + y * 4, 60 + (x + y) * 2], axis=-1)
    frames = []
    for t in range(N):
        f = base + rs.randint(-2, 3, (H, W, 3))
        f[4 + 2 * t:16 + 2 * t, 36 + t:48 + t] = rs.randint(0, 256, (12, 12, 3))
        frames.append(np.clip(f, 0, 255).astype(np.uint8))
    return np.stack(frames)


def _ditherer(kind):
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer, IntegerErrorDiffusionDitherStrategy
    if kind == "bayer":
        return ImageDitherer(16, DitherMode.BAYER, list(PALETTE), dither_params={"size": "4x4"})
    return ImageDitherer(16, IntegerErrorDiffusionDitherStrategy("floyd_steinberg"), list(PALETTE))


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    frames = []
    for i in range(im.n_frames):
        im.seek(i)
        frames.append(np.asarray(im.convert("RGB")).copy())
    return frames


def _expected(T, be, frames, d, hold):
    """The statement applied to process_frames_indexed's planes, enlarged as the pipeline enlarges them -> RGB [N, 2H, 2W, 3]"""
    from dither_pie_amd.video_processor import process_frames_indexed
    planes, colours = process_frames_indexed(T.from_numpy(frames).cuda(), d, None, 64, None)
    cell, tol, share = hold
    held, refreshed, _ = hr.hold(frames, planes.cpu().numpy(), None, cell, tol, int(round(share * 256)))
    big = be.resize_nearest_plane(T.from_numpy(held).cuda(), 2 * frames.shape[1], 2 * frames.shape[2]).cpu().numpy()
    return np.asarray(colours, np.uint8)[big], refreshed


@pytest.fixture
def video(T, tmp_path, monkeypatch):
    from dither_pie_amd.video_processor import VideoProcessor
    frames = _clip()
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(VideoProcessor, "PIPE_SLOT_BYTES", BATCH * H * W * 3)      # 12 frames: 5 + 5 + 2, the state crosses batches
    return frames, VideoProcessor(devices=[0]), tmp_path


def test_gif_with_an_identity_hold_is_the_file_without(video):
    frames, vp, tmp = video
    d = _ditherer("bayer")
    assert vp.process_video_gif("in.mp4", str(tmp / "plain.gif"), d, None, 64, 2) == N
    assert vp.process_video_gif("in.mp4", str(tmp / "held.gif"), d, None, 64, 2, hold=(1, 0, 0)) == N
    assert vp.last_scan_stats["batch_frames"] == BATCH
    assert (tmp / "held.gif").read_bytes() == (tmp / "plain.gif").read_bytes()


def test_gif_with_hold_decodes_to_the_statement_and_keeps_the_static_half(T, be, video):
    frames, vp, tmp = video
    d = _ditherer("fs")
    want, refreshed = _expected(T, be, frames, d, HOLD)
    # the cells the block covers and those it has just left (at most 4 x 4 of them each), never the left half
    assert refreshed[0] == H * W and (refreshed[1:] > 0).all() and (refreshed[1:] <= 2 * 16 * 64).all() and 2 * 16 * 64 < H * W
    stream = be.HoldStream(cell=HOLD[0], tol=HOLD[1], share=HOLD[2])
    assert vp.process_video_gif("in.mp4", str(tmp / "held.gif"), d, None, 64, 2, hold=stream) == N
    assert vp.process_video_gif("in.mp4", str(tmp / "plain.gif"), d, None, 64, 2) == N
    got = _decode((tmp / "held.gif").read_bytes())
    assert len(got) == N
    for i in range(N):
        assert np.array_equal(got[i], want[i]), i
        assert np.array_equal(got[i][:, :W], got[0][:, :W]), i           # the static half (enlarged twice: W columns) is frame 0's
    plain = _decode((tmp / "plain.gif").read_bytes())
    assert any(not np.array_equal(plain[i][:, :W], plain[0][:, :W]) for i in range(1, N))             # ... which it is not without
    held_bytes, plain_bytes = (tmp / "held.gif").stat().st_size, (tmp / "plain.gif").stat().st_size
    print(f"GIF bytes: {held_bytes} held, {plain_bytes} plain")
    assert held_bytes <= plain_bytes
    # the same stream object again: a file is a stream of its own, so the result is the same (settings tuple or object)
    assert vp.process_video_gif("in.mp4", str(tmp / "again.gif"), d, None, 64, 2, hold=stream) == N
    assert vp.process_video_gif("in.mp4", str(tmp / "tuple.gif"), d, None, 64, 2, hold=HOLD) == N
    assert (tmp / "again.gif").read_bytes() == (tmp / "held.gif").read_bytes() == (tmp / "tuple.gif").read_bytes()
    with pytest.raises(ValueError):
        vp.process_video_gif("in.mp4", str(tmp / "bad.gif"), d, None, 64, 2, hold=(3, 4, 0.1))


def test_apng_with_hold_decodes_to_the_statement(T, be, video):
    frames, vp, tmp = video
    d = _ditherer("fs")
    want, _ = _expected(T, be, frames, d, HOLD)
    assert vp.process_video_apng("in.mp4", str(tmp / "held.png"), d, None, 64, 2, hold=HOLD) == N
    assert vp.process_video_apng("in.mp4", str(tmp / "plain.png"), d, None, 64, 2) == N
    got = _decode((tmp / "held.png").read_bytes())
    assert len(got) == N
    for i in range(N):
        assert np.array_equal(got[i], want[i]), i
        assert np.array_equal(got[i][:, :W], got[0][:, :W]), i
    held_bytes, plain_bytes = (tmp / "held.png").stat().st_size, (tmp / "plain.png").stat().st_size
    print(f"APNG bytes: {held_bytes} held, {plain_bytes} plain")
    assert held_bytes <= plain_bytes


def test_process_frames_indexed_resets_when_the_palette_changes(T, be):
    from dither_pie_amd.video_processor import process_frames_indexed
    frames = _clip()[:4]
    x = T.from_numpy(frames).cuda()
    d, other = _ditherer("fs"), _ditherer("fs")
    other.palette = list(PALETTE[::-1])
    stream = be.HoldStream(cell=8, tol=255, share=0)                     # tol 255: nothing refreshes but what reset() lets through
    fresh = [process_frames_indexed(x[i:i + 1], dd, None, 64, None)[0].cpu().numpy()[0] for i, dd in ((0, d), (2, other))]
    a = process_frames_indexed(x[:2], d, None, 64, None, hold=stream)[0].cpu().numpy()
    assert np.array_equal(a[0], fresh[0]) and np.array_equal(a[1], fresh[0])
    b = process_frames_indexed(x[2:], other, None, 64, None, hold=stream)[0].cpu().numpy()     # another palette: frame 2 is fresh
    assert np.array_equal(b[0], fresh[1]) and np.array_equal(b[1], fresh[1])
    c = process_frames_indexed(x[:1], other, None, 64, None, hold=stream)[0].cpu().numpy()     # the same palette: held
    assert np.array_equal(c[0], fresh[1])
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    rs = np.random.RandomState(2)
    many = ImageDitherer(300, DitherMode.BAYER, [tuple(int(v) for v in c) for c in rs.randint(0, 256, (300, 3))], dither_params={"size": "4x4"})
    with pytest.raises(ValueError, match="256 colours"):
        process_frames_indexed(x[:1], many, None, 64, None, hold=stream)


def test_under_scene_palettes_every_scene_starts_fully_refreshed(T, tmp_path, monkeypatch):
    """tol = 255 holds everything for ever, so whatever changes in the file was let through by a reset: with scene_palettes the
    first frame of each scene is the fresh dither of that frame with the scene's palette, and every later frame of the scene
    repeats it."""
    import copy
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    from dither_pie_amd.scenes import Scene
    from dither_pie_amd.video_processor import VideoProcessor, process_frames
    palettes = [[(10, 20, 30), (70, 200, 40), (40, 90, 200), (75, 230, 250)], [(100, 0, 0), (150, 250, 250), (120, 120, 120)],
                [(180, 0, 0), (250, 250, 250), (200, 100, 50), (255, 0, 255), (181, 250, 250)]]
    frames = sr.three_scene_clip()[0]
    scenes = [Scene(0, 15, palettes[0]), Scene(15, 20, palettes[1]), Scene(20, 36, palettes[2])]
    base = ImageDitherer(16, DitherMode.BAYER, [(0, 0, 0), (255, 255, 255)], dither_params={"size": "4x4"})
    first = {}
    for s in scenes:
        d = copy.copy(base)
        d.palette = list(s.palette)
        first[s.start] = process_frames(T.from_numpy(frames[s.start:s.start + 1]).cuda(), d, None, 64, 2).cpu().numpy()[0]
    fake_ffmpeg_tools(tmp_path, monkeypatch, frames)
    monkeypatch.setattr(VideoProcessor, "PIPE_SLOT_BYTES", 4 * sr.H * sr.W * 3)      # the cut at 15 inside a batch, at 20 on an edge
    vp = VideoProcessor(devices=[0])
    assert vp.process_video_gif("in.mp4", str(tmp_path / "o.gif"), base, None, 64, 2, scene_palettes=scenes, hold=(8, 255, 0)) == 40
    got = _decode((tmp_path / "o.gif").read_bytes())
    assert len(got) == 40
    for i in range(40):
        start = max(s.start for s in scenes if s.start <= i)
        assert np.array_equal(got[i], first[start]), (i, start)
