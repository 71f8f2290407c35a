"""CPU tier of the per-scene palettes (include/ditherpie_hip_scene.h, dither_pie_amd/scenes.py): the agreement of the header,
the ctypes table and the memory-discipline module (the rule tests/test_clip_palette_cpu.py keeps for the clip header); the
refusals of the two entry points, which happen before any HIP call; the pure host functions scene_cuts and split_at on
hand-built cases; the numpy restatement (tests/scene_ref.py) on the synthetic clip the GPU tier uses."""
import os
import re

import numpy as np
import pytest

import scene_ref as sr
from conftest import ROOT


# ---------------------------------------------------------------------------------------------------- header, binding, matrix
def _header_functions():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_scene.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = {}
    for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        found[m.group(1)] = bool(re.search(r"\w+_dev\b", m.group(2)))
    return found


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_scene_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert len(found) == 2 and set(found) == set(_lib.EXPORTS_SCENE), set(found) ^ set(_lib.EXPORTS_SCENE)
    assert not set(_lib.EXPORTS_SCENE) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED) | set(_lib.EXPORTS_CLIP))
    with_dev = {n for n, d in found.items() if d}
    assert with_dev == {"dp_frame_signatures_u8", "dp_signature_distances"}
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = with_dev - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev and isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_library_exports_the_extension_and_keeps_its_abi_version():
    import subprocess
    from dither_pie_amd import _lib
    L = _lib.load()
    for name in _lib.EXPORTS_SCENE:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: scene.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_SCENE:
            assert re.search(rf"\bT {name}\b", sym), (path, name)


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def _refused(lib, rc, code, *words):
    msg = lib.dp_last_error().decode()
    assert rc == code, (rc, msg)
    assert not re.search(r"DP_[A-Z0-9_]{3,}", msg), msg                # (the product library spells out no status name)
    for w in words:
        assert w in msg, (w, msg)


def test_signature_refusals(lib):
    fn = "dp_frame_signatures_u8"
    ok = dict(frames=0x1001, n=3, h=4, w=5, sig=0x2000010)             # pointers are never dereferenced
    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_frame_signatures_u8(v["frames"], v["n"], v["h"], v["w"], v["sig"], None)
    for bad in (dict(frames=None), dict(sig=None), dict(h=0), dict(w=0), dict(h=-1), dict(w=-7), dict(n=-1), dict(h=65536, w=65536),
                dict(h=2 ** 31 - 1, w=3), dict(sig=0x2000008), dict(sig=0x2000004), dict(sig=0x2000001)):
        _refused(lib, call(**bad), 1, fn, "bad argument")               # DP_EINVAL
    for bad in (dict(n=65536), dict(n=2 ** 31 - 1)):
        _refused(lib, call(**bad), 2, fn, "65535")                      # DP_EUNSUPPORTED
    assert call(n=0) == 0                                               # nothing to do is not an error, and launches nothing


def test_distance_refusals(lib):
    fn = "dp_signature_distances"
    ok = dict(sig=0x2000010, n=3, prev=0x3000010, has=1, dist=0x4000008)
    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_signature_distances(v["sig"], v["n"], v["prev"], v["has"], v["dist"], None)
    for bad in (dict(sig=None), dict(prev=None), dict(dist=None), dict(n=-1), dict(sig=0x2000008), dict(prev=0x3000008), dict(prev=0x3000004),
                dict(dist=0x4000004), dict(dist=0x4000001), dict(prev=None, has=0)):
        _refused(lib, call(**bad), 1, fn, "bad argument")
    assert call(n=0) == 0 and call(n=0, has=0) == 0


# ---------------------------------------------------------------------------------------------------- scene_cuts, split_at
def test_scene_cuts_compares_strictly():
    from dither_pie_amd.scenes import scene_cuts
    n_px = 1000                                                         # threshold * 2 * n_px = 800.0 exactly
    assert scene_cuts([0, 0, 800, 0], n_px, 0.4, 1) == ([], 4)          # equality is not a cut
    assert scene_cuts([0, 0, 801, 0], n_px, 0.4, 1) == ([2], 2)
    assert scene_cuts([0, 2000], n_px, 1.0, 1) == ([], 2)               # the largest distance there is, at threshold 1
    assert scene_cuts([0, 0, np.int64(801)], n_px, 0.4, 1)[0] == [2]    # (numpy integers as they come off the device)
    n_px = 3                                                            # 0.1 * 2 * 3 = 0.6000000000000001: a float product, not a ratio
    assert scene_cuts([0, 1], n_px, 0.1, 1) == ([1], 1) and scene_cuts([0, 0], n_px, 0.1, 1) == ([], 2)
    assert scene_cuts([], 10, 0.4, 8) == ([], 0) and scene_cuts([], 10, 0.4, 8, carry=5) == ([], 5)
    assert scene_cuts([2000], 1000, 0.4, 1) == ([], 1)                  # the first frame of a stream opens the first scene: no cut


def test_scene_cuts_min_scene_frames():
    from dither_pie_amd.scenes import scene_cuts
    big = 2000
    d = [0, 0, 0, big, 0, big, big, big, 0, 0]
    assert scene_cuts(d, 1000, 0.4, 1)[0] == [3, 5, 6, 7]
    assert scene_cuts(d, 1000, 0.4, 2)[0] == [3, 5, 7]                  # 6 is one frame after 5: suppressed, 7 is the next eligible
    assert scene_cuts(d, 1000, 0.4, 3)[0] == [3, 6]                     # 5 suppressed (two frames after 3), 6 cuts, 7 suppressed
    assert scene_cuts(d, 1000, 0.4, 4)[0] == [5]                        # 3 itself comes too early; 5 is the next eligible frame
    assert scene_cuts(d, 1000, 0.4, 3) == ([3, 6], 4)


def test_scene_cuts_carry_makes_batching_invisible():
    from dither_pie_amd.scenes import scene_cuts
    rs = np.random.RandomState(2)
    d = (rs.randint(0, 3, 60) == 0) * 2000
    d[0] = 0
    for need in (1, 2, 5, 8):
        want, held = scene_cuts(d.tolist(), 1000, 0.4, need)
        assert want == sr.cut_starts(d, 1000, 0.4, need)                # the restatement, over the whole clip at once
        for sizes in ((60,), (1, 59), (30, 30), (7,) * 8 + (4,), (1,) * 60):
            got, carry, at = [], 0, 0
            for n in sizes:
                starts, carry = scene_cuts(d[at:at + n].tolist(), 1000, 0.4, need, carry)
                got += [at + s for s in starts]
                at += n
            assert at == 60 and got == want and carry == held, (need, sizes)


def test_scene_cuts_value_errors():
    from dither_pie_amd.scenes import scene_cuts
    for thr in (0, 0.0, -0.1, 1.0000001, 2, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            scene_cuts([0], 10, thr, 8)
    assert scene_cuts([0], 10, 1.0, 8) == ([], 1) and scene_cuts([0], 10, 1e-9, 8) == ([], 1)
    for need in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_scene_frames"):
            scene_cuts([0], 10, 0.4, need)
    with pytest.raises(ValueError, match="n_px"):
        scene_cuts([0], 0, 0.4, 8)
    with pytest.raises(ValueError, match="carry"):
        scene_cuts([0], 10, 0.4, 8, carry=-1)


def test_split_at():
    from dither_pie_amd.scenes import split_at
    assert list(split_at(10, 5, [])) == [(10, 15)]
    assert list(split_at(10, 5, [10])) == [(10, 15)]                    # a start at the batch's first frame cuts nothing
    assert list(split_at(10, 5, [14])) == [(10, 14), (14, 15)]          # at its last frame
    assert list(split_at(10, 5, [15])) == [(10, 15)]                    # the next batch's first frame
    assert list(split_at(10, 5, [0, 9, 15, 99])) == [(10, 15)]          # outside it
    assert list(split_at(10, 5, [13, 11, 12])) == [(10, 11), (11, 12), (12, 13), (13, 15)]   # several, in any order
    assert list(split_at(10, 5, [3, 10, 12, 12, 14, 20])) == [(10, 12), (12, 14), (14, 15)]
    assert list(split_at(0, 1, [0])) == [(0, 1)] and list(split_at(7, 0, [7])) == []
    for first, n, starts in ((0, 17, [5, 6, 16]), (100, 4, [101, 103]), (3, 9, range(20))):
        pieces = list(split_at(first, n, starts))
        assert pieces[0][0] == first and pieces[-1][1] == first + n
        assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])) and all(lo < hi for lo, hi in pieces)
        assert all(not any(lo < s < hi for s in starts) for lo, hi in pieces)


def test_scene_palette_lists_are_checked_on_the_host():
    from dither_pie_amd.scenes import Scene, check_scene_palettes, scene_of
    pal = [(0, 0, 0), (255, 255, 255)]
    good = [Scene(0, 15, pal), Scene(15, 20, pal), Scene(20, 40, pal)]
    assert check_scene_palettes(good) == good and check_scene_palettes([tuple(s) for s in good]) == good
    assert Scene(3, 9, None)._fields == ("start", "end", "palette")
    for bad, word in (([], "empty"), ([Scene(0, 15, pal), Scene(14, 20, pal)], "overlap"), ([Scene(15, 20, pal), Scene(0, 15, pal)], "overlap"),
                      ([Scene(0, 15, pal), Scene(15, 20, None)], "no palette"), ([Scene(0, 15, [])], "no palette"), ([Scene(5, 5, pal)], "no frame")):
        with pytest.raises(ValueError, match=word):
            check_scene_palettes(bad)
    assert [scene_of(good, i) for i in (0, 14, 15, 19, 20, 39, 40, 1000)] == [0, 0, 1, 1, 2, 2, 2, 2]   # past the end: the last palette
    assert scene_of([Scene(5, 9, pal), Scene(12, 20, pal)], 2) == 0 and scene_of([Scene(5, 9, pal), Scene(12, 20, pal)], 10) == 0


def test_streaming_refuses_bad_scene_lists_before_anything_starts(tmp_path):
    from dither_pie_amd.scenes import Scene
    from dither_pie_amd.video_processor import VideoProcessor
    pal = [(0, 0, 0), (255, 255, 255)]
    vp = VideoProcessor()
    vp.get_video_info = None                                            # anything past the argument checks would call it
    out = str(tmp_path / "o.mp4")
    for bad in ([], [Scene(0, 9, pal), Scene(5, 12, pal)], [Scene(0, 9, None)]):
        with pytest.raises(ValueError):
            vp.process_video_streaming("in.mp4", out, None, scene_palettes=bad)
    with pytest.raises(ValueError, match="use_pipes"):
        vp.process_video_streaming("in.mp4", out, None, use_pipes=False, scene_palettes=[Scene(0, 9, pal)])
    for kw in (dict(threshold=0.0), dict(threshold=1.5), dict(min_scene_frames=0), dict(source="octree"), dict(max_frames=0), dict(every=0),
               dict(source="kmeans", num_colors=257)):
        with pytest.raises(ValueError):
            vp.scan_scenes("in.mp4", **kw)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_on_the_synthetic_clip():
    frames, moved = sr.three_scene_clip()
    assert frames.shape == (40, sr.H, sr.W, 3) and len(moved) == 3
    sig = sr.signatures(frames)
    assert sig.shape == (40, 4096) and (sig.sum(axis=1) == sr.H * sr.W).all()
    brute = np.zeros(4096, np.int64)
    for r, g, b in frames[7].reshape(-1, 3).tolist():
        brute[(r >> 4) << 8 | (g >> 4) << 4 | (b >> 4)] += 1
    assert np.array_equal(sig[7], brute)
    d = sr.distances(sig)
    want = np.zeros(40, np.int64)
    want[[15, 20]] = 2 * sr.H * sr.W                                    # the scenes share no cell
    for m in moved:
        want[[m, m + 1]] = 2 * sr.MOVED                                 # into the changed frame and out of it
    assert np.array_equal(d, want)
    assert 2 * sr.MOVED < 0.4 * 2 * sr.H * sr.W < 2 * sr.H * sr.W       # the in-scene change stays under the default threshold
    assert sr.cut_starts(d, sr.H * sr.W, 0.4, 3) == [15, 20]
    assert sr.cut_starts(d, sr.H * sr.W, 0.4, 8) == [15]                # the middle scene is shorter than min_scene_frames
    assert sr.cut_starts(d, sr.H * sr.W, 0.05, 1) == sorted([15, 20] + [k for m in moved for k in (m, m + 1)])
    assert sr.scene_ranges(40, [15, 20]) == [(0, 15), (15, 20), (20, 40)] and sr.scene_ranges(40, []) == [(0, 40)]
    assert int(sr.distances(sig[5:6], prev=sig[30])[0]) == 2 * sr.H * sr.W and int(sr.distances(sig[5:6])[0]) == 0
