"""CPU tier of the clip-wide palettes (include/ditherpie_hip_clip.h): the agreement of the header, the ctypes table and the
memory-discipline module (the rule tests/test_indexed_cpu.py keeps for the indexed header); the numpy restatement of
stream-distinct and rank-sample (tests/clip_palette_ref.py) against brute-force Python; the reference's palettes of the clip
fixtures (tests/golden/clip.{json,npz}) against the host tail -- numpy distinct, then dp_median_cut_host; and the refusals of
the entry points, which happen before any HIP call."""
import json
import os
import re

import numpy as np
import pytest

import clip_palette_ref as cr
from clip_spec import clip_frames
from conftest import GOLDEN, ROOT


# ---------------------------------------------------------------------------------------------------- header, binding, matrix
def _header_functions():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_clip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = {}
    for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        found[m.group(1)] = bool(re.search(r"\w+_dev\b", m.group(2)))
    return found


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_clip_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert len(found) == 6 and set(found) == set(_lib.EXPORTS_CLIP), set(found) ^ set(_lib.EXPORTS_CLIP)
    assert not set(_lib.EXPORTS_CLIP) & (set(_lib.EXPORTS) | set(_lib.EXPORTS_INDEXED))
    with_dev = {n for n, d in found.items() if d}
    assert with_dev == {"dp_distinct_stream_reset", "dp_distinct_stream_add_u8", "dp_hist_sample_u8"}
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = with_dev - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev and isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_library_exports_the_extension_and_keeps_its_abi_version():
    from dither_pie_amd import _lib
    L = _lib.load()
    for name in _lib.EXPORTS_CLIP:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION
    assert L.dp_distinct_stream_state_bytes() == 1 << 21
    for n in (0, 1, 2048, 2049, 300007):
        assert L.dp_distinct_stream_workspace_bytes(n) % 16 == 0 and L.dp_distinct_stream_workspace_bytes(n) >= (64 << 20) + n // 8
    assert L.dp_distinct_stream_workspace_bytes(-1) == 0
    assert L.dp_hist_sample_workspace_bytes() % 16 == 0 and L.dp_hist_sample_workspace_bytes() >= 8 * 4097


# ---------------------------------------------------------------------------------------------------- the restatement
def _brute_distinct(px):
    seen, out = set(), []
    for p in map(tuple, np.asarray(px).reshape(-1, 3).tolist()):
        if p not in seen:
            seen.add(p)
            out.append(p)
    return np.array(out, np.uint8).reshape(-1, 3)


def test_restated_stream_distinct_is_brute_force():
    rs = np.random.RandomState(3)
    for n_colours in (1, 3, 40):
        cols = rs.randint(0, 256, (n_colours, 3)).astype(np.uint8)
        bufs = [cols[rs.randint(0, n_colours, n)] for n in (1, 0, 7, 64, 5, 200)]
        assert np.array_equal(cr.distinct_first(np.concatenate(bufs)), _brute_distinct(np.concatenate(bufs)))
        s = cr.DistinctStream()
        for i, b in enumerate(bufs):
            s.add(b)
            assert np.array_equal(s.colours(), _brute_distinct(np.concatenate(bufs[:i + 1])))
        s.reset()
        assert len(s.colours()) == 0
        assert np.array_equal(s.add(bufs[3]).colours(), _brute_distinct(bufs[3]))


def test_restated_rank_sample_is_brute_force():
    rs = np.random.RandomState(4)
    px = np.concatenate([rs.randint(0, 256, (300, 3)), np.repeat([[17, 200, 3]], 40, axis=0), np.repeat([[16, 200, 3]], 2, axis=0),
                         np.repeat([[255, 255, 255]], 5, axis=0), np.zeros((3, 3), int)]).astype(np.uint8)
    slots = cr.slot_of(px)
    assert np.array_equal(cr.colour_of(slots), px)                     # the slot is a bijection of the colour
    r, g, b = 0xAB, 0xCD, 0xEF
    assert int(cr.slot_of([[r, g, b]])[0]) == (0xA << 20 | 0xC << 16 | 0xE << 12 | 0xB << 8 | 0xD << 4 | 0xF)
    laid_out = px[np.argsort(slots, kind="stable")]                    # the pixels in slot order, every colour count times
    ranks = np.concatenate([np.arange(len(px)), [0, len(px) - 1, 5, 5], [-1, len(px), 1 << 40, -(1 << 40)]])
    got, bad = cr.rank_sample(cr.histogram(px), ranks)
    assert bad == 4 and not got[-4:].any()
    assert np.array_equal(got[:-4], laid_out[ranks[:-4]])
    empty, bad = cr.rank_sample(np.zeros(1 << 24, np.int64), [0])
    assert bad == 1 and not empty.any()


# ---------------------------------------------------------------------------------------------------- the reference's palettes
@pytest.fixture(scope="module")
def clips():
    with open(os.path.join(GOLDEN, "clip.json")) as f:
        return json.load(f), np.load(os.path.join(GOLDEN, "clip.npz"))


def test_fixture_set_is_what_the_tiers_expect(clips):
    spec, arrays = clips
    assert spec["num_colors"] == [2, 16, 20, 64, 256] and len(spec["clips"]) == 8
    assert sum(1 for c in spec["clips"].values() if c["use_gamma"]) == 1
    for name, c in spec["clips"].items():
        assert 2 <= len(c["frames"]) <= 5
        for n, pal in c["palettes"].items():
            full = 1 << int(np.log2(int(n)))                           # (fewer where a bucket ran empty above the leaves)
            assert len(pal) == full or (name == "few_colours" and len(pal) < full), (name, n)
    black = clip_frames(spec["clips"]["first_frame_flat_black"]["frames"])
    assert not black[0].any() and black[1].any()
    nothing = clip_frames(spec["clips"]["later_frames_add_nothing"]["frames"])
    assert len(cr.distinct_first(np.concatenate([f.reshape(-1, 3) for f in nothing]))) == len(cr.distinct_first(nothing[0]))


def test_host_tail_reproduces_the_reference_on_stacked_frames(clips):
    """numpy stream-distinct over the regenerated frames (one add per frame), then ColorReducer's tail (dp_median_cut_host with
    its set-order replay): the palettes the reference's reduce_colors gave for the frames stacked top to bottom."""
    from dither_pie_amd import _tables
    from dither_pie_amd.dithering_lib import ColorReducer
    spec, arrays = clips
    assert ColorReducer._pyset_replay_ok()
    for name, c in spec["clips"].items():
        s = cr.DistinctStream()
        for f in clip_frames(c["frames"]):
            s.add(_tables.LUT_IN[f] if c["use_gamma"] else f)
        assert np.array_equal(s.colours(), arrays[name + "/distinct"]), name
        for n, want in c["palettes"].items():
            got = ColorReducer._median_cut_of_distinct(s.colours(), int(n))
            assert got == [tuple(p) for p in want], (name, n)


def test_reduce_colors_still_goes_through_the_same_tail():
    from PIL import Image
    from dither_pie_amd.dithering_lib import ColorReducer
    from oracle.oracle import rnd
    img = rnd(24, 32, 5)
    for n in (2, 16, 20):
        assert ColorReducer.reduce_colors(Image.fromarray(img), n) == ColorReducer._median_cut_of_distinct(cr.distinct_first(img), n)


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def _refused(lib, rc, *words):
    msg = lib.dp_last_error().decode()
    assert rc == 1, (rc, msg)                                       # DP_EINVAL
    for w in words:
        assert w in msg, (w, msg)


def test_stream_refusals(lib):
    fn = "dp_distinct_stream_add_u8"
    need = lib.dp_distinct_stream_workspace_bytes(100)
    ok = dict(px=0x1001, n=100, state=0x200000, lst=0x3001, cnt=0x4008, ws=0x5000010, wb=need)   # pointers are never dereferenced
    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_distinct_stream_add_u8(v["px"], v["n"], v["state"], v["lst"], v["cnt"], v["ws"], v["wb"], None)
    for bad in (dict(px=None), dict(state=None), dict(lst=None), dict(cnt=None), dict(n=-1), dict(n=(1 << 32) - 15), dict(state=0x200008),
                dict(cnt=0x4004)):
        _refused(lib, call(**bad), fn, "bad argument")
    for bad in (dict(ws=None), dict(ws=0x5000008), dict(wb=need - 1), dict(wb=0)):
        _refused(lib, call(**bad), fn, "workspace", str(need))
    assert call(n=0) == 0 and call(n=0, px=None, ws=None, wb=0) == 0        # nothing to do is not an error
    fn = "dp_distinct_stream_reset"
    _refused(lib, lib.dp_distinct_stream_reset(None, 0x4008, None), fn)
    _refused(lib, lib.dp_distinct_stream_reset(0x200000, None, None), fn)
    _refused(lib, lib.dp_distinct_stream_reset(0x200004, 0x4008, None), fn)
    _refused(lib, lib.dp_distinct_stream_reset(0x200000, 0x4004, None), fn)


def test_sample_refusals(lib):
    fn = "dp_hist_sample_u8"
    need = lib.dp_hist_sample_workspace_bytes()
    ok = dict(hist=0x1000000, ranks=0x2008, n=10, out=0x3001, cnt=0x4008, ws=0x5000010, wb=need)
    def call(**kw):
        v = dict(ok, **kw)
        return lib.dp_hist_sample_u8(v["hist"], v["ranks"], v["n"], v["out"], v["cnt"], v["ws"], v["wb"], None)
    for bad in (dict(hist=None), dict(ranks=None), dict(out=None), dict(cnt=None), dict(n=-1), dict(n=16385), dict(hist=0x1000008),
                dict(ranks=0x2004), dict(cnt=0x4004)):
        _refused(lib, call(**bad), fn, "bad argument")
    for bad in (dict(ws=None), dict(ws=0x5000008), dict(wb=need - 1)):
        _refused(lib, call(**bad), fn, "workspace", str(need))
    assert call(n=0) == 0 and call(n=0, ranks=None, out=None, ws=None, wb=0) == 0
