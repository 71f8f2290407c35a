"""CPU tier of the temporal hold (include/ditherpie_hip_hold.h, backend.hold_host): dp_hold_host_u8 through ctypes against the numpy
statement (tests/hold_ref.py), bit for bit in out, refreshed and the final state; the properties the definition promises (any cut of
a batch into two calls, the identity at cell 1 / tol 0, the full hold at tol 255, the anchor rule, the share rule on a clipped cell)
on the statement AND on the host entry point; every refusal that happens before a HIP call, each naming its function; the agreement
of the header, the ctypes table and the exported symbols; the `hold` mode of the stand-alone host_asan harness (nothing preloaded)
against the statement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hold_ref as hr
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
DP_OK, DP_EINVAL, DP_EUNSUPPORTED = 0, 1, 2


def _host(src, planes, state, cell, tol, share256):
    from dither_pie_amd import backend
    return backend.hold_host(src, planes, state, cell, tol, share256)


IMPLS = {"statement": hr.hold, "host": _host}


@pytest.fixture(scope="module")
def cases():
    """case -> (src, planes, the statement's out, refreshed, state): computed once, shared, never modified"""
    made = {}
    for i, (n, h, w, cell, tol, share256) in enumerate(hr.CASES):
        src, planes = hr.clip(n, h, w, cell, tol, 100 + i)
        made[(n, h, w, cell, tol, share256)] = (src, planes) + hr.hold(src, planes, None, cell, tol, share256)
    for v in made.values():
        for a in v[:4] + v[4]:
            a.setflags(write=False)
    return made


def _same(got, want, what):
    (out, refreshed, state), (wout, wrefreshed, wstate) = got, want
    assert out.dtype == np.uint8 and refreshed.dtype == np.int64
    assert np.array_equal(out, wout), what
    assert np.array_equal(refreshed, wrefreshed), (what, refreshed.tolist(), wrefreshed.tolist())
    assert np.array_equal(state[0], wstate[0]) and np.array_equal(state[1], wstate[1]), what


def test_the_cases_are_the_issues_and_see_both_outcomes(cases):
    assert hr.CASES[:5] == [(5, 17, 19, 16, 3, 0), (4, 1, 1, 1, 0, 0), (6, 9, 67, 4, 2, 64), (5, 33, 5, 8, 0, 256), (3, 16, 16, 16, 1, 1)]
    assert {(c[3], c[5]) for c in hr.CASES[5:]} == {(2, 128), (8, 128)}
    for (n, h, w, cell, tol, share256), (_, _, out, refreshed, _) in cases.items():
        assert refreshed[0] == h * w
        if tol == 0:
            continue
        later = refreshed[1:]
        if h > cell or w > cell:        # a frame of several cells: some frame refreshes a part of them and holds the rest
            assert ((later > 0) & (later < h * w)).any(), (n, h, w, cell, refreshed.tolist())
        else:                           # ONE cell is the whole frame: it refreshes (all of it) or holds; both must occur
            assert (later == h * w).any() and (later == 0).any(), (n, h, w, cell, refreshed.tolist())
        assert (later == 0).any()       # ... and the noise alone (at most tol between any two frames) refreshes nothing


@pytest.mark.parametrize("case", hr.CASES, ids=lambda c: "x".join(map(str, c)))
def test_host_statement_equals_the_numpy_statement(cases, case):
    n, h, w, cell, tol, share256 = case
    src, planes, out, refreshed, state = cases[case]
    _same(_host(src, planes, None, cell, tol, share256), (out, refreshed, state), case)
    # with state: continue the stream by the same frames reversed, from the state the batch left
    more = (np.ascontiguousarray(src[::-1]), np.ascontiguousarray(planes[::-1]))
    before = (state[0].copy(), state[1].copy())
    _same(_host(*more, state, cell, tol, share256), hr.hold(*more, state, cell, tol, share256), case)
    assert np.array_equal(state[0], before[0]) and np.array_equal(state[1], before[1])    # the given state is not modified


@pytest.mark.parametrize("impl", sorted(IMPLS))
@pytest.mark.parametrize("case", hr.CASES, ids=lambda c: "x".join(map(str, c)))
def test_every_cut_into_two_calls_gives_the_same(cases, case, impl):
    n, h, w, cell, tol, share256 = case
    src, planes, out, refreshed, state = cases[case]
    f = IMPLS[impl]
    for k in range(n + 1):
        o1, r1, s1 = f(src[:k], planes[:k], None, cell, tol, share256)
        assert (s1 is None) == (k == 0)
        o2, r2, s2 = f(src[k:], planes[k:], s1, cell, tol, share256)
        got = (np.concatenate([o1, o2]), np.concatenate([r1, r2]), s2 if s2 is not None else s1)
        _same(got, (out, refreshed, state), (case, k))


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_cell_1_tol_0_leaves_planes_of_position_and_colour_unchanged(impl):
    """Planes that are a function of the position and the source colour only (what an ordered dither is): a pixel either changed,
    and takes the fresh index, or did not, and its held index IS the fresh one."""
    rng = np.random.default_rng(5)
    n, h, w = 6, 13, 22
    src = rng.integers(0, 2, (n, h, w, 3)).astype(np.uint8) * 200         # eight colours: one pixel in eight repeats its colour
    yy, xx = np.mgrid[0:h, 0:w]
    planes = ((src.astype(np.int64) * (3, 5, 7)).sum(-1) + 11 * yy + 13 * xx).astype(np.uint8)
    out, refreshed, _ = IMPLS[impl](src, planes, None, 1, 0, 0)
    assert np.array_equal(out, planes)
    assert 0 < refreshed[1:].min() and refreshed[1:].max() < h * w          # and both outcomes occurred


@pytest.mark.parametrize("impl", sorted(IMPLS))
@pytest.mark.parametrize("cell", hr.CELLS)
def test_tol_255_holds_everything(impl, cell):
    rng = np.random.default_rng(6 + cell)
    n, h, w = 4, 19, 21
    src = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    planes = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    out, refreshed, state = IMPLS[impl](src, planes, None, cell, 255, 0)
    assert (out == out[0]).all() and np.array_equal(out[0], planes[0])
    assert refreshed.tolist() == [h * w, 0, 0, 0]
    assert np.array_equal(state[0], src[0]) and np.array_equal(state[1], planes[0])


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_frames_within_tol_of_frame_0_refresh_nothing(impl):
    """The anchor rule: the comparison is with the source at the last refresh (frame 0 here), not with the frame before, so frames
    that differ from frame 0 by at most tol never refresh -- though two of them differ by up to 2 tol from each other."""
    rng = np.random.default_rng(8)
    n, h, w, tol = 6, 18, 25, 7
    base = rng.integers(tol, 256 - tol, (h, w, 3))
    src = np.stack([base] + [base + rng.integers(-tol, tol + 1, (h, w, 3)) for _ in range(n - 1)]).astype(np.uint8)
    assert np.abs(src[1:].astype(int) - src[:-1].astype(int)).max() > tol
    planes = rng.integers(0, 16, (n, h, w)).astype(np.uint8)
    for cell, share256 in ((1, 0), (4, 1), (16, 0)):
        out, refreshed, state = IMPLS[impl](src, planes, None, cell, tol, share256)
        assert refreshed.tolist() == [h * w] + [0] * (n - 1)
        assert (out == planes[0]).all() and np.array_equal(state[0], src[0])
    # ... and a slow drift of 1 per frame accumulates against the anchor and does trigger one: at frame tol + 1
    drift = np.stack([base // 2 + f for f in range(tol + 2)]).astype(np.uint8)
    planes = rng.integers(0, 16, (tol + 2, h, w)).astype(np.uint8)
    _, refreshed, _ = IMPLS[impl](drift, planes, None, 8, tol, 256)
    assert refreshed.tolist() == [h * w] + [0] * tol + [h * w]


@pytest.mark.parametrize("impl", sorted(IMPLS))
def test_a_clipped_cell_of_3_pixels_needs_all_3_at_share_256(impl):
    h, w, cell = 3, 9, 8                                                # the cell at x = 8 is 1 wide and 3 high: 3 pixels
    src = np.full((5, h, w, 3), 100, np.uint8)
    src[1, 0, 8] = 200                                                  # one of the three changed
    src[2, :2, 8] = 200                                                 # two
    src[3, :, 8] = 200                                                  # all three: the cell refreshes
    src[4, :, 8] = 200                                                  # the same again: nothing changed against the new anchor
    planes = (np.arange(5, dtype=np.uint8)[:, None, None] + np.zeros((h, w), np.uint8)).astype(np.uint8)
    out, refreshed, _ = IMPLS[impl](src, planes, None, cell, 10, 256)
    assert refreshed.tolist() == [h * w, 0, 0, 3, 0]
    assert (out[:, :, :8] == 0).all() and out[:, :, 8].tolist() == [[0] * 3, [0] * 3, [0] * 3, [3] * 3, [3] * 3]
    _, refreshed, _ = IMPLS[impl](src, planes, None, cell, 10, 171)    # 2 of 3 pixels are 170.67 / 256: not enough at 171 ...
    assert refreshed.tolist() == [h * w, 0, 0, 3, 0]
    _, refreshed, _ = IMPLS[impl](src, planes, None, cell, 10, 170)    # ... enough at 170: the cell refreshes at frame 2, and the
    assert refreshed.tolist() == [h * w, 0, 3, 0, 0]                   # third pixel alone (1 of 3) does not refresh it again


# ---------------------------------------------------------------------------------------------------- refusals
def _args(_lib, **kw):
    n, h, w = 2, 5, 7
    keep = dict(src=np.zeros((n, h, w, 3), np.uint8), planes=np.zeros((n, h, w), np.uint8), anchor=np.zeros((h, w, 3), np.uint8),
                held=np.zeros((h, w), np.uint8), out=np.full((n, h, w), 9, np.uint8), refreshed=np.full(n + 1, -5, np.int64))
    ok = dict(struct_size=C.sizeof(_lib.HoldArgs), src_dev=keep["src"].ctypes.data, planes_dev=keep["planes"].ctypes.data, n_frames=n, h=h, w=w,
              cell=8, tol=4, share256=16, anchor_dev=keep["anchor"].ctypes.data, held_dev=keep["held"].ctypes.data, has_state=0,
              out_dev=keep["out"].ctypes.data, refreshed_dev=keep["refreshed"].ctypes.data, stream=None)
    return _lib.HoldArgs(**dict(ok, **kw)), keep, ok


@pytest.mark.parametrize("fn", ["dp_hold_u8", "dp_hold_host_u8"])
def test_every_refusal_names_its_function_and_happens_before_any_hip_call(fn):
    """No device here: a dp_hold_u8 that reached a HIP call would answer DP_EHIP, not the code asked for."""
    from dither_pie_amd import _lib
    L = _lib.load()
    f = getattr(L, fn)
    _, keep, ok = _args(_lib)
    px = 5 * 7
    size = ok["struct_size"]
    refusals = [(dict(struct_size=size - 8), DP_EINVAL), (dict(struct_size=size + 8), DP_EINVAL), (dict(struct_size=0), DP_EINVAL),
                (dict(src_dev=None), DP_EINVAL), (dict(planes_dev=None), DP_EINVAL), (dict(anchor_dev=None), DP_EINVAL), (dict(held_dev=None), DP_EINVAL),
                (dict(out_dev=None), DP_EINVAL), (dict(refreshed_dev=None), DP_EINVAL), (dict(n_frames=-1), DP_EINVAL),
                (dict(h=0), DP_EINVAL), (dict(w=0), DP_EINVAL), (dict(h=-3), DP_EINVAL), (dict(h=1 << 16, w=1 << 15), DP_EINVAL),
                (dict(cell=0), DP_EINVAL), (dict(cell=3), DP_EINVAL), (dict(cell=32), DP_EINVAL), (dict(cell=-8), DP_EINVAL),
                (dict(tol=-1), DP_EINVAL), (dict(tol=256), DP_EINVAL), (dict(share256=-1), DP_EINVAL), (dict(share256=257), DP_EINVAL),
                (dict(refreshed_dev=ok["refreshed_dev"] + 4), DP_EINVAL), (dict(refreshed_dev=ok["refreshed_dev"] + 1), DP_EINVAL),
                (dict(out_dev=ok["planes_dev"]), DP_EINVAL), (dict(out_dev=ok["planes_dev"] + 2 * px - 1), DP_EINVAL),
                (dict(out_dev=ok["src_dev"] + 5), DP_EINVAL), (dict(out_dev=ok["anchor_dev"] + 3 * px - 1), DP_EINVAL),
                (dict(out_dev=ok["held_dev"]), DP_EINVAL), (dict(anchor_dev=ok["src_dev"] + 3), DP_EINVAL),
                (dict(held_dev=ok["planes_dev"] + px), DP_EINVAL), (dict(held_dev=ok["src_dev"]), DP_EINVAL),
                (dict(anchor_dev=ok["planes_dev"]), DP_EINVAL), (dict(held_dev=ok["anchor_dev"] + 1), DP_EINVAL),
                (dict(n_frames=65536), DP_EUNSUPPORTED)]
    for kw, code in refusals:
        a = _lib.HoldArgs(**dict(ok, **kw))
        rc = f(C.byref(a))
        msg = L.dp_last_error()
        assert rc == code and fn.encode() in msg and (fn != "dp_hold_u8" or b"dp_hold_host_u8" not in msg), (kw, rc, msg)
    assert f(None) == DP_EINVAL and fn.encode() in L.dp_last_error()
    # n_frames = 0: DP_OK, nothing touched, the buffers may be NULL
    assert f(C.byref(_lib.HoldArgs(**dict(ok, n_frames=0)))) == DP_OK
    assert f(C.byref(_lib.HoldArgs(**dict(ok, n_frames=0, src_dev=None, planes_dev=None, anchor_dev=None, held_dev=None, out_dev=None,
                                          refreshed_dev=None)))) == DP_OK
    assert (keep["out"] == 9).all() and (keep["refreshed"] == -5).all() and not keep["anchor"].any()


def test_state_bytes():
    from dither_pie_amd import _lib
    L = _lib.load()
    a, b = C.c_size_t(1), C.c_size_t(1)
    assert L.dp_hold_state_bytes(1080, 1920, C.byref(a), C.byref(b)) == DP_OK and (a.value, b.value) == (3 * 1080 * 1920, 1080 * 1920)
    assert L.dp_hold_state_bytes(1, 1, C.byref(a), C.byref(b)) == DP_OK and (a.value, b.value) == (3, 1)
    for h, w, pa, pb in ((0, 4, a, b), (4, 0, a, b), (1 << 16, 1 << 15, a, b), (4, 4, None, b), (4, 4, a, None)):
        rc = L.dp_hold_state_bytes(h, w, C.byref(pa) if pa is not None else None, C.byref(pb) if pb is not None else None)
        assert rc == DP_EINVAL and b"dp_hold_state_bytes" in L.dp_last_error(), (h, w)


def test_the_python_layer_refuses_before_the_library():
    from dither_pie_amd import backend
    src, planes = np.zeros((2, 4, 6, 3), np.uint8), np.zeros((2, 4, 6), np.uint8)
    for kw in (dict(cell=3), dict(cell=0), dict(cell=32), dict(cell=2.5), dict(tol=-1), dict(tol=256), dict(tol=1.5), dict(share256=-1),
               dict(share256=257), dict(cell="x")):
        with pytest.raises(ValueError):
            backend.hold_host(src, planes, None, **dict(dict(cell=8, tol=4, share256=16), **kw))
    with pytest.raises(ValueError, match="256 colours"):              # two-byte planes: the limit is named
        backend.hold_host(src, planes.astype(np.int16), None, 8, 4, 16)
    with pytest.raises(ValueError):
        backend.hold_host(src, planes[:1], None, 8, 4, 16)
    with pytest.raises(ValueError):
        backend.hold_host(src, planes, (np.zeros((4, 6, 3), np.uint8), np.zeros((4, 5), np.uint8)), 8, 4, 16)
    out, refreshed, state = backend.hold_host(src[:0], planes[:0], None, 8, 4, 16)      # an empty batch: empty results, no state
    assert out.shape == (0, 4, 6) and refreshed.shape == (0,) and refreshed.dtype == np.int64 and state is None
    for bad in ((8, 4), (3, 4, 0.5), "x", (8, 4, 0.5, 1), (8, 300, 0.1)):
        with pytest.raises(ValueError):
            backend.check_hold_argument(bad)
    assert backend.check_hold_argument(None) is None and backend.check_hold_argument((8, 4, 1 / 16)) == (8, 4, 1 / 16)


# ---------------------------------------------------------------------------------------------------- header, binding
def _header_text():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_hold.h")) as f:
        return f.read()


def test_header_and_binding_agree():
    from dither_pie_amd import _lib, backend
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    found = {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}
    assert set(found) == {"dp_hold_u8", "dp_hold_host_u8", "dp_hold_state_bytes"} == set(_lib.EXPORTS_HOLD)
    others = set()
    for name in dir(_lib):
        if name.startswith("EXPORTS") and name != "EXPORTS_HOLD":
            others |= set(getattr(_lib, name))
    assert len(others) > 100 and not set(_lib.EXPORTS_HOLD) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        assert len(_lib._SIGS_HOLD[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    # no prototype of this header has a stream parameter: the stream is a field (tests/test_gpu_hold_streams.py has its cases)
    assert not any(re.search(r"void\s*\*\s*stream\b", a) for a in found.values())
    body = re.search(r"typedef\s+struct\s+dp_hold_args\s*\{(.*?)\}\s*dp_hold_args\s*;", text, flags=re.S).group(1)
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in _lib.HoldArgs._fields_] == ["struct_size", "src_dev", "planes_dev", "n_frames", "h", "w", "cell", "tol", "share256",
                                                               "anchor_dev", "held_dev", "has_state", "out_dev", "refreshed_dev", "stream"]
    assert C.sizeof(_lib.HoldArgs) == 104 and _lib.HoldArgs.struct_size.offset == 0 and _lib.HoldArgs.stream.offset == 96
    assert int(re.search(r"#define\s+DP_HOLD_MAX_CELL\s+(\d+)", text).group(1)) == max(_lib.HOLD_CELLS) == max(hr.CELLS) == 16
    assert int(re.search(r"#define\s+DP_HOLD_MAX_FRAMES\s+(\d+)", text).group(1)) == _lib.HOLD_MAX_FRAMES == backend.HOLD_MAX_FRAMES == 65535
    assert backend.HOLD_CELLS == hr.CELLS


def test_library_exports_the_extension_and_keeps_its_abi_version():
    from dither_pie_amd import _lib
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: hold.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_HOLD:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert re.search(r"^SRCS = .*\bhold\.hip\b", f.read(), flags=re.M)


def test_the_video_path_takes_hold_and_defaults_to_none():
    import inspect
    from dither_pie_amd import video_processor as vp
    for fn in (vp.process_frames_indexed, vp.VideoProcessor.process_video_gif, vp.VideoProcessor.process_video_apng):
        assert inspect.signature(fn).parameters["hold"].default is None, fn
    for fn in (vp.process_frames, vp.process_frames_png, vp.VideoProcessor.process_video_pngs, vp.VideoProcessor.process_video_streaming):
        assert "hold" not in inspect.signature(fn).parameters, fn           # out of scope


# ---------------------------------------------------------------------------------------------------- host logic under ASan / UBSan
@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(*args):
        r = subprocess.run([os.path.join(CSRC, "build", "host_asan")] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        return r.stdout.strip().split("\n")
    return run


def test_host_statement_under_the_sanitizers_equals_the_statement(harness, tmp_path, cases):
    """Every case through `host_asan hold` -- as one call, cut in the middle, and continued from a state -- on vectors of exactly the
    stated sizes; without state the record's state bytes are noise that must not show."""
    rng = np.random.default_rng(77)
    todo = []
    for case, (src, planes, out, refreshed, state) in cases.items():
        n, h, w, cell, tol, share256 = case
        noise = (rng.integers(0, 256, (h, w, 3)).astype(np.uint8), rng.integers(0, 256, (h, w)).astype(np.uint8))
        todo.append((case, src, planes, noise, 0, -1, (out, refreshed, state)))
        todo.append((case, src, planes, noise, 0, n // 2, (out, refreshed, state)))
        more = (np.ascontiguousarray(src[::-1]), np.ascontiguousarray(planes[::-1]))
        todo.append((case, *more, state, 1, 1, hr.hold(*more, state, cell, tol, share256)))
    bad = [(2, 4, 4, 3, 0, 0), (2, 4, 4, 8, 256, 0), (2, 4, 4, 8, 0, 257), (2, 0, 4, 8, 0, 0), (65536, 4, 4, 8, 0, 0)]   # rules 3, 4, 5, 2, 6
    with open(tmp_path / "cases.bin", "wb") as f:
        for (n, h, w, cell, tol, share256), src, planes, st, has_state, cut, _ in todo:
            f.write(np.array([n, h, w, cell, tol, share256, has_state, cut], "<i4").tobytes())
            f.write(src.tobytes() + planes.tobytes() + st[0].tobytes() + st[1].tobytes())
        for n, h, w, cell, tol, share256 in bad:
            f.write(np.array([n, h, w, cell, tol, share256, 0, -1], "<i4").tobytes())
    lines = harness("hold", tmp_path / "cases.bin", len(todo) + len(bad), tmp_path / "out.bin")
    assert len(lines) == len(todo) + len(bad)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    at = 0
    for i, ((case, src, planes, st, has_state, cut, want), line) in enumerate(zip(todo, lines)):
        n, h, w = case[:3]
        assert line.split() == ["hold", str(i), "0", str(int(want[1].sum()))], (line, case)
        px = h * w
        out = raw[at:at + n * px].reshape(n, h, w)
        refreshed = raw[at + n * px:at + n * px + 8 * n].view(np.int64)
        anchor = raw[at + n * px + 8 * n:at + n * px + 8 * n + 3 * px].reshape(h, w, 3)
        held = raw[at + n * px + 8 * n + 3 * px:at + n * px + 8 * n + 4 * px].reshape(h, w)
        at += n * px + 8 * n + 4 * px
        _same((out, refreshed, (anchor, held)), want, (case, has_state, cut))
    assert at == len(raw)
    assert [ln.split()[2] for ln in lines[len(todo):]] == ["3", "4", "5", "2", "6"]
