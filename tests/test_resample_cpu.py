"""CPU tier of the filtered resize (include/ditherpie_hip_resample.h, backend.resample): the numpy statement
(tests/resample_ref.py) against Pillow's Image.resize itself -- the oracle travels with the suite --; dp_resample_host through
ctypes against the statement, byte for byte; the coefficient tables of resample_coeffs (host_logic.h) and the whole host
statement through the stand-alone host_asan harness (nothing preloaded) against the statement's; the agreement of the header,
the ctypes table, the exported symbols and the memory-discipline module (the rule tests/test_idiff_cpu.py keeps for its header);
every refusal that happens before a HIP call, of the entry points and of the Python layer."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

import resample_ref as rr
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
PIL_FILTER = {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def _pixelization_geometries():
    """What _even_dimensions makes of 270 x 480, 480 x 270 and 101 x 67 frames at max_size 64 and 17: (h, w, oh, ow)."""
    from dither_pie_amd.video_processor import _even_dimensions
    out = []
    for h, w in ((270, 480), (480, 270), (101, 67)):
        for max_size in (64, 17):
            tw, th = _even_dimensions(w, h, max_size)
            out.append((h, w, th, tw))
    return out


def _pillow(frame, oh, ow, name):
    return np.asarray(Image.fromarray(frame, "RGB").resize((ow, oh), PIL_FILTER[name]))


def _cases():
    """(label, filter, frames [n, h, w, 3], oh, ow): the sweep (9 geometries x 3 contents x 5 filters) and the pixelization
    geometries (noise and pure 0 / 255)."""
    out = []
    for gi, (h, w, oh, ow) in enumerate(rr.GEOMETRIES):
        for ci, kind in enumerate(rr.CONTENTS):
            frames = rr.content(kind, 1, h, w, 10 * gi + ci)
            for name in rr.FILTERS:
                out.append((f"{h}x{w}->{oh}x{ow} {kind} {name}", name, frames, oh, ow))
    for gi, (h, w, oh, ow) in enumerate(_pixelization_geometries()):
        for ci, kind in enumerate(("noise", "extremes")):
            frames = rr.content(kind, 1, h, w, 100 + 10 * gi + ci)
            for name in rr.FILTERS:
                out.append((f"pixelize {h}x{w}->{oh}x{ow} {kind} {name}", name, frames, oh, ow))
    return out


@pytest.fixture(scope="module")
def cases():
    """The cases with the statement's output, computed once: (label, filter, frames, oh, ow, want)."""
    return [c + (rr.resample(c[2], c[3], c[4], c[1]),) for c in _cases()]


# ---------------------------------------------------------------------------------------------------- the statement against Pillow
def test_the_sweep_has_the_geometries_the_header_names():
    g = rr.GEOMETRIES
    assert len(g) == 9 and len(rr.CONTENTS) == 3 and len(rr.FILTERS) == 5
    assert (8, 8, 1, 1) in g and (5, 300, 5, 7) in g and (33, 2, 3, 5) in g
    assert any(oh > h and ow > w for h, w, oh, ow in g)                               # an upscale
    assert any(oh == h and ow != w for h, w, oh, ow in g) and any(ow == w and oh != h for h, w, oh, ow in g)   # one axis only
    assert any(oh == h and ow == w for h, w, oh, ow in g)                               # the copy
    assert _pixelization_geometries() == [(270, 480, 64, 114), (270, 480, 16, 28), (480, 270, 114, 64), (480, 270, 28, 16),
                                          (101, 67, 96, 64), (101, 67, 24, 16)]


def test_statement_equals_pillow(cases):
    bad = []
    for label, name, frames, oh, ow, want in cases:
        pil = _pillow(frames[0], oh, ow, name)
        if not np.array_equal(want[0], pil):
            bad.append((label, int((want[0] != pil).sum())))
    assert not bad, bad[:8]
    assert len(cases) == 135 + 6 * 2 * 5


def test_overshoot_reaches_both_ends_of_the_clamp():
    """Pure 0 / 255 input: BICUBIC and LANCZOS sums leave 0 .. 255 on both sides, so the clamp is exercised (and the arithmetic
    shift floors the negative ones)."""
    frames = rr.content("extremes", 1, 37, 53, 5)
    for name in ("bicubic", "lanczos"):
        p = rr.plan(name, 37, 53, 37, 20)
        src = frames[0].astype(np.int64)
        lo = hi = 0
        for xx, (xmin, cnt) in enumerate(p["hor"][1].tolist()):
            s = (1 << 21) + (src[:, xmin:xmin + cnt] * p["hor"][2][xx, :cnt].astype(np.int64)[None, :, None]).sum(axis=1)
            lo, hi = min(lo, int((s >> 22).min())), max(hi, int((s >> 22).max()))
        print(name, "unclamped range", lo, hi)
        assert lo < 0 and hi > 255
        assert np.array_equal(rr.resample(frames[0], 37, 20, name), _pillow(frames[0], 37, 20, name))


def test_a_batch_is_its_frames_and_shapes_are_kept():
    frames = rr.content("noise", 3, 12, 9, 4)
    got = rr.resample(frames, 5, 14, "hamming")
    assert got.shape == (3, 5, 14, 3) and got.dtype == np.uint8
    for i in range(3):
        assert np.array_equal(got[i], rr.resample(frames[i], 5, 14, "hamming"))
    same = rr.resample(frames, 12, 9, "lanczos")
    assert np.array_equal(same, frames) and same is not frames
    assert rr.workspace_bytes("box", 3, 12, 9, 5, 14) == (3 * 12 * 14 * 3 + 15) // 16 * 16   # box 12 -> 5 reads every source row
    assert rr.workspace_bytes("box", 3, 12, 9, 12, 14) == 0 == rr.workspace_bytes("box", 3, 12, 9, 5, 9) == rr.workspace_bytes("box", 0, 12, 9, 5, 14)


# ---------------------------------------------------------------------------------------------------- dp_resample_host
def test_host_entry_point_equals_the_statement(cases):
    from dither_pie_amd import backend
    for label, name, frames, oh, ow, want in cases:
        got = backend.resample_host(frames, oh, ow, name)
        assert got.shape == want.shape and np.array_equal(got, want), label
    frames = rr.content("noise", 3, 12, 9, 4)                                            # a batch, and a single [H, W, 3] frame
    assert np.array_equal(backend.resample_host(frames, 5, 14, "bicubic"), rr.resample(frames, 5, 14, "bicubic"))
    assert backend.resample_host(frames[1], 5, 14, "bicubic").shape == (5, 14, 3)


# ---------------------------------------------------------------------------------------------------- header, binding
def _header_text():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_resample.h")) as f:
        return f.read()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_resample_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert set(found) == {"dp_resample_plan_create", "dp_resample_plan_destroy", "dp_resample_workspace_bytes", "dp_resample_u8",
                          "dp_resample_host"} == set(_lib.EXPORTS_RESAMPLE)
    others = set()
    for name in dir(_lib):
        if name.startswith("EXPORTS") and name != "EXPORTS_RESAMPLE":
            others |= set(getattr(_lib, name))
    assert len(others) > 100 and not set(_lib.EXPORTS_RESAMPLE) & others
    for name, args in found.items():                                    # the ctypes table has as many arguments as the header
        assert len(_lib._SIGS_RESAMPLE[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    # no prototype of this header has a stream parameter (the rule of tests/test_streams_cpu.py does not see it: the stream is a
    # field of the descriptor, and tests/test_gpu_resample_streams.py has its cases)
    assert not any(re.search(r"void\s*\*\s*stream\b", a) for a in found.values())
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+dp_resample_args\s*\{(.*?)\}\s*dp_resample_args\s*;", text, flags=re.S).group(1)
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [n for n, _ in _lib.ResampleArgs._fields_] == ["struct_size", "in_dev", "out_dev", "n_frames", "plan", "workspace_dev",
                                                                  "workspace_bytes", "stream"]
    assert C.sizeof(_lib.ResampleArgs) == 64 and _lib.ResampleArgs.struct_size.offset == 0
    # the device entry points: what takes the descriptor (its *_dev fields), and the call that uploads the tables
    with_dev = {n for n, a in found.items() if "dp_resample_args" in a} | {"dp_resample_plan_create"}
    assert with_dev == {"dp_resample_u8", "dp_resample_plan_create"}
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = with_dev - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev and isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name
    import test_gpu_resample_streams as sd                              # ... and its stalled-stream cases exist
    assert sd.ENTRY == "dp_resample_u8" and callable(sd.test_resample_on_a_stalled_stream)


def test_library_exports_the_extension_and_keeps_its_abi_version():
    from dither_pie_amd import _lib, backend
    L = _lib.load()
    for name in _lib.EXPORTS_RESAMPLE:
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        header_version = int(re.search(r"#define\s+DP_ABI_VERSION\s+(\d+)", f.read()).group(1))
    assert L.dp_version() == header_version == _lib.ABI_VERSION == 103
    for path in (_lib.PRODUCT_PATH, _lib.EXPERIMENTS_PATH):          # csrc/Makefile: resample.hip is in both libraries
        sym = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        for name in _lib.EXPORTS_RESAMPLE:
            assert re.search(rf"\bT {name}\b", sym), (path, name)
    text = _header_text()
    for i, name in enumerate(rr.FILTERS):
        assert int(re.search(rf"#define\s+DP_RESAMPLE_{name.upper()}\s+(\d+)", text).group(1)) == i == _lib.RESAMPLE_FILTERS.index(name)
    assert int(re.search(r"#define\s+DP_RESAMPLE_MAX_SIZE\s+(\d+)", text).group(1)) == backend.RESAMPLE_MAX_SIZE == rr.MAX_SIZE == 16384
    assert backend.RESAMPLE_FILTERS == ("nearest", "box", "bilinear", "hamming", "bicubic", "lanczos") == ("nearest",) + rr.FILTERS
    assert L.dp_resample_workspace_bytes(None, 3) == 0                  # no plan: nothing, and no HIP call
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    assert "-ffp-contract=off" in mk and re.search(r"^SRCS = .*\bresample\.hip\b", mk, flags=re.M)


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


COEFF_CASES = [(n_in, n_out, f) for f in range(5) for n_in, n_out in ((53, 10), (23, 50), (8, 1), (300, 7), (300, 2), (2, 5), (1, 1), (1, 9), (64, 64),
                                                                     (480, 114), (270, 64), (1080, 64), (3, 2))]


def test_coefficient_tables_equal_the_statements(harness, tmp_path):
    with open(tmp_path / "cases.bin", "wb") as f:
        for c in COEFF_CASES:
            f.write(np.array(c, "<i4").tobytes())
    lines = harness("resamplecoeffs", tmp_path / "cases.bin", len(COEFF_CASES))
    assert len(lines) == len(COEFF_CASES)
    for i, ((n_in, n_out, fi), line) in enumerate(zip(COEFF_CASES, lines)):
        got = line.split()
        ksize, bounds, k = rr.coeffs(n_in, n_out, rr.FILTERS[fi])
        assert got[:3] == ["coeffs", str(i), str(ksize)], (line[:80], n_in, n_out, fi)
        vals = np.array(got[3:], np.int64)
        assert len(vals) == 2 * n_out + n_out * ksize
        assert np.array_equal(vals[:2 * n_out].reshape(n_out, 2), bounds), (n_in, n_out, fi)
        assert np.array_equal(vals[2 * n_out:].reshape(n_out, ksize), k), (n_in, n_out, fi)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] <= ksize).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds[:, 0] + bounds[:, 1]) >= 0).all()   # what the staged kernel's span relies on
        assert abs(int(k.sum(axis=1).min()) - (1 << 22)) <= ksize and abs(int(k.sum(axis=1).max()) - (1 << 22)) <= ksize


def _record(fi, frames, oh, ow):
    n, h, w, _ = frames.shape
    return np.array([fi, n, h, w, oh, ow], "<i4").tobytes() + frames.tobytes()


def test_host_statement_under_the_sanitizers_equals_the_statement(harness, tmp_path, cases):
    """The same cases through `host_asan resample`: input and output vectors of exactly the stated size, clean output, equal bytes;
    what the plan records (y0, y1, the passes, max |k|, the accumulator bound) equals the statement's, and no case needs the
    32-bit-multiply instance."""
    extra = [("batch", "lanczos", rr.content("noise", 3, 12, 9, 4), 5, 14, rr.resample(rr.content("noise", 3, 12, 9, 4), 5, 14, "lanczos")),
             ("row", "lanczos", rr.content("noise", 1, 1, 300, 6), 1, 2, rr.resample(rr.content("noise", 1, 1, 300, 6), 1, 2, "lanczos")),
             # a window of 400 pixels (1200 bytes) is wider than a staged row: the planner's rule sends it to the naive kernel
             ("wide", "lanczos", rr.content("noise", 1, 3, 400, 7), 3, 2, rr.resample(rr.content("noise", 1, 3, 400, 7), 3, 2, "lanczos"))]
    todo = list(cases) + extra
    with open(tmp_path / "cases.bin", "wb") as f:
        for _, name, frames, oh, ow, _ in todo:
            f.write(_record(rr.FILTERS.index(name), frames, oh, ow))
    lines = harness("resample", tmp_path / "cases.bin", len(todo), tmp_path / "out.bin")
    assert len(lines) == len(todo)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    at = 0
    kernels = set()
    for i, ((label, name, frames, oh, ow, want), line) in enumerate(zip(todo, lines)):
        got = line.split()
        assert got[:3] == ["resample", str(i), "0"], (line, label)
        y0, y1, need_h, need_v, mul32, h_kernel, max_abs, max_sum = (int(v) for v in got[3:])
        p = rr.plan(name, frames.shape[1], frames.shape[2], oh, ow)
        assert (y0, y1, need_h, need_v) == (p["y0"], p["y1"], int(p["need_h"]), int(p["need_v"])), label
        big, need = rr.plan_sums(name, frames.shape[1], frames.shape[2], oh, ow)
        if need_h and need_v:
            assert (max_abs, max_sum) == (big, need), label
        assert max_sum < 1 << 31 and max_abs < 1 << 23 and mul32 == 0, label
        if need_h:
            kernels.add(h_kernel)
        assert np.array_equal(raw[at:at + want.size], want.reshape(-1)), label
        at += want.size
    assert at == raw.size
    assert kernels == {0, 1} and lines[-1].split()[8] == "0"             # both horizontal kernels have plans among the cases


def test_plan_refusals_in_the_harness(harness, tmp_path):
    z = np.zeros((1, 1, 1, 3), np.uint8)
    cases = [((5, z, 1, 1), 1), ((-1, z, 1, 1), 1), ((0, z, 0, 1), 2), ((0, z, 1, 16385), 2), ((0, z, -3, 4), 2), ((4, z, 16384, 1), 0)]
    with open(tmp_path / "cases.bin", "wb") as f:
        for (fi, frames, oh, ow), rule in cases:
            f.write(_record(fi, frames, oh, ow)[:None if rule == 0 else 24])   # (a refused record is its six numbers: no pixels are read)
    lines = harness("resample", tmp_path / "cases.bin", len(cases), tmp_path / "out.bin")
    for i, ((_, rule), line) in enumerate(zip(cases, lines)):
        assert line.split()[:3] == ["resample", str(i), str(rule)], line
        assert rule == 0 or len(line.split()) == 3                       # a refused plan reads no input and writes nothing
    assert os.path.getsize(tmp_path / "out.bin") == 16384 * 3


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


def test_plan_create_refusals(lib):
    fn = "dp_resample_plan_create"
    h = C.c_void_p(0x1234)
    _refused(lib, lib.dp_resample_plan_create(0, 4, 4, 2, 2, None), 1, fn, "out is NULL")
    for filt in (-1, 5, 100):
        _refused(lib, lib.dp_resample_plan_create(filt, 4, 4, 2, 2, C.byref(h)), 1, fn, "filter")
        assert h.value is None                                          # a refused create leaves NULL behind
        h = C.c_void_p(0x1234)
    for sizes in ((0, 4, 2, 2), (4, 0, 2, 2), (4, 4, 0, 2), (4, 4, 2, 0), (-1, 4, 2, 2), (16385, 4, 2, 2), (4, 16385, 2, 2), (4, 4, 16385, 2),
                  (4, 4, 2, 16385)):
        _refused(lib, lib.dp_resample_plan_create(4, *sizes, C.byref(h)), 1, fn, "16384")
    lib.dp_resample_plan_destroy(None)                                  # NULL is fine


def test_resample_u8_refusals(lib):
    """With a stand-in plan (zeroed: no pass needed, no workspace): every refusal comes before the plan is looked into further
    and before any HIP call.  The device addresses are never dereferenced.  The workspace-too-small refusal needs a real plan:
    tests/test_gpu_resample_memory.py."""
    from dither_pie_amd import _lib
    fn = "dp_resample_u8"
    fake = C.create_string_buffer(4096)
    size = C.sizeof(_lib.ResampleArgs)
    ok = dict(struct_size=size, in_dev=0x1001, out_dev=0x2000003, n_frames=3, plan=C.cast(fake, C.c_void_p).value, workspace_dev=0x3000000,
              workspace_bytes=1 << 20, stream=None)

    def call(**kw):
        a = _lib.ResampleArgs(**dict(ok, **kw))
        return lib.dp_resample_u8(C.byref(a))

    _refused(lib, lib.dp_resample_u8(None), 1, fn, "descriptor")
    for bad in (0, size - 8, size + 8, 1):
        _refused(lib, call(struct_size=bad), 1, fn, "struct_size", str(size))
    for bad in (dict(in_dev=None), dict(out_dev=None), dict(plan=None), dict(n_frames=-1), dict(n_frames=-(1 << 40))):
        _refused(lib, call(**bad), 1, fn, "bad argument")
    _refused(lib, call(out_dev=ok["in_dev"]), 1, fn, "in_dev")
    for ws in (0x3000001, 0x3000008):
        _refused(lib, call(workspace_dev=ws), 1, fn, "16-byte aligned")
    assert call(n_frames=0) == 0 and call(n_frames=0, in_dev=None, out_dev=None, workspace_dev=None, workspace_bytes=0) == 0   # nothing to do
    _refused(lib, call(n_frames=0, plan=None), 1, fn, "bad argument")   # ... but a bad argument still is an error
    _refused(lib, call(n_frames=0, struct_size=8), 1, fn, "struct_size")


def test_resample_host_refusals(lib):
    fn = "dp_resample_host"
    a = np.zeros((2, 4, 4, 3), np.uint8)
    o = np.full((2, 2, 2, 3), 7, np.uint8)
    pa, po = a.ctypes.data, o.ctypes.data
    _refused(lib, lib.dp_resample_host(0, None, po, 2, 4, 4, 2, 2), 1, fn, "bad argument")
    _refused(lib, lib.dp_resample_host(0, pa, None, 2, 4, 4, 2, 2), 1, fn, "bad argument")
    _refused(lib, lib.dp_resample_host(0, pa, po, -1, 4, 4, 2, 2), 1, fn, "bad argument")
    for filt in (-1, 5):
        _refused(lib, lib.dp_resample_host(filt, pa, po, 2, 4, 4, 2, 2), 1, fn, "filter")
    for sizes in ((0, 4, 2, 2), (4, 4, 0, 2), (4, 4, 2, 16385), (16385, 4, 2, 2)):
        _refused(lib, lib.dp_resample_host(0, pa, po, 2, *sizes), 1, fn, "16384")
    assert (o == 7).all()                                               # a refused call writes nothing
    assert lib.dp_resample_host(0, None, None, 0, 4, 4, 2, 2) == 0      # nothing to do
    assert lib.dp_resample_host(0, pa, po, 2, 4, 4, 2, 2) == 0 and (o == 0).all()


# ---------------------------------------------------------------------------------------------------- Python surface
def test_python_layer_refusals_come_before_the_device():
    import torch
    from dither_pie_amd import backend, video_processor as vp
    from dither_pie_amd.dithering_lib import ImageDitherer
    listed = "nearest, box, bilinear, hamming, bicubic, lanczos"
    for bad in ("cubic", "NEAREST", "", None, 3, ("box",)):
        with pytest.raises(ValueError, match=listed):
            backend.resample(None, 4, 4, bad)
        with pytest.raises(ValueError, match=listed):
            vp.process_frames(None, None, "regular", 64, None, downscale_filter=bad)
        with pytest.raises(ValueError, match=listed):
            vp.process_frames_indexed(None, None, "regular", 64, None, downscale_filter=bad)
        with pytest.raises(ValueError, match=listed):
            vp.process_frames_png(None, None, "regular", 64, None, downscale_filter=bad)
        with pytest.raises(ValueError, match=listed):
            vp.pixelize_regular(Image.new("RGB", (8, 8)), 4, resample=bad)
        V = vp.VideoProcessor()
        for call in (lambda: V.process_video_streaming("in.mp4", "out.mp4", None, downscale_filter=bad),
                     lambda: V.process_video_gif("in.mp4", "out.gif", None, downscale_filter=bad),
                     lambda: V.process_video_apng("in.mp4", "out.png", None, downscale_filter=bad),
                     lambda: V.process_video_pngs("in.mp4", "f_%05d.png", None, downscale_filter=bad),
                     lambda: V._stream_through_pipes("in.mp4", "out.mp4", None, "regular", 64, 4, None, {}, downscale_filter=bad)):
            with pytest.raises(ValueError, match=listed):
                call()
    with pytest.raises(ValueError, match="box, bilinear, hamming, bicubic, lanczos"):   # a plan is of an averaging filter
        backend.ResamplePlan("nearest", 4, 4, 2, 2)
    with pytest.raises(ValueError, match="box, bilinear"):
        backend.resample_host(np.zeros((4, 4, 3), np.uint8), 2, 2, "nearest")
    for sizes in ((0, 4, 2, 2), (4, 4, 2, 16385), (4, 4, 2.0, 2), (4, 4, True, 2)):
        with pytest.raises(ValueError, match="16384"):
            backend.ResamplePlan("box", *sizes)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            backend.resample_host(bad, 2, 2, "box")
    with pytest.raises(ValueError, match="16384"):
        backend.resample_host(np.zeros((4, 4, 3), np.uint8), 0, 2, "box")
    with pytest.raises(TypeError, match="CUDA uint8"):                  # frames on the host are not resized behind the caller's back
        backend.resample(torch.zeros((4, 4, 3), dtype=torch.uint8), 2, 2, "box")
    with pytest.raises(TypeError, match="CUDA uint8"):
        backend.resample(np.zeros((4, 4, 3), np.uint8), 2, 2, "nearest")
    assert isinstance(ImageDitherer, type)


def test_the_keyword_is_everywhere_and_defaults_to_nearest():
    from dither_pie_amd import video_processor as vp
    V = vp.VideoProcessor
    for fn in (vp.process_frames, vp.process_frames_indexed, vp.process_frames_png, vp._process_single_frame, V._process_batch,
               V._stream_through_pipes, V.process_video_streaming, V.process_video_gif, V.process_video_apng, V.process_video_pngs):
        p = inspect.signature(fn).parameters
        assert "downscale_filter" in p and p["downscale_filter"].default == "nearest", fn
        assert list(p)[-1] == "downscale_filter", fn                    # added at the end: positional callers see no change
    p = inspect.signature(vp.pixelize_regular).parameters
    assert list(p) == ["image", "max_size", "resample"] and p["resample"].default == "nearest"
    assert list(inspect.signature(vp.output_size).parameters) == ["h", "w", "pixelize_method", "max_size", "final_resize_multiplier"]
