"""CPU tier of the indexed output (include/ditherpie_hip_indexed.h): the host builder of the colour -> index hash table
(host_logic.h: index_map_build) under ASan / UBSan through the host_sanitize.cpp harness, judged by tests/indexed_ref.py; the
agreement of the header, the ctypes table and the memory-discipline module (the rule tests/test_arena_cpu.py keeps for the
main header); and every refusal of the entry points, which happen before any HIP call."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import indexed_ref as ir
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
MAX_PROBE = 6      # the displacement bound the kernels are compiled for (host_logic.h: kIndexMapMaxProbe)
N_ABSENT = 10000


@pytest.fixture(scope="module")
def asan():
    subprocess.check_call(["make", "-s", "-C", CSRC, "host_asan"])
    return os.path.join(CSRC, "build", "host_asan")


def _absent(colors, n, seed):
    have = set(ir._codes(colors).tolist())
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        for c in rs.randint(0, 1 << 24, n).tolist():
            if c not in have and len(out) < n:
                out.append(c)
    # half of them one bit away from an entry: the near misses a weak comparison would take for hits
    near = ir._codes(colors)[rs.randint(0, len(colors), n // 2)] ^ (1 << rs.randint(0, 24, n // 2))
    for k, c in enumerate(near.tolist()):
        if c not in have:
            out[k] = c
    a = np.array(out, np.int64)
    return np.stack([a & 255, (a >> 8) & 255, (a >> 16) & 255], axis=1).astype(np.uint8)


def _check_lists(tool, lists, tmp_path):
    """Every list through the harness in one process; the harness's lookups against the numpy contract."""
    path = tmp_path / "lists.bin"
    with open(path, "wb") as f:
        for k, colors in enumerate(lists):
            q = _absent(colors, N_ABSENT, 100 + k)
            f.write(struct.pack("<ii", len(colors), len(q)) + np.ascontiguousarray(colors, np.uint8).tobytes() + q.tobytes())
    r = subprocess.run([tool, "indexmap", str(path), str(len(lists))], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 3 * len(lists), r.stdout[-2000:]
    for k, colors in enumerate(lists):
        head, idx, absent = lines[3 * k:3 * k + 3]
        info = dict(kv.split("=") for kv in head.split()[2:])
        K = len(colors)
        assert head.split()[:2] == ["map", str(k)] and int(info["K"]) == K, head
        assert int(info["slots"]) == (2048 if K <= 512 else 4096) and int(info["rest_bits"]) == (13 if K <= 512 else 12), head
        assert 0 <= int(info["max_probe"]) <= int(info["bound"]) == MAX_PROBE, head
        assert int(info["mult"]) % 2 == 1 and int(info["mult"]) < 1 << 24, head            # odd: a bijection of the 24-bit colours
        want = ir.lowest_index(colors)
        assert int(info["used"]) == len(set(want.tolist())), head                          # one slot per distinct colour
        assert np.array_equal(np.array(idx.split()[1:], np.int64), want), (k, K)
        assert absent == f"absent_hits=0 of {N_ABSENT}", (k, absent)


def _random_list(rs):
    K = int(rs.choice([rs.randint(1, 17), rs.randint(17, 257), rs.randint(257, 1025)]))
    kind = rs.randint(0, 4)
    if kind == 0:      # anywhere in the cube
        c = rs.randint(0, 256, (K, 3))
    elif kind == 1:    # crowded: an extracted palette
        c = np.clip(np.round(rs.randint(20, 230) + rs.randn(K, 3) * 6), 0, 255)
    elif kind == 2:    # a grey ramp and its neighbours: arithmetic progressions of the 24-bit code
        g = rs.randint(0, 256, K)
        c = np.stack([g, g, np.clip(g + rs.randint(0, 2, K), 0, 255)], axis=1)
    else:              # with duplicates
        c = rs.randint(0, 256, (max(K // 3, 1), 3))[rs.randint(0, max(K // 3, 1), K)]
    return c.astype(np.uint8)


def test_builder_on_the_size_classes_and_degenerate_lists(asan, tmp_path):
    rs = np.random.RandomState(1)
    lists = [rs.randint(0, 256, (K, 3)).astype(np.uint8) for K in (1, 2, 256, 257, 1024)]
    lists += [np.full((K, 3), 7, np.uint8) for K in (1, 2, 256, 257, 1024)]                  # all entries equal
    lists += [np.repeat(rs.randint(0, 256, (1, 3)), 512, axis=0).astype(np.uint8)]
    grey = np.arange(1024) // 4
    lists += [np.stack([grey, grey, grey], axis=1).astype(np.uint8)]                          # 256 colours, each four times
    seq = np.arange(1024)
    lists += [np.stack([seq & 255, seq >> 8, np.zeros_like(seq)], axis=1).astype(np.uint8)]   # consecutive 24-bit codes
    lists += [np.stack([np.zeros_like(seq), seq & 255, seq >> 8], axis=1).astype(np.uint8)]   # ... with a stride of 256
    _check_lists(asan, lists, tmp_path)


def test_builder_on_the_reference_s_palettes(asan, tmp_path):
    with open(os.path.join(GOLDEN, "palettes.json")) as f:
        pals = json.load(f)
    assert len(pals) == 25
    lists = [np.array([[int(c[i:i + 2], 16) for i in (1, 3, 5)] for c in p["colors"]], np.uint8) for p in pals]
    _check_lists(asan, lists, tmp_path)


def test_builder_on_200_random_lists(asan, tmp_path):
    rs = np.random.RandomState(2)
    _check_lists(asan, [_random_list(rs) for _ in range(200)], tmp_path)


# ---------------------------------------------------------------------------------------------------- the contract's statement
def test_reference_statement_itself():
    colors = np.array([[1, 2, 3], [9, 9, 9], [1, 2, 3], [0, 0, 0], [9, 9, 9]], np.uint8)
    assert ir.lowest_index(colors).tolist() == [0, 1, 0, 3, 1]
    rgb = np.array([[[9, 9, 9], [1, 2, 3]], [[5, 5, 5], [0, 0, 0]]], np.uint8)
    idx, missing, n = ir.to_indices(rgb, colors)
    assert idx.tolist() == [[1, 0], [0, 3]] and missing.tolist() == [[False, False], [True, False]] and n == 1
    back, bad, nb = ir.from_indices(np.array([[1, 0], [7, 3]], np.int16), colors)
    assert np.array_equal(back[~missing], rgb[~missing]) and nb == 1 and bad[1, 0] and back[1, 0].tolist() == [1, 2, 3]
    assert ir.from_indices(np.array([-1], np.int16), colors)[2] == 1                      # 0xFFFF, not -1


@pytest.mark.parametrize("geom", [(5, 7, 15, 21), (6, 9, 4, 5), (31, 17, 64, 64), (1, 1, 3, 2), (64, 48, 7, 5), (9, 13, 10, 26)])
def test_reference_plane_resize_is_pillow_s_nearest(geom):
    from PIL import Image
    h, w, oh, ow = geom
    plane = np.random.RandomState(h * w).randint(0, 256, (1, h, w)).astype(np.uint8)
    want = np.asarray(Image.fromarray(plane[0], "L").resize((ow, oh), Image.NEAREST))
    assert np.array_equal(ir.resize_nearest_plane(plane, oh, ow)[0], want)


# ---------------------------------------------------------------------------------------------------- header, binding, matrix
def _header_functions():
    with open(os.path.join(ROOT, "include", "ditherpie_hip_indexed.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"typedef struct \w+ \{.*?\} \w+;", " ", text, flags=re.S)
    found = {}
    for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        found[m.group(1)] = bool(re.search(r"\w+_dev\b", m.group(2)))
    return found


def test_header_binding_and_memory_matrix_agree():
    import test_gpu_indexed_memory as md
    from dither_pie_amd import _lib
    found = _header_functions()
    assert len(found) == 6 and set(found) == set(_lib.EXPORTS_INDEXED), set(found) ^ set(_lib.EXPORTS_INDEXED)
    assert not set(_lib.EXPORTS_INDEXED) & set(_lib.EXPORTS)
    with_dev = {n for n, d in found.items() if d}
    assert with_dev == {"dp_index_from_rgb_u8", "dp_rgb_from_index_u8", "dp_resize_nearest_plane_u8"}
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
    for name in _lib.EXPORTS_INDEXED:
        assert hasattr(L, name), name
    assert L.dp_version() == 103 == _lib.ABI_VERSION


def test_a_library_without_the_extension_is_refused_with_the_rebuild_message(tmp_path, monkeypatch):
    """load() resolves EXPORTS_INDEXED together with EXPORTS: a build of the right ABI version that has every function of the
    main table (here: a table cut down to dp_version) but lacks the extension is refused, and the message says `rebuild it`."""
    from dither_pie_amd import _lib
    src = tmp_path / "stub.c"
    src.write_text("int dp_version(void) { return %d; }\n" % _lib.ABI_VERSION)
    so = tmp_path / "libstub.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_SIGS", {"dp_version": _lib._SIGS["dp_version"]})
    with pytest.raises(_lib.DitherPieError, match="does not export dp_index_map_create: rebuild it"):
        _lib.load()
    assert str(so) not in _lib._loaded


# ---------------------------------------------------------------------------------------------------- refusals, no GPU needed
@pytest.fixture(scope="module")
def lib():
    from dither_pie_amd import _lib
    return _lib.load()


def _map(lib, K, seed=0):
    colors = np.random.RandomState(seed).randint(0, 256, (K, 3)).astype(np.uint8)
    h = C.c_void_p()
    assert lib.dp_index_map_create(colors.ctypes.data_as(C.c_void_p), K, C.byref(h)) == 0, lib.dp_last_error()
    return h


def _refused(lib, rc, *words):
    msg = lib.dp_last_error().decode()
    assert rc == 1, (rc, msg)                                       # DP_EINVAL
    for w in words:
        assert w in msg, (w, msg)


def test_map_creation_info_and_refusals(lib):
    colors = np.zeros((4, 3), np.uint8)
    ptr = colors.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    for K in (0, -1, 1025):
        _refused(lib, lib.dp_index_map_create(ptr, K, C.byref(h)), "dp_index_map_create", "[1, 1024]", str(K))
    _refused(lib, lib.dp_index_map_create(None, 4, C.byref(h)), "dp_index_map_create", "NULL")
    _refused(lib, lib.dp_index_map_create(ptr, 4, None), "dp_index_map_create", "NULL")
    _refused(lib, lib.dp_index_map_info(None, None, None, None), "dp_index_map_info", "NULL")
    lib.dp_index_map_destroy(None)
    for K, slots in ((1, 2048), (512, 2048), (513, 4096), (1024, 4096)):
        m = _map(lib, K, K)
        k, s, p = C.c_int(), C.c_int(), C.c_int()
        assert lib.dp_index_map_info(m, C.byref(k), C.byref(s), C.byref(p)) == 0
        assert (k.value, s.value) == (K, slots) and 0 <= p.value <= MAX_PROBE
        assert lib.dp_index_map_info(m, None, None, None) == 0
        lib.dp_index_map_destroy(m)


@pytest.mark.parametrize("fn", ["dp_index_from_rgb_u8", "dp_rgb_from_index_u8"])
def test_conversion_refusals(lib, fn):
    f = getattr(lib, fn)
    small, large = _map(lib, 16), _map(lib, 257)
    # pointers are never dereferenced by a refused call; (a, b) = (rgb, index) or (index, rgb)
    plane_first = fn == "dp_rgb_from_index_u8"
    def call(rgb=0x1000, index=0x2000, n=8, m=small, nb=1, cnt=0x3000):
        a, b = (index, rgb) if plane_first else (rgb, index)
        return f(a, b, n, m, nb, cnt, None)
    _refused(lib, call(rgb=None), fn, "NULL")
    _refused(lib, call(index=None), fn, "NULL")
    _refused(lib, call(m=None), fn, "NULL")
    _refused(lib, call(cnt=None), fn, "NULL")
    _refused(lib, call(n=-1), fn, "negative")
    for nb in (0, 3, 4, -1):
        _refused(lib, call(nb=nb), fn, "index_bytes must be 1 or 2", str(nb))
    _refused(lib, call(m=large, nb=1), fn, "one-byte", "257")
    _refused(lib, call(index=0x2001, nb=2), fn, "even address")
    _refused(lib, call(index=0x2001, m=large, nb=2), fn, "even address")
    _refused(lib, call(cnt=0x3004), fn, "8-byte aligned")
    # nothing to do is not an error, and needs neither a device nor an upload
    assert call(n=0) == 0 and call(n=0, m=large, nb=2) == 0 and call(n=0, index=0x2001) == 0
    lib.dp_index_map_destroy(small)
    lib.dp_index_map_destroy(large)


def test_plane_resize_refusals(lib):
    fn = "dp_resize_nearest_plane_u8"
    f = lib.dp_resize_nearest_plane_u8
    ok = dict(a=0x1000, b=0x2000, n=1, h=4, w=4, oh=8, ow=8, eb=1)
    def call(**kw):
        v = dict(ok, **kw)
        return f(v["a"], v["b"], v["n"], v["h"], v["w"], v["oh"], v["ow"], v["eb"], None)
    _refused(lib, call(a=None), fn, "NULL")
    _refused(lib, call(b=None), fn, "NULL")
    for bad in (dict(n=-1), dict(h=0), dict(w=0), dict(oh=0), dict(ow=-3)):
        _refused(lib, call(**bad), fn, "sizes")
    for eb in (0, 3, 4):
        _refused(lib, call(eb=eb), fn, "elem_bytes must be 1 or 2", str(eb))
    _refused(lib, call(a=0x1001, eb=2), fn, "even address")
    _refused(lib, call(b=0x2001, eb=2), fn, "even address")
    for big in (dict(oh=65536), dict(n=65536)):
        assert call(**big) == 2 and fn.encode() in lib.dp_last_error()      # DP_EUNSUPPORTED
    assert call(n=0) == 0
