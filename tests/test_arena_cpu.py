"""CPU tier of the guarded arena (tests/arena.py): the layout arithmetic, the sensitivity of check() / unchanged() to the
five kinds of misbehaviour the GPU matrix relies on it to see (fake kernels on CPU tensors), and the rule that keeps the
matrix complete: every dp_* function of include/ditherpie_hip.h that takes a device pointer is named in the matrix
module's coverage table or in its exclusion list."""
import os
import re

import numpy as np
import pytest
import torch

import arena as ar
from conftest import ROOT


# ---------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("cursor", [0, 1, 15, 16, 17, 31, 32, 4096, 4099, 0x7f0000001230])
@pytest.mark.parametrize("off", [0, 1, 2, 3, 4, 8, 9, 13, 15])
@pytest.mark.parametrize("nbytes", [0, 1, 3, 16, 1000])
def test_place_residue_alignment_and_guards(cursor, off, nbytes):
    guard = 64
    start, end, nxt = ar.place(cursor, nbytes, off, guard)
    assert end - start == nbytes and nxt - end == guard           # exact size; the guard after begins at the next byte
    assert start % 16 == off                                      # the residue asked for
    if off == 0:
        assert start % 32 == 16                                   # 16-aligned and NOT 32-aligned
    else:
        low = off & -off
        assert start % low == 0 and start % (2 * low) != 0        # exactly as aligned as the residue's lowest bit
    assert guard <= start - cursor < guard + 32                   # the guard before: at least `guard`, no gap beyond the period


def test_place_with_a_wider_alignment_and_bad_arguments():
    start, _, _ = ar.place(5, 10, 0, 8, align=256)
    assert start % 512 == 256
    start, _, _ = ar.place(5, 10, 48, 8, align=256)
    assert start % 256 == 48
    for bad in (dict(align=8), dict(align=48), dict(offset_mod16=16), dict(offset_mod16=-1), dict(nbytes=-1), dict(guard=0)):
        kw = dict(cursor=0, nbytes=4, offset_mod16=0, guard=8, align=16)
        kw.update(bad)
        with pytest.raises(ValueError):
            ar.place(**kw)


def test_guard_rule():
    assert ar.guard_bytes(1) == 1 << 20 and ar.guard_bytes(3 << 20) == 3 << 20 and ar.guard_bytes(1 << 30) == 16 << 20


def _arena(seed=3):
    a = ar.Arena(ar.capacity_for([(100, 64), (37, 64), (64, 64), (24, 64)]), "cpu", seed)
    a.carve("in", 100, 1, 64)
    a.carve("out", 37, 3, 64)
    a.carve("ws", 64, 0, 64)
    a.carve("tab", 24, 9, 64)
    return a


def test_regions_do_not_overlap_and_have_the_asked_sizes_and_addresses():
    a = _arena()
    spans = []
    for name, (n, off) in {"in": (100, 1), "out": (37, 3), "ws": (64, 0), "tab": (24, 9)}.items():
        r = a.regions[name]
        v = a.view(name)
        assert v.numel() == n == r["end"] - r["start"] and v.data_ptr() == a.ptr(name) and a.ptr(name) % 16 == off
        assert r["start"] - r["g0"] >= 64 and r["g1"] - r["end"] == 64
        spans.append((r["g0"], r["g1"]))
    assert a.ptr("ws") % 32 == 16
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 == b0 and a0 < a1                               # back to back: every byte is a guard or a region
    assert spans[0][0] == 0 and spans[-1][1] <= a.buf.numel()
    a.check()
    with pytest.raises(ValueError):
        a.carve("in", 4, 0, 64)                                   # the name is taken
    with pytest.raises(ValueError):
        a.carve("huge", a.buf.numel(), 0, 64)                     # the arena is full
    with pytest.raises(ValueError):
        ar.Arena(1 << 12, "cpu", 0, min_guard=128).carve("x", 4, 0, 64)   # a guard below the arena's minimum


def test_patterns_are_seeded_not_constant_and_fills_mean_what_they_say():
    p = ar.pattern(4096, 1, 0)
    assert len(set(p.tolist())) > 200                             # every byte value occurs: no constant passes as the pattern
    assert torch.equal(p[100:200], ar.pattern(100, 1, 100))       # a function of (seed, arena offset)
    assert not torch.equal(p, ar.pattern(4096, 2, 0))
    a = _arena()
    a.fill("ws", "ones")
    assert np.isnan(a.get("ws", np.float32)).all() and np.isnan(a.get("ws", np.float64)).all()
    assert (a.get("ws", np.int32) == -1).all() and (a.get("ws", np.uint32) == 0xFFFFFFFF).all()
    a.fill("ws", "zeros")
    assert not a.get("ws").any()
    a.fill("ws", ar.noise(5))
    x = a.get("ws").copy()
    a.fill("ws", ar.noise(6))
    assert not np.array_equal(x, a.get("ws"))
    with pytest.raises(ValueError):
        a.fill("ws", "sevens")
    g = a.buf[a.regions["ws"]["end"]:a.regions["ws"]["g1"]].clone()
    a.reseed(99)
    assert not torch.equal(g, a.buf[a.regions["ws"]["end"]:a.regions["ws"]["g1"]])
    a.check()


# ---------------------------------------------------------------------------------------------------- sensitivity
def _fake_op(a, out_extra=0, out_before=0, touch_input=False, read_ws_first=False):
    """out = in[:37] + 1, through raw arena offsets as a kernel would address memory; the keyword arguments are its bugs."""
    src = a.view("in")
    r = a.regions["out"]
    n = 37
    val = src[:n] + 1
    if read_ws_first:
        val = val + a.view("ws")[:n]                              # scratch read before it was written
    a.view("ws")[:n] = val                                        # (a well-behaved op writes its scratch, then uses it)
    a.buf[r["start"] - out_before:r["start"] + n + out_extra] = torch.cat(
        [torch.full((out_before,), 7, dtype=torch.uint8), a.view("ws")[:n], torch.full((out_extra,), 7, dtype=torch.uint8)])
    if touch_input:
        src[50] ^= 1


def test_a_well_behaved_op_passes():
    a = _arena()
    a.put("in", np.arange(100, dtype=np.uint8))
    a.fill("tab", ar.noise(4))
    _fake_op(a)
    a.check()
    a.unchanged("in")
    a.unchanged("tab")
    assert np.array_equal(a.get("out"), np.arange(1, 38, dtype=np.uint8))


def test_one_byte_past_the_end_is_reported():
    a = _arena()
    _fake_op(a, out_extra=1)
    with pytest.raises(ar.ArenaError) as e:
        a.check()
    assert (e.value.region, e.value.side, e.value.offset, e.value.count) == ("out", "after", 0, 1)
    assert "'out' (after)" in str(e.value) and "offset 0" in str(e.value)


def test_one_byte_before_the_start_is_reported():
    a = _arena()
    _fake_op(a, out_before=1)
    with pytest.raises(ar.ArenaError) as e:
        a.check()
    assert (e.value.region, e.value.side, e.value.offset, e.value.count) == ("out", "before", -1, 1)


def test_the_guard_s_own_value_at_a_wrong_position_is_reported():
    """A constant-filled guard would accept its constant anywhere; the pattern does not: copy the guard's byte 5 to byte 9."""
    a = _arena()
    r = a.regions["out"]
    g = a.buf[r["end"]:r["g1"]]
    k = next(k for k in range(6, 64) if g[k] != g[5])
    g[k] = g[5]
    with pytest.raises(ar.ArenaError) as e:
        a.check()
    assert (e.value.region, e.value.side, e.value.offset, e.value.count) == ("out", "after", k, 1)


def test_a_modified_input_is_reported():
    a = _arena()
    a.put("in", np.arange(100, dtype=np.uint8))
    _fake_op(a, touch_input=True)
    a.check()                                                     # (no guard was hit: only unchanged() sees it)
    with pytest.raises(ar.ArenaError) as e:
        a.unchanged("in")
    assert (e.value.region, e.value.side, e.value.offset, e.value.count) == ("in", "inside", 50, 1)
    b = _arena()
    b.fill("tab", "ones")
    b.view("tab")[3] = 0
    with pytest.raises(ar.ArenaError) as e:
        b.unchanged("tab")
    assert (e.value.region, e.value.offset) == ("tab", 3)


def test_a_read_of_uninitialised_scratch_shows_as_fill_dependent_output():
    outs = []
    for fill in ("zeros", "ones", ar.noise(8)):
        a = _arena()
        a.put("in", np.arange(100, dtype=np.uint8))
        a.fill("ws", fill)
        _fake_op(a, read_ws_first=True)
        a.check()
        outs.append(a.get("out").copy())
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])
    good = []
    for fill in ("zeros", "ones", ar.noise(8)):
        a = _arena()
        a.put("in", np.arange(100, dtype=np.uint8))
        a.fill("ws", fill)
        _fake_op(a)
        good.append(a.get("out").copy())
    assert np.array_equal(good[0], good[1]) and np.array_equal(good[0], good[2])


# ---------------------------------------------------------------------------------------------------- coverage cannot rot
def _device_entry_points():
    with open(os.path.join(ROOT, "include", "ditherpie_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"typedef struct \w+ \{.*?\} \w+;", " ", text, flags=re.S)
    found = {}
    for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        found[m.group(1)] = bool(re.search(r"\w+_dev\b", m.group(2)))
    return found


def test_every_device_entry_point_is_in_the_matrix_or_excluded_with_a_reason():
    import test_gpu_memory_discipline as md
    from dither_pie_amd import _lib
    found = _device_entry_points()
    assert set(found) == set(_lib.EXPORTS), set(found) ^ set(_lib.EXPORTS)   # the parser sees the whole header
    with_dev = {n for n, d in found.items() if d}
    assert len(with_dev) >= 19 and {"dp_ordered_u8", "dp_halftone_pow_flags", "dp_ign_thresholds", "dp_kmeans_update"} <= with_dev
    assert not set(md.COVERAGE) & set(md.EXCLUDED)
    missing = with_dev - set(md.COVERAGE) - set(md.EXCLUDED)
    assert not missing, f"device entry points without a memory-discipline case: {sorted(missing)}"
    for name, tests in md.COVERAGE.items():
        assert name in found, name
        assert tests and all(callable(getattr(md, t, None)) and t.startswith("test_") for t in tests), (name, tests)
    for name, reason in md.EXCLUDED.items():
        assert name in with_dev, name
        assert isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name   # a one-line reason
