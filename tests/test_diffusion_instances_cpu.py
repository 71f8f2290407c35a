"""CPU tier: tests/diffusion_instances.py against itself, against the launchers' text and against the host tree builder.

The table names what tests/test_gpu_diffusion_instances.py must reach; here it is checked for consistency (every `expect` is a named
instance, the expects are NAMED - UNREACHED, UNREACHED holds only what it may), the boundary widths are recomputed from the launchers'
LDS conditions without the bisection, the conditions and constants restated in the table are looked up in csrc, and the inner-node
counts the queue choice depends on come from dp_kdtree_build_host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import diffusion_instances as di
from conftest import ROOT


def _src(name):
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "dither_pie_amd", "csrc", name)).read())


def test_table_is_consistent():
    expects = {c.expect[0] for c in di.CASES}
    assert expects <= di.NAMED, sorted(expects - di.NAMED)
    assert set(di.UNREACHED) <= di.NAMED
    assert not expects & set(di.UNREACHED), sorted(expects & set(di.UNREACHED))
    assert expects == di.NAMED - set(di.UNREACHED), f"in neither CASES nor UNREACHED: {sorted(di.NAMED - set(di.UNREACHED) - expects)}"
    assert all(isinstance(r, str) and len(r.strip()) > 20 for r in di.UNREACHED.values())
    for c in di.CASES:
        assert c.why.strip() and c.pal in di.PALETTES and c.entry in ("error_diffusion", "error_diffusion_numba", "hybrid_numba",
                                                                      "variable_diffusion", "variance_gate"), c


def test_unreached_holds_only_what_it_may():
    """only row-serial instances of kQueueLarge: never a whole family, a model of var_serial, a fused radius or a schedule"""
    for inst in di.UNREACHED:
        assert inst[0] in ("ed_rowserial", "os_rowserial") and inst[1] == di.QL, inst
    left = di.NAMED - set(di.UNREACHED)
    assert {i[0] for i in left} == {i[0] for i in di.NAMED}
    assert {("var_serial", cap, m) for cap in (di.QS, di.QL) for m in (1, 2, 3, 4)} <= left
    assert {("fused", r) for r in range(5)} | {("two_pass",)} <= left
    # every schedule of every family has a row
    fam = {"error_diffusion": "python", "error_diffusion_numba": "numba", "hybrid_numba": "numba", "variable_diffusion": "variable"}
    have = {(fam[c.entry], c.expect[1]) for c in di.CASES if c.expect[0][0] in ("ed_wavefront", "var_wavefront")}
    assert have == {(f, s) for f in di.FAMILIES for s in di.SCHEDULES}, have


def test_the_counts_of_the_issue():
    by = lambda k: {i for i in di.NAMED if i[0] == k}
    assert len([i for i in by("ed_wavefront") if not i[5]]) == 42 and len([i for i in by("ed_wavefront") if i[5]]) == 2
    assert [len(by(k)) for k in ("ed_rowserial", "ed_serial", "var_wavefront", "os_rowserial", "var_serial", "fused", "two_pass")] == [6, 3, 8, 6, 8, 5, 1]


def test_boundary_rows_equal_the_launchers_expressions():
    """the widest row solved from the inequality in closed form; the table's rows sit exactly there and one beyond"""
    for pal in di.ROWSERIAL_PALETTES:
        K = di.PALETTES[pal]
        extra = K * 16 if K > 64 else 0
        # (9 w + 4) * 4 + extra + 512 <= 161792  <=>  w <= ((161792 - 512 - extra) / 4 - 4) / 9
        w_ed = ((158 * 1024 - 512 - extra) // 4 - 4) // 9
        # (8 w + 768) * 4 + extra + 512 <= 161792  <=>  w <= ((161792 - 512 - extra) / 4 - 768) / 8
        w_os = ((158 * 1024 - 512 - extra) // 4 - 768) // 8
        assert di.BOUNDARY["ed", pal] == w_ed and di.BOUNDARY["os", pal] == w_os, (pal, w_ed, w_os)
        assert di.ed_rowserial_fits(w_ed, K) and not di.ed_rowserial_fits(w_ed + 1, K)
        assert di.os_rowserial_fits(w_os, K) and not di.os_rowserial_fits(w_os + 1, K)
        assert di.ed_rowserial_lds(w_ed, K) + 512 <= di.LDS_LIMIT and di.os_rowserial_lds(w_os, K) + 512 <= di.LDS_LIMIT
        widths = {c.shape[2] for c in di.CASES if c.pal == pal and c.id.startswith("edr-")}
        assert widths == {w_ed, w_ed + 1}, (pal, widths)
        widths = {c.shape[2] for c in di.CASES if c.pal == pal and c.id.startswith("osr-")}
        assert widths == {w_os, w_os + 1}, (pal, widths)
    # the figures of palettes of at most 64, of 256 and of 1024 colours
    assert (di.BOUNDARY["ed", "palr16"], di.BOUNDARY["ed", "palr256"], di.BOUNDARY["ed", "palr1024"]) == (4479, 4365, 4024)
    assert (di.BOUNDARY["os", "palr16"], di.BOUNDARY["os", "palr256"], di.BOUNDARY["os", "palr1024"]) == (4944, 4816, 4432)


def test_the_restated_conditions_are_the_launchers():
    ed, var, host = _src("ediff.hip"), _src("vardiff.hip"), _src("host_logic.h")
    assert "constexpr int kQueueSmall = 64;" in host and "constexpr int kQueueLarge = 256;" in host
    assert "constexpr int kMaxTaps = 16;" in ed and "constexpr int kMaxWaves = 16;" in ed and "constexpr int kNbWaves = 8;" in ed
    assert "constexpr int kVWaves = 12;" in var and "kGateMaxR = 4" in var
    assert "((size_t)9 * w + 4) * sizeof(float) + (pal.K > 64 ? (size_t)pal.K * 16 : 0) + 512 <= (size_t)158 * 1024" in ed
    assert "((((size_t)9 * w + 3) & ~(size_t)3)) * sizeof(float) + (pal.K > 64 ? (size_t)pal.K * 16 : 0)" in ed
    assert "((size_t)8 * w + 768) * sizeof(float) + (pal.K > 64 ? (size_t)pal.K * 16 : 0) + 512 <= (size_t)158 * 1024" in var
    assert "!serpentine && skew * 2 + 2 <= kRing && w < 60000" in ed and "!(model == 4 && serpentine) && w < 60000" in var
    assert "n_frames * 2 <= cus && n_bands >= 4 && w >= 64" in ed and "n_frames * 2 <= cus && n_bands >= 4 && w >= 64" in var
    assert ed.count("G == 1 && nw > 4 && cus > 0 && n_frames > cus") == 1 and var.count("G == 1 && nw > 4 && cus > 0 && n_frames > cus") == 1
    for n, exact in di.TAP_INSTANCES:      # the tap counts with an instance of their own
        assert (f"case {n}: DP_EDN({n}, true);" in ed) if exact else ("default: DP_EDN(kMaxTaps, false);" in ed)
    assert len(re.findall(r"case \d+: DP_EDN", ed)) == len(di.TAP_INSTANCES) - 1
    assert [int(r) for r in re.findall(r"case (\d): DP_GATE", var)] == [0, 1, 2, 3] and "default: DP_GATE(4);" in var


def test_parse_trace():
    err = ("dp_diffusion: kernel=ed_wavefront CAP=kQueueLarge NT=kMaxTaps EXACT=false MAXW=kMaxWaves NB=false PALS=0 schedule=persistent G=1 "
           "grid=256 waves=6 lds=0 K=300 n_inner=32 model=0 numba=0 serpentine=0 repair=0\nnoise\n"
           "dp_diffusion: kernel=var_serial CAP=kQueueSmall schedule=serial G=1 grid=2 waves=1 lds=0 K=16 n_inner=1 model=3 numba=0 serpentine=0 repair=0\n"
           "dp_diffusion: kernel=os_rowserial CAP=kQueueLarge M=4 schedule=rowserial G=1 grid=2 waves=1 lds=160384 K=200 n_inner=76 model=4 numba=0 serpentine=1 repair=0\n"
           "dp_variance_gate: kernel=fused radius=4 chunk=3\ndp_variance_gate: kernel=two_pass radius=2 chunk=1\n")
    t = di.parse_trace(err)
    assert [x.instance for x in t] == [("ed_wavefront", 256, 16, False, 16, False, 0), ("var_serial", 64, 3), ("os_rowserial", 256, 4),
                                       ("fused", 4), ("two_pass",)]
    assert t[0].schedule == "persistent" and t[0].grid == 256 and t[0].K == 300 and t[2].lds == 160384 and t[2].serpentine == 1
    assert all(x.instance in di.NAMED for x in t)


@pytest.fixture(scope="module")
def lib():
    import dither_pie_amd
    if not os.path.exists(dither_pie_amd._lib.LIB_PATH):
        dither_pie_amd.build()
    return dither_pie_amd.load()


def _n_inner(lib, P):
    P = np.ascontiguousarray(P, np.float64)
    K = len(P)
    n = 2 * K + 2
    idx = np.zeros(K, np.int32)
    sd, st, en, le, gr = (np.zeros(n, np.int32) for _ in range(5))
    sp = np.zeros(n, np.float64)
    nn = C.c_int()
    assert lib.dp_kdtree_build_host(P.ctypes.data, K, idx.ctypes.data, sd.ctypes.data, sp.ctypes.data, st.ctypes.data, en.ctypes.data,
                                    le.ctypes.data, gr.ctypes.data, C.byref(nn)) == 0
    return int((sd[:nn.value] >= 0).sum())


def test_inner_nodes_of_the_palettes(lib, orc):
    """the queue choice of every row rests on these; degenerate200 is the palette of 65 .. 256 colours with more than 64 inner nodes"""
    for name, K in di.PALETTES.items():
        P = di.palette_f32(orc, name)
        assert P.shape == (K, 3) and P.dtype == np.float32 and P.min() >= 0 and P.max() <= 255
        assert _n_inner(lib, P) == di.N_INNER[name], name
    assert 64 < di.PALETTES["degenerate200"] <= 256 and di.N_INNER["degenerate200"] > di.QS
    assert all(di.N_INNER[n] <= K - 1 for n, K in di.PALETTES.items())


def test_custom_tap_sets_are_what_they_claim():
    for name, (taps, div) in di.CUSTOM_TAPS.items():
        assert len(taps) <= 16 and sum(t[2] for t in taps) <= div
        assert all((dy > 0 or (dy == 0 and dx > 0)) and dy <= 2 and -2 <= dx <= 2 for dx, dy, _ in taps), name
        order = sorted(range(len(taps)), key=lambda i: (-taps[i][1], -taps[i][0]))
        if name != "row2":
            assert order != list(range(len(taps))), f"{name} is already in visiting order"
            pos = [t[:2] for t in taps]
            dup = {p for p in pos if pos.count(p) == 2}
            assert dup and all(len({t[2] for t in taps if t[:2] == p}) == 2 for p in dup), name
        assert (di.TAP_COUNTS[name], True) not in di.TAP_INSTANCES, f"{name} would take a tap-count instance, not the generic one"
    assert {t[1] for t in di.CUSTOM_TAPS["row2"][0]} == {2}
    assert len(di.CUSTOM_TAPS["custom5"][0]) == 5 and len(di.CUSTOM_TAPS["custom16"][0]) == 16
    assert len({t[:2] for t in di.CUSTOM_TAPS["custom16"][0]}) == 12      # every causal position of the window
