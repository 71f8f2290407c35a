"""CPU tier of the ordered dither's fine table (dither_pie_amd/csrc/host_logic.h: fine_pack -- candidate windows of 4 + 2 palette
entries shared by the 32^3 cells of 8 colours a side) and of the choice of its kernel (ordered_fine.h: fine_replaces).

The stand-alone host_asan build (`finepack`) brute-forces the sets of every cell -- N: the entries nearest to some colour of the
cell, T: everything up to the second distance -- packs them within the LDS budget and writes the table; this file checks the
table's invariants against sets computed here with numpy on a fixed sample of 512 cells, every one of their 512 colours:
  * a window holds six distinct palette entries, and its colours are those entries';
  * a cell mapped to window i > 0 has N inside the quad A[i] and T inside A[i] + the pair B[i];
  * a cell is wide (window 0) exactly when |N| > 4 or |T| > 6, and its flat list holds T, sixteen entries in index order;
  * the image the kernel stages is the parts in their order, and it fits the budget next to the thresholds of Bayer 8x8;
  * palr(256,7) leaves at most 2 % of the cells wide (measured: 1.13 %); a palette crowded into a corner of the cube is refused.
`fineplan` prints, for records of plan facts and fine-table facts, whether the fine kernel replaces the plan: compared case by
case with the restatement below."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import ordered_plan_ref as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
FINE_CELLS, QUAD, WINDOW, WIDE_LIST, FINE_IDS = 32 ** 3, 4, 6, ref.K_WIDE_LIST, 512
SAMPLE = np.sort(np.random.RandomState(5).choice(FINE_CELLS, 512, replace=False))


def fine_table_bytes(n_win, n_wide):
    return n_win * WINDOW * 4 + n_wide * WIDE_LIST * 4 + FINE_CELLS * 2 + FINE_IDS * 2


def fine_replaces(plan, ff):
    """ordered_fine.h, restated: the plain lean kernel on 8-entry blocks with integer thresholds in LDS, and everything fits."""
    return int(bool(ff["present"]) and plan["family"] == "lean" and plan["mode"] == 1 and plan["bw"] == 8 and plan["table"] == "plain8" and
               not plan["adapt"] and not plan["warp"] and not plan["half"] and
               fine_table_bytes(ff["n_win"], ff["n_wide"]) + ff["thr_bytes"] <= ref.K_LEAN_TAB_BYTES)


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


def _pack(harness, tmp_path, pal):
    pal = np.asarray(pal, np.uint8).reshape(-1, 3)
    K = len(pal)
    pal.tofile(tmp_path / "pal.u8")
    out = tmp_path / "fine.bin"
    line = harness("finepack", tmp_path / "pal.u8", K, out)[-1]
    raw = out.read_bytes()
    ok, n_win, n_wide, words = np.frombuffer(raw, "<i4", 4)
    t = dict(ok=int(ok), n_win=int(n_win), n_wide=int(n_wide), words=int(words), line=line)
    if not ok:
        return t
    at = 16
    for name, dt, n in (("off", "<u2", FINE_CELLS), ("win_idx", "<u2", n_win * WINDOW), ("wide_cell", "<u2", n_wide),
                        ("wide_idx", "<u2", n_wide * WIDE_LIST), ("quad", "<u4", n_win * QUAD), ("pair", "<u4", n_win * (WINDOW - QUAD)),
                        ("wide", "<u4", n_wide * WIDE_LIST), ("image", "<u4", words)):
        t[name] = np.frombuffer(raw, dt, n, at).astype(np.int64)
        at += n * int(dt[2])
    assert at == len(raw)
    return t


def _sets(pal, cell):
    """N and T of one cell by brute force: every one of its 512 colours against the whole palette."""
    pal = np.asarray(pal, np.int64).reshape(-1, 3)
    i = np.arange(512)
    x = np.stack([(cell & 31) * 8 + (i & 7), ((cell >> 5) & 31) * 8 + ((i >> 3) & 7), (cell >> 10) * 8 + (i >> 6)], -1)
    d = ((x[:, None, :] - pal[None, :, :]) ** 2).sum(-1)
    ds = np.sort(d, axis=1)
    return set(np.nonzero((d == ds[:, :1]).any(0))[0].tolist()), set(np.nonzero((d <= ds[:, 1:2]).any(0))[0].tolist())


def _check_table(pal, t):
    pal = np.asarray(pal, np.int64).reshape(-1, 3)
    K = len(pal)
    packed = pal[:, 0] | (pal[:, 1] << 8) | (pal[:, 2] << 16)
    win = t["win_idx"].reshape(-1, WINDOW)
    assert (win < K).all() and (win[0] == 0).all()                                 # the reserved window: entry 0 six times
    assert all(len(set(w.tolist())) == WINDOW for w in win[1:]), "a window repeats an entry"
    assert np.array_equal(t["quad"].reshape(-1, QUAD), packed[win[:, :QUAD]]) and np.array_equal(t["pair"].reshape(-1, 2), packed[win[:, QUAD:]])
    assert (t["off"] < t["n_win"]).all()
    wide_cells = t["wide_cell"].tolist()
    assert wide_cells == sorted(set(wide_cells)) and set(wide_cells) == set(np.nonzero(t["off"] == 0)[0].tolist())
    lists = t["wide_idx"].reshape(-1, WIDE_LIST)
    assert (lists < K).all() and (np.diff(lists, axis=1) > 0).all(), "a flat list is not in ascending index order"
    assert np.array_equal(t["wide"].reshape(-1, WIDE_LIST), packed[lists])
    n_wide_seen = 0
    for cell in SAMPLE.tolist():
        N, T = _sets(pal, cell)
        w = int(t["off"][cell])
        assert (w == 0) == (len(N) > QUAD or len(T) > WINDOW), (cell, w, sorted(N), sorted(T))
        if w == 0:
            n_wide_seen += 1
            assert len(T) <= WIDE_LIST and T <= set(lists[wide_cells.index(cell)].tolist()), (cell, sorted(T))
        else:
            assert N <= set(win[w, :QUAD].tolist()) and T <= set(win[w].tolist()), (cell, w, sorted(N), sorted(T), win[w].tolist())
    # the staged image: A | wide lists | B | windows of the cells | wide cell numbers padded with 0xffff
    ids = np.full(FINE_IDS, 0xffff, np.int64)
    ids[:t["n_wide"]] = t["wide_cell"]
    u16 = np.concatenate([t["off"], ids])
    image = np.concatenate([t["quad"], t["wide"], t["pair"], u16[0::2] | (u16[1::2] << 16)])
    assert np.array_equal(t["image"], image)
    assert len(image) * 4 == fine_table_bytes(t["n_win"], t["n_wide"]) and t["n_wide"] <= FINE_IDS
    assert len(image) % 2 == 0                              # the kernel stages it two words at a time, thresholds right behind
    assert len(image) * 4 + 8 * 11 * 4 <= ref.K_LEAN_TAB_BYTES, "table + Bayer 8x8 thresholds exceed the lean kernel's LDS"
    return n_wide_seen


@pytest.mark.parametrize("K,seed", [(256, 7), (256, 11), (64, 3)])
def test_packer_invariants_random_palettes(harness, tmp_path, K, seed):
    from oracle import oracle as orc
    pal = orc.palr(K, seed)
    t = _pack(harness, tmp_path, pal)
    print(t["line"])
    assert t["ok"] == 1, t["line"]
    seen = _check_table(pal, t)
    if (K, seed) == (256, 7):
        assert t["n_wide"] <= FINE_CELLS * 2 // 100, t["line"]      # measured: 370 cells, 1.13 %
        assert seen > 0, "the sample holds no wide cell"


def test_packer_refuses_a_crowded_palette(harness, tmp_path):
    """A median-cut palette of dark content: its colours crowd a corner of the cube, where the cells' sets exceed every list."""
    from PIL import Image
    from dither_pie_amd.dithering_lib import ColorReducer
    from oracle import oracle as orc
    pal = ColorReducer.reduce_colors(Image.fromarray(orc.imgl(120, 203, 5, "dark"), "RGB"), 256)
    assert 200 <= len(pal) <= 256
    longest = max(len(_sets(pal, (c[0] >> 3) | ((c[1] >> 3) << 5) | ((c[2] >> 3) << 10))[1]) for c in pal[::16])
    t = _pack(harness, tmp_path, pal)
    print(t["line"], "longest sampled T:", longest)
    assert t["ok"] == 0, t["line"]


# the pieces the cases of the kernel's choice are built from (here and in tests/test_ordered_fine_choice_cpu.py)
PLAIN8 = dict(cell_tab=1, tab_words=4096 * 8, tab_total=4096 * 8)
BAYER8 = dict(m=1, mpad=1, fpad=1, th_h=8, th_w=8, tw_pad=11)
BASE = dict(mode=ref.MATRIX, K=256, is_integer=1, n_inner=51, n_px=3 * 120 * 203, hw=120 * 203, w=203, y0=0, x0=0, aligned=1, cell_tab=0,
            tab_words=0, tab_total=0, cell_tab4=0, tab4_words=0, warp_tab=0, warp_words=0, warp_total=0, warp_bw=0, warp_adapt=0, adapt=0,
            cell_perm=0, cell_perm4=0, n_wide=0, n_wide4=0, comp_tab=0, comp_words=0, comp_warp=0, ftab=0, ftab_words=0, m=0, mpad=0,
            fpad=0, th_h=1, th_w=1, tw_pad=0, n_cus=8)
NO_SWITCH = dict.fromkeys(ref.SWITCH_FIELDS, 0)


def test_choice_of_the_fine_kernel(harness, tmp_path):
    plain8, bayer8, base, no_switch = PLAIN8, BAYER8, BASE, NO_SWITCH
    fine = dict(present=1, n_win=1793, n_wide=370)
    room = ref.K_LEAN_TAB_BYTES - fine_table_bytes(0, 370) - 8 * 11 * 4
    tables = (plain8, dict(plain8, cell_tab4=1, tab4_words=4096 * 4), dict(plain8, warp_tab=1, warp_bw=8, warp_words=33000, warp_total=33400),
              dict(plain8, adapt=1), dict(plain8, cell_perm=1, n_wide=3), {})
    thresholds = (bayer8, dict(m=1, mpad=1, fpad=1, th_h=16, th_w=16, tw_pad=19), dict(fpad=1, th_h=8, th_w=8, tw_pad=11),
                  dict(m=1, mpad=1, fpad=1, th_h=64, th_w=64, tw_pad=67))
    fines = (fine, dict(fine, present=0), dict(fine, n_win=room // 24), dict(fine, n_win=room // 24 + 1), dict(present=1, n_win=2, n_wide=0))
    cases = []
    for tab, thr, ff, mode, integer, aligned, fast_all in itertools.product(tables, thresholds, fines, (ref.NEAREST, ref.MATRIX, ref.IGN), (1, 0),
                                                                          (1, 0), (0, 1)):
        f = dict(base, **tab, **thr, mode=mode, is_integer=integer, aligned=aligned)
        cases.append((f, dict(no_switch, fast_all=fast_all), dict(ff, thr_bytes=f["th_h"] * f["tw_pad"] * 4)))
    want = [(ref.plan(f, sw), ff) for f, sw, ff in cases]
    answers = [fine_replaces(p, ff) for p, ff in want]
    assert 0 < sum(answers) < len(answers)
    # the headline case and the budget's edge, by hand
    head = [a for (p, ff), a, (f, sw, _) in zip(want, answers, cases) if f == dict(base, **plain8, **bayer8) and not sw["fast_all"]]
    assert head == [1, 0, 1, 0, 1], head
    rec = np.array([[f[k] for k in ref.FACT_FIELDS] + [sw[k] for k in ref.SWITCH_FIELDS] + [ff[k] for k in ("present", "n_win", "n_wide", "thr_bytes")]
                    for f, sw, ff in cases], dtype=np.int64).astype("<i4")
    rec.tofile(tmp_path / "cases.bin")
    got = harness("fineplan", tmp_path / "cases.bin", len(cases))
    assert len(got) == len(cases)
    for i, (line, (p, ff), a) in enumerate(zip(got, want, answers)):
        assert line == "fine %d %s %d" % (i, p["family"], a), (i, line, p, ff, cases[i][0])
