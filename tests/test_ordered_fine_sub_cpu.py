"""CPU tier of the two-level fine table of the ordered dither (dither_pie_amd/csrc/host_logic.h: fine_pack_sub -- the 8-wide cells whose
sets are too long for a window of 4 + 2 get a row of eight windows, one per 4-wide sub-cell) and of the choice of its kernel level
(ordered_fine.h: fine_sub_level).

The stand-alone host_asan build (`finesub`) brute-forces the sets of every cell, packs cells and sub-cells together, twice, checks every
sub-cell's window against sets over the whole palette itself, and writes the table.  This file checks against numpy brute force:
  * every sub-cell of a wide cell that is not wide itself has a window with N(sub) inside the quad and T(sub) inside the six; every
    still-wide one has row entry 0 (the reserved window) and is listed;
  * every cell that is not wide satisfies what tests/test_ordered_fine_cpu.py checks for fine_pack (on the same sample of 512 cells);
    a wide cell's entry is the tag plus its rank, the rows are in ascending wide-cell order, the flat lists hold T;
  * the image is the parts in their order and as large as the budget function says; the LDS layout fits beside Bayer 8x8;
  * palr(256,7): 370 wide cells, 2063 windows, 82 sub-cells still wide (the figures DESIGN 4.1 records);
  * fine_sub_level case by case against a restatement, with a table one window over the budget and 513 wide cells;
  * on 4096 seeded colours of wide cells the window reached through the row ranks (m0, m1, m2) as the whole palette does;
  * tests/golden/fine_sub_palr256_7.npz (the wide cells and the still-wide sub-cells; the GPU tier draws its frames from it) is what the
    harness reports now."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import fine_sub_ref as fs
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
SAMPLE = np.sort(np.random.RandomState(5).choice(fs.FINE_CELLS, 512, replace=False))   # the sample of test_ordered_fine_cpu.py


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


_TABLES = {}   # (K, seed) -> (palette, table): packed once, never written again


def _table(harness, tmp_path_factory, K, seed):
    if (K, seed) not in _TABLES:
        from oracle import oracle as orc
        pal = np.asarray(orc.palr(K, seed), np.uint8).reshape(-1, 3)
        d = tmp_path_factory.mktemp("finesub")
        pal.tofile(d / "pal.u8")
        line = harness("finesub", d / "pal.u8", K, d / "sub.bin")[-1]
        t = fs.read_table((d / "sub.bin").read_bytes())
        t["line"] = line
        print(line)
        _TABLES[(K, seed)] = (pal.astype(np.int64), t)
    return _TABLES[(K, seed)]


@pytest.mark.parametrize("K,seed", [(256, 7), (256, 11), (64, 3)])
def test_table_against_brute_force(harness, tmp_path_factory, K, seed):
    pal, t = _table(harness, tmp_path_factory, K, seed)
    assert t["ok"] == 1 and " bad=0" in t["line"], t["line"]
    packed = pal[:, 0] | (pal[:, 1] << 8) | (pal[:, 2] << 16)
    win = t["win_idx"].reshape(-1, fs.WINDOW)
    assert (win < K).all() and (win[0] == 0).all()
    assert all(len(set(w.tolist())) == fs.WINDOW for w in win[1:]), "a window repeats an entry"
    assert np.array_equal(t["quad"].reshape(-1, fs.QUAD), packed[win[:, :fs.QUAD]]) and np.array_equal(t["pair"].reshape(-1, 2), packed[win[:, fs.QUAD:]])
    wide_cells = t["wide_cell"].tolist()
    rows = t["rows"].reshape(-1, 8)
    lists = t["wide_idx"].reshape(-1, fs.WIDE_LIST)
    # tags: exactly the wide cells, each with its rank; the rows in ascending wide-cell order
    assert wide_cells == sorted(set(wide_cells)) and len(wide_cells) == t["n_wide"] <= fs.FINE_IDS
    tagged = np.nonzero(t["off"] >= fs.TAG)[0]
    assert tagged.tolist() == wide_cells and np.array_equal(t["off"][tagged], fs.TAG | np.arange(len(tagged)))
    plain = t["off"][t["off"] < fs.TAG]
    assert ((plain > 0) & (plain < t["n_win"])).all() and (rows < t["n_win"]).all()
    assert (lists < K).all() and (np.diff(lists, axis=1) > 0).all() and np.array_equal(t["wide"].reshape(-1, fs.WIDE_LIST), packed[lists])
    # every sub-cell of every wide cell
    still = []
    for k, cell in enumerate(wide_cells):
        Nc, Tc = fs.sets(pal, fs.colours(cell))
        assert len(Nc) > fs.QUAD or len(Tc) > fs.WINDOW, (cell, "is tagged but not wide")
        assert Tc <= set(lists[k].tolist())
        for s in range(8):
            x = fs.colours(cell, s)
            assert (fs.cell_of(x) == cell).all() and (fs.sub_of(x) == s).all()
            N, T = fs.sets(pal, x)
            w = int(rows[k, s])
            if len(N) > fs.QUAD or len(T) > fs.WINDOW:
                assert w == 0, (cell, s, "still wide, but its row entry is", w)
                still.append(8 * k + s)
            else:
                assert w > 0 and N <= set(win[w, :fs.QUAD].tolist()) and T <= set(win[w].tolist()), (cell, s, w, sorted(N), sorted(T), win[w].tolist())
    assert still == t["sub_wide"].tolist() and len(still) == t["n_still"]
    # the cells that are not wide: as for fine_pack
    n_wide_seen = 0
    for cell in SAMPLE.tolist():
        N, T = fs.sets(pal, fs.colours(cell))
        w = int(t["off"][cell])
        assert (w >= fs.TAG) == (len(N) > fs.QUAD or len(T) > fs.WINDOW), (cell, w, sorted(N), sorted(T))
        if w >= fs.TAG:
            n_wide_seen += 1
        else:
            assert N <= set(win[w, :fs.QUAD].tolist()) and T <= set(win[w].tolist()), (cell, w, sorted(N), sorted(T), win[w].tolist())
    # the image: A | flat lists | B | off | rows, two u16 per word
    u16 = np.concatenate([t["off"], t["rows"]])
    image = np.concatenate([t["quad"], t["wide"], t["pair"], u16[0::2] | (u16[1::2] << 16)])
    assert np.array_equal(t["image"], image)
    assert len(image) * 4 == fs.fine_sub_image_bytes(t["n_win"], t["n_wide"]) <= fs.LEAN_TAB_BYTES and len(image) % 2 == 0
    assert ("bytes=%d " % fs.fine_sub_bytes(t["n_win"], t["n_wide"])) in t["line"]
    assert fs.fine_sub_fits(t["n_win"], t["n_wide"])
    assert fs.fine_sub_bytes(t["n_win"], t["n_wide"]) + 8 * 11 * 4 <= fs.LEAN_TAB_BYTES, "table + Bayer 8x8 thresholds exceed the kernel's LDS"
    if (K, seed) == (256, 7):
        assert n_wide_seen > 0, "the sample holds no wide cell"
        assert (t["n_wide"], t["n_win"], t["n_still"]) == (370, 2063, 82), t["line"]


def test_fixture_is_what_the_harness_reports(harness, tmp_path_factory):
    _, t = _table(harness, tmp_path_factory, 256, 7)
    fx = np.load(fs.FIXTURE)
    assert sorted(fx.files) == ["sub_wide", "wide_cell"]
    assert np.array_equal(fx["wide_cell"], t["wide_cell"]) and np.array_equal(fx["sub_wide"], t["sub_wide"])
    assert len(fx["wide_cell"]) == 370 and os.path.getsize(fs.FIXTURE) < 4096
    rgb = fs.wide_only_colours(256 * 64, 1).astype(np.int64)
    assert set(fs.cell_of(rgb).tolist()) == set(t["wide_cell"].tolist())
    assert len(set((fs.cell_of(rgb) * 8 + fs.sub_of(rgb)).tolist())) == 8 * 370


def test_level_function(harness, tmp_path):
    bayer8, m16, m64 = 8 * 11 * 4, 16 * 19 * 4, 64 * 67 * 4
    edge = (fs.LEAN_TAB_BYTES - bayer8 - fs.FINE_CELLS * 2 - 370 * 16) // 40   # the most windows that fit beside Bayer 8x8 and 370 rows
    cases = []
    for present, (n_win, n_wide), thr, keys, cap in itertools.product((1, 0), ((2063, 370), (edge, 370), (edge + 1, 370), (1500, 512), (1500, 513), (2, 0)),
                                                                  (bayer8, m16, m64), (0, 1, 2), (0, 1, 2, 3)):
        cases.append(dict(present=present, n_win=n_win, n_wide=n_wide, thr_bytes=thr, keys=keys, cap=cap))
    want = [fs.fine_sub_level(c) for c in cases]
    assert 0 < sum(1 for w in want if w) < len(want)

    def by_hand(**kw):
        return fs.fine_sub_level(dict(dict(present=1, n_win=2063, n_wide=370, thr_bytes=bayer8, keys=1, cap=2), **kw))
    assert by_hand() == 2 and by_hand(n_win=edge) == 2 and by_hand(n_win=edge + 1) == 0, "one window over the budget keeps today's layout"
    assert by_hand(n_win=1500, n_wide=512) == 2 and by_hand(n_win=1500, n_wide=513) == 0
    assert by_hand(keys=0) == 0 and by_hand(keys=2) == 0 and by_hand(cap=0) == 0 and by_hand(cap=1) == 1 and by_hand(cap=3) == 2 and by_hand(present=0) == 0 and by_hand(thr_bytes=m64) == 0
    rec = np.array([[c[k] for k in ("present", "n_win", "n_wide", "thr_bytes", "keys", "cap")] for c in cases], dtype="<i4")
    rec.tofile(tmp_path / "cases.bin")
    got = harness("finesublevel", tmp_path / "cases.bin", len(cases))
    assert got == ["sub %d %d" % (i, w) for i, w in enumerate(want)]


def test_key_identity_through_the_rows(harness, tmp_path_factory):
    """4096 seeded colours of wide cells: the keys of the six entries of the window reached through the row -- (|c|^2 << 8) + 4 * position
    - 2 * (x . c) << 8, what cand4k / cand6k rank -- put the same entries first, second and third, by true distance, as the whole palette."""
    pal, t = _table(harness, tmp_path_factory, 256, 7)
    win = t["win_idx"].reshape(-1, fs.WINDOW)
    rows = t["rows"].reshape(-1, 8)
    rgb = fs.wide_only_colours(4096, 2).astype(np.int64)
    rank = t["off"][fs.cell_of(rgb)] - fs.TAG
    assert (rank >= 0).all()
    w = rows[rank, fs.sub_of(rgb)]
    seen = 0
    for x, wi in zip(rgb, w):
        if wi == 0:
            continue
        seen += 1
        c = pal[win[wi]]
        keys = ((c * c).sum(-1) << 8) + 4 * np.arange(fs.WINDOW) - ((2 * (c * x).sum(-1)) << 8)
        order = np.sort(keys)[:3]
        d_win = (order >> 8) + int((x * x).sum())
        d_all = np.sort(((pal - x) ** 2).sum(-1))
        assert d_win[0] == d_all[0] and d_win[1] == d_all[1], (x.tolist(), int(wi), d_win.tolist(), d_all[:3].tolist())
        # every entry at the nearest distance is in the quad; the third key's distance is the palette's third unless further ties hide
        near = set(np.nonzero(((pal - x) ** 2).sum(-1) == d_all[0])[0].tolist())
        assert near <= set(win[wi, :fs.QUAD].tolist())
        if d_all[2] == d_all[1]:
            assert d_win[2] == d_all[2], (x.tolist(), int(wi))
        else:
            assert d_win[2] >= d_all[2]
    assert seen > 3000
