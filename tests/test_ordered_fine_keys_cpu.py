"""CPU tier of the key levels of ordered_fine_kernel (dither_pie_amd/csrc/ordered.hip, ordered_fine.h: fine_keys_level).

At levels 1 and 2 the kernel stages, next to the colours of a window, the part of every candidate key that does not depend on the
pixel -- N_j = (|c_j|^2 << 8) + 4 j -- and forms a key with two instructions, v_dot4_u32_u8 (x . c) and v_mad_i32_i24 (p, -512, N),
where level 0 takes four.  The level is a pure function of the table's size and the thresholds' (what LDS holds; the library launches it up to
kFineKeysShipped, the experiments build up to DP_FINE_KEYS_MAX):
  * `finekeys` of the stand-alone host_asan build prints it for records of FineFacts; compared here case by case with a restatement,
    over window counts on both sides of every edge of the budget, and by hand for the headline and the two edges;
  * the identity the change rests on, with numpy on the table `finepack` writes for palr(256,7): for every window (window 0, six equal
    entries, included) and 4096 random colours, N + sext24(-512) * sext24(x . c) in 32-bit arithmetic is today's key
    ((|c|^2 - 2 x . c) << 8) + 4 j, and both factors are within the 24 bits the multiply reads."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import ordered_plan_ref as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "dither_pie_amd", "csrc")
FINE_CELLS, QUAD, WINDOW, WIDE_LIST, FINE_IDS = 32 ** 3, 4, 6, ref.K_WIDE_LIST, 512
LOCAL_BITS = 8
NEG2 = -(2 << LOCAL_BITS)


def fine_keys_bytes(level, n_win):
    """ordered_fine.h, restated: quads A and their norms, 16 B each, pairs B of 8 B (level 1) or records B' of 16 B (level 2), the
    window of every cell and the numbers of the wide cells; the flat lists stay in global memory."""
    return n_win * (48 if level == 2 else 40) + FINE_CELLS * 2 + FINE_IDS * 2


def fine_keys_level(ff):
    if not ff["present"]:
        return 0
    for level in (2, 1):
        if fine_keys_bytes(level, ff["n_win"]) + ff["thr_bytes"] <= ref.K_LEAN_TAB_BYTES:
            return level
    return 0


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


def _levels(harness, tmp_path, facts):
    rec = np.array([[ff[k] for k in ("present", "n_win", "n_wide", "thr_bytes")] for ff in facts], dtype=np.int64).astype("<i4")
    rec.tofile(tmp_path / "keys.bin")
    got = harness("finekeys", tmp_path / "keys.bin", len(facts))
    assert len(got) == len(facts)
    out = []
    for i, line in enumerate(got):
        word, idx, level = line.split()
        assert word == "keys" and int(idx) == i, line
        out.append(int(level))
    return out


def test_level_against_the_restatement(harness, tmp_path):
    wins = (2, 1793, 1830, 1831, 1848, 1849, 2219, 2220, 2710)
    thr_words = (8 * 11, 16 * 19, 64 * 67)
    facts = [dict(present=present, n_win=n, n_wide=370, thr_bytes=t * 4) for n, t, present in itertools.product(wins, thr_words, (1, 0))]
    want = [fine_keys_level(ff) for ff in facts]
    assert {0, 1, 2} == set(want)
    got = _levels(harness, tmp_path, facts)
    for ff, w, g in zip(facts, want, got):
        assert g == w, (ff, w, g)


def test_level_by_hand(harness, tmp_path):
    bayer8 = 8 * 11 * 4
    assert bayer8 == 352
    # beside the thresholds of Bayer 8x8: 48 n + 66560 + 352 <= 155648 up to n = 1848, 40 n + ... up to n = 2218
    facts = [dict(present=1, n_win=n, n_wide=370, thr_bytes=bayer8) for n in (1821, 1848, 1849, 2218, 2219, 2220)]
    # beside those of a 16 x 16 matrix (1216 B): level 2 up to n = 1830
    facts.append(dict(present=1, n_win=1830, n_wide=370, thr_bytes=16 * 19 * 4))
    facts.append(dict(present=1, n_win=1831, n_wide=370, thr_bytes=16 * 19 * 4))
    assert _levels(harness, tmp_path, facts) == [2, 2, 1, 1, 0, 0, 2, 1]


def _sext24(v):
    v = np.asarray(v, np.int64) & 0xffffff
    return np.where(v & 0x800000, v - (1 << 24), v)


def _wrap32(v):
    v = np.asarray(v, np.int64) & 0xffffffff
    return np.where(v & 0x80000000, v - (1 << 32), v)


def test_staged_norm_keys_equal_todays(harness, tmp_path):
    from oracle import oracle as orc
    pal = np.asarray(orc.palr(256, 7), np.uint8).reshape(-1, 3)
    pal.tofile(tmp_path / "pal.u8")
    out = tmp_path / "fine.bin"
    line = harness("finepack", tmp_path / "pal.u8", len(pal), out)[-1]
    raw = out.read_bytes()
    ok, n_win, n_wide, words = (int(v) for v in np.frombuffer(raw, "<i4", 4))
    assert ok == 1, line
    at = 16 + 2 * (FINE_CELLS + n_win * WINDOW + n_wide + n_wide * WIDE_LIST)
    quad = np.frombuffer(raw, "<u4", n_win * QUAD, at).astype(np.int64).reshape(n_win, QUAD)
    pair = np.frombuffer(raw, "<u4", n_win * (WINDOW - QUAD), at + 4 * n_win * QUAD).astype(np.int64).reshape(n_win, WINDOW - QUAD)
    win = np.concatenate([quad, pair], axis=1)                          # [n_win, 6] colour words, top byte 0
    assert (win >> 24 == 0).all() and (win[0] == win[0, 0]).all()       # window 0: six equal entries
    c = np.stack([win & 255, (win >> 8) & 255, (win >> 16) & 255], -1)  # [n_win, 6, 3]
    tag = 4 * np.arange(WINDOW, dtype=np.int64)
    norm = (c * c).sum(-1)                                              # what v_dot4_u32_u8(c, c) gives
    staged = _wrap32((norm << LOCAL_BITS) + tag)                        # the word the stager writes
    assert (staged >= 0).all() and (staged & 0xff == tag).all()
    x = np.random.RandomState(17).randint(0, 256, (4096, 3)).astype(np.int64)
    x[:4] = [[0, 0, 0], [255, 255, 255], [255, 0, 255], [0, 255, 0]]
    for lo in range(0, n_win, 256):                                     # (in slices: 1821 x 6 x 4096 keys)
        cw = c[lo:lo + 256]
        p = np.einsum("wjk,nk->nwj", cw, x)                             # v_dot4_u32_u8(x, c)
        assert p.min() >= 0 and p.max() < 1 << 23 and -(1 << 23) <= NEG2    # both factors are 24-bit signed values
        key = _wrap32(_sext24(p) * _sext24(NEG2) + staged[None, lo:lo + 256])   # v_mad_i32_i24(p, neg2, N)
        today = ((norm[None, lo:lo + 256] - 2 * p) << LOCAL_BITS) + tag
        assert (np.abs(today) < 1 << 31).all()
        assert np.array_equal(key, today)
        if lo == 0:                                                     # window 0: equal distances, told apart by the tag alone
            assert (key[:, 0, :] >> LOCAL_BITS == key[:, 0, :1] >> LOCAL_BITS).all()
