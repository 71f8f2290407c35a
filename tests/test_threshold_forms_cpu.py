"""CPU tier of the threshold-form catalogue (tests/threshold_forms.py): its self-checks, and the oracle against the plain
statement of the matrix rule on every catalogue matrix at every geometry -- non-square matrices, widths below the pad, tables
without a padded copy, origins up to 2^30: shapes and origins the golden fixtures (square matrices, small origins) never
reached.  The GPU tier compares the kernels with the oracle on the same cases (tests/test_gpu_threshold_forms.py)."""
import numpy as np
import pytest

import threshold_forms as tf

UNDECIDED_MAX = 0.01   # share of pixels per case whose two (or second and third) nearest entries are equally far: a condition


def test_catalogue_claims_hold():
    tf.check_catalogue()
    names = [n for n, _, _ in tf.CATALOGUE]
    assert len(set(names)) == len(names) >= 19
    forms = tf.FORMS
    assert any(f["sh"] >= 0 and f["padded"] for f in forms.values())         # integer form behind padded rows
    assert any(f["sh"] < 0 and f["padded"] for f in forms.values())          # float32 only
    assert any(f["sh"] >= 0 and not f["padded"] for f in forms.values())     # integer form, no padded copy
    assert any(f["sh"] < 0 and not f["padded"] for f in forms.values())
    assert any(f["sh"] == tf.MAX_SHIFT for f in forms.values())
    assert {f["pow2"] for f in forms.values()} == {True, False}
    assert sum(f["nibbles"] is not None and f["nibbles"].any() for f in forms.values()) >= 4


def test_class_nibbles_follow_the_construction():
    """_classes: bit q of nibble (r, p) is set exactly when (p + q) % 4 == r % 4."""
    for name in ("cls4x64", "cls2x128", "cls1x256", "cls16x16"):
        nib = tf.FORMS[name]["nibbles"]
        th_h, th_w = nib.shape
        want = np.array([[sum(1 << q for q in range(4) if (p + q) % 4 == r % 4) for p in range(th_w)] for r in range(th_h)])
        assert np.array_equal(nib, want), name
    # the leading run of the wide rows: nibbles over 64 consecutive columns (a wrong lane stride) would set bits the rule clears
    for name in ("cls1x256", "cls2x128"):
        m = tf.MATRICES[name]
        th_w = m.shape[1]
        for p0 in range(4):
            assert all(m[0, (p0 + lane + q) % th_w] >= 0.5 for lane in range(64) for q in range(4)), name
            assert tf.FORMS[name]["nibbles"][0, p0] != 15


def test_host_form_on_known_matrices(orc):
    """The restated host rules on the matrices the suite had so far: Bayer matrices are dyadic, carry classes (columns x and
    x + 4 k coincide, or lie on the same side of 1/2), and the 16 x 16 one holds t = 1.0 = 256 / 256."""
    for size, th in (("2x2", 2), ("4x4", 4), ("8x8", 8), ("16x16", 16)):
        b = tf.host_form(orc.bayer_matrix(size))
        assert 0 <= b["sh"] <= 8 and b["pow2"] and b["tw_pad"] == th + 3 and b["nibbles"] is not None and b["nibbles"].any(), size
    assert tf.host_form(orc.bayer_matrix("16x16"))["sh"] == 8 and orc.bayer_matrix("16x16").max() == 1.0
    bn = tf.host_form(orc.blue_noise(33, 5))
    assert not bn["pow2"] and bn["padded"] and bn["tw_pad"] == 36 and bn["nibbles"] is None


def test_padded_rows_and_integer_table():
    m = tf.MATRICES["col5x1"]
    assert np.array_equal(tf.padded_rows(m), np.repeat(m, 4, axis=1))          # th_w = 1: the pad wraps three times
    assert np.array_equal(tf.padded_rows(tf.MATRICES["m3x2"])[:, 2:], tf.MATRICES["m3x2"][:, [0, 1, 0]])
    assert tf.integer_table(m, 3).reshape(-1).tolist() == [0, 3, 5, 8, 1]
    t = tf.integer_table(tf.MATRICES["sh13_128x64"], 13)
    assert t.max() == 8192 and t.min() == 0 and 8191 in t


def test_geometries():
    for name, m, _ in tf.CATALOGUE:
        geo = tf.geometries(m.shape)
        assert len(geo) == 5 and geo[0] == (37, 131, 0, 0) and geo[1] == (37, 131, 5, 3)
        th_h, th_w = m.shape
        h, w, y0, x0 = geo[2]
        assert 0 <= y0 < th_h and 0 <= x0 < th_w
        if th_h > 20:
            assert y0 + 20 == th_h                                             # the row wrap falls inside the 37 rows
        if th_w > 60:
            assert x0 + 60 == th_w
        h, w, y0, x0 = geo[3]
        assert y0 + h == 1 << 30 and x0 + w == 1 << 30
        assert all(y0 + h <= 1 << 30 and x0 + w <= 1 << 30 and y0 >= 0 and x0 >= 0 for h, w, y0, x0 in geo)


def test_matrix_rule_on_a_hand_case():
    """Two entries, one pixel: d0 = 1, d1 = 9, factor = 0.1; thresholds on both sides of it and exactly on it."""
    pal = np.array([[10, 0, 0], [14, 0, 0]], np.float32)
    outc = pal.astype(np.uint8)
    px = np.array([[[11, 0, 0]]], np.uint8)
    for t, want in ((0.25, 10), (0.0625, 14), (np.float32(0.1), 10)):          # float32(0.1) > 0.1: nearest
        out, und = tf.matrix_rule(px, pal, outc, None, np.array([[t]], np.float32), 7, 9)
        assert out[0, 0, 0] == want and not und.any()
    out, und = tf.matrix_rule(np.array([[[12, 0, 0]]], np.uint8), pal, outc, None, np.array([[0.75]], np.float32), 0, 0)
    assert und.all()
    out, und = tf.matrix_rule(np.array([[[10, 0, 0]]], np.uint8), pal, outc, None, np.array([[0.0]], np.float32), 0, 0)
    assert out[0, 0, 0] == 10 and not und.any()                                # total > 0, factor 0 <= 0
    # the position in the matrix: Python-integer modulo of the origin plus the pixel
    thr = np.array([[0.0625, 0.25, 0.0625]], np.float32)
    row = np.repeat(px, 4, axis=1)
    out, _ = tf.matrix_rule(row, pal, outc, None, thr, 0, (1 << 30) - 4)       # (2^30 - 4) % 3 = 0
    assert out[0, :, 0].tolist() == [14, 10, 14, 14]


PALETTES = [("palr16", 16, 7, False), ("gamma64", 64, 7, True)]


@pytest.mark.parametrize("pal_name,K,pseed,gamma", PALETTES, ids=[p[0] for p in PALETTES])
@pytest.mark.parametrize("name", [n for n, _, _ in tf.CATALOGUE])
def test_oracle_follows_the_matrix_rule(orc, capsys, name, pal_name, K, pseed, gamma):
    pal_f32, outc, lut = orc.prepare_palette(orc.palr(K, pseed), gamma)
    thr = tf.MATRICES[name]
    for i, (h, w, y0, x0) in enumerate(tf.geometries(thr.shape)):
        arr = orc.rnd(h, w, 300 + i)
        want, undecided = tf.matrix_rule(arr, pal_f32, outc, lut, thr, y0, x0)
        got = orc.ordered_u8(arr, pal_f32, outc, lut, "matrix", thr=thr, y0=y0, x0=x0)
        share = undecided.mean()
        with capsys.disabled():
            print(f"\n  {name} {pal_name} origin ({y0}, {x0}): undecided {100.0 * share:.3f} %", end="")
        assert share <= UNDECIDED_MAX, (name, pal_name, (y0, x0), share)
        bad = np.argwhere((got != want).any(-1) & ~undecided)
        assert len(bad) == 0, (f"{name} {pal_name} origin ({y0}, {x0}): the oracle differs from the matrix rule on {len(bad)} decided "
                               f"pixels, first at {bad[:4].tolist()}: colours {arr[tuple(bad[0])].tolist()}")
