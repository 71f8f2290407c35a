"""GPU tier of the threshold-form catalogue (tests/threshold_forms.py): dp_ordered_u8 in matrix mode on every form of threshold
table the host derives (integer / float32 only, power of two or not, padded copy or none, class nibbles, widths below the
pad), on every kernel family, at origins up to 2^30 -- bytes equal to the CPU oracle, which tests/test_threshold_forms_cpu.py
holds to the plain statement of the matrix rule on the same cases.

  (a) every catalogue matrix x every geometry on ten families; on the experiments library the trace line of every launch is held to
      the plan (family, MODE, which kernel), and the catalogue must reach all four threshold paths: MODE 1 from LDS, MODE 2 from
      padded float rows with an integer form present, MODE 2 from float-only rows, and the fall-back without a padded copy;
      the same cases run on the library that ships;
  (b) the tile stride of the persistent grid (more tiles than workgroups) with matrices that are no power of two, tie-rich frames;
      and the class nibbles of wide tables in frames wide enough for a wave to consult them;
  (c) the Oklab kernel (its own position code) on non-square, narrow and unpadded matrices;
  (d) the device-side constructors against from_matrix of what they built;
  (e) the edge of acceptance: 2^20 entries, one row more, and the two sides of the padded copy's limit."""
import ctypes as C
import re

import numpy as np
import pytest

import metric_ref
import ordered_plan_ref as plan_ref
import threshold_forms as tf
from test_gpu_memory_discipline import FALLBACK, ORD_BIG, _ordered_family

pytestmark = pytest.mark.gpu

TRACE = re.compile(r"dp_ordered_u8: pass 1 = (\w+) \(4-byte aligned frames: (\d)\) mode=(\d) bw=(\d) adapt=(\d) warp=(\d) half=(\d) "
                   r"table=(\w+) fix_big_queue=\d kernel=(\w+)")
TABLE_KERNELS = {"lean", "fast", "compact"}
FLOAT_KERNELS = {"lean_float", "compact_float"}
NAMES = [n for n, _, _ in tf.CATALOGUE]

FAMILIES = ["brute16", "leanhalf27", "lean256", "compact64", "w8lean300", "lean300", "compactfloat256", "leanfloat64", "brutefloat300",
            "cell256"]


def _recipe(orc, family):
    """-> dict(pal, gamma, accel, env, odd, family): the palette and switches of a kernel family (the recipes of
    tests/test_gpu_memory_discipline.py where it has one), and the pass-1 family a padded matrix must reach with it."""
    rec = dict(gamma=False, accel=True, env={}, odd=False)
    if family == "leanhalf27":        # a lattice palette: 4-entry blocks with few split cells, small enough for two workgroups per CU
        rec.update(pal=orc.generate_uniform_palette(27), family="lean")
    elif family == "w8lean300":       # the 8-entry table over warped cells, forced: the warped, adaptive lean kernel
        rec.update(pal=orc.palr(300, 2), env={"DP_FORCE_TABLE": "w8"}, family="lean")
    elif family == "leanfloat64":     # use_gamma without the compact float kernel (tests/test_gpu_kernels.py: test_float_palette_cell_table)
        rec.update(pal=orc.palr(64, 31), gamma=True, env={"DP_NO_COMPACT_KERNEL": "1"}, family="lean_float")
    elif family == "cell256":         # the lean256 palette at odd addresses: the whole-table kernel
        pal, gamma, accel, _ = _ordered_family(orc, "lean256")
        rec.update(pal=pal, gamma=gamma, accel=accel, odd=True, family="cell")
    else:
        pal, gamma, accel, expect = _ordered_family(orc, family)
        rec.update(pal=pal, gamma=gamma, accel=accel, family=expect["bayer"])
    return rec


def _dev(a, odd=False):
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if not odd:
        return t
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() & 1
    return v


def _palette(be, orc, rec):
    pal_f32, out_colors, lut_in = orc.prepare_palette(rec["pal"], rec["gamma"])
    return be.Palette(pal_f32, out_colors, lut_in, accel=rec["accel"]), (pal_f32, out_colors, lut_in)


def _run(be, orc, P, prep, arr, thr_np, T, y0, x0, odd=False, capfd=None):
    """One call against the oracle -> (mismatch text or None, the trace tuples of its launches)."""
    import torch
    frames = arr if arr.ndim == 4 else arr[None]
    if capfd is not None:
        capfd.readouterr()
    out = _dev(np.zeros_like(arr), odd) if odd else None
    got = be.ordered(_dev(arr, odd), P, be.MODE_MATRIX, thr=T, y0=y0, x0=x0, out=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy().reshape(frames.shape)
    seen = TRACE.findall(capfd.readouterr().err) if capfd is not None else []
    ref = np.stack([orc.ordered_u8(f, *prep, "matrix", thr=thr_np, y0=y0, x0=x0) for f in frames])
    bad = np.argwhere((got != ref).any(-1))
    if len(bad) == 0:
        return None, seen
    b = tuple(bad[0])
    return (f"{len(bad)} pixels differ from the oracle, first at {bad[:4].tolist()}: colours {frames[b].tolist()}, "
            f"got {got[b].tolist()} for {ref[b].tolist()}"), seen


# ================================================================================================ (a) forms x families
# The MODE of a launch on an integer-form matrix is 1 when the padded integer rows fit in LDS behind the cell table, else 2.
# Where the size of that table can be read (the plain 8-entry table: dp_palette_accel_info) the plan's rule is restated;
# where it cannot, the catalogue's largest rows that fit behind the family's table and its smallest that do not are stated per
# family (bytes: int17x24 1 836, int64x32 8 960, sh13_128x64 34 304, int181x181 133 216): rows up to the first take MODE 1,
# rows from the second on MODE 2, and the catalogue has none in between.  No table leaves room for int181x181: the smallest,
# 4096 blocks of 4 entries, is 65 536 bytes of the lean kernels' 155 648; the compact kernel's table here is larger than the
# 27 808 bytes that would be left.
ROWS_FIT = {"leanhalf27": (34304, 133216), "compact64": (34304, 133216), "w8lean300": (1836, 8960)}


def _table_bytes(P, fam, table, warp):
    if fam == "lean" and table == "plain8" and not warp and P.accel_entries > 0:
        return 4 * P.accel_entries
    return None


def _expect(family, rec, P, name, traced):
    """What the plan (tests/ordered_plan_ref.py) says about one trace line, as far as the line and the palette tell its facts.
    -> (list of complaints, the threshold path the launch took)."""
    form, m = tf.FORMS[name], tf.MATRICES[name]
    fam, aligned, mode, bw, adapt, warp, half, table, kernel = traced
    mode, bw, adapt, warp, half = int(mode), int(bw), int(adapt), int(warp), int(half)
    rows_bytes = m.shape[0] * form["tw_pad"] * 4
    int_thr_ok = form["sh"] >= 0 and m.size <= 256
    integer_pal = not rec["gamma"]
    errs = []
    if (aligned == "1") == rec["odd"]:
        errs.append(f"aligned={aligned}")
    if rec["family"] == "brute":
        want_fam = {"brute"}
    elif rec["odd"]:
        want_fam = {"cell"}
    elif not form["padded"]:
        want_fam = FALLBACK               # no padded rows: no table kernel reads this matrix
    else:
        want_fam = {rec["family"]}
    if fam not in want_fam:
        errs.append(f"family {fam}, not {sorted(want_fam)}")
    if fam in FALLBACK:
        want_mode = 1 if integer_pal and int_thr_ok else 2
    elif fam in FLOAT_KERNELS or form["sh"] < 0:
        want_mode = 2
    else:
        tab = _table_bytes(P, fam, table, warp)
        if tab is not None:
            want_mode = 1 if tab + rows_bytes <= plan_ref.K_LEAN_TAB_BYTES else 2
        else:
            fits, too_large = ROWS_FIT.get(family, (0, 0))
            want_mode = 1 if rows_bytes <= fits else (2 if rows_bytes >= too_large > 0 else None)
    if want_mode is None:
        errs.append(f"mode {mode} has no stated expectation")
    elif mode != want_mode:
        errs.append(f"mode {mode}, not {want_mode}")
    fine_shape = fam == "lean" and mode == 1 and bw == 8 and table == "plain8" and not (adapt or warp or half)
    if kernel != fam and not (kernel == "fine" and fine_shape and family == "lean256"):
        errs.append(f"kernel {kernel} behind family {fam}")
    if fam in FALLBACK:
        path = "unpadded" if not form["padded"] else ("small_int" if mode == 1 else "own_modulo")
    elif mode == 1:
        path = "int_lds"
    elif form["sh"] >= 0:
        path = "int_form_float_rows"
    else:
        path = "float_rows"
    return errs, path


def _catalogue_on_family(be, orc, family, capfd=None):
    rec = _recipe(orc, family)
    P, prep = _palette(be, orc, rec)
    frames = {}
    complaints, paths, kernels, shapes, lines = [], set(), set(), set(), []
    for name in NAMES:
        thr_np = tf.MATRICES[name]
        T = be.Thresholds.from_matrix(thr_np)
        assert T.shape == thr_np.shape and T.integer_form == (tf.FORMS[name]["sh"] >= 0), name
        for i, (h, w, y0, x0) in enumerate(tf.geometries(thr_np.shape)):
            if i not in frames:
                frames[i] = orc.rnd(h, w, 300 + i)
            bad, seen = _run(be, orc, P, prep, frames[i], thr_np, T, y0, x0, rec["odd"], capfd)
            if bad:
                complaints.append(f"{family} {name} origin ({y0}, {x0}): {bad}")
            if capfd is not None:
                if len(seen) != 1:
                    complaints.append(f"{family} {name} origin ({y0}, {x0}): {len(seen)} launches traced")
                for traced in seen:
                    errs, path = _expect(family, rec, P, name, traced)
                    paths.add(path)
                    kernels.add(traced[8])
                    shapes.add((traced[0],) + traced[3:8])             # family, bw, adapt, warp, half, table
                    if i == 0:
                        lines.append(f"{family} {name}: {' '.join(traced)} -> {path}")
                    if errs:
                        complaints.append(f"{family} {name} origin ({y0}, {x0}): {'; '.join(errs)} in {traced}")
        del T
    return rec, complaints, paths, kernels, shapes, lines


@pytest.mark.parametrize("family", FAMILIES)
def test_every_form_traced(orc, switches, capfd, family):
    """The experiments library with DP_ORDERED_TRACE=1 (and the recipe's switches): oracle bytes, and every launch's family,
    MODE and kernel as the plan has them.  The threshold paths a family has must all be reached by the catalogue."""
    from dither_pie_amd import backend as be
    for k, v in _recipe(orc, family)["env"].items():
        switches.setenv(k, v)
    switches.setenv("DP_ORDERED_TRACE", "1")
    rec, complaints, paths, kernels, shapes, lines = _catalogue_on_family(be, orc, family, capfd)
    with capfd.disabled():
        print(f"\n  {family}: paths {sorted(paths)}, kernels {sorted(kernels)}", end="")
    assert not complaints, f"{len(complaints)} complaints:\n" + "\n".join(complaints[:12]) + "\nthe first launch per matrix:\n" + "\n".join(lines)
    if rec["family"] in TABLE_KERNELS:
        assert paths == {"int_lds", "int_form_float_rows", "float_rows", "unpadded"}, paths
    elif rec["family"] in FLOAT_KERNELS:
        assert paths == {"int_form_float_rows", "float_rows", "unpadded"}, paths
    elif rec["gamma"]:
        assert paths == {"own_modulo", "unpadded"}, paths          # the float64 brute-force kernel has no integer decision
    else:
        assert paths == {"small_int", "own_modulo", "unpadded"}, paths
    if family == "lean256":
        assert kernels == {"fine", "lean", "cell"} or kernels == {"fine", "lean", "brute"}, kernels
    if family == "leanhalf27":        # <MODE, 4, false, false, HALF>: two workgroups per CU while table and rows fit in half of LDS
        assert {("lean", "4", "0", "0", "1", "plain4"), ("lean", "4", "0", "0", "0", "plain4")} <= shapes, shapes
    if family == "w8lean300":         # <MODE, 8, ADAPT, WARP>
        assert {sh for sh in shapes if sh[0] == "lean"} == {("lean", "8", "1", "1", "0", "warped")}, shapes


@pytest.mark.parametrize("family", [f for f in FAMILIES if f != "w8lean300"])
def test_every_form_product_library(orc, family):
    """The same cases on the library that ships (its dispatch is the same code; it has no trace and reads no switch: the forced
    warped table is left out, and the use_gamma palette of 64 colours runs on the float kernel of the library's own choice)."""
    from dither_pie_amd import backend as be
    _, complaints, _, _, _, _ = _catalogue_on_family(be, orc, family)
    assert not complaints, f"{len(complaints)} complaints:\n" + "\n".join(complaints[:12])


# ================================================================================================ (b) the persistent grid's stride
STRIDE_FAMILIES = ["lean256", "leanhalf27", "compact64", "leanfloat64"]
STRIDE_MATRICES = ["cls4x64", "int17x24", "row1x7", "f33x20", "cls1x256", "cls2x128"]   # (rows of 1789 pixels: the classes are in use)


def _tie_rich(orc, pal, n, h, w, seed):
    """Noise with a third of the pixels on palette colours and midpoints of palette pairs (distance ties): the wave queues drain."""
    rs = np.random.RandomState(seed)
    pa = np.asarray(pal, np.int64)
    frames = np.stack([orc.rnd(h, w, seed + i) for i in range(n)])
    pick = rs.randint(0, len(pa), (n, h, w))
    mid = ((pa[pick] + pa[(pick + 1) % len(pa)]) // 2).astype(np.uint8)
    own = pa[pick].astype(np.uint8)
    sel = rs.randint(0, 6, (n, h, w, 1))
    return np.where(sel == 0, mid, np.where(sel == 1, own, frames))


@pytest.mark.parametrize("name", STRIDE_MATRICES)
@pytest.mark.parametrize("family", STRIDE_FAMILIES)
def test_tile_stride_with_awkward_matrices(orc, switches, capfd, family, name):
    """More 4096-pixel tiles than workgroups: every workgroup advances by the grid's stride, tracking a table that is no power of
    two (or 64 wide) from a tile origin of (5, 3); two frames where two workgroups share a CU."""
    from dither_pie_amd import backend as be
    rec = _recipe(orc, family)
    for k, v in rec["env"].items():
        switches.setenv(k, v)
    switches.setenv("DP_ORDERED_TRACE", "1")
    P, prep = _palette(be, orc, rec)
    _, h, w = ORD_BIG
    n = 2 if family == "leanhalf27" else 1
    arr = _tie_rich(orc, rec["pal"], n, h, w, 40 + len(name))
    thr_np = tf.MATRICES[name]
    bad, seen = _run(be, orc, P, prep, arr, thr_np, be.Thresholds.from_matrix(thr_np), 5, 3, capfd=capfd)
    assert not bad, f"{family} {name}: {bad}"
    assert len(seen) == 1 and seen[0][0] == rec["family"], seen
    errs, _ = _expect(family, rec, P, name, seen[0])
    assert not errs, (errs, seen)
    if family == "leanhalf27":
        assert seen[0][6] == "1", seen                               # two workgroups per CU


# ================================================================================================ the class nibbles in use
# A wave consults the class nibble of its first pixel only when its 256 pixels lie in one image row: never in a frame 131 wide.
# Rows of 772 = 3 * 256 + 4 pixels hold three such waves each, and the first of row y starts 4 y columns before a multiple of
# 256: with the origins below the waves of the first rows start inside the leading run of cls1x256 and cls2x128
# (tests/threshold_forms.py: _classes), where nibbles computed over consecutive columns would claim every slot nearest-only.
CLASS_FRAME = (5, 772)
CLASS_ORIGINS = [(0, 0), (5, 3), (1, 250), (tf.ORIGIN_LIMIT - 5, tf.ORIGIN_LIMIT - 772)]
CLASS_MATRICES = ["cls4x64", "cls2x128", "cls1x256", "cls16x16"]
CLASS_FAMILIES = ["lean256", "leanhalf27", "compact64", "lean300", "leanfloat64"]


def _class_cases(be, orc, family, capfd=None):
    rec = _recipe(orc, family)
    P, prep = _palette(be, orc, rec)
    h, w = CLASS_FRAME
    for name in CLASS_MATRICES:
        thr_np = tf.MATRICES[name]
        T = be.Thresholds.from_matrix(thr_np)
        for i, (y0, x0) in enumerate(CLASS_ORIGINS):
            bad, seen = _run(be, orc, P, prep, _tie_rich(orc, rec["pal"], 1, h, w, 80 + i)[0], thr_np, T, y0, x0, capfd=capfd)
            assert not bad, f"{family} {name} origin ({y0}, {x0}): {bad}"
            if capfd is not None:
                assert len(seen) == 1 and seen[0][0] == rec["family"], seen
                errs, _ = _expect(family, rec, P, name, seen[0])
                assert not errs, (errs, seen)


@pytest.mark.parametrize("family", CLASS_FAMILIES)
def test_class_nibbles_on_wide_rows(orc, switches, capfd, family):
    from dither_pie_amd import backend as be
    for k, v in _recipe(orc, family)["env"].items():
        switches.setenv(k, v)
    switches.setenv("DP_ORDERED_TRACE", "1")
    _class_cases(be, orc, family, capfd)


@pytest.mark.parametrize("family", CLASS_FAMILIES)
def test_class_nibbles_on_wide_rows_product_library(orc, family):
    from dither_pie_amd import backend as be
    _class_cases(be, orc, family)


# ================================================================================================ (c) the Oklab kernel
@pytest.mark.parametrize("name", ["col5x1", "m2x3", "int17x24", "f33x20", "nopad600x450"])
def test_oklab_kernel(name):
    """metric_ordered_kernel finds its position in the matrix by its own code: a % per group of four pixels, then increments."""
    import torch
    from dither_pie_amd import backend as be
    rs = np.random.RandomState(61)
    pal = rs.randint(0, 256, (16, 3)).astype(np.float32)
    outc = rs.randint(0, 256, (16, 3)).astype(np.uint8)
    P = be.Palette(pal, outc, metric="oklab")
    m = tf.MATRICES[name]
    T = be.Thresholds.from_matrix(m)
    frames = [rs.randint(0, 256, (2, 2, 3, 3)).astype(np.uint8),      # two frames of 18 bytes: the byte path
              rs.randint(0, 256, (1, 37, 132, 3)).astype(np.uint8)]    # whole dwords
    for base in frames:
        n, h, w, _ = base.shape
        base[0].reshape(-1, 3)[:4] = pal[:4].astype(np.uint8)          # d0 = 0
        dev = torch.from_numpy(base).cuda()
        for _, _, y0, x0 in tf.geometries(m.shape):
            y0, x0 = min(y0, tf.ORIGIN_LIMIT - h), min(x0, tf.ORIGIN_LIMIT - w)
            want = metric_ref.ordered_u8(base, pal, outc, m, y0, x0)
            got = be.ordered(dev, P, be.MODE_MATRIX, thr=T, y0=y0, x0=x0).cpu().numpy()
            bad = np.argwhere((got != want).any(-1))
            assert len(bad) == 0, f"{name} {(n, h, w)} origin ({y0}, {x0}): {len(bad)} pixels differ, first at {bad[:4].tolist()}"


# ================================================================================================ (d) constructors agree
@pytest.mark.parametrize("make,integer", [(("blue_noise", 33, 5), False), (("void_cluster", 13, 9, 3), None),
                                          (("void_cluster", 64, 64, 42), True)], ids=["blue33", "vac13x9", "vac64-sh13"])
def test_constructors_agree_with_from_matrix(orc, make, integer):
    """A matrix built on the device and the same values through from_matrix are the same thresholds: shape, form, bytes."""
    from dither_pie_amd import backend as be
    T = getattr(be.Thresholds, make[0])(*make[1:])
    m = T.numpy()
    F = be.Thresholds.from_matrix(m)
    form = tf.host_form(m)
    assert F.shape == T.shape == m.shape and F.integer_form == T.integer_form == (form["sh"] >= 0)
    if integer is not None:
        assert T.integer_form == integer
    if make[1:] == (64, 64, 42):
        assert form["sh"] == tf.MAX_SHIFT
    for family in ("lean256", "brute16"):
        rec = _recipe(orc, family)
        P, prep = _palette(be, orc, rec)
        for i, (h, w, y0, x0) in enumerate(tf.geometries(m.shape)):
            arr = orc.rnd(h, w, 500 + i)
            dev = _dev(arr)
            a = be.ordered(dev, P, be.MODE_MATRIX, thr=T, y0=y0, x0=x0).cpu().numpy()
            b = be.ordered(dev, P, be.MODE_MATRIX, thr=F, y0=y0, x0=x0).cpu().numpy()
            assert np.array_equal(a, b), (make, family, y0, x0, int((a != b).any(-1).sum()))
            ref = orc.ordered_u8(arr, *prep, "matrix", thr=m, y0=y0, x0=x0)
            assert np.array_equal(b, ref), (make, family, y0, x0, int((b != ref).any(-1).sum()))


# ================================================================================================ (e) the edge of acceptance
def test_largest_matrix_and_one_row_more(orc):
    from dither_pie_amd import _lib, backend as be
    thr_np = tf.MATRICES["max1024"]
    T = be.Thresholds.from_matrix(thr_np)
    assert T.shape == (1024, 1024) and T.integer_form
    for family in ("brute16", "lean256"):
        rec = _recipe(orc, family)
        P, prep = _palette(be, orc, rec)
        for i, (h, w, y0, x0) in enumerate(tf.geometries(thr_np.shape)):
            bad, _ = _run(be, orc, P, prep, orc.rnd(h, w, 600 + i), thr_np, T, y0, x0)
            assert not bad, f"{family} max1024 origin ({y0}, {x0}): {bad}"
    L = _lib.load()
    big = np.zeros((1024, 1025), np.float32)
    handle = C.c_void_p()
    rc = L.dp_thresholds_create(big.ctypes.data_as(C.c_void_p), 1024, 1025, C.byref(handle))
    assert rc == _lib.DP_EINVAL and not handle.value
    assert b"dp_thresholds_create" in (L.dp_last_error() or b"")


def test_both_sides_of_the_padded_limit(orc, switches, capfd):
    """2^18 padded entries keep the table kernel (float rows from global memory); one column more and no padded copy exists."""
    from dither_pie_amd import backend as be
    switches.setenv("DP_ORDERED_TRACE", "1")
    rec = _recipe(orc, "lean256")
    P, prep = _palette(be, orc, rec)
    seen = {}
    for name in ("pad_edge_1x262141", "nopad_1x262142"):
        thr_np = tf.MATRICES[name]
        T = be.Thresholds.from_matrix(thr_np)
        for i, (h, w, y0, x0) in enumerate(tf.geometries(thr_np.shape)):
            bad, traced = _run(be, orc, P, prep, orc.rnd(h, w, 700 + i), thr_np, T, y0, x0, capfd=capfd)
            assert not bad, f"{name} origin ({y0}, {x0}): {bad}"
            assert len(traced) == 1
            seen.setdefault(name, set()).add((traced[0][0], traced[0][2]))
    assert seen["pad_edge_1x262141"] == {("lean", "2")}, seen
    assert len(seen["nopad_1x262142"]) == 1 and next(iter(seen["nopad_1x262142"]))[0] in FALLBACK, seen
    assert seen["pad_edge_1x262141"] != seen["nopad_1x262142"]
