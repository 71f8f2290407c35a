"""CPU tier of the address arithmetic of the fine kernel's main loop (dither_pie_amd/csrc/ordered_fine.h: fine_cell_offset,
fine_stage_tag, fine_tag_rank, fine_stage_tags2, fine_row_offset, fine_row_address -- the functions ordered_fine_kernel and its
deferred path call, with a plain C++ dot product in place of v_dot4_u32_u8).

`fineaddr <first> <n>` of the stand-alone host_asan build checks
  * on the n colours from `first` on: the cell offset equals 2 * fine_cell(r, g, b), also from a base and with garbage in bits 24-31;
  * for every rank 0 .. 511 and every sub-cell 0 .. 7, on all 64 colours of the sub-cell: the row address of the staged tag equals
    rows_at + 16 * rank + 2 * sub-cell, for the address SUB 2 has the rows at and two others, and in the form the main loop reads it
    (a constant plus fine_row_offset);
  * the staged tag has bit 15 set, fits 16 bits and decodes to its rank, alone and two to a word beside ordinary window numbers
and prints the counts.  Here: all 2^24 colours; the counts are what they must be; and the arithmetic once more in numpy, written from
the statement of the layout (off: a u16 per cell; a row: eight u16 per wide cell) and not from the C++, on a sample."""
import numpy as np

import fine_sub_ref as fs
from test_ordered_fine_cpu import harness  # noqa: F401  (the fixture)


def _line(out):
    (line,) = [ln for ln in out if ln.startswith("fineaddr ")]
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split()[1:])}


def test_every_colour_every_rank(harness):  # noqa: F811
    got = _line(harness("fineaddr", 0, 1 << 24))
    assert got == dict(colours=1 << 24, rows=fs.FINE_IDS * 8 * 64, bad_cell=0, bad_row=0, bad_tag=0), got


def test_a_range_of_colours(harness):  # noqa: F811
    got = _line(harness("fineaddr", (1 << 24) - 4097, 4097))
    assert got == dict(colours=4097, rows=fs.FINE_IDS * 8 * 64, bad_cell=0, bad_row=0, bad_tag=0), got


def _dot4(a, b, c):
    a, b = np.asarray(a, np.int64), np.int64(b)
    return sum(((a >> s) & 255) * ((b >> s) & 255) for s in (0, 8, 16, 24)) + c


def test_the_forms_in_numpy():
    """the two dot products as the header states them, against cell_of / sub_of of fine_sub_ref.py"""
    rs = np.random.RandomState(5)
    rgb = rs.randint(0, 256, (20000, 3)).astype(np.int64)
    x = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)
    z = (x >> 3) & 0x1F1F1F
    assert np.array_equal(_dot4(z, 0x00004002, (z >> 16) << 11), 2 * fs.cell_of(rgb))
    rank = rs.randint(0, fs.FINE_IDS, len(x))
    staged = fs.TAG | (rank << 4)
    assert staged.max() <= 0xFFFF and np.array_equal((staged >> 4) & (fs.FINE_IDS - 1), rank)
    rows_at = 2 * fs.FINE_CELLS
    assert np.array_equal(_dot4((x >> 2) & 0x010101, 0x00080402, staged) + (rows_at - fs.TAG), rows_at + 16 * rank + 2 * fs.sub_of(rgb))
