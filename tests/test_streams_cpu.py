"""CPU tier of the stalled-stream harness (tests/streams.py): the rule that keeps the GPU matrix of
tests/test_gpu_stream_discipline.py complete -- every dp_* function of include/*.h that takes a `void *stream` is named in
that module's coverage table or in its exclusion list -- and the host-side parts of the harness (the case's own checks, the
error's fields, the refusal of a stall beyond the limit)."""
import glob
import os
import re

import numpy as np
import pytest

import streams as st
from conftest import ROOT


def _stream_entry_points():
    """name -> header, for every exported function whose argument list has a `void *stream` (comments stripped)."""
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        for m in re.finditer(r"\b(dp_\w+)\s*\(([^;{}]*?)\)\s*;", text):
            if re.search(r"void\s*\*\s*stream\b", m.group(2)):
                found[m.group(1)] = os.path.basename(path)
    return found


def test_every_stream_entry_point_is_in_the_matrix_or_excluded_with_a_reason():
    import test_gpu_stream_discipline as sd
    from dither_pie_amd import _lib
    found = _stream_entry_points()
    assert len(found) >= 47, sorted(found)
    # _lib.EXPORTS is pinned to ditherpie_hip.h; every other header has its own EXPORTS_* tuple, and load() resolves them all
    exports = {n for key, names in vars(_lib).items() if key.startswith("EXPORTS") for n in names}
    assert set(_lib.EXPORTS) <= exports and set(found) <= exports, set(found) - exports
    assert {n for n, h in found.items() if h == "ditherpie_hip.h"} <= set(_lib.EXPORTS)
    per_header = {}
    for name, header in found.items():
        per_header[header] = per_header.get(header, 0) + 1
    assert per_header["ditherpie_hip.h"] >= 20 and per_header["ditherpie_hip_okfit.h"] >= 4 and len(per_header) >= 15, per_header
    assert {"dp_ordered_u8", "dp_thresholds_blue_noise", "dp_okfit_fit", "dp_signature_distances", "dp_distinct_stream_reset"} <= set(found)
    both = set(sd.COVERAGE) & set(sd.EXCLUDED)
    assert not both, f"in COVERAGE and in EXCLUDED: {sorted(both)}"
    missing = set(found) - set(sd.COVERAGE) - set(sd.EXCLUDED)
    assert not missing, f"entry points with a stream parameter and no stream-discipline case: {sorted(missing)}"
    for name, tests in sd.COVERAGE.items():
        assert name in found, name
        assert tests and all(t.startswith("test_") and callable(getattr(sd, t, None)) for t in tests), (name, tests)
    for name, reason in sd.EXCLUDED.items():
        assert name in found, name
        assert isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name   # a one-line reason


def test_a_missing_entry_is_named(monkeypatch):
    import test_gpu_stream_discipline as sd
    cov = dict(sd.COVERAGE)
    del cov["dp_index_delta_u8"]
    monkeypatch.setattr(sd, "COVERAGE", cov)
    with pytest.raises(AssertionError, match="dp_index_delta_u8"):
        test_every_stream_entry_point_is_in_the_matrix_or_excluded_with_a_reason()


def test_the_error_names_entry_variant_and_condition():
    e = st.StreamOrderError("dp_riemersma_u8", "A", "bytes", "'out': 3 bytes differ")
    assert isinstance(e, AssertionError) and (e.entry, e.variant, e.condition) == ("dp_riemersma_u8", "A", "bytes")
    assert "dp_riemersma_u8" in str(e) and "variant A" in str(e) and "bytes" in str(e)


def test_a_case_checks_its_decoy_on_the_host():
    x, d = np.arange(16, dtype=np.uint8), np.arange(16, dtype=np.uint8)[::-1].copy()
    call = lambda inp, outs, state: {"out": inp["in"]}                    # noqa: E731
    st.Case("op", {"in": (x, d)}, {"out": x}, call, decoy_ref={"out": d})
    with pytest.raises(ValueError, match="could not fail"):              # the decoy's output equals the real one
        st.Case("op", {"in": (x, d)}, {"out": x}, call, decoy_ref={"out": x.copy()})
    with pytest.raises(ValueError, match="shape and dtype"):
        st.Case("op", {"in": (x, d[:8])}, {"out": x}, call, decoy_ref={"out": d})
    with pytest.raises(ValueError, match="reference output of its decoy"):
        st.Case("op", {"in": (x, d)}, {"out": x}, call)
    with pytest.raises(ValueError, match="kind"):
        st.Case("op", {}, {"out": x}, call, kind="lazy")
    with pytest.raises(ValueError, match="T_ms"):
        st.Case("op", {}, {"out": x}, call, kind="cold")
    st.Case("op", {}, {"out": x}, call)                                   # no inputs: no decoy to give


def test_a_stall_beyond_the_limit_is_refused():
    assert st.MAX_STALL_MS == 1000.0 and st.MIN_STALL_MS == 20.0
    for ms in (1000.5, 5000, -1):
        with pytest.raises(ValueError):
            st.stall(ms)
