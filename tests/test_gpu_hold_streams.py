"""GPU tier: dp_hold_u8 (include/ditherpie_hip_hold.h) on a stalled side stream -- variants A (late input) and B (busy default
stream) of tests/streams.py, as tests/test_gpu_resample_streams.py runs them for the other entry point that takes its stream in a
descriptor (the completeness rule of tests/test_streams_cpu.py does not see either).  The decoy of a batch is the batch reversed.
Both the clearing of the counters and the kernel must sit on the caller's stream: a first call of a stream (no state: the state
buffers are written only) and a call that continues one (the state, uploaded while the device is idle, is read and updated), on the
dword and on the byte instance of the kernel."""
import numpy as np
import pytest

import hold_ref as hr
import streams as st

pytestmark = pytest.mark.gpu

ENTRY = "dp_hold_u8"


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend
    yield backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n, h, w, cell, tol, share256, with_state", [
    (6, 33, 128, 16, 2, 32, False),     # the dword instance, cells across two waves
    (6, 33, 128, 8, 2, 32, True),       # ... continuing a stream
    (5, 17, 19, 16, 3, 0, True),        # the byte instance
    (6, 9, 67, 4, 2, 64, False),
    (4, 20, 27, 1, 0, 0, False),        # cells of one pixel: no vote, the counters alone cross the barrier
])
def test_hold_on_a_stalled_stream(gpu, n, h, w, cell, tol, share256, with_state):
    import torch
    be = gpu
    src, planes = hr.clip(n, h, w, cell, tol, 900 + h + cell)
    before = None
    if with_state:                       # the state an earlier batch (other frames of the same scene) left
        other = hr.clip(3, h, w, cell, tol, 950 + h)
        before = hr.hold(other[0], other[1], None, cell, tol, share256)[2]
    decoy = (np.ascontiguousarray(src[::-1]), np.ascontiguousarray(planes[::-1]))
    names = ("out", "refreshed", "anchor", "held")

    def ref(s, p):
        out, refreshed, state = hr.hold(s, p, before, cell, tol, share256)
        return dict(zip(names, (out, refreshed, state[0], state[1])))

    def prepare(variant):                # (the device is idle here: the upload is not part of the call)
        return None if before is None else (torch.from_numpy(before[0].copy()).cuda(), torch.from_numpy(before[1].copy()).cuda())

    def call(inp, outs, state):
        out, refreshed, state = be.hold(inp["src"], inp["planes"], state, cell, tol, share256, out=outs["out"])
        return dict(zip(names, (out, refreshed, state[0], state[1])))

    stat = st.run_case(st.Case(ENTRY, {"src": (src, decoy[0]), "planes": (planes, decoy[1])}, ref(src, planes), call, decoy_ref=ref(*decoy),
                               outs={"out": (planes.shape, torch.uint8)}, prepare=prepare, label=f"{n}x{h}x{w} cell {cell} state {with_state}"))
    assert stat["slack_A_ms"] is not None and stat["slack_B_ms"] is not None      # both variants asked for a pending event
