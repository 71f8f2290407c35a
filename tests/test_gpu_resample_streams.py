"""GPU tier: dp_resample_u8 (include/ditherpie_hip_resample.h) on a stalled side stream -- variants A (late input) and B (busy
default stream) of tests/streams.py, as tests/test_gpu_stream_discipline.py runs them for the entry points that take a `void
*stream` parameter.  This entry point takes its stream in a descriptor, so the completeness rule of tests/test_streams_cpu.py
does not see it; these are its cases.  The decoy of a batch is the batch reversed.  The plan is made by the warm run (a blocking
upload, allowed there); runs A and B find it cached and only launch: both passes (the intermediate lives in the stream's
workspace), one pass, and the copy of equal sizes."""
import numpy as np
import pytest

import resample_ref as rr
import streams as st

pytestmark = pytest.mark.gpu

ENTRY = "dp_resample_u8"


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend
    yield backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("h, w, oh, ow, name", [
    (37, 53, 8, 10, "box"),          # horizontal (the naive kernel) into the workspace, then vertical
    (130, 70, 66, 35, "lanczos"),    # the same through several blocks of the staged horizontal kernel
    (29, 18, 7, 18, "bicubic"),      # vertical only
    (24, 31, 24, 9, "hamming"),      # horizontal only
    (21, 19, 21, 19, "bilinear"),    # equal sizes: a copy on the stream
])
def test_resample_on_a_stalled_stream(gpu, h, w, oh, ow, name):
    import torch
    be = gpu
    frames = rr.content("noise", 3, h, w, 1100 + h)
    want = rr.resample(frames, oh, ow, name)
    decoy, dwant = np.ascontiguousarray(frames[::-1]), np.ascontiguousarray(want[::-1])

    def call(inp, outs, state):
        be.resample(inp["in"], oh, ow, name, out=outs["out"])
        return {"out": outs["out"]}

    stat = st.run_case(st.Case(ENTRY, {"in": (frames, decoy)}, {"out": want}, call, decoy_ref={"out": dwant},
                               outs={"out": (want.shape, torch.uint8)}, label=f"{name} {h}x{w}->{oh}x{ow}"))
    assert stat["slack_A_ms"] is not None and stat["slack_B_ms"] is not None      # both variants asked for a pending event
