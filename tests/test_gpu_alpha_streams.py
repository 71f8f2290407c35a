"""GPU tier: the device entry points of include/ditherpie_hip_alpha.h on a stalled side stream -- variants A (late input) and B (busy
default stream) of tests/streams.py, as tests/test_gpu_hold_streams.py runs them for the other entry points that take their stream in
a descriptor (the completeness rule of tests/test_streams_cpu.py does not see them).  The decoy of a batch is the batch reversed.  For
the split both the clearing of the counters and the kernel must sit on the caller's stream; the diffusions run warm (the palette's
table is built by the harness's warm run, while the device is idle)."""
import numpy as np
import pytest

import alpha_ref as ar
import dotdiff_ref as dr
import idiff_ref as ir
import streams as st

pytestmark = pytest.mark.gpu

BLACK_WHITE = [(0, 0, 0), (255, 255, 255)]
FILL = (5, 6, 250)


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import backend, dithering_lib
    yield backend, dithering_lib
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def rev(a):
    return np.ascontiguousarray(a[::-1])


def both(stat):
    assert stat["slack_A_ms"] is not None and stat["slack_B_ms"] is not None      # both variants asked for a pending event


@pytest.mark.parametrize("n, h, w, kw", [
    (4, 33, 128, dict(mode="threshold", threshold=128)),                # the dword instance
    (3, 17, 19, dict(mode="ordered", m=4, y0=2, x0=9)),                 # the byte instance
])
def test_split_on_a_stalled_stream(gpu, n, h, w, kw):
    be, _ = gpu
    src = np.random.default_rng(h).integers(0, 256, (n, h, w, 4)).astype(np.uint8)
    names = ("rgb", "mask", "masked")
    bkw = {("matrix" if k == "m" else k): v for k, v in kw.items()}

    def ref(s):
        return dict(zip(names, ar.split(s, matte=(9, 99, 199), **kw)))

    def call(inp, outs, state):
        return dict(zip(names, be.alpha_split(inp["rgba"], matte=(9, 99, 199), **bkw)))

    both(st.run_case(st.Case("dp_alpha_split_u8", {"rgba": (src, rev(src))}, ref(src), call, decoy_ref=ref(rev(src)), label=f"{n}x{h}x{w} {kw['mode']}")))


@pytest.mark.parametrize("n, h, w", [(4, 33, 128), (3, 17, 19)])
def test_key_and_join_on_a_stalled_stream(gpu, n, h, w):
    import torch
    be, _ = gpu
    rng = np.random.default_rng(w)
    planes = rng.integers(0, 200, (n, h, w)).astype(np.uint8)
    rgb = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    mask = rng.integers(0, 2, (n, h, w)).astype(np.uint8)

    def key_call(inp, outs, state):
        return {"out": be.alpha_key(inp["planes"], inp["mask"], 201, out=outs["out"])}

    both(st.run_case(st.Case("dp_alpha_key_u8", {"planes": (planes, rev(planes)), "mask": (mask, rev(mask))}, {"out": ar.key(planes, mask, 201)}, key_call,
                             decoy_ref={"out": ar.key(rev(planes), rev(mask), 201)}, outs={"out": (planes.shape, torch.uint8)}, label=f"{n}x{h}x{w}")))

    def join_call(inp, outs, state):
        return {"rgba": be.alpha_join(inp["rgb"], inp["mask"], FILL, out=outs["rgba"])}

    both(st.run_case(st.Case("dp_alpha_join_u8", {"rgb": (rgb, rev(rgb)), "mask": (mask, rev(mask))}, {"rgba": ar.join(rgb, mask, FILL)}, join_call,
                             decoy_ref={"rgba": ar.join(rev(rgb), rev(mask), FILL)}, outs={"rgba": ((n, h, w, 4), torch.uint8)}, label=f"{n}x{h}x{w}")))


def grey_frames(n, h, w):
    rs = np.random.RandomState(7500 + 10 * h + w)
    v = rs.randint(0, 128, (n, h, w)) + (np.arange(w) * 127 // max(w - 1, 1))[None, None, :]
    return np.ascontiguousarray(np.repeat(v.astype(np.uint8)[..., None], 3, axis=-1))


def test_the_masked_diffusions_on_a_stalled_stream(gpu, orc):
    import torch
    be, dl = gpu
    spec = dl.prepare_palette(BLACK_WHITE, False)
    P = be.Palette(*spec)
    n, h, w = 3, 70, 37                                                  # two bands; two tiles across nothing, one down
    frames = grey_frames(n, h, w)
    masks = np.stack([ar.mask_family(m, h, w, 3) for m in ("half", "sixteenth", "checker")])
    taps, div = ir.KERNELS["floyd_steinberg"]

    def idiff_ref(f, k):
        return {"out": np.stack([ar.idiff_masked_u8(orc, a, b, *spec, taps, div, 256, FILL) for a, b in zip(f, k)])}

    def idiff_call(inp, outs, state):
        return {"out": be.idiff_masked(inp["frames"], inp["mask"], P, taps, div, 256, fill=FILL, out=outs["out"])}

    inputs = {"frames": (frames, rev(frames)), "mask": (masks, rev(masks))}
    both(st.run_case(st.Case("dp_alpha_idiff_u8", inputs, idiff_ref(frames, masks), idiff_call, decoy_ref=idiff_ref(rev(frames), rev(masks)),
                             outs={"out": (frames.shape, torch.uint8)}, label=f"{n}x{h}x{w}")))

    def dot_ref(f, k):
        return {"out": np.stack([ar.dotdiff_masked_u8(orc, a, b, *spec, dr.KNUTH, 256, FILL) for a, b in zip(f, k)])}

    def dot_call(inp, outs, state):
        return {"out": be.dotdiff_masked(inp["frames"], inp["mask"], P, dr.KNUTH, 256, fill=FILL, out=outs["out"])}

    both(st.run_case(st.Case("dp_alpha_dotdiff_u8", inputs, dot_ref(frames, masks), dot_call, decoy_ref=dot_ref(rev(frames), rev(masks)),
                             outs={"out": (frames.shape, torch.uint8)}, label=f"{n}x{h}x{w}")))
