"""GPU tier of the tile addresses of the ordered kernels beyond 2^31 bytes (dither_pie_amd/csrc/ordered.hip: the look-ahead load and
the tile store of ordered_fine_kernel): 90 copies of one 4K noise frame in ONE call -- 2.24 GB in, 2.24 GB out, one launch (fewer than
2^30 pixels), byte offsets beyond 2^31 -- on the product library.  Every copy must come out the same: output frames 0, 44 and 89 are
equal, and frame 0 equals frame 0 of a 24-frame call.  No oracle run of that size is needed: the small shapes are compared with the
oracle elsewhere (tests/test_gpu_ordered_one_launch.py), here only the addressing is in question."""
import pytest

pytestmark = pytest.mark.gpu

H, W, COPIES = 2160, 3840, 90


def test_ninety_4k_frames_in_one_call(orc):
    import torch
    from dither_pie_amd import backend as be
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    assert COPIES * H * W < 1 << 30 and COPIES * H * W * 3 > 1 << 31   # one launch, offsets past 2^31
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    frame = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    P = be.Palette(*orc.prepare_palette(orc.palr(256, 7), False), accel=True)
    thr = be.Thresholds.from_matrix(orc.bayer_matrix("8x8"))
    first = be.ordered(frame.expand(24, H, W, 3).contiguous(), P, be.MODE_MATRIX, thr=thr)[0].clone()
    out = be.ordered(frame.expand(COPIES, H, W, 3).contiguous(), P, be.MODE_MATRIX, thr=thr)
    torch.cuda.synchronize()
    assert len(torch.unique(first.reshape(-1, 3), dim=0)) > 200   # (a dithered frame, not a cleared buffer)
    for i in (0, 44, 89):
        if not torch.equal(out[i], first):
            bad = torch.nonzero((out[i] != first).any(-1))
            raise AssertionError(f"frame {i}: {len(bad)} pixels differ from frame 0 of the 24-frame call, first at {bad[:4].tolist()}")
    del out
    be.release_workspaces()
