"""GPU tier: memory discipline of the device entry points of include/ditherpie_hip_clip.h on the guarded arena
(tests/arena.py), as tests/test_gpu_indexed_memory.py is for the indexed header: every pointer the library sees lies inside
one arena; byte buffers have exactly their documented size and sit at odd addresses; the state, the counters and the ranks are
as aligned as the header asks and no better; the workspace is exactly *_workspace_bytes() long, 16- but not 32-byte aligned,
and pre-filled with zeros, 0xFF and noise (the result must not depend on it); guards of >= 1 MiB stay intact; inputs are
unchanged; a workspace one byte short is refused with DP_EINVAL and leaves state, list and count as they were.
tests/test_clip_palette_cpu.py checks COVERAGE against the header.  No test here is meant to fault."""
import numpy as np
import pytest

import arena as ar
import clip_palette_ref as cr

pytestmark = pytest.mark.gpu

COVERAGE = {
    "dp_distinct_stream_reset": ["test_stream_add_and_reset"],
    "dp_distinct_stream_add_u8": ["test_stream_add_and_reset"],
    "dp_hist_sample_u8": ["test_hist_sample"],
}
EXCLUDED = {}

DP_OK, DP_EINVAL = 0, 1
FILLS = ("zeros", "ones", ar.noise(77))
LIST_BYTES = 3 << 24


@pytest.fixture
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tier needs a HIP device")
    from dither_pie_amd import _lib, backend
    yield _lib.load(), backend
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _batches(rs):
    """Three buffers: odd lengths, colours repeated inside and across buffers, more than one compaction block."""
    cols = rs.randint(0, 256, (3000, 3)).astype(np.uint8)
    a = cols[rs.randint(0, 1500, 4099)]
    b = cols[rs.randint(1000, 3000, 2049)]
    c = np.concatenate([a[:5], cols[rs.randint(0, 3000, 1)]])
    return [a, b, c]


def test_stream_add_and_reset(gpu):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(11)
    bufs = _batches(rs)
    state_bytes = L.dp_distinct_stream_state_bytes()
    needs = [L.dp_distinct_stream_workspace_bytes(len(b)) for b in bufs]
    ws_bytes = max(needs)
    specs = [(b.nbytes, g) for b in bufs] + [(state_bytes, g), (LIST_BYTES, g), (8, g), (ws_bytes, g)]
    A = ar.Arena(ar.capacity_for(specs), "cuda", 21)
    for i, (b, res) in enumerate(zip(bufs, (1, 3, 15))):          # pixels at odd addresses
        A.carve(f"px{i}", b.nbytes, res, g)
        A.put(f"px{i}", b)
    A.carve("state", state_bytes, 0, g)                            # 16-byte aligned and no better
    A.carve("list", LIST_BYTES, 5, g)                              # exactly 3 * 2^24 bytes at an odd address
    A.carve("cnt", 8, 8, g)                                        # 8-byte aligned and no better
    A.carve("ws", ws_bytes, 0, g)                                  # 16- but not 32-byte aligned
    assert A.ptr("ws") % 32 == 16 and A.ptr("state") % 32 == 16 and A.ptr("cnt") % 16 == 8 and A.ptr("list") % 2 == 1
    st = be._stream()
    want = cr.DistinctStream()
    lists = []
    for k, fill in enumerate(FILLS):
        A.reseed(500 + k)
        A.fill("state", ar.noise(k))                               # reset must clear whatever the state held
        A.fill("cnt", ar.noise(k + 9))
        A.fill("list", fill)
        assert L.dp_distinct_stream_reset(A.ptr("state"), A.ptr("cnt"), st) == DP_OK, L.dp_last_error()
        torch.cuda.synchronize()
        assert int(A.get("cnt", np.int64)[0]) == 0 and not A.get("state").any()
        want.reset()
        for i, b in enumerate(bufs):
            A.fill("ws", FILLS[(k + i) % 3])
            # a workspace of exactly the bytes this call needs (the region is as long as the largest of the three)
            rc = L.dp_distinct_stream_add_u8(A.ptr(f"px{i}"), len(b), A.ptr("state"), A.ptr("list"), A.ptr("cnt"), A.ptr("ws"), needs[i], st)
            torch.cuda.synchronize()
            assert rc == DP_OK, (i, rc, L.dp_last_error())
            want.add(b)
            n = int(A.get("cnt", np.int64)[0])
            assert n == len(want.colours()), (k, i, n)
            assert np.array_equal(A.view("list")[:3 * n].cpu().numpy().reshape(-1, 3), want.colours()), (k, i)
            A.check()
            A.unchanged(f"px{i}")
        n = len(want.colours())
        # what lies behind the list's end still holds its fill: nothing is written past entry n_distinct
        tail = A.view("list")[3 * n:]
        if fill == "zeros":
            assert not bool(tail.any())
        elif fill == "ones":
            assert bool((tail == 0xFF).all())
        lists.append(A.view("list")[:3 * n].cpu().numpy().copy())
        seen = np.unpackbits(A.get("state"), bitorder="little")
        assert int(seen.sum()) == n                                # one bit per listed colour, no other
        codes = want.colours().astype(np.int64)
        assert seen[codes[:, 0] | (codes[:, 1] << 8) | (codes[:, 2] << 16)].all()
    assert all(np.array_equal(lists[0], x) for x in lists[1:])

    # refusals launch nothing: state, list and count keep what they hold
    for name in ("state", "list", "cnt"):
        A.put(name, A.get(name).copy())
    A.fill("ws", "zeros")
    for ptr, nbytes in ((A.ptr("ws"), needs[0] - 1), (A.ptr("ws") + 8, needs[0]), (None, needs[0])):
        rc = L.dp_distinct_stream_add_u8(A.ptr("px0"), len(bufs[0]), A.ptr("state"), A.ptr("list"), A.ptr("cnt"), ptr, nbytes, st)
        torch.cuda.synchronize()
        assert rc == DP_EINVAL and b"dp_distinct_stream_add_u8" in L.dp_last_error(), (rc, L.dp_last_error())
        for name in ("state", "list", "cnt", "ws"):
            A.unchanged(name)
    assert L.dp_distinct_stream_add_u8(A.ptr("px0"), 0, A.ptr("state"), A.ptr("list"), A.ptr("cnt"), None, 0, st) == DP_OK    # n = 0: a no-op
    torch.cuda.synchronize()
    for name in ("state", "list", "cnt"):
        A.unchanged(name)
    A.check()
    del A


def test_hist_sample(gpu):
    import torch
    L, be = gpu
    g = ar.MIN_GUARD
    rs = np.random.RandomState(12)
    px = np.concatenate([rs.randint(0, 256, (5000, 3)), np.repeat([[17, 200, 3]], 700, axis=0), rs.randint(32, 48, (3000, 3))]).astype(np.uint8)
    hist = be.ColourHistogram(torch.from_numpy(px).cuda())
    table = cr.histogram(px)
    need = L.dp_hist_sample_workspace_bytes()
    hist_bytes = hist.buf.numel()
    for case, n_ranks in enumerate((1, 7, 1000, 16384)):
        ranks = rs.randint(0, len(px), n_ranks).astype(np.int64)
        ranks[0] = len(px) - 1
        n_bad = 0
        if n_ranks >= 7:
            ranks[1:5] = (-1, len(px), 0, 1 << 40)
            n_bad = 3
        want, bad = cr.rank_sample(table, ranks)
        assert bad == n_bad
        specs = [(hist_bytes, g), (ranks.nbytes, g), (3 * n_ranks, g), (8, g), (need, g)]
        A = ar.Arena(ar.capacity_for(specs), "cuda", 40 + case)
        A.carve("hist", hist_bytes, 0, g)
        A.view("hist").copy_(hist.buf)
        A.expected["hist"] = ("data", A.view("hist").clone())
        A.carve("ranks", ranks.nbytes, 8, g)
        A.put("ranks", ranks)
        A.carve("out", 3 * n_ranks, (1, 3, 7, 15)[case], g)
        A.carve("cnt", 8, 8, g)
        A.carve("ws", need, 0, g)
        assert A.ptr("ws") % 32 == 16 and A.ptr("hist") % 32 == 16 and A.ptr("ranks") % 16 == 8
        outs = []
        for k, fill in enumerate(FILLS):
            A.reseed(700 + 10 * case + k)
            A.fill("out", fill)
            A.fill("ws", FILLS[(k + 1) % 3])
            A.fill("cnt", (ar.noise(5), "zeros", "ones")[k])
            before = int(A.get("cnt", np.uint64)[0])
            rc = L.dp_hist_sample_u8(A.ptr("hist"), A.ptr("ranks"), n_ranks, A.ptr("out"), A.ptr("cnt"), A.ptr("ws"), need, be._stream())
            torch.cuda.synchronize()
            assert rc == DP_OK, (rc, L.dp_last_error())
            got = A.get("out").reshape(-1, 3).copy()
            assert np.array_equal(got, want), (case, fill)
            assert int(A.get("cnt", np.uint64)[0]) == (before + n_bad) % (1 << 64)      # added to, not stored
            A.check()
            A.unchanged("hist")
            A.unchanged("ranks")
            outs.append(got)
        A.fill("out", ar.noise(3))
        A.fill("cnt", "zeros")
        for ptr, nbytes in ((A.ptr("ws"), need - 1), (A.ptr("ws") + 8, need)):
            rc = L.dp_hist_sample_u8(A.ptr("hist"), A.ptr("ranks"), n_ranks, A.ptr("out"), A.ptr("cnt"), ptr, nbytes, be._stream())
            torch.cuda.synchronize()
            assert rc == DP_EINVAL and b"dp_hist_sample_u8" in L.dp_last_error()
            A.unchanged("out")
            A.unchanged("cnt")
        A.check()
        del A
