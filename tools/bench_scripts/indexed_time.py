"""Times of the indexed output on one MI355X (HIP events, warm clocks, >= 30 repeats; median and spread = the 10th..90th
percentile range).

  python tools/bench_scripts/indexed_time.py            this tree: the index kernels beside a device copy of the same byte
                                                         count, apply_dithering_indexed beside apply_dithering, and the
                                                         headline apply_dithering_frames call
  python tools/bench_scripts/indexed_time.py --parent   a tree without the indexed output (the parent commit): only what
                                                         exists there -- apply_dithering and apply_dithering_frames

Run from the root of the tree to be measured; prints one JSON line per figure."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())

N_FRAMES, H, W = 24, 2160, 3840


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def time_gpu(fn, repeats=40, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def time_host(fn, repeats=40, warmup=5):
    import time
    import torch
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def emit(what, ms, nbytes=None, **extra):
    rec = {"what": what, **stats(ms), **extra}
    if nbytes is not None:
        rec["algorithmic_bytes"] = int(nbytes)
        rec["GBps_at_median"] = round(nbytes / (rec["median_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", action="store_true", help="the tree has no indexed output: time only what exists there")
    ap.add_argument("--repeats", type=int, default=40)
    args = ap.parse_args()
    import torch
    from PIL import Image
    from dither_pie_amd import backend as be
    from dither_pie_amd import dithering_lib as dl
    assert torch.cuda.is_available(), "needs a HIP device"
    rs = np.random.RandomState(0)
    tree = "parent" if args.parent else "this"

    # warm clocks: a second of copies
    big = torch.empty(N_FRAMES * H * W * 3, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(big)
    for _ in range(200):
        dst.copy_(big)
    torch.cuda.synchronize()

    # the headline call: 24 x 4K, Bayer 8x8, 256 colours (must not move between the trees)
    pal256 = [tuple(int(v) for v in c) for c in rs.randint(0, 256, (256, 3))]
    frames = torch.from_numpy(rs.randint(0, 256, (N_FRAMES, H, W, 3), dtype=np.uint8)).cuda()
    it = dl.ImageDitherer(256, dl.DitherMode.BAYER, pal256, False, {"size": "8x8"})
    it.prepare()
    out = torch.empty_like(frames)
    emit("apply_dithering_frames 24x4K bayer8x8 K=256", time_gpu(lambda: it.apply_dithering_frames(frames, out=out), args.repeats), tree=tree)

    # one PIL 4K image
    img = Image.fromarray(rs.randint(0, 256, (H, W, 3), dtype=np.uint8))
    for K in (16, 256):
        pal = pal256[:K]
        one = dl.ImageDitherer(K, dl.DitherMode.BAYER, pal, False, {"size": "8x8"})
        emit(f"apply_dithering PIL 4K bayer8x8 K={K}", time_host(lambda: one.apply_dithering(img), args.repeats), tree=tree)
        if not args.parent:
            emit(f"apply_dithering_indexed PIL 4K bayer8x8 K={K}", time_host(lambda: one.apply_dithering_indexed(img), args.repeats), tree=tree)
    if args.parent:
        return

    n_px = N_FRAMES * H * W
    for K, nb in ((16, 1), (256, 1), (1024, 2)):
        code = rs.permutation(np.unique(rs.randint(0, 1 << 24, 4 * K)))[:K]
        colours = np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=1).astype(np.uint8)
        imap = be.IndexMap(colours)
        idx = torch.randint(0, K, (N_FRAMES, H, W), device="cuda")
        rgb = torch.from_numpy(colours).cuda()[idx]
        del idx
        planes = be.to_indices(rgb, imap, index_bytes=nb)
        back = torch.empty_like(rgb)
        nbytes = n_px * (3 + nb)
        a, b = big[:nbytes // 2], dst[:nbytes // 2]          # a copy that reads and writes nbytes in all
        emit(f"device copy of {3 + nb} B/px", time_gpu(lambda: b.copy_(a), args.repeats), nbytes)
        emit(f"index_from_rgb K={K} {nb} B planes", time_gpu(lambda: be.to_indices(rgb, imap, index_bytes=nb, out=planes, strict=False), args.repeats),
             nbytes, slots=imap.slots, max_probe=imap.max_probe)
        emit(f"rgb_from_index K={K} {nb} B planes", time_gpu(lambda: be.from_indices(planes, imap, out=back, strict=False), args.repeats), nbytes)
        assert torch.equal(back, rgb)
        del rgb, planes, back
        torch.cuda.empty_cache()

    # what the extra pass costs behind the headline call (the price of not writing indices from the dither kernels)
    pl = torch.empty((N_FRAMES, H, W), dtype=torch.uint8, device="cuda")
    emit("apply_dithering_frames_indexed 24x4K bayer8x8 K=256", time_gpu(lambda: it.apply_dithering_frames_indexed(frames, out=pl), args.repeats), tree=tree)


if __name__ == "__main__":
    main()
