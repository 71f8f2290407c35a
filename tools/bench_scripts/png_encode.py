"""Times and file sizes of the PNG-8 output (HIP events for the device part, perf_counter for whole calls; warm clocks,
median [p10-p90]).

  python tools/bench_scripts/png_encode.py [--repeats 20] [--segs 2048,8192,32768] [--batch 64] [--skip-4k] [--blocks fixed|dynamic|both] [--assemble host|both]
  python tools/bench_scripts/png_encode.py --sizes-only      (no GPU: stream sizes of the host statement against zlib)
  python tools/bench_scripts/png_encode.py --assemble both   (host-assembled against device-assembled files, and nothing else)

  * dp_png_deflate_encode_u8 alone (HIP events) on photo-like and noise planes of 16 and 256 colours at 1080p and 4K, one
    frame and a batch of --batch frames, at every seg_bytes of --segs; beside it a device copy of the plane bytes;
  * png.encode_png of the same planes end to end (wall clock), and of that the host part: the size read-back and block copy,
    and the container with its CRCs (zlib.crc32), timed on their own;
  * ImageDitherer.apply_dithering_png(image) against the route the tree offered before for the same file on disk,
    apply_dithering_indexed(image).save(buf, "PNG"), A then B then A ... in ONE process (interleaved, so that clock and
    cache state are shared), with the bytes of both files;
  * --sizes-only: bytes of the host statement over the filtered size at every seg_bytes, with zlib level 1, level 6 and level
    1 restricted to fixed codes (Z_FIXED) beside it, on the 512 x 768 photo-like planes of tests/png_ref.py.
  * --blocks: the block types the encoder may write beside stored ones ("fixed", the default; "dynamic"; "both" times the two
    A then B then A ... in the same process and reports each, with the workspace either needs).
  * --assemble both: png.encode_png(assemble="host") and png.encode_png(assemble="device") of the same planes, taking turns
    inside every repeat in ONE process, each timed with HIP events (what the stream was busy or waited for) and by the wall
    clock (what the caller waits for), median [p10-p90]; the files are compared byte for byte first.  Beside them
    dp_png_file_assemble_u8 alone (HIP events: the CRC, layout and copy kernels) and the copy of the finished bytes to the
    host.  The host path is the code this option was added beside, unchanged: it is the yardstick.  Only this comparison
    runs.
Run from the root of the tree; prints one JSON line per figure."""
import argparse
import io
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def emit(what, ms=None, **extra):
    print(json.dumps({"what": what, **(stats(ms) if ms is not None else {}), **extra}), flush=True)


def time_gpu(fn, repeats, warmup=3):
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


def time_gpu_interleaved(fns, repeats, warmup=3):
    """[ms per repeat] per function, the functions taking turns inside every repeat (shared clock and cache state)."""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for fn, acc in zip(fns, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return out


def time_wall(fn, repeats, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def time_both_interleaved(fns, repeats, warmup=2):
    """([HIP-event ms], [wall ms]) per function, the functions taking turns inside every repeat."""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    ev, wall = [[] for _ in fns], [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall[i].append(1e3 * (time.perf_counter() - t0))
            ev[i].append(a.elapsed_time(b))
    return ev, wall


def assemble_both(a, geometries, modes):
    import torch
    from dither_pie_amd import backend, png
    for h, w in geometries:
        for k in (16, 256):
            d = backend.png_depth(k)
            palette = np.random.RandomState(4).randint(0, 256, (k, 3)).astype(np.uint8)
            for kind in ("photo", "noise"):
                for n in (1, a.batch if (h, w) == (1080, 1920) else max(1, a.batch // 4)):
                    dev = torch.from_numpy(planes_of(kind, k, n, h, w)).cuda()
                    for blocks in modes:
                        tag = dict(h=h, w=w, k=k, kind=kind, frames=n, blocks=blocks)
                        host_files = png.encode_png(dev, palette, blocks=blocks)
                        dev_files = png.encode_png(dev, palette, blocks=blocks, assemble="device")
                        payload, sizes = backend.png_deflate(dev, d, blocks=blocks)
                        s = sizes.cpu().tolist()
                        pay = payload.cpu().numpy()
                        one_chunk = [png.container(w, h, d, palette, pay[f, :m].tobytes(), idat_bytes=2 ** 31 - 1) for f, m in enumerate(s)]
                        emit("files", same_as_one_idat_container=dev_files == one_chunk, same_as_host_assembled=dev_files == host_files,
                             bytes=sum(len(f) for f in dev_files), **tag)
                        ev, wall = time_both_interleaved([lambda: png.encode_png(dev, palette, blocks=blocks),
                                                          lambda: png.encode_png(dev, palette, blocks=blocks, assemble="device")], a.repeats)
                        for i, name in enumerate(("host", "device")):
                            emit("encode_png, HIP events", ev[i], assemble=name, **tag)
                            emit("encode_png, wall clock", wall[i], assemble=name, **tag)
                        head = png.container(w, h, d, palette, b"")
                        made = {}
                        def assemble():
                            made["out"] = backend.png_file_assemble(payload, sizes, pre=head[:-24], post=head[-12:])
                        emit("  dp_png_file_assemble_u8 alone (with its prefix upload)", time_gpu(assemble, a.repeats), **tag)
                        out, offsets = made["out"]
                        emit("  offsets and finished bytes to the host", time_wall(lambda: out[:int(offsets[-1].item())].cpu(), a.repeats), **tag)
                        del host_files, dev_files, one_chunk, pay


def zfixed1(data):
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    return co.compress(data) + co.flush()


def sizes_only(segs, modes):
    import png_ref as pr
    from dither_pie_amd import backend
    for k in (16, 256):
        plane, d = pr.photo_plane(k), pr.depth_of(k)
        raw = pr.filtered(plane, d)
        F = len(raw)
        emit("zlib", k=k, level1=round(len(zlib.compress(raw, 1)) / F, 4), level6=round(len(zlib.compress(raw, 6)) / F, 4),
             fixed_level1=round(len(zfixed1(raw)) / F, 4))
        for seg in segs:
            for blocks in modes:
                n = len(backend.png_deflate_host(plane, d, seg, blocks=blocks)[0])
                emit("host statement", k=k, seg_bytes=seg, blocks=blocks, bytes=n, of_filtered=round(n / F, 4),
                     of_zlib_fixed_level1=round(n / len(zfixed1(raw)), 4), of_zlib_level1=round(n / len(zlib.compress(raw, 1)), 4))


def planes_of(kind, k, n, h, w):
    import png_ref as pr
    rs = np.random.RandomState(3)
    if kind == "noise":
        return rs.randint(0, k, (n, h, w)).astype(np.uint8)
    one = pr.photo_plane(k, h, w)
    return np.stack([np.roll(one, 7 * i, axis=1) for i in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--segs", default="2048,8192,32768")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--skip-4k", action="store_true")
    ap.add_argument("--sizes-only", action="store_true")
    ap.add_argument("--blocks", choices=("fixed", "dynamic", "both"), default="fixed")
    ap.add_argument("--assemble", choices=("host", "both"), default="host")
    a = ap.parse_args()
    segs = [int(s) for s in a.segs.split(",")]
    modes = ["fixed", "dynamic"] if a.blocks == "both" else [a.blocks]
    if a.sizes_only:
        return sizes_only(segs, modes)
    import torch
    from PIL import Image
    from dither_pie_amd import _lib, backend, png
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    L = _lib.load()
    entry = {"fixed": "dp_png_deflate_encode_u8", "dynamic": "dp_png_deflate_dyn_encode_u8"}
    ws_of = {"fixed": L.dp_png_deflate_workspace_bytes, "dynamic": L.dp_png_deflate_dyn_workspace_bytes}
    emit("device", name=torch.cuda.get_device_name(0), default_seg_bytes=backend.PNG_SEG_BYTES)
    geometries = [(1080, 1920)] + ([] if a.skip_4k else [(2160, 3840)])
    if a.assemble == "both":
        return assemble_both(a, geometries, modes)
    for h, w in geometries:
        for k in (16, 256):
            d = backend.png_depth(k)
            palette = np.random.RandomState(4).randint(0, 256, (k, 3)).astype(np.uint8)
            for kind in ("photo", "noise"):
                for n in (1, a.batch if (h, w) == (1080, 1920) else max(1, a.batch // 4)):
                    dev = torch.from_numpy(planes_of(kind, k, n, h, w)).cuda()
                    tag = dict(h=h, w=w, k=k, kind=kind, frames=n)
                    emit("device copy of the planes", time_gpu(lambda: dev.clone(), a.repeats), **tag)
                    for seg in segs:
                        out = {}
                        def runner(blocks):
                            def run():
                                out[blocks] = backend.png_deflate(dev, d, seg, blocks=blocks)
                            return run
                        for blocks, ms in zip(modes, time_gpu_interleaved([runner(b) for b in modes], a.repeats)):
                            emit(entry[blocks], ms, seg_bytes=seg, blocks=blocks, bytes_per_frame=int(out[blocks][1].sum().item()) // n,
                                 plane_bytes=h * w, workspace_bytes=int(ws_of[blocks](n, h, w, d, seg)), **tag)
                    for blocks in modes:
                        ms = time_wall(lambda: png.encode_png(dev, palette, blocks=blocks), a.repeats)
                        emit("encode_png end to end", ms, blocks=blocks, **tag)
                    payload, sizes = backend.png_deflate(dev, d, blocks=modes[-1])
                    def back():
                        s = sizes.cpu().tolist()
                        block = payload[:, :max(s)].cpu().numpy()
                        return [block[f, :m].tobytes() for f, m in enumerate(s)]
                    emit("  of it: sizes and block to the host", time_wall(back, a.repeats), **tag)
                    streams = back()
                    emit("  of it: container and CRCs", time_wall(lambda: [png.container(w, h, d, palette, s) for s in streams], a.repeats), **tag)
    # the single-image routes, A / B interleaved in one process
    for h, w in geometries:
        y, x = np.mgrid[0:h, 0:w]
        field = 0.5 + 0.4 * np.sin(x / 37.0) * np.cos(y / 53.0)            # the photo-like field of the size tests, per channel
        rs = np.random.RandomState(1)
        photo = np.stack([np.clip(np.roll(field, 40 * c, axis=1) + rs.normal(0, 0.02, (h, w)), 0, 1) * 255 for c in range(3)], axis=-1)
        for content, arr in (("photo", photo.astype(np.uint8)), ("noise", rs.randint(0, 256, (h, w, 3)).astype(np.uint8))):
            img = Image.fromarray(arr, "RGB")
            for k, mode, params in ((16, DitherMode.BAYER, {"size": "4x4"}), (256, DitherMode.ERROR_DIFFUSION, {"variant": "floyd_steinberg"})):
                pal = [tuple(int(v) for v in c) for c in np.random.RandomState(5).randint(0, 256, (k, 3))]
                dit = ImageDitherer(k, mode, pal, dither_params=params)
                def route_a(blocks=modes[0]):
                    return dit.apply_dithering_png(img, blocks=blocks)
                def route_d():
                    return route_a(modes[-1])
                def route_b():
                    buf = io.BytesIO()
                    dit.apply_dithering_indexed(img).save(buf, "PNG")
                    return buf.getvalue()
                for _ in range(2):
                    fa, fb, fd = route_a(), route_b(), route_d()
                ta, tb, td = [], [], []
                for _ in range(max(5, a.repeats // 2)):
                    for fn, acc in ((route_a, ta), (route_b, tb)) + (((route_d, td),) if len(modes) > 1 else ()):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        acc.append(1e3 * (time.perf_counter() - t0))
                same = np.array_equal(np.asarray(Image.open(io.BytesIO(fa)).convert("RGB")), np.asarray(Image.open(io.BytesIO(fb)).convert("RGB")))
                emit("apply_dithering_png", ta, h=h, w=w, k=k, mode=mode.name, content=content, blocks=modes[0], file_bytes=len(fa),
                     decodes_like_the_other=bool(same))
                if len(modes) > 1:
                    same = np.array_equal(np.asarray(Image.open(io.BytesIO(fd)).convert("RGB")), np.asarray(Image.open(io.BytesIO(fb)).convert("RGB")))
                    emit("apply_dithering_png", td, h=h, w=w, k=k, mode=mode.name, content=content, blocks=modes[-1], file_bytes=len(fd),
                         decodes_like_the_other=bool(same))
                emit("apply_dithering_indexed + Image.save", tb, h=h, w=w, k=k, mode=mode.name, content=content, file_bytes=len(fb))


if __name__ == "__main__":
    main()
