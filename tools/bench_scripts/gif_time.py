"""Times and file sizes of the animated GIF output (HIP events, warm clocks, 40 repeats; median [p10-p90]).

  python tools/bench_scripts/gif_time.py [--repeats 40] [--skip-video] [--chunks 4096,8192,16384,32768]
  python tools/bench_scripts/gif_time.py --sizes-only        (no GPU: the file-size cost of chunking, from the host statement)

  * dp_index_delta_u8 and dp_gif_lzw_encode_u8 per batch of 15 x 1080p and 5 x 4K index planes, at every chunk_px of --chunks:
    Bayer 4x4 at 16 colours, Floyd-Steinberg at 256 colours (both dithered on the device from image-like frames) and a flat
    plane; beside each, in the same run, a device copy of the plane bytes and Pillow's save(format="GIF") of the same planes
    on the host; the bytes the encoder produced, and the two ways of bringing them to the host (one strided block of
    max(sizes) bytes a frame, as gif.py does, against a copy per frame);
  * VideoProcessor.process_video_gif frames/s on the compiled decoder stand-in (tools/pipe_standin.c) with the bare decoder
    pipe beside it;
  * --sizes-only: bytes of the host statement at every chunk_px as a ratio to the unchunked stream, on one 1080p frame of each
    dithered content made by the C oracle.
Run from the root of the tree; prints one JSON line per figure."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tools"))

GEOMETRIES = ((15, 1080, 1920), (5, 2160, 3840))


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def time_gpu(fn, repeats=40, warmup=3):
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


def emit(what, ms=None, **extra):
    print(json.dumps({"what": what, **(stats(ms) if ms is not None else {}), **extra}), flush=True)


def image_like_np(n, h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    rs = np.random.RandomState(1)
    out = []
    for t in range(n):
        f = np.stack([x * (200.0 / w) + 2 * t + 20, y * (180.0 / h) + t + 30, (x + y) * (150.0 / (w + h)) + 40], axis=-1)
        out.append(np.clip(f + rs.randint(0, 3, f.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


def ditherers():
    from dither_pie_amd.dithering_lib import DitherMode, ImageDitherer
    rs = np.random.RandomState(2)
    def pal(k):
        return [tuple(int(v) for v in c) for c in rs.randint(0, 256, (k, 3))]
    return {"bayer4x4 16 colours": ImageDitherer(16, DitherMode.BAYER, pal(16), dither_params={"size": "4x4"}),
            "floyd-steinberg 256 colours": ImageDitherer(256, DitherMode.ERROR_DIFFUSION, pal(256), dither_params={"variant": "floyd_steinberg"})}


def pillow_gif_ms(planes, colours):
    from PIL import Image
    t = time.perf_counter()
    total = 0
    for p in planes:
        im = Image.fromarray(p, "P")
        im.putpalette(np.asarray(colours, np.uint8).tobytes())
        buf = io.BytesIO()
        im.save(buf, format="GIF")
        total += buf.tell()
    return (time.perf_counter() - t) * 1e3, total


def sizes_only(chunks):
    from dither_pie_amd import backend as be
    from oracle import oracle as orc
    frame = image_like_np(1, 1080, 1920)[0]
    rs = np.random.RandomState(2)
    for name, k, mode, params in (("bayer4x4 16 colours", 16, "bayer", {"size": "4x4"}),
                                  ("floyd-steinberg 256 colours", 256, "error_diffusion", {"variant": "floyd_steinberg", "serpentine": "false"})):
        pal = [tuple(int(v) for v in c) for c in rs.randint(0, 256, (k, 3))]
        rgb = orc.apply_dithering(frame, pal, mode, params)
        lut = {c: i for i, c in reversed(list(enumerate(pal)))}
        packed = rgb[..., 0].astype(np.int64) << 16 | rgb[..., 1].astype(np.int64) << 8 | rgb[..., 2]
        keys = np.array([c[0] << 16 | c[1] << 8 | c[2] for c in lut]), np.array(list(lut.values()))
        order = np.argsort(keys[0])
        plane = keys[1][order][np.searchsorted(keys[0][order], packed)].astype(np.uint8)
        mcs = max(2, int(np.ceil(np.log2(k + 1 if k < 256 else k))))
        whole = len(be.gif_lzw_host(plane, mcs, plane.size)[0])
        ms, pil = pillow_gif_ms([plane], pal)
        emit(f"host statement, one 1080p frame, {name}", unchunked_bytes=whole, pillow_bytes=pil, pillow_ms=round(ms, 1),
             ratio_to_unchunked={str(c): round(len(be.gif_lzw_host(plane, mcs, c)[0]) / whole, 4) for c in chunks})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--skip-video", action="store_true")
    ap.add_argument("--sizes-only", action="store_true")
    ap.add_argument("--chunks", default="4096,8192,16384,32768")
    args = ap.parse_args()
    chunks = [int(c) for c in args.chunks.split(",")]
    if args.sizes_only:
        return sizes_only(chunks)
    import torch
    from dither_pie_amd import _lib
    from dither_pie_amd import backend as be
    assert torch.cuda.is_available(), "needs a HIP device"
    R = args.repeats
    L = _lib.load()
    warm_a = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    warm_b = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    for _ in range(200):   # warm clocks: a second of copies
        warm_b.copy_(warm_a)
    torch.cuda.synchronize()
    del warm_a, warm_b

    for n, h, w in GEOMETRIES:
        geo = f"{n} x {h}p"
        frames = torch.from_numpy(image_like_np(n, h, w)).cuda()
        contents = {}
        for name, d in ditherers().items():
            planes, colours = d.apply_dithering_frames_indexed(frames)
            contents[name] = (planes, colours)
        contents["flat plane"] = (torch.full((n, h, w), 3, dtype=torch.uint8, device="cuda"), [(i, i, i) for i in range(16)])
        del frames
        for name, (planes, colours) in contents.items():
            k = len(colours)
            mcs = max(2, int(np.ceil(np.log2(k + 1 if k < 256 else k))))
            nbytes = planes.numel()
            copy_to = torch.empty_like(planes)
            emit(f"device copy of the plane bytes, {geo}", time_gpu(lambda: copy_to.copy_(planes), R), bytes=nbytes)
            prev = torch.empty(h * w, dtype=torch.uint8, device="cuda")
            changed = torch.empty(n, dtype=torch.int64, device="cuda")
            emit(f"dp_index_delta_u8 {geo} {name}",
                 time_gpu(lambda: be.check(L.dp_index_delta_u8(planes.data_ptr(), n, h * w, prev.data_ptr(), 1, min(k, 255), copy_to.data_ptr(),
                                                               changed.data_ptr(), be._stream())), R), bytes=nbytes)
            host_planes = planes.cpu().numpy()
            ms, pil_bytes = pillow_gif_ms(host_planes, colours)
            emit(f"Pillow save(format='GIF') on the host, {geo} {name}", pillow_ms=round(ms, 1), pillow_bytes=pil_bytes)
            for chunk in chunks:
                stride = int(L.dp_gif_lzw_bound_bytes(h, w, chunk))
                need = int(L.dp_gif_lzw_workspace_bytes(n, h, w, chunk))
                out = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
                sizes = torch.empty(n, dtype=torch.int64, device="cuda")
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                def encode():
                    be.check(L.dp_gif_lzw_encode_u8(planes.data_ptr(), n, h, w, mcs, chunk, out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), need,
                                                    be._stream()))
                t = time_gpu(encode, R)
                got = sizes.cpu().tolist()
                emit(f"dp_gif_lzw_encode_u8 {geo} {name} chunk_px {chunk}", t, encoded_bytes=sum(got), plane_bytes=nbytes, workspace_bytes=need)
                if chunk == chunks[len(chunks) // 2]:
                    def block():
                        s = sizes.cpu().tolist()
                        return out[:, :max(s)].cpu()
                    def per_frame():
                        s = sizes.cpu().tolist()
                        return [out[f, :m].cpu() for f, m in enumerate(s)]
                    for label, fn in (("one strided block", block), ("a copy per frame", per_frame)):
                        fn()
                        t0 = time.perf_counter()
                        for _ in range(10):
                            fn()
                        emit(f"payload to the host, {label}, {geo} {name}", host_ms_per_batch=round((time.perf_counter() - t0) * 100, 3))
                del out, ws
            del copy_to
        del contents
        torch.cuda.empty_cache()

    if args.skip_video:
        return
    import shutil
    import subprocess
    import tempfile
    import pipe_standin as ps
    from dither_pie_amd import video_processor as vproc
    if shutil.which("gcc") is None:
        emit("process_video_gif", error="no gcc: the decoder stand-in could not be built")
        return
    tmp = tempfile.mkdtemp(prefix="dp_gif_")
    n_frames, h, w = 300, 1080, 1920
    d = ps.build(os.path.join(tmp, "bin"))
    env = ps.environment(d, n_frames, h, w, distinct=8, keep=2)
    os.environ.update({k: v for k, v in env.items() if k == "PATH" or k.startswith("DP_STANDIN_")})
    fb = h * w * 3
    stage = torch.empty(15 * fb, dtype=torch.uint8, pin_memory=True)
    view = memoryview(stage.numpy())

    def read_ceiling():
        p = subprocess.Popen([os.path.join(d, "ffmpeg"), "-s", f"{w}x{h}", "pipe:1"], stdout=subprocess.PIPE, bufsize=0, env=env)
        vproc.VideoProcessor._widen_pipe(p.stdout)
        t, total = time.perf_counter(), 0
        while True:
            got = 0
            while got < len(view):
                n = p.stdout.readinto(view[got:])
                if not n:
                    break
                got += n
            total += got
            if got < len(view):
                break
        dt = time.perf_counter() - t
        p.stdout.close()
        p.wait()
        return total / fb / dt

    vp = vproc.VideoProcessor(devices=[torch.cuda.current_device()])
    dith = ditherers()["bayer4x4 16 colours"]
    runs = {"pipe": [], "process_video_gif": []}
    out_path = os.path.join(tmp, "o.gif")
    for _ in range(3):
        runs["pipe"].append(read_ceiling())
        t = time.perf_counter()
        done = vp.process_video_gif("standin.mp4", out_path, dith)
        runs["process_video_gif"].append(done / (time.perf_counter() - t))
    emit("300 x 1080p on the decoder stand-in, Bayer 4x4 at 16 colours, frames/s", fps_runs={k: [round(f, 1) for f in v] for k, v in runs.items()},
         file_bytes=os.path.getsize(out_path), stats={k: (round(v, 3) if isinstance(v, float) else v) for k, v in vp.last_gif_stats.items()})
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
