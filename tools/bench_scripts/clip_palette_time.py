"""Times of the clip-wide palettes on one MI355X (HIP events, warm clocks, 40 repeats; median [p10-p90]).

  python tools/bench_scripts/clip_palette_time.py [--repeats 40] [--skip-scan]

  * dp_distinct_stream_add_u8 per 24 x 4K batch: the FIRST batch (every colour new; reset + add, the reset timed beside it)
    and STEADY state (nothing new), on noise and on image-like content, with dp_distinct_first_u8 over the same bytes in the
    same run beside each -- the resident kernel is the yardstick;
  * dp_hist_sample_u8 for 10 000 ranks;
  * ClipPalette.kmeans(32) on a 100-frame 1080p clip (accumulate + fit, and the fit alone) beside kmeans.fit_palette on one frame;
  * VideoProcessor.scan_palette frames/s on the compiled decoder stand-in (tools/pipe_standin.c) beside the decoder pipe alone.
Run from the root of the tree; prints one JSON line per figure."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tools"))

N_FRAMES, H, W = 24, 2160, 3840


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(a[int(0.1 * (len(a) - 1))]), 4),
            "p90_ms": round(float(a[int(round(0.9 * (len(a) - 1)))]), 4), "repeats": len(a)}


def time_gpu(fn, repeats=40, warmup=3, before=None):
    import torch
    out = []
    for i in range(warmup + repeats):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return out


def emit(what, ms, **extra):
    print(json.dumps({"what": what, **stats(ms), **extra}), flush=True)


def image_like(torch, n, h, w):
    """Smooth ramps with grain, generated on the device: a few hundred thousand distinct colours, long runs of near-equal pixels."""
    y = torch.arange(h, device="cuda").view(1, h, 1).float()
    x = torch.arange(w, device="cuda").view(1, 1, w).float()
    t = torch.arange(n, device="cuda").view(n, 1, 1).float()
    g = torch.Generator(device="cuda").manual_seed(1)
    ch = [(x * (200.0 / w) + t * 2 + 20), (y * (180.0 / h) + t + 30), ((x + y) * (150.0 / (w + h)) + 40)]
    f = torch.stack([c.expand(n, h, w) for c in ch], dim=-1)
    f = f + torch.randint(0, 3, f.shape, device="cuda", generator=g).float()
    return f.clamp_(0, 255).to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--skip-scan", action="store_true")
    args = ap.parse_args()
    import torch
    from dither_pie_amd import backend as be
    from dither_pie_amd import kmeans
    from dither_pie_amd.clip_palette import ClipPalette
    assert torch.cuda.is_available(), "needs a HIP device"
    R = args.repeats

    big = torch.empty(N_FRAMES * H * W * 3, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(big)
    for _ in range(200):   # warm clocks: a second of copies
        dst.copy_(big)
    torch.cuda.synchronize()
    del dst

    n_px = N_FRAMES * H * W
    for name in ("noise", "image-like"):
        if name == "noise":
            frames = torch.randint(0, 256, (N_FRAMES, H, W, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        else:
            frames = image_like(torch, N_FRAMES, H, W)
        px = frames.view(-1, 3)
        s = be.DistinctStream()
        emit(f"dp_distinct_first_u8 24x4K {name}", time_gpu(lambda: be.distinct_first(px), R), pixels=n_px)
        emit("dp_distinct_stream_reset", time_gpu(lambda: s.reset(), R))
        emit(f"dp_distinct_stream_add_u8 24x4K {name}: first batch (all new)", time_gpu(lambda: s.add(px), R, before=lambda: s.reset()), pixels=n_px)
        s.reset().add(px)
        n_distinct = len(s)
        emit(f"dp_distinct_stream_add_u8 24x4K {name}: steady state (nothing new)", time_gpu(lambda: s.add(px), R), pixels=n_px, n_distinct=n_distinct)
        assert len(s) == n_distinct
        del frames, px, s
        torch.cuda.empty_cache()
    del big
    torch.cuda.empty_cache()

    # rank sample: 10 000 ranks of a 100-frame 1080p clip's histogram (noise: every cell occupied)
    clip = ClipPalette()
    t0 = time.perf_counter()
    for i in range(10):
        batch = image_like(torch, 10, 1080, 1920) if i % 2 else torch.randint(0, 256, (10, 1080, 1920, 3), dtype=torch.uint8, device="cuda")
        clip.add(batch)
    torch.cuda.synchronize()
    emit("ClipPalette.add of 100 x 1080p in batches of 10 (incl. generating them)", [(time.perf_counter() - t0) * 1e3])
    ranks = torch.from_numpy(np.random.RandomState(42).randint(0, clip.n_pixels, 10000).astype(np.int64)).cuda()
    emit("dp_hist_sample_u8 10 000 ranks", time_gpu(lambda: clip._hist.sample(ranks), R), pixels=clip.n_pixels)

    def host_ms(fn, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return out
    emit("ClipPalette.kmeans(32) on 100 x 1080p: the fit alone (host wall)", host_ms(lambda: clip.kmeans(32), 7), n_distinct=clip.n_distinct)
    emit("ClipPalette.median_cut(256) on 100 x 1080p: download + host cut (host wall)", host_ms(lambda: clip.median_cut(256), 5))
    one = image_like(torch, 1, 1080, 1920).view(-1, 3)
    emit("kmeans.fit_palette(32) on one 1080p frame (host wall)", host_ms(lambda: kmeans.fit_palette(one, 32), 7))
    del clip
    torch.cuda.empty_cache()

    if args.skip_scan:
        return
    import shutil
    import subprocess
    import tempfile
    import pipe_standin as ps
    from dither_pie_amd import video_processor as vproc
    if shutil.which("gcc") is None:
        print(json.dumps({"what": "scan_palette", "error": "no gcc: the decoder stand-in could not be built"}))
        return
    tmp = tempfile.mkdtemp(prefix="dp_scan_")
    n_frames, h, w = 600, 1080, 1920
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
    ceiling = [read_ceiling() for _ in range(3)]
    vp = vproc.VideoProcessor(devices=[torch.cuda.current_device()])
    for source in ("median_cut", "kmeans"):
        fps = []
        for _ in range(3):
            t = time.perf_counter()
            vp.scan_palette("standin.mp4", source, 32)
            fps.append(n_frames / (time.perf_counter() - t))
        print(json.dumps({"what": f"scan_palette {source} 600 x 1080p on the decoder stand-in", "fps_runs": [round(f, 1) for f in fps],
                          "decoder_pipe_to_pinned_buffer_fps_runs": [round(c, 1) for c in ceiling], "stats": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in vp.last_scan_stats.items()}}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
