"""Times of the scene-cut detection on one MI355X (HIP events, warm clocks, 40 repeats; median [p10-p90]).

  python tools/bench_scripts/scene_time.py [--repeats 40] [--skip-scan]

  * dp_frame_signatures_u8 on 24 x 4K resident frames: noise, image-like content and ONE flat colour (every lane on the same
    LDS address), with a device copy of the same byte count in the same run beside each;
  * dp_signature_distances for the same batch;
  * VideoProcessor.scan_scenes(source="median_cut") frames/s on the compiled decoder stand-in (tools/pipe_standin.c), with
    scan_palette on the same clip and the bare decoder pipe beside it in the same run, and the stage times of
    last_scan_stats.
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


def emit(what, ms, nbytes=None, **extra):
    rec = {"what": what, **stats(ms), **extra}
    if nbytes is not None:
        rec["algorithmic_bytes"] = int(nbytes)
        rec["GBps_at_median"] = round(nbytes / (rec["median_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(rec), flush=True)


def image_like(torch, n, h, w):
    """Smooth ramps with grain, generated on the device (as tools/bench_scripts/clip_palette_time.py)."""
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
    from dither_pie_amd import _lib
    from dither_pie_amd import backend as be
    assert torch.cuda.is_available(), "needs a HIP device"
    R = args.repeats
    L = _lib.load()

    nbytes = N_FRAMES * H * W * 3
    big = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    half = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    for _ in range(200):   # warm clocks: a second of copies
        half.copy_(big[:nbytes // 2])
    torch.cuda.synchronize()

    sig = torch.empty((N_FRAMES, be.SCENE_BINS), dtype=torch.int32, device="cuda")
    prev = torch.zeros(be.SCENE_BINS, dtype=torch.int32, device="cuda")
    dist = torch.empty(N_FRAMES, dtype=torch.int64, device="cuda")
    for name in ("noise", "image-like", "flat"):
        if name == "noise":
            frames = torch.randint(0, 256, (N_FRAMES, H, W, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        elif name == "image-like":
            frames = image_like(torch, N_FRAMES, H, W)
        else:
            frames = torch.empty((N_FRAMES, H, W, 3), dtype=torch.uint8, device="cuda")
            frames[:] = torch.tensor([200, 17, 99], dtype=torch.uint8, device="cuda")

        def signatures():
            be.check(L.dp_frame_signatures_u8(frames.data_ptr(), N_FRAMES, H, W, sig.data_ptr(), be._stream()))

        # a copy that reads and writes nbytes in all; the signatures read nbytes and write next to nothing
        emit("device copy of 24x4K RGB bytes (half read, half written)", time_gpu(lambda: half.copy_(big[:nbytes // 2]), R), nbytes)
        emit(f"dp_frame_signatures_u8 24x4K {name}", time_gpu(signatures, R), nbytes, occupied_bins_frame0=int((sig[0] != 0).sum().item()))
        assert int(sig.to(torch.int64).sum().item()) == N_FRAMES * H * W
        emit(f"dp_signature_distances 24 signatures ({name})",
             time_gpu(lambda: be.check(L.dp_signature_distances(sig.data_ptr(), N_FRAMES, prev.data_ptr(), 1, dist.data_ptr(), be._stream())), R),
             2 * N_FRAMES * be.SCENE_BINS * 4)
        del frames
        torch.cuda.empty_cache()
    del big, half
    torch.cuda.empty_cache()

    if args.skip_scan:
        return
    import shutil
    import subprocess
    import tempfile
    import pipe_standin as ps
    from dither_pie_amd import video_processor as vproc
    if shutil.which("gcc") is None:
        print(json.dumps({"what": "scan_scenes", "error": "no gcc: the decoder stand-in could not be built"}))
        return
    tmp = tempfile.mkdtemp(prefix="dp_scene_")
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

    vp = vproc.VideoProcessor(devices=[torch.cuda.current_device()])
    runs = {"pipe": [], "scan_palette": [], "scan_scenes": [], "scan_scenes_boundaries_only": []}
    kept = {}
    for _ in range(3):   # interleaved: the three share whatever the machine does meanwhile
        runs["pipe"].append(read_ceiling())
        t = time.perf_counter()
        vp.scan_palette("standin.mp4", "median_cut", 16)
        runs["scan_palette"].append(n_frames / (time.perf_counter() - t))
        kept["scan_palette"] = dict(vp.last_scan_stats)
        t = time.perf_counter()
        scenes = vp.scan_scenes("standin.mp4", "median_cut", 16)
        runs["scan_scenes"].append(n_frames / (time.perf_counter() - t))
        kept["scan_scenes"] = dict(vp.last_scan_stats)
        t = time.perf_counter()
        vp.scan_scenes("standin.mp4", None)
        runs["scan_scenes_boundaries_only"].append(n_frames / (time.perf_counter() - t))
        kept["scan_scenes_boundaries_only"] = dict(vp.last_scan_stats)

    def rounded(s):
        return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in s.items()}
    print(json.dumps({"what": "600 x 1080p on the decoder stand-in, median cut 16, frames/s", "fps_runs": {k: [round(f, 1) for f in v] for k, v in runs.items()},
                      "scan_scenes_over_scan_palette": round(float(np.median(runs["scan_scenes"]) / np.median(runs["scan_palette"])), 3),
                      "scenes_found": len(scenes), "stats": {k: rounded(v) for k, v in kept.items()}}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
