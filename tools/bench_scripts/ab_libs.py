"""A/B of two BUILDS in one process: libditherpie_hip.so (A) against libditherpie_hip_exp.so (B), alternating, for a kernel change
that was compiled into only one of them (build A from the committed sources, apply the change, `make ../libditherpie_hip_exp.so`).
Box-to-box spread on this pool is +-4 %: differences smaller than that can only be seen this way.
usage: ab_libs.py [case ...]   cases: variant:K:frames  (e.g. floyd_steinberg:16:1 atkinson:16:1 floyd_steinberg:256:1 floyd_steinberg:16:256)
       a fourth field "s" asks for the serpentine scan (floyd_steinberg:16:64:s, ostromoukhov:16:64:s) and riemersma:K:frames runs
       ImageDitherer(DitherMode.RIEMERSMA).apply_dithering_frames (one backend.riemersma launch underneath): the three
       one-wave-per-frame kernels, on 1080p frames (a step of theirs is a pixel, ~0.5 s a launch: one warm-up and three timed
       launches per repetition; profiles/HISTORY.md has the A/A noise of these cases)
       or integer error diffusion (idiff.hip) with a variant's taps on 4K frames: idiff_floyd_steinberg:16:1, idiff_jjn:256:24
       or ordered modes on 1080p frames: bayer4:K:frames, bayer8:K:frames, none:K:frames, ign:K:frames (bayer4:16:100 = C5's launch;
       K <= 64: the uniform palette, else palr(K, 7); the cell table is built before the timing)
       or the PNG-8 encoder's fixed-mode entry point on photo-like 1080p planes: png:K:frames (dp_png_deflate_encode_u8 at the default
       seg_bytes; run these on their own, not mixed with the cases above)"""
import sys; sys.path.insert(0, '.')
import numpy as np, torch
from dither_pie_amd import _lib, dithering_lib
from dither_pie_amd.dithering_lib import ImageDitherer, DitherMode, ColorReducer
cases = sys.argv[1:] or ["floyd_steinberg:16:1", "atkinson:16:1", "floyd_steinberg:256:1", "floyd_steinberg:16:256"]
if all(c.startswith("png:") for c in cases):
    sys.path.insert(0, 'tests')
    import png_ref as pr
    from dither_pie_amd import backend
    for case in cases:
        _, K, nf = case.split(":"); K = int(K); nf = int(nf)
        one = pr.photo_plane(K, 1080, 1920)
        planes = torch.from_numpy(np.stack([np.roll(one, 7 * i, axis=1) for i in range(nf)])).cuda()
        best, outs = {False: [], True: []}, {}
        for rep in range(3):
            for exp in (False, True):
                _lib.select(exp)
                for _ in range(2): outs[exp] = backend.png_deflate(planes, backend.png_depth(K))
                torch.cuda.synchronize()
                ts = []
                for _ in range(12):
                    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                    e0.record(); outs[exp] = backend.png_deflate(planes, backend.png_depth(K)); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
                best[exp].append(min(ts))
        a, b = min(best[False]), min(best[True])
        m = int(outs[False][1].max())
        same = torch.equal(outs[False][1], outs[True][1]) and torch.equal(outs[False][0][:, :m], outs[True][0][:, :m])
        print(f"{case:28s} A (product) {a:8.3f} ms   B (experiments twin) {b:8.3f} ms   B/A {b / a:.3f}   identical bytes: {same}"
              f"   [A runs {' '.join('%.3f' % v for v in best[False])} | B runs {' '.join('%.3f' % v for v in best[True])}]", flush=True)
    sys.exit(0)
g = torch.Generator(device='cuda'); g.manual_seed(1)
ORDERED = {"none": (DitherMode.NONE, {}), "bayer8": (DitherMode.BAYER, {"size": "8x8"}), "bayer4": (DitherMode.BAYER, {"size": "4x4"}),
           "ign": (DitherMode.INTERLEAVED_GRADIENT_NOISE, {})}
def one_wave(c): return c.startswith("riemersma:") or c.endswith(":s")
nmax = max(int(c.split(":")[2]) for c in cases)
small = all(c.split(":")[0] in ORDERED for c in cases)
f = torch.randint(0, 256, (nmax, 1080, 1920, 3) if small else (nmax, 2160, 3840, 3), dtype=torch.uint8, device='cuda', generator=g)
outs = {False: torch.empty_like(f), True: torch.empty_like(f)}
f1080 = f[:max([int(c.split(":")[2]) for c in cases if one_wave(c)] or [0]), :1080, :1920].contiguous()
for case in cases:
    variant, K, nf = case.split(":")[:3]; K = int(K); nf = int(nf)
    serp = "true" if case.endswith(":s") else "false"
    src = f1080 if one_wave(case) else f
    pal = ColorReducer.generate_uniform_palette(K) if K <= 64 else [tuple(int(v) for v in c) for c in np.random.RandomState(7).randint(0, 256, (K, 3))]
    best = {False: [], True: []}
    for rep in range(3):
        for exp in (False, True):
            _lib.select(exp)
            dithering_lib.drop_device_caches()
            if variant in ORDERED:
                d = ImageDitherer(K, ORDERED[variant][0], pal, False, ORDERED[variant][1]).prepare()
            elif variant == "riemersma":
                d = ImageDitherer(K, DitherMode.RIEMERSMA, pal, False, {})
            elif variant.startswith("idiff_"):
                d = ImageDitherer(K, dithering_lib.IntegerErrorDiffusionDitherStrategy(variant[6:]), pal, False, {})
            elif variant in ("perceptual", "hybrid", "adaptive_variance", "ostromoukhov"):
                d = ImageDitherer(K, DitherMode(variant), pal, False, {"serpentine": serp} if variant == "ostromoukhov" else {})
            else:
                d = ImageDitherer(K, DitherMode.ERROR_DIFFUSION, pal, False, {"variant": variant, "serpentine": serp})
            o = outs[exp].view(-1)[:src[:nf].numel()].view(src[:nf].shape)
            for _ in range(1 if one_wave(case) else 2): d.apply_dithering_frames(src[:nf], out=o)
            torch.cuda.synchronize()
            ts = []
            for _ in range(12 if small else (3 if one_wave(case) else 5)):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); d.apply_dithering_frames(src[:nf], out=o); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
            best[exp].append(min(ts))
            del d
    a, b = min(best[False]), min(best[True])
    n_out = src[:nf].numel()
    same = torch.equal(outs[False].view(-1)[:n_out], outs[True].view(-1)[:n_out])
    print(f"{case:28s} A (product) {a:8.3f} ms   B (experiments twin) {b:8.3f} ms   B/A {b / a:.3f}   identical bytes: {same}"
          f"   [A runs {' '.join('%.3f' % v for v in best[False])} | B runs {' '.join('%.3f' % v for v in best[True])}]", flush=True)
