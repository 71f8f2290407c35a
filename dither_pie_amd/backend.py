"""Thin tensor-level wrappers over the C ABI: frames live in torch uint8 tensors on the GPU
(PyTorch-ROCm is used for device memory and streams only), kernels come from
libditherpie_hip.so.  Nothing here computes pixels on the host."""
from __future__ import annotations

import ctypes as C
import threading
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import MODE_IGN, MODE_MATRIX, MODE_NEAREST, DitherPieError, check


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu():
    if not torch.cuda.is_available():
        raise DitherPieError(-2, "no HIP device visible: the MI355X backend has no CPU fallback")


METRICS = ("rgb", "oklab")   # DP_METRIC_RGB, DP_METRIC_OKLAB (include/ditherpie_hip_metric.h)


class Palette:
    """dp_palette: scipy-order KD-tree + colour tables resident in HBM.

    pal_f32 [K,3] float32 as the KD-tree sees it; out_colors [K,3] uint8 written for each entry;
    lut_in optional 256-entry uint8 map applied to the input bytes."""

    # Building the search accelerator (KD-tree aside: a scan of all 2^24 colours, cell table, tie codes) takes ~3.5 ms up to 256
    # colours and ~25 ms at 1024 (rounds 1-4: 7-12 ms; tools/bench_scripts/accel_build_stages.py), once per palette; the brute-force
    # kernels need ~9 K vector instructions per pixel against ~70 with it.  A palette therefore runs on the brute-force kernels
    # until the pixels it has served would have paid for the build (break-even ~ 1.4e10 / K pixels up to 256 colours: 56 Mpixel
    # = seven 4K frames at 256, 0.9 Gpixel at 16) and builds it then -- never more than twice the cost of the better choice,
    # whatever follows.  One image or a GUI preview never builds it; a video does within its first frames.  build_accel() forces
    # it (long-running jobs that know what is coming).
    ACCEL_BUILD_SECONDS = 0.0038                 # (3.7-3.9 ms at 256 colours since the scan also keeps the nearest sets of the 8-wide sub-cells)
    ACCEL_BUILD_SECONDS_LARGE = 0.025            # more than 256 colours (128-byte membership masks, deeper tables)
    BRUTE_SECONDS_PER_PIXEL_PER_COLOUR = 2.46e-13

    def accel_break_even_pixels(self):
        build = self.ACCEL_BUILD_SECONDS if self.K <= 256 else self.ACCEL_BUILD_SECONDS_LARGE
        return build / (self.BRUTE_SECONDS_PER_PIXEL_PER_COLOUR * max(self.K, 1))

    def note_pixels(self, n_px):
        """Account n_px pixels about to be processed; builds the accelerator once they have paid for it."""
        if self._accel_done:
            return
        self._px_served += int(n_px)
        if self._px_served >= self.accel_break_even_pixels():
            self.build_accel()

    def __init__(self, pal_f32, out_colors, lut_in=None, accel=False, metric="rgb"):
        """metric: "rgb" (squared Euclidean RGB distance, the reference's) or "oklab" (include/ditherpie_hip_metric.h: an
        integer Oklab, at most 256 colours, integer palette values, no lut_in).  A metric palette is searched through its own
        top-2 table only: ordered(), pattern(), dotdiff() and idiff() use it, every other mode refuses it."""
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
        if metric != "rgb" and lut_in is not None:
            raise ValueError(f"a palette with the {metric!r} metric takes no lut_in (Oklab linearises by itself)")
        require_gpu()
        self.pal_f32 = np.ascontiguousarray(pal_f32, dtype=np.float32).reshape(-1, 3)
        self.out_colors = np.ascontiguousarray(out_colors, dtype=np.uint8).reshape(-1, 3)
        if self.pal_f32.shape != self.out_colors.shape:
            raise ValueError("pal_f32 and out_colors must both be [K,3]")
        self.lut_in = None if lut_in is None else np.ascontiguousarray(lut_in, dtype=np.uint8)
        if self.lut_in is not None and self.lut_in.size != 256:
            raise ValueError("lut_in must have 256 entries")
        self.K = self.pal_f32.shape[0]
        self._h = C.c_void_p()
        self._destroy = _lib.load().dp_palette_destroy
        self.metric = metric
        if metric == "rgb":
            check(_lib.load().dp_palette_create(_np_ptr(self.pal_f32), _np_ptr(self.out_colors), self.K,
                                                _np_ptr(self.lut_in), C.byref(self._h)))
        else:
            check(_lib.load().dp_palette_create_metric(_np_ptr(self.pal_f32), _np_ptr(self.out_colors), self.K,
                                                       METRICS.index(metric), C.byref(self._h)))
        k, integer, nodes = C.c_int(), C.c_int(), C.c_int()
        check(_lib.load().dp_palette_info(self._h, C.byref(k), C.byref(integer), C.byref(nodes)))
        self.is_integer = bool(integer.value)
        self.n_nodes = nodes.value
        self.accel_entries = self.accel_max_list = 0
        self._accel_done = metric != "rgb"   # a metric palette never builds the accelerator: its table is its only search
        self._px_served = 0
        self._accel_lock = threading.Lock()
        self.device = torch.device("cuda", torch.cuda.current_device())
        if accel:
            self.build_accel()

    def build_accel(self):
        """Build the LDS cell table + tie codes (synchronous, idempotent; a no-op for palettes that do
        not qualify).  Thread-safe: concurrent builders wait for the one build; threads that are launching with the
        palette meanwhile are safe because the library builds into a private copy of the device record and publishes it
        with one assignment, and every launch works on a snapshot of that record (host.cpp: snapshot / publish) - such a
        launch simply still runs without the accelerator."""
        if self._accel_done:
            return
        with self._accel_lock:
            if self._accel_done:
                return
            with torch.cuda.device(self.device):
                check(_lib.load().dp_palette_build_accel(self._h))
            pe, mc = C.c_int(), C.c_int()
            check(_lib.load().dp_palette_accel_info(self._h, C.byref(pe), C.byref(mc)))
            self.accel_entries, self.accel_max_list = pe.value, mc.value
            self._accel_done = True

    def pattern_prepare(self):
        """Build the pattern-dither search table of this palette now (dp_pattern_prepare: 16 MiB of device memory, 0.3 ms at 16
        colours and 1.3 - 1.7 ms at 256 on one MI355X, synchronous, idempotent) instead of at the first pattern() call -- which
        is also what a caller who captures pattern() into a graph has to do first.  The C entry point takes no stream: the
        build runs on the device's null stream, not on torch's current one, and is waited for before the call returns; the
        lock of the current (device, stream) is held meanwhile, as for every launch.  Returns the table's size in bytes."""
        with torch.cuda.device(self.device), _Launch(self.device, None):
            check(_lib.load().dp_pattern_prepare(self._h))
        return int(_lib.load().dp_pattern_table_bytes(self._h))

    def metric_prepare(self):
        """Build the top-2 table of a metric palette now (dp_metric_prepare: 32 MiB of device memory, synchronous, idempotent,
        on the device's null stream) instead of at the first ordered() / pattern() / dotdiff() call with it -- which is also
        what a caller who captures one of them into a graph has to do first.  Returns the table's size in bytes."""
        if self.metric == "rgb":
            raise ValueError("metric_prepare() needs a palette with a metric (Palette(..., metric='oklab'))")
        with torch.cuda.device(self.device), _Launch(self.device, None):
            check(_lib.load().dp_metric_prepare(self._h))
        return int(_lib.load().dp_metric_table_bytes(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._destroy(h)
            self._h = None


class Thresholds:
    """dp_thresholds: a threshold matrix resident in HBM."""

    def __init__(self, handle):
        self._h = handle
        self._destroy = _lib.load().dp_thresholds_destroy
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(_lib.load().dp_thresholds_shape(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.shape = (a.value, b.value)
        self.integer_form = bool(c.value)

    @classmethod
    def from_matrix(cls, m):
        require_gpu()
        m = np.ascontiguousarray(m, dtype=np.float32)
        if m.ndim != 2:
            raise ValueError("threshold matrix must be 2-D")
        h = C.c_void_p()
        check(_lib.load().dp_thresholds_create(_np_ptr(m), m.shape[0], m.shape[1], C.byref(h)))
        return cls(h)

    @classmethod
    def blue_noise(cls, size, seed):
        require_gpu()
        h = C.c_void_p()
        check(_lib.load().dp_thresholds_blue_noise(int(size), int(seed) & 0xFFFFFFFF, _stream(), C.byref(h)))
        return cls(h)

    @classmethod
    def void_cluster(cls, h, w, seed, sigma=1.5):
        """The void-and-cluster matrix of include/ditherpie_hip_voidcluster.h, generated on the device, as thresholds."""
        h, w, s256 = _void_cluster_args(h, w, sigma)
        require_gpu()
        t = C.c_void_p()
        check(_lib.load().dp_thresholds_void_cluster(h, w, int(seed) & 0xFFFFFFFF, s256, _stream(), C.byref(t)))
        return cls(t)

    def numpy(self):
        out = np.empty(self.shape, np.float32)
        check(_lib.load().dp_thresholds_download(self._h, _np_ptr(out)))
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._destroy(h)
            self._h = None


def _check_palette_device(pal, f):
    if getattr(pal, "device", f.device) != f.device:
        raise ValueError(f"palette lives on {pal.device}, frames on {f.device}")


def _frames(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
        raise TypeError("frames must be a CUDA uint8 tensor")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[-1] != 3:
        raise ValueError("frames must be [N,H,W,3] or [H,W,3]")
    return t.contiguous()


def _check_out(out, f):
    """A caller-supplied output buffer must be exactly what the kernel writes: uint8, contiguous, same device,
    as many elements as the frames.  Returns it viewed in the frames' [N,H,W,3] shape."""
    if out is None:
        return torch.empty_like(f)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8):
        raise TypeError("out must be a CUDA uint8 tensor")
    if out.device != f.device:
        raise ValueError(f"out is on {out.device}, frames on {f.device}")
    if out.numel() != f.numel() or not out.is_contiguous():
        raise ValueError("out must be contiguous and hold exactly as many bytes as the frames")
    return out.view(f.shape)


# Scratch per (device, stream): the launch sequences of one call (memset, pass 1, fix-up; progress words, wavefront
# kernel) use it in stream order, so two host threads on the SAME stream must not interleave their sequences (ctypes
# drops the GIL): workspace acquisition + launches run under the lock of that (device, stream).  Different streams
# have different workspaces and run concurrently.
_WS_KEEP_MIN = 16            # (device, stream) scratch buffers kept at least; see _ws_keep()
_WS_SHRINK = 8               # a buffer more than this many times larger than a request is replaced by a smaller one
_ws_cache = OrderedDict()    # key -> [tensor, lock, users]: users = launches inside or waiting for the entry
_ws_guard = threading.Lock()


def _ws_keep():
    """How many (device, stream) scratch buffers are kept before the least recently used idle one is dropped: every device
    with its default stream, its worker stream (sharding.process_on_devices) and its pipe stream (video_processor), plus
    slack -- 8 GPUs in one process are 24 live keys, and a fixed 8 evicted and re-allocated one per batch."""
    return max(_WS_KEEP_MIN, 3 * torch.cuda.device_count() + 4)


class _Launch:
    """with _Launch(device, nbytes) as ws: ... -- the (device, stream) lock held, ws a scratch tensor of >= nbytes
    (nbytes None: a call without workspace, only the lock; ws is None and the cached scratch is left as it is)."""

    def __init__(self, device, nbytes):
        self.key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        self.device, self.nbytes = device, None if nbytes is None else max(int(nbytes), 1)

    def __enter__(self):
        with _ws_guard:
            ent = _ws_cache.get(self.key)
            if ent is None:
                ent = _ws_cache[self.key] = [None, threading.RLock(), 0]
            ent[2] += 1
            _ws_cache.move_to_end(self.key)
            if len(_ws_cache) > _ws_keep():
                # least recently used first; an entry somebody is inside of (or queued for) is never dropped: its lock is
                # what serialises that stream's launch sequences, a fresh entry for the same key would hand out a second one
                for k in [k for k, e in _ws_cache.items() if e[2] == 0]:
                    if len(_ws_cache) <= _ws_keep():
                        break
                    del _ws_cache[k]
        self.ent = ent
        ent[1].acquire()
        if self.nbytes is None:
            return None
        try:
            t = ent[0]
            if t is None or t.numel() < self.nbytes or t.numel() > _WS_SHRINK * max(self.nbytes, 1 << 20):
                t = ent[0] = torch.empty(max(self.nbytes, 1 << 20), dtype=torch.uint8, device=self.device)
        except BaseException:   # out of memory on a grow: __exit__ will not run, the stream's lock must not stay held
            ent[1].release()
            with _ws_guard:
                ent[2] -= 1
            raise
        return t

    def __exit__(self, *exc):
        self.ent[1].release()
        with _ws_guard:
            self.ent[2] -= 1
        return False


def release_workspaces():
    """Drop every cached scratch buffer nobody is using (they are re-created on demand)."""
    with _ws_guard:
        for k in [k for k, e in _ws_cache.items() if e[2] == 0]:
            del _ws_cache[k]


def ordered(frames, pal: Palette, mode, thr: Thresholds | None = None, ign_scale=1.0, ign_seed=0, y0=0, x0=0,
            out=None):
    """nearest / threshold-matrix / IGN dithering of uint8 frames already in HBM -> uint8 frames."""
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    L = _lib.load()
    if getattr(pal, "metric", "rgb") != "rgb":   # a metric palette: one gather per pixel from its top-2 table (dp_metric_ordered_u8)
        if int(mode) == MODE_IGN:
            raise ValueError(f"interleaved gradient noise is not supported with the {pal.metric!r} metric")
        with torch.cuda.device(f.device), _Launch(f.device, None):
            check(L.dp_metric_ordered_u8(f.data_ptr(), out.data_ptr(), n, h, w, int(y0), int(x0), pal._h, int(mode),
                                         thr._h if thr is not None else None, _stream()))
        return out.view(frames.shape)
    ws_bytes = L.dp_ordered_workspace_bytes(n, h, w)
    with torch.cuda.device(f.device):
        pal.note_pixels(n * h * w)
        with _Launch(f.device, ws_bytes) as ws:
            check(L.dp_ordered_u8(f.data_ptr(), out.data_ptr(), n, h, w, int(y0), int(x0), pal._h, int(mode),
                                  thr._h if thr is not None else None, float(ign_scale), int(ign_seed),
                                  ws.data_ptr(), ws.numel(), _stream()))
    return out.view(frames.shape)


def metric_lab(pixels):
    """(L, a, b) of uint8 RGB pixels in HBM ([..., 3], contiguous) under the Oklab metric -> int32 tensor of the same shape
    (dp_metric_lab_u8: the device function the metric's kernels use)."""
    if not (isinstance(pixels, torch.Tensor) and pixels.is_cuda and pixels.dtype == torch.uint8 and pixels.dim() >= 1
            and pixels.shape[-1] == 3):
        raise TypeError("pixels must be a CUDA uint8 tensor [..., 3]")
    p = pixels.contiguous()
    out = torch.empty(p.shape, dtype=torch.int32, device=p.device)
    with torch.cuda.device(p.device), _Launch(p.device, None):
        check(_lib.load().dp_metric_lab_u8(p.data_ptr(), out.data_ptr(), p.numel() // 3, _stream()))
    return out


def _rgb_host(rgb):
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    if a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("rgb must be [..., 3]")
    return a


def metric_lab_host(rgb):
    """The host statement of metric_lab (dp_metric_lab_host; no device): uint8 [..., 3] -> int32 [..., 3]."""
    a = _rgb_host(rgb)
    out = np.empty(a.shape, np.int32)
    check(_lib.load().dp_metric_lab_host(_np_ptr(a), a.size // 3, _np_ptr(out)))
    return out


def metric_top2_host(rgb, pal_f32, metric="oklab"):
    """The host statement of a metric palette's table (dp_metric_top2_host; no device): uint8 [..., 3] -> (nearest, second),
    uint8 [...] each: the two smallest (distance, index) pairs, the lowest index first on equal distance."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
    a = _rgb_host(rgb)
    pal = np.ascontiguousarray(pal_f32, dtype=np.float32).reshape(-1, 3)
    i0, i1 = np.empty(a.shape[:-1], np.uint8), np.empty(a.shape[:-1], np.uint8)
    check(_lib.load().dp_metric_top2_host(_np_ptr(a), a.size // 3, _np_ptr(pal), pal.shape[0], METRICS.index(metric), _np_ptr(i0),
                                          _np_ptr(i1)))
    return i0, i1


def error_diffusion(frames, pal: Palette, taps, divisor, serpentine=False, out=None, arithmetic="python"):
    """taps: [(dx, dy, weight)] in the reference's list order.  arithmetic: "python" -- the reference's pure-Python
    branch (dithering_lib.py:655-690: KD-tree nearest, float32 products and sums) -- or "numba" -- its
    _error_diffusion_numba branch (:213-308, typed per numba's unification rule: float64 linear-scan nearest, float64 error,
    float64 products and sums rounded on the store; parity-unpinned, fixtures pending)."""
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    dx = np.array([t[0] for t in taps], np.int32)
    dy = np.array([t[1] for t in taps], np.int32)
    L = _lib.load()
    ws_bytes = L.dp_error_diffusion_workspace_bytes(n, h, w)
    if arithmetic not in ("python", "numba"):
        raise ValueError("arithmetic must be 'python' or 'numba'")
    with torch.cuda.device(f.device), _Launch(f.device, ws_bytes) as ws:
        if arithmetic == "numba":
            wts = np.array([t[2] for t in taps], np.float32)  # the reference: np.array([...], dtype=np.float32)
            check(L.dp_error_diffusion_numba_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, _np_ptr(dx), _np_ptr(dy),
                                                _np_ptr(wts), float(divisor), len(taps), 1 if serpentine else 0,
                                                ws.data_ptr(), ws.numel(), _stream()))
        else:
            wq = np.array([t[2] / divisor for t in taps], np.float64).astype(np.float32)
            check(L.dp_error_diffusion_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, _np_ptr(dx), _np_ptr(dy),
                                          _np_ptr(wq), len(taps), 1 if serpentine else 0, ws.data_ptr(), ws.numel(),
                                          _stream()))
    return out.view(frames.shape)


def hybrid_numba(frames, pal: Palette, lum_factor=1.0, col_factor=0.2, out=None):
    """HybridDitherStrategy as the reference's numba branch computes it (_hybrid_numba, dithering_lib.py:1396-1494: clamped
    values, float64 linear-scan nearest, float64 luminance / colour split of the error, float64 pushes rounded on the store)."""
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    L = _lib.load()
    ws_bytes = L.dp_error_diffusion_workspace_bytes(n, h, w)
    with torch.cuda.device(f.device), _Launch(f.device, ws_bytes) as ws:
        check(L.dp_hybrid_numba_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, float(lum_factor), float(col_factor),
                                   ws.data_ptr(), ws.numel(), _stream()))
    return out.view(frames.shape)


def riemersma(frames, pal: Palette, out=None):
    """Riemersma dithering (RiemersmaDitherStrategy.dither, dithering_lib.py:812-841): error diffusion along the Hilbert curve
    of the next power-of-two square, the reference's float32 arithmetic and KD-tree nearest; uint8 frames in HBM."""
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    L = _lib.load()
    with torch.cuda.device(f.device), _Launch(f.device, None):   # (no workspace: the lock of the (device, stream) only)
        check(L.dp_riemersma_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, _stream()))
    return out.view(frames.shape)


PATTERN_MATRICES = (2, 4, 8)


def pattern(frames, pal: Palette, matrix, strength256, y0=0, x0=0, out=None):
    """Pattern (Knoll) dithering (include/ditherpie_hip_pattern.h) of uint8 frames already in HBM -> uint8 frames: per pixel
    matrix * matrix nearest-colour searches through the palette's 2^24-entry table (built at the first call with the palette),
    the Bayer rank matrix picks one candidate in luminance order.  Position-only: (y0, x0) are the global coordinates of each
    frame's first pixel.  matrix 2, 4 or 8; strength256 0 .. 256; at most 256 colours."""
    if matrix not in PATTERN_MATRICES:
        raise ValueError(f"pattern matrix must be one of {PATTERN_MATRICES}, not {matrix!r}")
    if not (isinstance(strength256, (int, np.integer)) and 0 <= strength256 <= 256):
        raise ValueError(f"pattern strength256 must be an integer in 0 .. 256, not {strength256!r}")
    if pal.K > 256:
        raise ValueError(f"pattern dithering supports at most 256 colours, the palette has {pal.K}")
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    L = _lib.load()
    with torch.cuda.device(f.device), _Launch(f.device, None):   # (no workspace: the lock of the (device, stream) only)
        check(L.dp_pattern_u8(f.data_ptr(), out.data_ptr(), n, h, w, int(y0), int(x0), pal._h, int(matrix), int(strength256),
                              _stream()))
    return out.view(frames.shape)


DOTDIFF_SIZES = (2, 4, 8, 16)   # class matrices of dp_dotdiff_u8 are m x m
DOTDIFF_MAX_REACH = 16          # DP_DOTDIFF_MAX_REACH: the halo of a tile of the kernel
DOTDIFF_TILE = 64               # the tile edge of the kernel (dotdiff.hip: kDotTile); tests build their multi-tile shapes on it


def _dotdiff_classes(classes):
    """An m x m class matrix -> its m * m bytes, row-major; ValueError unless it is a permutation of 0 .. m*m-1."""
    try:
        a = np.asarray(classes)
    except Exception:
        raise ValueError("dot diffusion: the class matrix must be an m x m array of integers") from None
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] not in DOTDIFF_SIZES or a.dtype.kind not in "iu":
        raise ValueError(f"dot diffusion: the class matrix must be m x m integers with m in {DOTDIFF_SIZES}, "
                         f"not {a.dtype} {a.shape}")
    if sorted(a.reshape(-1).tolist()) != list(range(a.size)):
        raise ValueError(f"dot diffusion: the class matrix must be a permutation of 0 .. {a.size - 1}")
    return np.ascontiguousarray(a, np.uint8)


def dotdiff_reach(classes):
    """The reach of a class matrix (dp_dotdiff_reach; include/ditherpie_hip_dotdiff.h): the longest path of king moves
    through the tiled matrix along which the class strictly increases.  Host code: no device is needed."""
    c = _dotdiff_classes(classes)
    r = int(_lib.load().dp_dotdiff_reach(_np_ptr(c), int(c.shape[0])))
    if r < 0:
        raise ValueError("dot diffusion: the library refused the class matrix")
    return r


def dotdiff(frames, pal: Palette, classes, strength256, out=None):
    """Dot diffusion (include/ditherpie_hip_dotdiff.h) of uint8 frames already in HBM -> uint8 frames: error diffusion in the
    order of the tiled class matrix `classes` (m x m, m in 2, 4, 8, 16, a permutation, reach at most 16), exact per tile with
    no scan.  The nearest search is the palette's 2^24-entry table, shared with pattern() (built at the first call of either
    with the palette; Palette.pattern_prepare() builds it ahead).  strength256 0 .. 256; at most 256 colours; `out` must not be
    the frames themselves."""
    c = _dotdiff_classes(classes)
    if not (isinstance(strength256, (int, np.integer)) and 0 <= strength256 <= 256):
        raise ValueError(f"dot diffusion strength256 must be an integer in 0 .. 256, not {strength256!r}")
    if pal.K > 256:
        raise ValueError(f"dot diffusion supports at most 256 colours, the palette has {pal.K}")
    reach = dotdiff_reach(c)
    if reach > DOTDIFF_MAX_REACH:
        raise ValueError(f"dot diffusion: the class matrix has reach {reach}, at most {DOTDIFF_MAX_REACH} is supported")
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    if n and out.data_ptr() == f.data_ptr():
        raise ValueError("dot diffusion does not work in place: out must not be the frames")
    _check_palette_device(pal, f)
    L = _lib.load()
    with torch.cuda.device(f.device), _Launch(f.device, None):   # (no workspace: the lock of the (device, stream) only)
        check(L.dp_dotdiff_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, _np_ptr(c), int(c.shape[0]), int(strength256),
                              _stream()))
    return out.view(frames.shape)


IDIFF_MAX_TAPS = 12   # DP_IDIFF_MAX_TAPS


def _idiff_taps(taps, divisor, strength256):
    """The argument rules of dp_idiff_u8 (include/ditherpie_hip_idiff.h) as ValueError -> (dx, dy, weight) int32 arrays."""
    try:
        t = [(int(a), int(b), int(c)) for a, b, c in taps]
        exact = all(a == ta and b == tb and c == tc for (a, b, c), (ta, tb, tc) in zip(t, taps))
    except (TypeError, ValueError):
        raise ValueError("integer error diffusion: taps must be (dx, dy, weight) triples of integers") from None
    if not exact:
        raise ValueError("integer error diffusion: taps must be (dx, dy, weight) triples of integers")
    if not 1 <= len(t) <= IDIFF_MAX_TAPS:
        raise ValueError(f"integer error diffusion takes 1 .. {IDIFF_MAX_TAPS} taps, not {len(t)}")
    if not (isinstance(divisor, (int, np.integer)) and 1 <= divisor < 2 ** 31):
        raise ValueError(f"integer error diffusion: the divisor must be an integer >= 1, not {divisor!r}")
    if not (isinstance(strength256, (int, np.integer)) and 0 <= strength256 <= 256):
        raise ValueError(f"integer error diffusion strength256 must be an integer in 0 .. 256, not {strength256!r}")
    for dx, dy, wt in t:
        if not (0 <= dy <= 2 and -2 <= dx <= 2 and (dy > 0 or dx >= 1)):
            raise ValueError(f"integer error diffusion: tap (dx={dx}, dy={dy}) is outside dy 0 .. 2, dx -2 .. 2, dy == 0 with dx >= 1")
        if wt < 0:
            raise ValueError(f"integer error diffusion: tap (dx={dx}, dy={dy}) has the negative weight {wt}")
    if len({(dx, dy) for dx, dy, _ in t}) != len(t):
        raise ValueError("integer error diffusion: a (dx, dy) is given twice")
    if sum(wt for _, _, wt in t) > divisor:
        raise ValueError(f"integer error diffusion: the weights sum to more than the divisor {divisor}")
    return tuple(np.array([x[i] for x in t], np.int32) for i in range(3))


def idiff(frames, pal: Palette, taps, divisor, strength256, out=None):
    """Integer error diffusion (include/ditherpie_hip_idiff.h) of uint8 frames already in HBM -> uint8 frames: the raster scan
    with the taps [(dx, dy, weight)] over `divisor` in sixteenths, the nearest colour from the palette's 2^24-entry table
    (shared with pattern() and dotdiff(); Palette.pattern_prepare() builds it ahead) -- under the palette's metric.
    strength256 0 .. 256; at most 256 colours; `out` must not be the frames."""
    dx, dy, wt = _idiff_taps(taps, divisor, strength256)
    if pal.K > 256:
        raise ValueError(f"integer error diffusion supports at most 256 colours, the palette has {pal.K}")
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    if n and out.data_ptr() == f.data_ptr():
        raise ValueError("integer error diffusion does not work in place: out must not be the frames")
    _check_palette_device(pal, f)
    L = _lib.load()
    ws_bytes = L.dp_idiff_workspace_bytes(n, h, w)
    with torch.cuda.device(f.device), _Launch(f.device, ws_bytes) as ws:
        check(L.dp_idiff_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, _np_ptr(dx), _np_ptr(dy), _np_ptr(wt), len(dx), int(divisor),
                            int(strength256), ws.data_ptr(), ws.numel(), _stream()))
    return out.view(frames.shape)


VOID_CLUSTER_SIZES = (8, 128)       # h and w of a void-and-cluster matrix (include/ditherpie_hip_voidcluster.h), inclusive
VOID_CLUSTER_SIGMA256 = (256, 768)   # its sigma in 1/256, inclusive


def _void_cluster_args(h, w, sigma):
    """-> (h, w, sigma256) as ints; ValueError outside the ranges of the header."""
    lo, hi = VOID_CLUSTER_SIZES
    for v in (h, w):
        if not (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= v <= hi):
            raise ValueError(f"void-and-cluster: h and w must be integers in {lo} .. {hi}, not {h!r} x {w!r}")
    try:
        s256 = int(round(float(sigma) * 256))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"void-and-cluster: sigma must be a number, not {sigma!r}") from None
    if not VOID_CLUSTER_SIGMA256[0] <= s256 <= VOID_CLUSTER_SIGMA256[1]:
        raise ValueError(f"void-and-cluster: sigma must lie in {VOID_CLUSTER_SIGMA256[0] / 256} .. {VOID_CLUSTER_SIGMA256[1] / 256}, "
                         f"not {sigma!r}")
    return int(h), int(w), s256


def _void_cluster_seeds(seeds):
    try:
        a = np.atleast_1d(np.asarray(seeds))
    except Exception:
        raise ValueError("void-and-cluster: seeds must be integers") from None
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"void-and-cluster: seeds must be an integer or a list of integers, not {seeds!r}")
    return np.ascontiguousarray(a.astype(np.int64) & 0xFFFFFFFF, np.uint32)


def void_cluster_ranks(h, w, seeds, sigma=1.5, device=None, out=None):
    """Void-and-cluster rank matrices (dp_void_cluster_u16; include/ditherpie_hip_voidcluster.h) generated on the device, one
    per seed: an int16 tensor [n, h, w], each matrix a permutation of 0 .. h*w-1 (at most 16383).  Launches only, so a call
    may be captured into a graph; `out`, a contiguous int16 tensor [n, h, w] on the device, is filled instead of a new one."""
    h, w, s256 = _void_cluster_args(h, w, sigma)
    sd = _void_cluster_seeds(seeds)
    require_gpu()
    if out is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        out = torch.empty((len(sd), h, w), dtype=torch.int16, device=dev)
    else:
        if not (out.is_cuda and out.dtype == torch.int16 and tuple(out.shape) == (len(sd), h, w) and out.is_contiguous()):
            raise ValueError(f"void-and-cluster: out must be a contiguous int16 tensor {(len(sd), h, w)} on the device")
        dev = out.device
    with torch.cuda.device(dev), _Launch(dev, None):
        check(_lib.load().dp_void_cluster_u16(out.data_ptr(), len(sd), _np_ptr(sd), h, w, s256, _stream()))
    return out


def void_cluster_ranks_host(h, w, seed, sigma=1.5):
    """The same matrix by the library's host statement (dp_void_cluster_host): uint16 [h, w].  No device is needed."""
    h, w, s256 = _void_cluster_args(h, w, sigma)
    sd = _void_cluster_seeds(seed)
    if len(sd) != 1:
        raise ValueError("void-and-cluster: the host entry point takes one seed")
    out = np.empty((h, w), np.uint16)
    check(_lib.load().dp_void_cluster_host(_np_ptr(out), h, w, int(sd[0]), s256))
    return out


def void_cluster_thresholds(ranks):
    """Step 6 of the header: float32 thresholds of a rank matrix, the centres of min(n, 4096) equal bins of (0, 1)."""
    r = np.asarray(ranks).astype(np.int64)
    n = r.size
    L = min(n, 4096)
    return ((2 * (r * L // n) + 1).astype(np.float64) / (2 * L)).astype(np.float32)


CELL_SIZES = (4, 8, 16)     # cells of dp_cells_u8 are cw x ch pixels, each of these
CELL_MATRICES = (2, 4, 8)   # the Bayer matrix of its perturbation
CELL_MAX_COLOURS = 16       # the palette of a cell-palette dither
CELL_MAX_CHOSEN = 4         # colours a cell chooses besides the fixed ones
CELL_MAX_GROUPS = 4


def _cell_masks(K, colours, fixed_mask, groups):
    """The arguments of the candidate enumeration, checked -> (fixed_mask, the groups as a uint16 array); ValueError."""
    if not (isinstance(K, (int, np.integer)) and 1 <= K <= CELL_MAX_COLOURS):
        raise ValueError(f"cell-palette dithering supports 1 .. {CELL_MAX_COLOURS} colours, the palette has {K!r}")
    if not (isinstance(colours, (int, np.integer)) and 1 <= colours <= CELL_MAX_CHOSEN):
        raise ValueError(f"cell-palette colours per cell must be an integer in 1 .. {CELL_MAX_CHOSEN}, not {colours!r}")
    if not (isinstance(fixed_mask, (int, np.integer)) and 0 <= fixed_mask < 1 << K):
        raise ValueError(f"cell-palette fixed_mask must name palette entries below {K}, not {fixed_mask!r}")
    if groups is None:
        groups = [(1 << K) - 1]
    try:
        groups = [g for g in groups]
    except TypeError:
        raise ValueError(f"cell-palette groups must be 1 .. {CELL_MAX_GROUPS} masks, not {groups!r}") from None
    if not 1 <= len(groups) <= CELL_MAX_GROUPS:
        raise ValueError(f"cell-palette groups must be 1 .. {CELL_MAX_GROUPS} masks, not {len(groups)}")
    for g in groups:
        if not (isinstance(g, (int, np.integer)) and 0 < g < 1 << K):
            raise ValueError(f"a cell-palette group must be a non-empty mask of palette entries below {K}, not {g!r}")
        if bin(int(g) & ~int(fixed_mask)).count("1") < colours:
            raise ValueError(f"cell-palette group {int(g):#x} has fewer than {colours} entries outside the fixed ones")
    return int(fixed_mask), np.array([int(g) for g in groups], np.uint16)


def cell_candidates(K, colours, fixed_mask=0, groups=None):
    """The number of colour sets dp_cells_u8 tries per cell (dp_cells_candidates; include/ditherpie_hip_cells.h has the
    enumeration): groups=None is one group of all K entries.  Host code: no device is needed."""
    fixed_mask, g = _cell_masks(K, colours, fixed_mask, groups)
    n = int(_lib.load().dp_cells_candidates(int(K), int(colours), fixed_mask, _np_ptr(g), len(g)))
    if n < 0:
        raise ValueError("cell-palette dithering: the library refused the groups")
    return n


def cells(frames, pal: Palette, cell, colours, matrix, spread, fixed_mask=0, groups=None, out=None, sets=None):
    """Cell-palette dithering (include/ditherpie_hip_cells.h) of uint8 frames already in HBM -> uint8 frames: the frame is cut
    into cells of cell = (cw, ch) pixels (each 4, 8 or 16), every cell shows `colours` (1 .. 4) palette entries of its choice,
    all from one of the `groups` (masks; None: one group of all entries), besides the entries of fixed_mask; every allowed set
    is tried on the pixels perturbed by the Bayer matrix (2, 4, 8) times spread (0 .. 255).  At most 16 colours.  `out` may be
    the frames.  sets: True or a uint16 tensor [N, ceil(H/ch), ceil(W/cw)] -> returns (out, sets), the mask each cell took."""
    try:
        cw, ch = cell
    except (TypeError, ValueError):
        raise ValueError(f"cell must be a pair (width, height) of {CELL_SIZES}, not {cell!r}") from None
    if cw not in CELL_SIZES or ch not in CELL_SIZES:
        raise ValueError(f"cell must be a pair (width, height) of {CELL_SIZES}, not {cell!r}")
    if matrix not in CELL_MATRICES:
        raise ValueError(f"cell-palette matrix must be one of {CELL_MATRICES}, not {matrix!r}")
    if not (isinstance(spread, (int, np.integer)) and 0 <= spread <= 255):
        raise ValueError(f"cell-palette spread must be an integer in 0 .. 255, not {spread!r}")
    fixed_mask, g = _cell_masks(pal.K, colours, fixed_mask, groups)
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    shape = (n, -(-h // ch), -(-w // cw))
    want_sets = sets is not None and sets is not False
    if sets is True:
        sets = torch.empty(shape, dtype=torch.uint16, device=f.device)
    elif want_sets:
        if not (isinstance(sets, torch.Tensor) and sets.is_cuda and sets.dtype == torch.uint16 and sets.device == f.device):
            raise TypeError("sets must be True or a CUDA uint16 tensor on the frames' device")
        if sets.numel() != shape[0] * shape[1] * shape[2] or not sets.is_contiguous():
            raise ValueError(f"sets must be contiguous with {shape[0]} x {shape[1]} x {shape[2]} elements")
    L = _lib.load()
    with torch.cuda.device(f.device), _Launch(f.device, None):   # (no workspace: the lock of the (device, stream) only)
        check(L.dp_cells_u8(f.data_ptr(), out.data_ptr(), sets.data_ptr() if want_sets else None, n, h, w, pal._h, int(cw), int(ch),
                            int(colours), fixed_mask, _np_ptr(g), len(g), int(matrix), int(spread), _stream()))
    out = out.view(frames.shape)
    if not want_sets:
        return out
    return out, sets.view(shape if frames.dim() == 4 else shape[1:])


class HalftoneParams(C.Structure):
    """struct dp_halftone_params (include/ditherpie_hip.h)."""
    _fields_ = [("cell_size", C.c_double), ("cos_a", C.c_double), ("sin_a", C.c_double), ("exponent", C.c_double),
                ("min_dot", C.c_double), ("max_dot", C.c_double), ("sharpness", C.c_double), ("exp_class", C.c_int32),
                ("shape", C.c_int32), ("paper_idx", C.c_int32), ("reserved", C.c_int32), ("fix_idx_dev", C.c_void_p),
                ("fix_thr_dev", C.c_void_p), ("n_fix", C.c_int64)]


HT_EXP_IDENTITY, HT_EXP_SQRT, HT_EXP_SQUARE, HT_EXP_POW = 0, 1, 2, 3
HT_SHAPES = {"circle": 0, "square": 1, "diamond": 2}   # any other name is a circle, as in the reference


def halftone_params(pal_f32, cell_size=8, angle=45.0, dot_gain=1.0, min_dot_size=0.0, max_dot_size=1.0, shape="circle",
                    sharpness=1.5):
    """The host half of HalftoneDitherStrategy (dithering_lib.py:1598-1693), done once per call in numpy as the reference
    does it: cos / sin of np.radians(angle), the exponent 1 / dot_gain and the path numpy's `**` takes for it, the paper
    entry (first argmax of the float32 brightness of pal_f32).  ValueError where the reference would crash or compute NaN:
    cell_size <= 0 or not finite, dot_gain <= 0 or not finite."""
    cs, dg = float(cell_size), float(dot_gain)
    if not (np.isfinite(cs) and cs > 0):
        raise ValueError(f"halftone cell_size must be a finite number > 0, not {cell_size!r}")
    if not (np.isfinite(dg) and dg > 0):
        raise ValueError(f"halftone dot_gain must be a finite number > 0, not {dot_gain!r}")
    a = np.radians(angle)
    e = 1.0 / dot_gain
    cls = {1.0: HT_EXP_IDENTITY, 0.5: HT_EXP_SQRT, 2.0: HT_EXP_SQUARE}.get(e, HT_EXP_POW)
    pal = np.asarray(pal_f32, np.float32).reshape(-1, 3)
    paper = int(np.argmax(0.299 * pal[:, 0] + 0.587 * pal[:, 1] + 0.114 * pal[:, 2]))
    return HalftoneParams(cs, float(np.cos(a)), float(np.sin(a)), float(e), float(min_dot_size), float(max_dot_size),
                          float(sharpness), cls, HT_SHAPES.get(shape, 0), paper, 0, None, None, 0)


def halftone_thresholds_at(idx, w, P: HalftoneParams):
    """float32 screen thresholds of pixels idx = y * w + x, by the reference's numpy expressions (dithering_lib.py:1661-1693)
    applied to those pixels only: np.power for the pixels dp_halftone_pow_flags lists."""
    idx = np.asarray(idx, np.int64)
    y, x = idx // w, idx % w
    cs = P.cell_size
    xr = x * P.cos_a - y * P.sin_a
    yr = x * P.sin_a + y * P.cos_a
    dx = (xr % cs) / cs - 0.5
    dy = (yr % cs) / cs - 0.5
    if P.shape == 1:
        dist, max_dist = np.maximum(np.abs(dx), np.abs(dy)), 0.5
    elif P.shape == 2:
        dist, max_dist = np.abs(dx) + np.abs(dy), 1.0
    else:
        dist, max_dist = np.sqrt(dx ** 2 + dy ** 2), 0.5
    t = np.power(np.clip(dist / max_dist, 0.0, 1.0), P.exponent)
    t = P.min_dot + t * (P.max_dot - P.min_dot)
    if P.sharpness != 1.0:
        t = 0.5 + (t - 0.5) * P.sharpness
    return np.clip(t, 0.0, 1.0).astype(np.float32)


_HT_FIXUPS = OrderedDict()   # (device, h, w, geometry) -> (sorted int32 pixel indices, float32 thresholds) on the device
_HT_FIXUPS_CAP = 32
_ht_guard = threading.Lock()


def halftone_fixups(device, h, w, P: HalftoneParams):
    """The pow class's fix-up list for an h x w frame (cached per geometry): the pixels dp_halftone_pow_flags lists, sorted,
    with thresholds from halftone_thresholds_at.  One host round trip the first time a geometry is seen."""
    key = (device.index, h, w, P.cell_size, P.cos_a, P.sin_a, P.exponent, P.min_dot, P.max_dot, P.sharpness, P.shape)
    with _ht_guard:
        hit = _HT_FIXUPS.get(key)
        if hit is not None:
            _HT_FIXUPS.move_to_end(key)
            return hit
    L = _lib.load()
    count = torch.zeros(1, dtype=torch.int64, device=device)
    cap = 1 << 16
    while True:
        idx = torch.empty(cap, dtype=torch.int32, device=device)
        check(L.dp_halftone_pow_flags(h, w, C.byref(P), idx.data_ptr(), cap, count.data_ptr(), _stream()))
        n = int(count.item())
        if n <= cap:
            break
        cap = n
    ids = np.sort(idx[:n].cpu().numpy())
    thr = halftone_thresholds_at(ids, w, P)
    hit = (torch.from_numpy(ids).to(device), torch.from_numpy(thr).to(device))
    torch.cuda.current_stream(device).synchronize()   # the list is complete before any stream of any thread can be handed it
    with _ht_guard:
        _HT_FIXUPS[key] = hit
        while len(_HT_FIXUPS) > _HT_FIXUPS_CAP:
            _HT_FIXUPS.popitem(last=False)
    return hit


def halftone(frames, pal: Palette, params, out=None):
    """Halftone dithering (HalftoneDitherStrategy.dither, dithering_lib.py:1498-1695) of uint8 frames in HBM; params: the
    reference's parameter dict (cell_size, angle, dot_gain, min_dot_size, max_dot_size, shape, sharpness; missing ones take
    the reference's defaults).  Frames are independent; no tiles."""
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    P = halftone_params(pal.pal_f32, **params)
    if n == 0 or h == 0 or w == 0:
        return out.view(frames.shape)
    L = _lib.load()
    with torch.cuda.device(f.device):
        keep = None
        if P.exp_class == HT_EXP_POW:
            keep = halftone_fixups(f.device, h, w, P)
            if keep[0].numel():
                # the cache may drop the list (another thread, 32 newer geometries) while this launch is in flight: the
                # allocator must not hand its memory out again before the launching stream is past it
                stream = torch.cuda.current_stream(f.device)
                keep[0].record_stream(stream)
                keep[1].record_stream(stream)
                P.fix_idx_dev, P.fix_thr_dev, P.n_fix = keep[0].data_ptr(), keep[1].data_ptr(), keep[0].numel()
        ws_bytes = L.dp_halftone_workspace_bytes(n, h, w, C.byref(P))
        with _Launch(f.device, max(ws_bytes, 1)) as ws:   # (0: a refused geometry; the call below says why)
            check(L.dp_halftone_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, C.byref(P), ws.data_ptr(), ws.numel(),
                                   _stream()))
    return out.view(frames.shape)


class WaveletParams(C.Structure):
    """struct dp_wavelet_params (include/ditherpie_hip.h)."""
    _fields_ = [("wavelet", C.c_int32), ("subband_quant", C.c_int32), ("uniforms_dev", C.c_void_p),
                ("n_uniforms", C.c_int64)]


WAVELETS = ("haar", "db1", "db2", "db4", "sym2", "sym4", "coif1", "bior1.3", "bior2.2")   # DP_WL_* order


def wavelet_check(wavelet="haar", subband_quant=8, seed=42):
    """(wavelet id, Q, seed) of WaveletDitherStrategy's parameters; ValueError for a wavelet outside the nine, a Q that is
    not an int in [1, 2^31 - 1], a seed outside [0, 2^32) (numpy's RandomState refuses those too)."""
    if wavelet not in WAVELETS:
        raise ValueError(f"wavelet must be one of {', '.join(WAVELETS)}, not {wavelet!r}")
    if isinstance(subband_quant, bool) or not isinstance(subband_quant, (int, np.integer)) or \
            not 1 <= int(subband_quant) <= 0x7fffffff:
        raise ValueError(f"subband_quant must be an int in [1, 2^31 - 1], not {subband_quant!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 32:
        raise ValueError(f"wavelet seed must be an int in [0, 2^32), not {seed!r}")
    return WAVELETS.index(wavelet), int(subband_quant), int(seed)


_WL_STREAMS = OrderedDict()   # (device, seed, n) -> float64 uniforms on the device
_WL_STREAMS_BYTES = 1 << 30   # the cache keeps at most this many bytes of streams (and always the newest one)
_wl_guard = threading.Lock()


def wavelet_stream(device, seed, n):
    """RandomState(seed).random_sample(n) on `device` (float64), cached per (device, seed, n): generated with numpy on the
    host -- its legacy MT19937 is the definition -- and uploaded the first time a geometry is seen."""
    key = (device.index, int(seed), int(n))
    with _wl_guard:
        hit = _WL_STREAMS.get(key)
        if hit is not None:
            _WL_STREAMS.move_to_end(key)
            return hit
    u = np.random.RandomState(seed).random_sample(n)
    hit = torch.from_numpy(u).to(device)
    torch.cuda.current_stream(device).synchronize()   # complete before any stream of any thread can be handed it
    with _wl_guard:
        _WL_STREAMS[key] = hit
        total = sum(t.numel() * 8 for t in _WL_STREAMS.values())
        while len(_WL_STREAMS) > 1 and total > _WL_STREAMS_BYTES:
            _, old = _WL_STREAMS.popitem(last=False)
            total -= old.numel() * 8
    return hit


def wavelet(frames, pal: Palette, params, out=None):
    """Wavelet dithering (WaveletDitherStrategy.dither, dithering_lib.py:846-941) of uint8 frames in HBM; params: the
    reference's parameter dict (wavelet, subband_quant, seed; missing ones take the reference's defaults).  Every frame
    uses the same random stream, as the reference's fresh RandomState(seed) per call does.  Frames are independent; no
    tiles."""
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    wid, q, seed = wavelet_check(**params)
    if n == 0 or h == 0 or w == 0:
        return out.view(frames.shape)
    L = _lib.load()
    with torch.cuda.device(f.device):
        need = L.dp_wavelet_uniforms_needed(h, w, wid)
        if need < 0:
            raise ValueError(f"wavelet: refused geometry {h} x {w}")
        u = wavelet_stream(f.device, seed, need)
        # the cache may drop the stream (another thread, newer geometries) while this launch is in flight: the allocator
        # must not hand its memory out again before the launching stream is past it
        u.record_stream(torch.cuda.current_stream(f.device))
        P = WaveletParams(wid, q, u.data_ptr(), u.numel())
        ws_bytes = L.dp_wavelet_workspace_bytes(n, h, w, C.byref(P))
        with _Launch(f.device, max(ws_bytes, 1)) as ws:   # (0: a refused geometry; the call below says why)
            check(L.dp_wavelet_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, C.byref(P), ws.data_ptr(), ws.numel(),
                                  _stream()))
    return out.view(frames.shape)


DIFFUSER_PERCEPTUAL, DIFFUSER_HYBRID, DIFFUSER_ADAPTIVE_VARIANCE, DIFFUSER_OSTROMOUKHOV = 1, 2, 3, 4


def variance_gate(frames, pal: Palette, var_threshold=300.0, window_radius=1):
    """uint8 gate map [N,H,W] of AdaptiveVarianceDitherStrategy (local variance >= threshold)."""
    f = _frames(frames)
    n, h, w, _ = f.shape
    gate = torch.empty((n, h, w), dtype=torch.uint8, device=f.device)
    _check_palette_device(pal, f)
    L = _lib.load()
    ws_bytes = L.dp_variance_gate_workspace_bytes(n, h, w)
    with torch.cuda.device(f.device), _Launch(f.device, ws_bytes) as ws:
        check(L.dp_variance_gate_u8(f.data_ptr(), gate.data_ptr(), n, h, w, pal._h, float(var_threshold),
                                    int(window_radius), ws.data_ptr(), ws.numel(), _stream()))
    return gate


def variable_diffusion(frames, pal: Palette, model, p0=0.0, p1=0.0, serpentine=False, gate=None, coef=None, out=None):
    """Perceptual / hybrid / adaptive-variance / Ostromoukhov diffusion of uint8 frames in HBM."""
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = _check_out(out, f)
    _check_palette_device(pal, f)
    L = _lib.load()
    ws_bytes = L.dp_error_diffusion_workspace_bytes(n, h, w)
    if gate is not None and n * h * w >= (1 << 20):
        # adaptive variance: gated-off (flat) regions query the palette with the pixels themselves; exact ties at integer
        # points are then resolved from the accelerator's tie codes instead of a traversal replay per pixel
        pal.build_accel()
    with torch.cuda.device(f.device), _Launch(f.device, ws_bytes) as ws:
        check(L.dp_variable_diffusion_u8(f.data_ptr(), out.data_ptr(), n, h, w, pal._h, int(model), float(p0), float(p1),
                                         1 if serpentine else 0, gate.data_ptr() if gate is not None else None,
                                         coef.data_ptr() if coef is not None else None, ws.data_ptr(), ws.numel(),
                                         _stream()))
    return out.view(frames.shape)


def ign_thresholds(h, w, scale=1.0, seed=0, y0=0, x0=0, device="cuda"):
    require_gpu()
    out = torch.empty((h, w), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        check(_lib.load().dp_ign_thresholds(out.data_ptr(), h, w, y0, x0, float(scale), int(seed), _stream()))
    return out


def kmeans_step(px, centers, mean=None):
    """px: CUDA uint8 [...,3]; centers: CUDA float64 [K,3]; mean: CUDA float64 [3] or None (sklearn's tie rule, see
    include/ditherpie_hip.h) -> (sums [K,3], counts [K], sumsq [K]) int64"""
    if not (px.is_cuda and px.dtype == torch.uint8 and px.shape[-1] == 3):
        raise TypeError("px must be a CUDA uint8 tensor [...,3]")
    px = px.contiguous()
    centers = centers.to(device=px.device, dtype=torch.float64).contiguous()
    K = centers.shape[0]
    sums = torch.empty((K, 3), dtype=torch.int64, device=px.device)
    counts = torch.empty((K,), dtype=torch.int64, device=px.device)
    sumsq = torch.empty((K,), dtype=torch.int64, device=px.device)
    with torch.cuda.device(px.device):
        if mean is not None:
            mean = mean.to(device=px.device, dtype=torch.float64).contiguous()
        check(_lib.load().dp_kmeans_step_u8(px.data_ptr(), px.numel() // 3, centers.data_ptr(),
                                            mean.data_ptr() if mean is not None else None, K, sums.data_ptr(),
                                            counts.data_ptr(), sumsq.data_ptr(), _stream()))
    return sums, counts, sumsq


def kmeans_step_into(px, centers, totals, want_sq=True, mean=None):
    """One Lloyd pass written into the planar totals buffer `totals` (int64 [5K]: sums [K,3] | counts [K] | squared
    norms [K]); with want_sq=False the last part is left alone.  No allocation, nothing read back.  mean: float64 [3]
    tensor on the device (already contiguous) or None."""
    K = centers.shape[0]
    base = totals.data_ptr()
    with torch.cuda.device(px.device):
        check(_lib.load().dp_kmeans_step_u8(px.data_ptr(), px.numel() // 3, centers.data_ptr(),
                                            mean.data_ptr() if mean is not None else None, K, base, base + 8 * 3 * K,
                                            (base + 8 * 4 * K) if want_sq else None, _stream()))


def distinct_first(px):
    """The distinct colours of the uint8 RGB pixels `px` (CUDA tensor [...,3]) in order of first occurrence
    (dp_distinct_first_u8) -> uint8 tensor [n_distinct, 3] on the device.  One host synchronisation (the count)."""
    if not (px.is_cuda and px.dtype == torch.uint8 and px.shape[-1] == 3):
        raise TypeError("px must be a CUDA uint8 tensor [...,3]")
    px = px.contiguous()
    n = px.numel() // 3
    out = torch.empty((n, 3), dtype=torch.uint8, device=px.device)
    nd = torch.zeros(1, dtype=torch.int64, device=px.device)
    L = _lib.load()
    with torch.cuda.device(px.device):
        with _Launch(px.device, L.dp_distinct_first_workspace_bytes(n)) as ws:
            check(L.dp_distinct_first_u8(px.data_ptr(), n, out.data_ptr(), nd.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
            k = int(nd.item())   # (synchronises: the workspace may be handed to the next call after this)
    return out[:k]


class DistinctStream:
    """The distinct colours of a STREAM of pixel buffers in order of first occurrence (dp_distinct_stream_*,
    include/ditherpie_hip_clip.h): after any sequence of add() calls, colours() equals distinct_first() of the
    concatenated buffers, however the stream was cut.  Resident state: a bitmap of one bit per colour (2 MiB), the list
    (48 MiB: every colour there is) and its length.  Calls into one object are ordered on one stream: add(), colours() and
    reset() run on the caller's current stream, and a caller that changes streams orders them itself."""

    LIST_BYTES = 3 << 24

    def __init__(self, device=None):
        require_gpu()
        dev = torch.device(device or "cuda")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        L = _lib.load()
        self.state = torch.empty(L.dp_distinct_stream_state_bytes(), dtype=torch.uint8, device=dev)
        self.list = torch.empty(self.LIST_BYTES, dtype=torch.uint8, device=dev)
        self.count = torch.empty(1, dtype=torch.int64, device=dev)
        self.reset()

    @property
    def device(self):
        return self.state.device

    def reset(self):
        with torch.cuda.device(self.device):
            check(_lib.load().dp_distinct_stream_reset(self.state.data_ptr(), self.count.data_ptr(), _stream()))
        return self

    def add(self, px):
        if not (isinstance(px, torch.Tensor) and px.is_cuda and px.dtype == torch.uint8 and px.shape[-1] == 3):
            raise TypeError("px must be a CUDA uint8 tensor [...,3]")
        if px.device != self.device:
            raise ValueError(f"the stream's state lives on {self.device}, pixels on {px.device}")
        px = px.contiguous()
        n = px.numel() // 3
        if n == 0:
            return self
        L = _lib.load()
        with torch.cuda.device(px.device), _Launch(px.device, L.dp_distinct_stream_workspace_bytes(n)) as ws:
            check(L.dp_distinct_stream_add_u8(px.data_ptr(), n, self.state.data_ptr(), self.list.data_ptr(), self.count.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream()))
        return self

    def __len__(self):
        return int(self.count.item())

    def colours(self):
        """-> uint8 tensor [n_distinct, 3] on the device (a view of the list: add() appends behind it, reset() reuses it).
        One host synchronisation (the count)."""
        return self.list[:3 * len(self)].view(-1, 3)


SCENE_BINS = 4096   # dp_frame_signatures_u8: the 16^3 cells of the colour cube
SCENE_MAX_FRAMES = 65535   # ... frames per call


def _signatures_into(f, sig):
    n, h, w = f.shape[0], f.shape[1], f.shape[2]
    L = _lib.load()
    for a in range(0, n, SCENE_MAX_FRAMES):
        b = min(n, a + SCENE_MAX_FRAMES)
        check(L.dp_frame_signatures_u8(f[a:b].data_ptr(), b - a, h, w, sig[a:b].data_ptr(), _stream()))


def frame_signatures(frames):
    """The coarse colour signature of every frame (dp_frame_signatures_u8, include/ditherpie_hip_scene.h): uint8 CUDA tensor
    [N,H,W,3] (or [H,W,3]) -> torch.int32 tensor [N,4096] on the device, row f the number of pixels of frame f in each 16^3
    cell bin = (r>>4)<<8 | (g>>4)<<4 | (b>>4).  The library's counts are uint32; torch has no such type, so the tensor holds
    their bit patterns as int32: equal to the counts for every frame of fewer than 2^31 pixels (a larger one can read
    negative in a bin that holds 2^31 pixels or more; .to(torch.int64) & 0xFFFFFFFF widens it).  Asynchronous on the
    current stream."""
    f = _frames(frames)
    if f.shape[1] < 1 or f.shape[2] < 1:
        raise ValueError("frames must have at least one pixel")
    sig = torch.empty((f.shape[0], SCENE_BINS), dtype=torch.int32, device=f.device)
    if f.shape[0]:
        with torch.cuda.device(f.device):
            _signatures_into(f, sig)
    return sig


class SceneStream:
    """The distance of every frame of a STREAM of frame batches to the frame before it (dp_frame_signatures_u8 +
    dp_signature_distances): add(frames) -> int64 tensor [N] on the device, distances[i] = sum over the 4096 cells of
    |signature[i] - signature[i-1]|, in 0 ... 2 H W.  The last signature is carried across calls (resident, 16 KB), so the
    distances do not depend on how the stream was cut into batches; the very first frame, and the first after reset(), has
    distance 0.  Calls into one object are ordered on one stream (the caller's current one)."""

    def __init__(self, device=None):
        require_gpu()
        dev = torch.device(device or "cuda")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.prev = torch.zeros(SCENE_BINS, dtype=torch.int32, device=dev)
        self._has_prev = False
        self._n_px = None

    def reset(self):
        """Forget the carried signature (and the geometry it belongs to): the next frame's distance is 0."""
        self._has_prev = False
        self._n_px = None
        return self

    def add(self, frames):
        f = _frames(frames)
        if f.device != self.device:
            raise ValueError(f"the scene stream lives on {self.device}, frames on {f.device}")
        n, n_px = f.shape[0], f.shape[1] * f.shape[2]
        if n_px < 1:
            raise ValueError("frames must have at least one pixel")
        if self._has_prev and n_px != self._n_px:
            raise ValueError(f"frames of {n_px} pixels follow frames of {self._n_px}: signatures of different sizes do not "
                             "compare; call reset() first")
        dist = torch.empty(n, dtype=torch.int64, device=self.device)
        if n == 0:
            return dist
        L = _lib.load()
        with torch.cuda.device(self.device):
            sig = torch.empty((n, SCENE_BINS), dtype=torch.int32, device=self.device)
            _signatures_into(f, sig)
            check(L.dp_signature_distances(sig.data_ptr(), n, self.prev.data_ptr(), 1 if self._has_prev else 0, dist.data_ptr(), _stream()))
        self._has_prev, self._n_px = True, n_px
        return dist


KMEANS_HIST_MAX_K = 256   # dp_kmeans_hist_step: one thread per centre in the list build
HIST_SAMPLE_MAX_RANKS = 16384   # dp_hist_sample_u8 (the sample limit of dp_kmeans_plusplus_u8)


class ColourHistogram:
    """count[colour] of uint8 RGB pixels over all 2^24 colours, resident in HBM (dp_kmeans_hist_*): the pixels of a k-means
    fit are read once into it, every Lloyd pass then runs over the histogram (same labels, same int64 totals)."""

    def __init__(self, px=None, device=None):
        require_gpu()
        dev = px.device if px is not None else torch.device(device or "cuda")
        self.buf = torch.empty(_lib.load().dp_kmeans_hist_bytes(), dtype=torch.uint8, device=dev)
        self.n = 0
        if px is not None:
            self.add(px, accumulate=False)

    def add(self, px, accumulate=True):
        if not (px.is_cuda and px.dtype == torch.uint8 and px.shape[-1] == 3):
            raise TypeError("px must be a CUDA uint8 tensor [...,3]")
        if px.device != self.buf.device:
            raise ValueError(f"histogram lives on {self.buf.device}, pixels on {px.device}")
        px = px.contiguous()
        n = px.numel() // 3
        if (self.n if accumulate else 0) + n >= 1 << 32:
            raise ValueError("a colour histogram holds fewer than 2^32 pixels")
        L = _lib.load()
        with torch.cuda.device(px.device), _Launch(px.device, L.dp_kmeans_hist_workspace_bytes(n)) as ws:
            check(L.dp_kmeans_hist_build_u8(px.data_ptr(), n, self.buf.data_ptr(), 1 if accumulate else 0, ws.data_ptr(), ws.numel(),
                                            _stream()))
        self.n = (self.n if accumulate else 0) + n
        return self

    def overflowed(self) -> bool:
        """True when an accumulating build carried a cell's 32-bit pixel count past 2^32 (the device-side check of
        dp_kmeans_hist_build_u8; add() refuses such totals up front, a direct caller of the C ABI must look)."""
        word = self.buf[(1 << 26) + 4 * 8193:(1 << 26) + 4 * 8194].view(torch.int32)
        return bool(int(word.item()) != 0)

    def sample(self, ranks):
        """The colours of the pixels with the zero-based `ranks` (int64, at most HIST_SAMPLE_MAX_RANKS of them; numpy array,
        sequence or tensor) when the histogram's pixels are laid out in its own slot order, every colour repeated count
        times (dp_hist_sample_u8) -> uint8 tensor [len(ranks), 3] on the device.  A sample of the colour multiset: it does
        not depend on the order the pixels were added in.  ValueError when a rank is < 0 or >= the number of pixels (the
        device counts them: one host synchronisation)."""
        dev = self.buf.device
        if isinstance(ranks, torch.Tensor):
            r = ranks.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        else:
            r = torch.from_numpy(np.ascontiguousarray(np.asarray(ranks, dtype=np.int64).reshape(-1))).to(dev)
        n = r.numel()
        if n > HIST_SAMPLE_MAX_RANKS:
            raise ValueError(f"at most {HIST_SAMPLE_MAX_RANKS} ranks per call, not {n}")
        out = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        if n == 0:
            return out
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        L = _lib.load()
        with torch.cuda.device(dev), _Launch(dev, L.dp_hist_sample_workspace_bytes()) as ws:
            check(L.dp_hist_sample_u8(self.buf.data_ptr(), r.data_ptr(), n, out.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream()))
            n_bad = int(bad.item())
        if n_bad:
            raise ValueError(f"{n_bad} of {n} ranks lie outside [0, {self.n}): the histogram holds {self.n} pixels")
        return out

    def step_into(self, centers, totals, want_sq=True, mean=None):
        """One Lloyd pass over the histogram into the planar totals buffer (see kmeans_step_into)."""
        K = centers.shape[0]
        base = totals.data_ptr()
        with torch.cuda.device(self.buf.device):
            check(_lib.load().dp_kmeans_hist_step(self.buf.data_ptr(), centers.data_ptr(), mean.data_ptr() if mean is not None else None,
                                                  K, base, base + 8 * 3 * K, (base + 8 * 4 * K) if want_sq else None, _stream()))

    def iterate(self, centers, totals, prev, status, ticket, tol, max_iter, first, mean=None):
        """One whole Lloyd iteration in one launch (dp_kmeans_hist_iterate: pass + centre update, single device).  `totals`
        (int64 [5K]) and `ticket` (int32 [1]) zero before the first iteration."""
        with torch.cuda.device(self.buf.device):
            check(_lib.load().dp_kmeans_hist_iterate(self.buf.data_ptr(), centers.data_ptr(), mean.data_ptr() if mean is not None else None,
                                                     centers.shape[0], totals.data_ptr(), prev.data_ptr(), status.data_ptr(),
                                                     ticket.data_ptr(), float(tol), int(max_iter), 1 if first else 0, _stream()))

    def step(self, centers, mean=None):
        """-> (sums [K,3], counts [K], sumsq [K]) int64, as kmeans_step"""
        centers = centers.to(device=self.buf.device, dtype=torch.float64).contiguous()
        K = centers.shape[0]
        totals = torch.empty(5 * K, dtype=torch.int64, device=self.buf.device)
        if mean is not None:
            mean = mean.to(device=self.buf.device, dtype=torch.float64).contiguous()
        self.step_into(centers, totals, True, mean)
        return totals[:3 * K].view(K, 3), totals[3 * K:4 * K], totals[4 * K:]

    def _okfit_scan(self, points, capacity):
        dev = self.buf.device
        n = torch.zeros(1, dtype=torch.int64, device=dev)
        L = _lib.load()
        with torch.cuda.device(dev), _Launch(dev, L.dp_okfit_hist_workspace_bytes()) as ws:
            if points is None:
                check(L.dp_okfit_hist_count(self.buf.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
            else:
                check(L.dp_okfit_hist_points(self.buf.data_ptr(), points.data_ptr() if capacity else None, capacity, n.data_ptr(), ws.data_ptr(),
                                             ws.numel(), _stream()))
            return int(n.item())

    def n_occupied(self) -> int:
        """The number of colours with a count above zero (dp_okfit_hist_count; one host synchronisation)."""
        if self.n == 0:
            return 0
        return self._okfit_scan(None, 0)

    def points(self, capacity=None):
        """The occupied colours as the point records of the Oklab fit, in ascending order of r << 16 | g << 8 | b
        (dp_okfit_hist_points) -> uint8 tensor [n, OKFIT_POINT_BYTES] on the device; okfit_points_numpy() reads one.  With a
        `capacity` only that many records are made room for: -> (tensor [min(n, capacity), 16], n), n the true number."""
        dev = self.buf.device
        if capacity is None:
            n = self.n_occupied()
            out = torch.empty((n, OKFIT_POINT_BYTES), dtype=torch.uint8, device=dev)
            if n:
                assert self._okfit_scan(out, n) == n
            return out
        capacity = int(capacity)
        if not 0 <= capacity <= OKFIT_MAX_POINTS:
            raise ValueError(f"capacity must be in [0, {OKFIT_MAX_POINTS}]")
        out = torch.empty((capacity, OKFIT_POINT_BYTES), dtype=torch.uint8, device=dev)
        n = self._okfit_scan(out, capacity) if self.n else 0
        return out[:min(n, capacity)], n


OKFIT_MAX_COLORS = _lib.OKFIT_MAX_COLORS     # DP_OKFIT_MAX_COLORS (include/ditherpie_hip_okfit.h)
OKFIT_MAX_ITER = _lib.OKFIT_MAX_ITER
OKFIT_MAX_POINTS = _lib.OKFIT_MAX_POINTS
OKFIT_POINT_BYTES = _lib.OKFIT_POINT_BYTES
OKFIT_POINT_DTYPE = np.dtype([("code", "<u4"), ("count", "<u4"), ("lab", "<i2", (3,)), ("zero", "<i2")])


def _okfit_args(K, max_iter):
    K, max_iter = int(K), int(max_iter)
    if K < 1:
        raise ValueError("num_colors must be >= 1")
    if K > OKFIT_MAX_COLORS:
        raise ValueError(f"an Oklab palette fit has at most {OKFIT_MAX_COLORS} colours, not {K}")
    if not 1 <= max_iter <= OKFIT_MAX_ITER:
        raise ValueError(f"max_iter must be in [1, {OKFIT_MAX_ITER}], not {max_iter}")
    return K, max_iter


def _okfit_arrays(codes, counts):
    codes = np.ascontiguousarray(np.asarray(codes).reshape(-1))
    counts = np.ascontiguousarray(np.asarray(counts).reshape(-1))
    if codes.size != counts.size or codes.size < 1:
        raise ValueError("codes and counts must have the same length, at least 1")
    if codes.size > OKFIT_MAX_POINTS:
        raise ValueError(f"at most {OKFIT_MAX_POINTS} points")
    c64, n64 = codes.astype(np.int64), counts.astype(np.int64)
    if c64.min() < 0 or c64.max() >= 1 << 24 or np.any(np.diff(c64) <= 0):
        raise ValueError("codes must be strictly ascending and below 2^24")
    if n64.min() < 1 or int(n64.sum()) >= 1 << 32:
        raise ValueError("counts must be >= 1 and their sum below 2^32")
    return c64.astype(np.uint32), n64.astype(np.uint32)


def okfit_points(codes, counts, device=None):
    """Point records from arrays (dp_okfit_points_u32): codes = r << 16 | g << 8 | b strictly ascending, counts >= 1 with a sum
    below 2^32 -> uint8 tensor [n, OKFIT_POINT_BYTES] on the device."""
    codes, counts = _okfit_arrays(codes, counts)
    require_gpu()
    dev = torch.device(device or "cuda")
    c, k = torch.from_numpy(codes.view(np.int32)).to(dev), torch.from_numpy(counts.view(np.int32)).to(dev)
    out = torch.empty((codes.size, OKFIT_POINT_BYTES), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _Launch(dev, None):
        check(_lib.load().dp_okfit_points_u32(c.data_ptr(), k.data_ptr(), codes.size, out.data_ptr(), _stream()))
    return out


def okfit_points_numpy(points):
    """A tensor of point records -> (codes uint32 [n], counts uint32 [n], lab int16 [n, 3])."""
    rec = points.cpu().numpy().reshape(-1).view(OKFIT_POINT_DTYPE)
    return rec["code"].copy(), rec["count"].copy(), rec["lab"].copy()


def okfit(points_or_hist, K, max_iter=100):
    """The Oklab palette fit (dp_okfit_fit) of a ColourHistogram or of a tensor of point records -> (palette uint8 [K, 3],
    centres int32 [K, 3], n_iter, distortion): a weighted k-means in the integer Oklab, all integer, a pure function of the
    colour multiset; every palette entry is a colour of the input.  Synchronises the current stream once per pass."""
    K, max_iter = _okfit_args(K, max_iter)
    pts = points_or_hist.points() if isinstance(points_or_hist, ColourHistogram) else points_or_hist
    if not (isinstance(pts, torch.Tensor) and pts.is_cuda and pts.dtype == torch.uint8 and pts.dim() == 2 and pts.shape[1] == OKFIT_POINT_BYTES):
        raise TypeError(f"points must be a ColourHistogram or a CUDA uint8 tensor [n, {OKFIT_POINT_BYTES}]")
    pts = pts.contiguous()
    n = pts.shape[0]
    if n < 1:
        raise ValueError("the fit needs at least one point")
    dev = pts.device
    pal = torch.empty((K, 3), dtype=torch.uint8, device=dev)
    centres = torch.empty((K, 3), dtype=torch.int32, device=dev)
    dist = torch.empty(1, dtype=torch.int64, device=dev)
    n_iter = C.c_int(0)
    L = _lib.load()
    with torch.cuda.device(dev), _Launch(dev, L.dp_okfit_workspace_bytes(n, K)) as ws:
        check(L.dp_okfit_fit(pts.data_ptr(), n, K, max_iter, pal.data_ptr(), centres.data_ptr(), dist.data_ptr(), C.byref(n_iter),
                             ws.data_ptr(), ws.numel(), _stream()))
    return pal.cpu().numpy(), centres.cpu().numpy(), int(n_iter.value), int(dist.cpu().numpy().view(np.uint64)[0])


def okfit_host(codes, counts, K, max_iter=100):
    """The host statement of the fit (dp_okfit_host; no device) -> (palette, centres, n_iter, distortion) as okfit()."""
    K, max_iter = _okfit_args(K, max_iter)
    codes, counts = _okfit_arrays(codes, counts)
    pal, centres = np.empty((K, 3), np.uint8), np.empty((K, 3), np.int32)
    n_iter, dist = C.c_int(0), C.c_uint64(0)
    check(_lib.load().dp_okfit_host(_np_ptr(codes), _np_ptr(counts), codes.size, K, max_iter, _np_ptr(pal), _np_ptr(centres), C.byref(n_iter),
                                    C.byref(dist)))
    return pal, centres, int(n_iter.value), int(dist.value)


def kmeans_update(totals, centers, prev, status, tol, max_iter):
    """The centre update of one Lloyd iteration on the device (dp_kmeans_update); everything stays in HBM."""
    with torch.cuda.device(centers.device):
        check(_lib.load().dp_kmeans_update(totals.data_ptr(), centers.data_ptr(), prev.data_ptr(), status.data_ptr(),
                                           centers.shape[0], float(tol), int(max_iter), _stream()))


KMEANS_PP_MAX_SAMPLE = 16384  # points dp_kmeans_plusplus_u8 holds in LDS


def kmeans_plusplus(sample, K, first, uniforms):
    """sklearn's k-means++ seeding on the device (dp_kmeans_plusplus_u8): `sample` uint8 [n,3] on the GPU, `first` the
    first centre's index, `uniforms` float64 numpy [(K-1), n_trials] drawn by the caller.  -> (ids int32 [K], centers
    float64 [K,3]) on the device, nothing read back."""
    s = sample.reshape(-1, 3)
    if not s.is_contiguous():
        s = s.contiguous()
    n = s.shape[0]
    u = torch.as_tensor(np.ascontiguousarray(uniforms, dtype=np.float64)).reshape(-1).to(s.device)
    n_trials = int(uniforms.shape[1]) if K > 1 else 1
    if K == 1:
        u = torch.zeros(1, dtype=torch.float64, device=s.device)
    ids = torch.empty(K, dtype=torch.int32, device=s.device)
    centers = torch.empty((K, 3), dtype=torch.float64, device=s.device)
    with torch.cuda.device(s.device):
        check(_lib.load().dp_kmeans_plusplus_u8(s.data_ptr(), n, int(K), int(first), u.data_ptr(), n_trials, ids.data_ptr(),
                                                centers.data_ptr(), _stream()))
    return ids, centers


def resize_nearest(frames, oh, ow):
    f = _frames(frames)
    n, h, w, _ = f.shape
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=f.device)
    with torch.cuda.device(f.device):
        check(_lib.load().dp_resize_nearest_u8(f.data_ptr(), out.data_ptr(), n, h, w, int(oh), int(ow), _stream()))
    return out if frames.dim() == 4 else out[0]


# ------------------------------------------------------------------------------------- filtered resize
# include/ditherpie_hip_resample.h: Pillow's Image.resize, bit for bit, for the filters that average.
RESAMPLE_FILTERS = ("nearest",) + _lib.RESAMPLE_FILTERS   # what resample() takes; "nearest" is resize_nearest()
RESAMPLE_MAX_SIZE = _lib.RESAMPLE_MAX_SIZE                # DP_RESAMPLE_MAX_SIZE


def _resample_filter(name, nearest=True):
    ok = RESAMPLE_FILTERS if nearest else _lib.RESAMPLE_FILTERS
    if not isinstance(name, str) or name not in ok:
        raise ValueError(f"unknown resize filter {name!r}: it must be one of {', '.join(ok)}")
    return name


def _resample_sizes(h, w, oh, ow):
    for v in (h, w, oh, ow):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= RESAMPLE_MAX_SIZE:
            raise ValueError(f"resize: every size must be an integer in 1 .. {RESAMPLE_MAX_SIZE}, not {v!r}")
    if int(h) * int(w) > 1 << 30:
        raise ValueError("resize: h * w must not exceed 2^30")
    return int(h), int(w), int(oh), int(ow)


class ResamplePlan:
    """dp_resample_plan: the coefficient tables of one geometry (h x w -> oh x ow) and one filter, resident on the current
    device.  Making one allocates and copies with a blocking call: not inside a graph capture."""

    def __init__(self, filter, h, w, oh, ow):
        self._h = None
        self.filter = _resample_filter(filter, nearest=False)
        self.h, self.w, self.oh, self.ow = _resample_sizes(h, w, oh, ow)
        require_gpu()
        L = _lib.load()
        self._destroy = L.dp_resample_plan_destroy
        self._lib_path = _lib.LIB_PATH
        self.device = torch.device("cuda", torch.cuda.current_device())
        handle = C.c_void_p()
        check(L.dp_resample_plan_create(_lib.RESAMPLE_FILTERS.index(self.filter), self.h, self.w, self.oh, self.ow, C.byref(handle)))
        self._h = handle

    def workspace_bytes(self, n_frames):
        return int(_lib.load().dp_resample_workspace_bytes(self._h, int(n_frames)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._destroy(h)
            self._h = None


_RESAMPLE_PLANS = OrderedDict()   # (library, device, filter, h, w, oh, ow) -> ResamplePlan
_RESAMPLE_PLANS_CAP = 16
_resample_guard = threading.Lock()


def _resample_plan(device, filter, h, w, oh, ow):
    key = (_lib.LIB_PATH, device.index, filter, h, w, oh, ow)   # (a plan stays with the library that made it)
    with _resample_guard:
        plan = _RESAMPLE_PLANS.get(key)
        if plan is not None:
            _RESAMPLE_PLANS.move_to_end(key)
            return plan
    with torch.cuda.device(device):
        plan = ResamplePlan(filter, h, w, oh, ow)
    with _resample_guard:
        plan = _RESAMPLE_PLANS.setdefault(key, plan)
        while len(_RESAMPLE_PLANS) > _RESAMPLE_PLANS_CAP:
            _RESAMPLE_PLANS.popitem(last=False)
    return plan


def drop_resample_plans():
    with _resample_guard:
        _RESAMPLE_PLANS.clear()


def resample(frames, oh, ow, filter="lanczos", out=None, plan=None):
    """Image.resize((ow, oh), filter) of uint8 RGB frames already in HBM, [N,H,W,3] or [H,W,3], bit-identical to Pillow for
    box, bilinear, hamming, bicubic and lanczos (include/ditherpie_hip_resample.h); "nearest" is resize_nearest(), unchanged.
    The plan of a geometry is made at its first use (a blocking upload: not inside a graph capture; pass `plan` there) and kept
    in a small cache; the intermediate of the two passes is the stream's workspace."""
    _resample_filter(filter)
    f = _frames(frames)
    n, h, w, _ = f.shape
    if filter == "nearest":
        if out is not None or plan is not None:
            raise ValueError("resample: the nearest filter takes neither out nor plan")
        return resize_nearest(frames, oh, ow)
    h, w, oh, ow = _resample_sizes(h, w, oh, ow)
    if plan is None:
        plan = _resample_plan(f.device, filter, h, w, oh, ow)
    elif (plan.filter, plan.h, plan.w, plan.oh, plan.ow, plan.device) != (filter, h, w, oh, ow, f.device):
        raise ValueError("resample: the plan was made for another filter, geometry or device")
    if out is None:
        out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=f.device)
    else:
        out = _check_buffer(out, f.device, (n, oh, ow, 3), torch.uint8, "out")
        if n and out.data_ptr() == f.data_ptr():
            raise ValueError("resample does not work in place: out must not be the frames")
    L = _lib.load()
    ws_bytes = plan.workspace_bytes(n)
    with torch.cuda.device(f.device), _Launch(f.device, ws_bytes if ws_bytes else None) as ws:
        a = _lib.ResampleArgs(C.sizeof(_lib.ResampleArgs), f.data_ptr() or None, out.data_ptr() or None, n, plan._h.value,
                              ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, _stream().value)
        check(L.dp_resample_u8(C.byref(a)))
    return out if frames.dim() == 4 else out[0]


def resample_host(frames, oh, ow, filter="lanczos"):
    """The same resize on the CPU (dp_resample_host: the host statement of the kernels): numpy uint8 [N,H,W,3] or [H,W,3] ->
    numpy.  Needs no device."""
    _resample_filter(filter, nearest=False)
    f = np.ascontiguousarray(frames)
    if f.dtype != np.uint8 or f.ndim not in (3, 4) or f.shape[-1] != 3:
        raise ValueError("frames must be [N,H,W,3] or [H,W,3] uint8")
    x = f[None] if f.ndim == 3 else f
    n, h, w, _ = x.shape
    h, w, oh, ow = _resample_sizes(h, w, oh, ow)
    out = np.empty((n, oh, ow, 3), np.uint8)
    check(_lib.load().dp_resample_host(_lib.RESAMPLE_FILTERS.index(filter), _np_ptr(x), _np_ptr(out), n, h, w, oh, ow))
    return out[0] if f.ndim == 3 else out


# ------------------------------------------------------------------------------------- indexed output
# include/ditherpie_hip_indexed.h.  A dithered frame holds only the K output colours of its palette; an index plane is
# the same image at one (two) byte(s) per pixel.
class IndexMap:
    """dp_index_map: the colour -> index hash table and the index -> colour list of K <= 1024 uint8 RGB colours
    (duplicates allowed: a colour's index is its LOWEST position).  Built on the host; the first launch uploads it to the
    current device, where it then stays."""

    def __init__(self, colors_u8):
        self.colors = np.ascontiguousarray(colors_u8, dtype=np.uint8).reshape(-1, 3)
        self.K = self.colors.shape[0]
        self._h = C.c_void_p()
        L = _lib.load()
        self._destroy = L.dp_index_map_destroy
        check(L.dp_index_map_create(_np_ptr(self.colors), self.K, C.byref(self._h)))
        k, slots, probe = C.c_int(), C.c_int(), C.c_int()
        check(L.dp_index_map_info(self._h, C.byref(k), C.byref(slots), C.byref(probe)))
        self.slots, self.max_probe = slots.value, probe.value
        self.index_bytes = 1 if self.K <= 256 else 2
        self.device = None   # set by the first launch

    def _on(self, device):
        if self.device is None:
            self.device = device
        elif self.device != device:
            raise ValueError(f"index map lives on {self.device}, data on {device}")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._destroy(h)
            self._h = None


_INDEX_DTYPES = {1: torch.uint8, 2: torch.int16}


def _index_bytes(imap, index_bytes):
    nb = imap.index_bytes if index_bytes is None else int(index_bytes)
    if nb not in (1, 2):
        raise ValueError(f"index_bytes must be 1 or 2, not {index_bytes!r}")
    if nb == 1 and imap.K > 256:
        raise ValueError(f"one-byte indices cannot hold {imap.K} colours")
    return nb


def _check_buffer(out, device, shape, dtype, what):
    """As _check_out: a caller-supplied buffer must be exactly what the kernel writes before its pointer reaches one."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dtype):
        raise TypeError(f"{what} must be a CUDA {str(dtype).replace('torch.', '')} tensor")
    if out.device != device:
        raise ValueError(f"{what} is on {out.device}, the input on {device}")
    n = 1
    for s in shape:
        n *= int(s)
    if out.numel() != n or not out.is_contiguous():
        raise ValueError(f"{what} must be contiguous and hold exactly {n} elements")
    return out.view(shape)


def _counted(count, strict, what, fn):
    if not strict:
        return count
    n = int(count.item())
    if n:
        raise DitherPieError(_lib.DP_EINVAL, f"{fn}: {n} {what}")
    return None


def to_indices(frames, imap: IndexMap, index_bytes=None, out=None, strict=True):
    """uint8 CUDA RGB frames [...,3] -> index planes [...]: torch.uint8 for one-byte indices (K <= 256, the default
    there), torch.int16 for two-byte ones (the default above 256, index_bytes=2 at any K; the values are < 1024, so the
    signed type holds them as they are).  A pixel that equals no colour of the map gets index 0 and is counted:
    strict=True reads the count back (one synchronisation) and raises DitherPieError naming it, and returns the planes;
    strict=False returns (planes, count) with count an int64 CUDA tensor of one element, nothing read back."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8):
        raise TypeError("frames must be a CUDA uint8 tensor")
    if frames.dim() < 1 or frames.shape[-1] != 3:
        raise ValueError("frames must be [...,3]")
    nb = _index_bytes(imap, index_bytes)
    f = frames.contiguous()
    planes = _check_buffer(out, f.device, tuple(f.shape[:-1]), _INDEX_DTYPES[nb], "out")
    imap._on(f.device)
    count = torch.zeros(1, dtype=torch.int64, device=f.device)
    with torch.cuda.device(f.device):
        if f.numel():
            check(_lib.load().dp_index_from_rgb_u8(f.data_ptr(), planes.data_ptr(), f.numel() // 3, imap._h, nb,
                                                   count.data_ptr(), _stream()))
    left = _counted(count, strict, "pixel(s) equal no colour of the index map", "to_indices")
    return planes if strict else (planes, left)


def from_indices(planes, imap: IndexMap, out=None, strict=True):
    """Index planes [...] (torch.uint8 or torch.int16, as to_indices returns them) -> uint8 RGB frames [...,3].  An
    index outside [0, K) is written as colour 0 and counted; strict as for to_indices."""
    if not (isinstance(planes, torch.Tensor) and planes.is_cuda and planes.dtype in (torch.uint8, torch.int16)):
        raise TypeError("planes must be a CUDA uint8 or int16 tensor")
    nb = 1 if planes.dtype == torch.uint8 else 2
    _index_bytes(imap, nb)
    p = planes.contiguous()
    rgb = _check_buffer(out, p.device, tuple(p.shape) + (3,), torch.uint8, "out")
    imap._on(p.device)
    count = torch.zeros(1, dtype=torch.int64, device=p.device)
    with torch.cuda.device(p.device):
        if p.numel():
            check(_lib.load().dp_rgb_from_index_u8(p.data_ptr(), rgb.data_ptr(), p.numel(), imap._h, nb, count.data_ptr(),
                                                   _stream()))
    left = _counted(count, strict, "index value(s) outside the index map", "from_indices")
    return rgb if strict else (rgb, left)


def resize_nearest_plane(planes, oh, ow):
    """NEAREST resize of index planes [N,H,W] or [H,W] (uint8 or int16) with Pillow's coordinates, as resize_nearest
    does for RGB frames: decoding the resized plane equals resizing the decoded frames."""
    if not (isinstance(planes, torch.Tensor) and planes.is_cuda and planes.dtype in (torch.uint8, torch.int16)):
        raise TypeError("planes must be a CUDA uint8 or int16 tensor")
    if planes.dim() not in (2, 3):
        raise ValueError("planes must be [N,H,W] or [H,W]")
    p = (planes if planes.dim() == 3 else planes.unsqueeze(0)).contiguous()
    n, h, w = p.shape
    out = torch.empty((n, int(oh), int(ow)), dtype=p.dtype, device=p.device)
    with torch.cuda.device(p.device):
        check(_lib.load().dp_resize_nearest_plane_u8(p.data_ptr(), out.data_ptr(), n, h, w, int(oh), int(ow),
                                                     p.element_size(), _stream()))
    return out if planes.dim() == 3 else out[0]


GIF_MAX_FRAMES = 65535      # dp_index_delta_u8, dp_gif_lzw_encode_u8: frames per call
GIF_CHUNK_PX = 32768        # the default chunk of dp_gif_lzw_encode_u8 (file size against parallelism)


def _planes_u8(planes):
    if not (isinstance(planes, torch.Tensor) and planes.is_cuda and planes.dtype == torch.uint8):
        raise TypeError("planes must be a CUDA uint8 tensor (one-byte indices)")
    if planes.dim() not in (2, 3):
        raise ValueError("planes must be [N,H,W] or [H,W]")
    p = (planes if planes.dim() == 3 else planes.unsqueeze(0)).contiguous()
    if p.shape[1] < 1 or p.shape[2] < 1:
        raise ValueError("planes must have at least one pixel")
    return p


def _check_transparent(transparent):
    t = int(transparent)
    if not 0 <= t <= 255:
        raise ValueError(f"transparent must be in 0 ... 255, not {transparent!r}")
    return t


def _delta_into(p, prev, has_prev, transparent, out, changed):
    n, n_px = p.shape[0], p.shape[1] * p.shape[2]
    L = _lib.load()
    for a in range(0, n, GIF_MAX_FRAMES):
        b = min(n, a + GIF_MAX_FRAMES)
        check(L.dp_index_delta_u8(p[a:b].data_ptr(), b - a, n_px, prev.data_ptr(), 1 if (has_prev or a) else 0, transparent,
                                  out[a:b].data_ptr(), changed[a:b].data_ptr(), _stream()))


def index_delta(planes, prev, transparent, out=None):
    """Inter-frame deltas of one-byte index planes (dp_index_delta_u8, include/ditherpie_hip_gif.h): uint8 CUDA planes [N,H,W]
    -> (out [N,H,W] uint8, changed [N] int64 on the device).  out[f] holds `transparent` where planes[f] equals planes[f-1]
    and planes[f] elsewhere; frame 0 is compared with `prev` ([H,W] uint8 on the same device) or, with prev=None, copied
    through.  changed[f] counts the pixels that differ (H W for a frame 0 without prev).  A given `prev` is UPDATED: after the
    call it holds planes[-1], which is what the next batch of the same stream compares with (DeltaStream does the
    bookkeeping).  `out` must not be the planes themselves.  Asynchronous on the current stream."""
    p = _planes_u8(planes)
    t = _check_transparent(transparent)
    n, h, w = p.shape
    if prev is not None:
        if not (isinstance(prev, torch.Tensor) and prev.is_cuda and prev.dtype == torch.uint8 and prev.is_contiguous()):
            raise TypeError("prev must be a contiguous CUDA uint8 tensor")
        if prev.device != p.device or prev.numel() != h * w:
            raise ValueError(f"prev must hold one plane of {h} x {w} on {p.device}")
    res = _check_buffer(out, p.device, (n, h, w), torch.uint8, "out")
    changed = torch.empty(n, dtype=torch.int64, device=p.device)
    if n:
        with torch.cuda.device(p.device):
            carried = prev if prev is not None else torch.empty(h * w, dtype=torch.uint8, device=p.device)
            _delta_into(p, carried, prev is not None, t, res, changed)
    return res, changed


class DeltaStream:
    """Inter-frame deltas over a STREAM of plane batches: add(planes, transparent) -> (out, changed) as index_delta, with the
    last plane carried across calls (resident, H W bytes), so the result does not depend on how the stream was cut into
    batches; the very first frame, and the first after reset(), goes out whole.  Calls into one object are ordered on one
    stream (the caller's current one)."""

    def __init__(self, device=None):
        require_gpu()
        dev = torch.device(device or "cuda")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.prev = None
        self._has_prev = False

    def reset(self):
        """Forget the carried plane: the next frame goes out whole."""
        self._has_prev = False
        return self

    def add(self, planes, transparent):
        p = _planes_u8(planes)
        if p.device != self.device:
            raise ValueError(f"the delta stream lives on {self.device}, planes on {p.device}")
        t = _check_transparent(transparent)
        n, h, w = p.shape
        if self._has_prev and self.prev.numel() != h * w:
            raise ValueError(f"planes of {h * w} pixels follow planes of {self.prev.numel()}: call reset() first")
        out = torch.empty_like(p)
        changed = torch.empty(n, dtype=torch.int64, device=self.device)
        if n == 0:
            return out, changed
        with torch.cuda.device(self.device):
            if self.prev is None or self.prev.numel() != h * w:
                self.prev = torch.empty(h * w, dtype=torch.uint8, device=self.device)
            _delta_into(p, self.prev, self._has_prev, t, out, changed)
        self._has_prev = True
        return out, changed

    def carry(self, plane):
        """Make `plane` ([H,W] uint8 on the stream's device) the plane the next frame is compared with, without computing a
        delta: for a caller that writes some frames whole."""
        p = _planes_u8(plane)
        if p.device != self.device or p.shape[0] != 1:
            raise ValueError(f"carry takes one plane on {self.device}")
        self.prev = p[0].reshape(-1).clone()
        self._has_prev = True
        return self


# ------------------------------------------------------------------------------------- temporal hold
# include/ditherpie_hip_hold.h.  Cells of a video whose source has not moved keep the indices they show; it sits between the
# dither's index planes and the inter-frame delta above.
HOLD_CELLS = _lib.HOLD_CELLS
HOLD_MAX_FRAMES = _lib.HOLD_MAX_FRAMES


def _hold_settings(cell, tol, share256):
    try:
        c, t, s = int(cell), int(tol), int(share256)
    except (TypeError, ValueError):
        raise ValueError(f"cell, tol and share256 must be integers, not {cell!r}, {tol!r}, {share256!r}") from None
    if c not in HOLD_CELLS or c != cell:
        raise ValueError(f"cell must be one of {HOLD_CELLS}, not {cell!r}")
    if not 0 <= t <= 255 or t != tol:
        raise ValueError(f"tol must be an integer in 0 ... 255, not {tol!r}")
    if not 0 <= s <= 256 or s != share256:
        raise ValueError(f"share256 must be an integer in 0 ... 256, not {share256!r}")
    return c, t, s


def _hold_geometry(n, h, w):
    if h < 1 or w < 1 or h * w >= 1 << 31:
        raise ValueError(f"frames of {h} x {w}: h and w must be >= 1 and h * w below 2^31")


def _hold_inputs(src, planes):
    """-> contiguous src [N,H,W,3] and planes [N,H,W] (uint8 CUDA tensors of one device and one geometry)"""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8):
        raise TypeError("src must be a CUDA uint8 tensor")
    if not (isinstance(planes, torch.Tensor) and planes.is_cuda):
        raise TypeError("planes must be a CUDA tensor")
    if planes.dtype != torch.uint8:
        raise ValueError(f"planes must be one-byte indices (torch.uint8), not {planes.dtype}: the hold takes at most 256 colours")
    if src.dim() != 4 or src.shape[-1] != 3 or planes.dim() != 3 or tuple(planes.shape) != tuple(src.shape[:3]):
        raise ValueError(f"src must be [N,H,W,3] and planes [N,H,W] of the same frames, not {tuple(src.shape)} and {tuple(planes.shape)}")
    if planes.device != src.device:
        raise ValueError(f"src is on {src.device}, planes on {planes.device}")
    return src.contiguous(), planes.contiguous()


def _hold_into(s, p, anchor, held, has_state, cell, tol, share256, out, refreshed):
    n, h, w = p.shape
    L = _lib.load()
    for a in range(0, n, HOLD_MAX_FRAMES):
        b = min(n, a + HOLD_MAX_FRAMES)
        args = _lib.HoldArgs(C.sizeof(_lib.HoldArgs), s[a:b].data_ptr(), p[a:b].data_ptr(), b - a, h, w, cell, tol, share256, anchor.data_ptr(),
                             held.data_ptr(), 1 if (has_state or a) else 0, out[a:b].data_ptr(), refreshed[a:b].data_ptr(), _stream().value)
        check(L.dp_hold_u8(C.byref(args)))


def hold(src, planes, state, cell, tol, share256, out=None):
    """The temporal hold of one batch (dp_hold_u8, include/ditherpie_hip_hold.h): src [N,H,W,3] uint8 CUDA frames as handed to the
    ditherer, planes [N,H,W] uint8 their fresh dither -> (out [N,H,W] uint8, refreshed [N] int64 on the device, state').
    state: None for the first frame of a stream, else the (anchor [H,W,3], held [H,W]) pair an earlier call returned; a given
    pair is UPDATED in place and returned (HoldStream does the bookkeeping).  A cell of cell x cell pixels refreshes -- takes the
    fresh indices -- when at least share256 / 256 of its pixels (and one at least) differ from their anchor by more than tol in
    some channel; every other pixel keeps what it showed.  One kernel launch per 65535 frames, nothing read back; `out` must not
    be the planes.  ValueError for two-byte planes: the hold takes at most 256 colours."""
    cell, tol, share256 = _hold_settings(cell, tol, share256)
    s, p = _hold_inputs(src, planes)
    n, h, w = p.shape
    _hold_geometry(n, h, w)
    dev = p.device
    if state is None:
        anchor = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        held = torch.empty((h, w), dtype=torch.uint8, device=dev)
    else:
        anchor = _check_buffer(state[0], dev, (h, w, 3), torch.uint8, "state anchor")
        held = _check_buffer(state[1], dev, (h, w), torch.uint8, "state held")
    res = _check_buffer(out, dev, (n, h, w), torch.uint8, "out")
    refreshed = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return res, refreshed, state
    if res.data_ptr() == p.data_ptr():
        raise ValueError("hold does not work in place: out must not be the planes")
    with torch.cuda.device(dev):
        _hold_into(s, p, anchor, held, state is not None, cell, tol, share256, res, refreshed)
    return res, refreshed, (anchor, held)


def hold_host(src, planes, state, cell, tol, share256):
    """The same on the CPU (dp_hold_host_u8: the host statement of the kernel): numpy arrays in and out, state None or (anchor,
    held), which is NOT modified -> (out, refreshed, state').  Needs no device."""
    cell, tol, share256 = _hold_settings(cell, tol, share256)
    s, p = np.ascontiguousarray(src), np.ascontiguousarray(planes)
    if s.dtype != np.uint8 or s.ndim != 4 or s.shape[-1] != 3:
        raise ValueError("src must be [N,H,W,3] uint8")
    if p.dtype != np.uint8:
        raise ValueError(f"planes must be one-byte indices (uint8), not {p.dtype}: the hold takes at most 256 colours")
    if p.shape != s.shape[:3]:
        raise ValueError(f"planes must be [N,H,W] of the same frames, not {p.shape} beside {s.shape}")
    n, h, w = p.shape
    _hold_geometry(n, h, w)
    if state is None:
        anchor, held = np.empty((h, w, 3), np.uint8), np.empty((h, w), np.uint8)
    else:
        anchor, held = np.array(state[0], dtype=np.uint8, order="C"), np.array(state[1], dtype=np.uint8, order="C")
        if anchor.shape != (h, w, 3) or held.shape != (h, w):
            raise ValueError(f"the state must be (anchor [{h},{w},3], held [{h},{w}])")
    out, refreshed = np.empty((n, h, w), np.uint8), np.empty(n, np.int64)
    if n == 0:
        return out, refreshed, state
    args = _lib.HoldArgs(C.sizeof(_lib.HoldArgs), s.ctypes.data, p.ctypes.data, n, h, w, cell, tol, share256, anchor.ctypes.data, held.ctypes.data,
                         0 if state is None else 1, out.ctypes.data, refreshed.ctypes.data, None)
    check(_lib.load().dp_hold_host_u8(C.byref(args)))
    return out, refreshed, (anchor, held)


class HoldStream:
    """The temporal hold over a STREAM of batches: add(src, planes) -> (out, refreshed) as hold(), with the anchor and the held
    indices resident between calls (4 H W bytes), so the result does not depend on how the stream was cut into batches; the very
    first frame, and the first after reset(), refreshes everywhere.  cell, tol and share (the fraction of a cell's pixels that must
    have changed, rounded to 256ths) are fixed for the object's life; the defaults (8, 4, 1/16) are untuned design choices
    (DESIGN.md 8).  `palette` is the caller's note of the palette the held indices belong to: process_frames_indexed resets the
    stream when it changes.  Calls into one object are ordered on one stream (the caller's current one)."""

    def __init__(self, device=None, cell=8, tol=4, share=1 / 16):
        require_gpu()
        dev = torch.device(device or "cuda")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.cell, self.tol, self.share256 = _hold_settings(cell, tol, min(256, max(0, int(round(float(share) * 256)))))
        self.anchor = self.held = None
        self._has_state = False
        self.palette = None

    @property
    def settings(self):
        """(cell, tol, share256)"""
        return self.cell, self.tol, self.share256

    def reset(self):
        """Forget the state: the next frame refreshes everywhere."""
        self._has_state = False
        self.palette = None
        return self

    def add(self, src, planes):
        s, p = _hold_inputs(src, planes)
        if p.device != self.device:
            raise ValueError(f"the hold stream lives on {self.device}, planes on {p.device}")
        n, h, w = p.shape
        if n == 0:
            return torch.empty_like(p), torch.empty(0, dtype=torch.int64, device=self.device)
        _hold_geometry(n, h, w)
        if self._has_state and tuple(self.held.shape) != (h, w):
            raise ValueError(f"frames of {h} x {w} follow frames of {self.held.shape[0]} x {self.held.shape[1]}: call reset() first")
        out = torch.empty_like(p)
        refreshed = torch.empty(n, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            if self.held is None or tuple(self.held.shape) != (h, w):
                self.anchor = torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
                self.held = torch.empty((h, w), dtype=torch.uint8, device=self.device)
            _hold_into(s, p, self.anchor, self.held, self._has_state, self.cell, self.tol, self.share256, out, refreshed)
        self._has_state = True
        return out, refreshed


def as_hold_stream(hold, device):
    """The `hold` argument of the video path: None, a HoldStream (of `device`), or the settings (cell, tol, share) of a new one."""
    if hold is None or isinstance(hold, HoldStream):
        if hold is not None and torch.device(device) != hold.device and torch.device(device).index is not None:
            raise ValueError(f"the hold stream lives on {hold.device}, the frames on {device}")
        return hold
    cell, tol, share = check_hold_argument(hold)
    return HoldStream(device, cell, tol, share)


def check_hold_argument(hold):
    """ValueError for a `hold` argument that is neither None, a HoldStream nor usable settings (cell, tol, share); no device
    needed, so the video path calls it before a decoder starts.  -> the argument."""
    if hold is None or isinstance(hold, HoldStream):
        return hold
    try:
        cell, tol, share = hold
        _hold_settings(cell, tol, min(256, max(0, int(round(float(share) * 256)))))
    except TypeError:
        raise ValueError(f"hold must be None, a HoldStream or a tuple (cell, tol, share), not {hold!r}") from None
    return hold


ALPHA_MODES = _lib.ALPHA_MODES
ALPHA_MATRICES = _lib.ALPHA_MATRICES
ALPHA_MAX_FRAMES = _lib.ALPHA_MAX_FRAMES


def _rgb_triple(c, what):
    """A colour as three bytes (a ctypes array for a descriptor); ValueError otherwise."""
    try:
        t = tuple(int(v) for v in c)
        exact = len(t) == 3 and all(a == b for a, b in zip(t, c)) and all(0 <= v <= 255 for v in t)
    except (TypeError, ValueError):
        exact = False
    if not exact:
        raise ValueError(f"{what} must be three integers in 0 .. 255, not {c!r}")
    return _lib._rgb3(*t)


def _alpha_settings(mode, threshold, matrix, matte, y0, x0):
    """The argument rules of dp_alpha_split_u8 as ValueError -> (mode index, threshold, m, has_matte, matte bytes, y0, x0)."""
    if mode not in ALPHA_MODES:
        raise ValueError(f"alpha mode must be one of {ALPHA_MODES}, not {mode!r}")
    if not (isinstance(threshold, (int, np.integer)) and 0 <= threshold <= 256):
        raise ValueError(f"alpha threshold must be an integer in 0 .. 256, not {threshold!r}")
    if matrix not in ALPHA_MATRICES:
        raise ValueError(f"alpha matrix must be one of {ALPHA_MATRICES}, not {matrix!r}")
    for v in (y0, x0):
        if not (isinstance(v, (int, np.integer)) and 0 <= v <= _lib.ALPHA_MAX_ORIGIN):
            raise ValueError(f"y0 and x0 must be integers in 0 .. 2^30, not {y0!r}, {x0!r}")
    m = _rgb_triple((0, 0, 0) if matte is None else matte, "matte")
    return ALPHA_MODES.index(mode), int(threshold), int(matrix), 0 if matte is None else 1, m, int(y0), int(x0)


def _alpha_geometry(h, w):
    if h < 1 or w < 1 or h * w >= 1 << 31:
        raise ValueError(f"frames of {h} x {w}: h and w must be >= 1 and h * w below 2^31")


def _alpha_tensor(t, last, what):
    """-> t as a contiguous [N,H,W(,last)] uint8 CUDA tensor and whether a frame axis was added"""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
        raise TypeError(f"{what} must be a CUDA uint8 tensor")
    dims = 3 if last is None else 4
    single = t.dim() == dims - 1
    if single:
        t = t.unsqueeze(0)
    if t.dim() != dims or (last is not None and t.shape[-1] != last):
        raise ValueError(f"{what} must be [N,H,W{'' if last is None else ',' + str(last)}] (or one frame), not {tuple(t.shape)}")
    return t.contiguous(), single


def alpha_split(rgba, mode="threshold", threshold=128, matrix=4, matte=None, y0=0, x0=0):
    """dp_alpha_split_u8 (include/ditherpie_hip_alpha.h): rgba [N,H,W,4] (or [H,W,4]) uint8 CUDA -> (rgb [..,3], mask [N,H,W] of 0 / 1,
    masked [N] int64 on the device: the transparent pixels per frame).  mode "threshold": transparent where alpha < threshold;
    "ordered": where the m x m Bayer matrix at the global position (y0 + y, x0 + x) says so.  matte: None, or the colour the RGB is
    composited over.  One clearing and one launch per 65535 frames, nothing read back."""
    md, thr, m, has_matte, mt, y0, x0 = _alpha_settings(mode, threshold, matrix, matte, y0, x0)
    f, single = _alpha_tensor(rgba, 4, "rgba")
    n, h, w, _ = f.shape
    _alpha_geometry(h, w)
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=f.device)
    mask = torch.empty((n, h, w), dtype=torch.uint8, device=f.device)
    masked = torch.empty(n, dtype=torch.int64, device=f.device)
    L = _lib.load()
    with torch.cuda.device(f.device), _Launch(f.device, None):
        for a in range(0, n, ALPHA_MAX_FRAMES):
            b = min(n, a + ALPHA_MAX_FRAMES)
            args = _lib.AlphaSplitArgs(C.sizeof(_lib.AlphaSplitArgs), f[a:b].data_ptr(), b - a, h, w, md, thr, m, y0, x0, has_matte, mt,
                                       rgb[a:b].data_ptr(), mask[a:b].data_ptr(), masked[a:b].data_ptr(), _stream().value)
            check(L.dp_alpha_split_u8(C.byref(args)))
    return (rgb[0], mask[0], masked) if single else (rgb, mask, masked)


def alpha_split_host(rgba, mode="threshold", threshold=128, matrix=4, matte=None, y0=0, x0=0):
    """The same on the CPU (dp_alpha_split_host_u8: the host statement of the kernel): numpy in and out.  Needs no device."""
    md, thr, m, has_matte, mt, y0, x0 = _alpha_settings(mode, threshold, matrix, matte, y0, x0)
    f = np.ascontiguousarray(rgba)
    single = f.ndim == 3
    f = f[None] if single else f
    if f.dtype != np.uint8 or f.ndim != 4 or f.shape[-1] != 4:
        raise ValueError("rgba must be [N,H,W,4] (or [H,W,4]) uint8")
    n, h, w, _ = f.shape
    _alpha_geometry(h, w)
    rgb, mask, masked = np.empty((n, h, w, 3), np.uint8), np.empty((n, h, w), np.uint8), np.empty(n, np.int64)
    for a in range(0, n, ALPHA_MAX_FRAMES):
        b = min(n, a + ALPHA_MAX_FRAMES)
        args = _lib.AlphaSplitArgs(C.sizeof(_lib.AlphaSplitArgs), f[a:b].ctypes.data, b - a, h, w, md, thr, m, y0, x0, has_matte, mt,
                                   rgb[a:b].ctypes.data, mask[a:b].ctypes.data, masked[a:b].ctypes.data, None)
        check(_lib.load().dp_alpha_split_host_u8(C.byref(args)))
    return (rgb[0], mask[0], masked) if single else (rgb, mask, masked)


def _alpha_key_value(key):
    if not (isinstance(key, (int, np.integer)) and 0 <= key <= 255):
        raise ValueError(f"the key index must be an integer in 0 .. 255, not {key!r}")
    return int(key)


def alpha_key(planes, mask, key, out=None):
    """dp_alpha_key_u8: planes [N,H,W] (or [H,W]) uint8 index planes, mask of the same shape -> planes with `key` at the masked
    pixels.  out=planes works in place.  ValueError for two-byte planes: the key is one byte."""
    key = _alpha_key_value(key)
    if isinstance(planes, torch.Tensor) and planes.dtype != torch.uint8:
        raise ValueError(f"planes must be one-byte indices (torch.uint8), not {planes.dtype}: the key index is one byte")
    p, single = _alpha_tensor(planes, None, "planes")
    k, _ = _alpha_tensor(mask, None, "mask")
    if k.shape != p.shape or k.device != p.device:
        raise ValueError(f"mask must be of the planes' shape and device, not {tuple(k.shape)} beside {tuple(p.shape)}")
    n, h, w = p.shape
    _alpha_geometry(h, w)
    res = _check_buffer(out, p.device, (n, h, w), torch.uint8, "out")
    L = _lib.load()
    with torch.cuda.device(p.device), _Launch(p.device, None):
        for a in range(0, n, ALPHA_MAX_FRAMES):
            b = min(n, a + ALPHA_MAX_FRAMES)
            args = _lib.AlphaKeyArgs(C.sizeof(_lib.AlphaKeyArgs), p[a:b].data_ptr(), k[a:b].data_ptr(), b - a, h, w, key, res[a:b].data_ptr(),
                                     _stream().value)
            check(L.dp_alpha_key_u8(C.byref(args)))
    return res[0] if single else res


def alpha_key_host(planes, mask, key):
    """The same on the CPU (dp_alpha_key_host_u8): numpy in and out."""
    key = _alpha_key_value(key)
    p, k = np.ascontiguousarray(planes), np.ascontiguousarray(mask)
    if p.dtype != np.uint8 or k.dtype != np.uint8 or p.shape != k.shape or p.ndim not in (2, 3):
        raise ValueError("planes and mask must be uint8 arrays of one shape, [N,H,W] or [H,W]")
    q, kk = (p[None], k[None]) if p.ndim == 2 else (p, k)
    n, h, w = q.shape
    _alpha_geometry(h, w)
    out = np.empty_like(q)
    for a in range(0, n, ALPHA_MAX_FRAMES):
        b = min(n, a + ALPHA_MAX_FRAMES)
        args = _lib.AlphaKeyArgs(C.sizeof(_lib.AlphaKeyArgs), q[a:b].ctypes.data, kk[a:b].ctypes.data, b - a, h, w, key, out[a:b].ctypes.data, None)
        check(_lib.load().dp_alpha_key_host_u8(C.byref(args)))
    return out.reshape(p.shape)


def alpha_join(rgb, mask, fill=(0, 0, 0), out=None):
    """dp_alpha_join_u8: rgb [N,H,W,3] (or [H,W,3]) and mask [N,H,W] -> rgba [N,H,W,4]: (fill, 0) at the masked pixels, (rgb, 255)
    elsewhere."""
    fl = _rgb_triple(fill, "fill")
    f, single = _alpha_tensor(rgb, 3, "rgb")
    k, _ = _alpha_tensor(mask, None, "mask")
    if tuple(k.shape) != tuple(f.shape[:3]) or k.device != f.device:
        raise ValueError(f"mask must be [N,H,W] of the frames and on their device, not {tuple(k.shape)} beside {tuple(f.shape)}")
    n, h, w, _ = f.shape
    _alpha_geometry(h, w)
    res = _check_buffer(out, f.device, (n, h, w, 4), torch.uint8, "out")
    L = _lib.load()
    with torch.cuda.device(f.device), _Launch(f.device, None):
        for a in range(0, n, ALPHA_MAX_FRAMES):
            b = min(n, a + ALPHA_MAX_FRAMES)
            args = _lib.AlphaJoinArgs(C.sizeof(_lib.AlphaJoinArgs), f[a:b].data_ptr(), k[a:b].data_ptr(), b - a, h, w, fl, res[a:b].data_ptr(),
                                      _stream().value)
            check(L.dp_alpha_join_u8(C.byref(args)))
    return res[0] if single else res


def alpha_join_host(rgb, mask, fill=(0, 0, 0)):
    """The same on the CPU (dp_alpha_join_host_u8): numpy in and out."""
    fl = _rgb_triple(fill, "fill")
    f, k = np.ascontiguousarray(rgb), np.ascontiguousarray(mask)
    if f.dtype != np.uint8 or k.dtype != np.uint8 or f.ndim not in (3, 4) or f.shape[-1] != 3 or k.shape != f.shape[:-1]:
        raise ValueError("rgb must be [N,H,W,3] (or [H,W,3]) uint8 and mask [N,H,W] (or [H,W]) uint8 of the same frames")
    q, kk = (f[None], k[None]) if f.ndim == 3 else (f, k)
    n, h, w, _ = q.shape
    _alpha_geometry(h, w)
    out = np.empty((n, h, w, 4), np.uint8)
    for a in range(0, n, ALPHA_MAX_FRAMES):
        b = min(n, a + ALPHA_MAX_FRAMES)
        args = _lib.AlphaJoinArgs(C.sizeof(_lib.AlphaJoinArgs), q[a:b].ctypes.data, kk[a:b].ctypes.data, b - a, h, w, fl, out[a:b].ctypes.data, None)
        check(_lib.load().dp_alpha_join_host_u8(C.byref(args)))
    return out[0] if f.ndim == 3 else out


def _masked_inputs(frames, mask, out, what):
    f = _frames(frames)
    k, _ = _alpha_tensor(mask, None, "mask")
    if tuple(k.shape) != tuple(f.shape[:3]) or k.device != f.device:
        raise ValueError(f"mask must be [N,H,W] of the frames and on their device, not {tuple(k.shape)} beside {tuple(f.shape)}")
    out = _check_out(out, f)
    if f.shape[0] and out.data_ptr() in (f.data_ptr(), k.data_ptr()):
        raise ValueError(f"{what} does not work in place: out must be neither the frames nor the mask")
    return f, k, out


def idiff_masked(frames, mask, pal: Palette, taps, divisor, strength256, fill=(0, 0, 0), out=None):
    """idiff() under a mask (dp_alpha_idiff_u8, include/ditherpie_hip_alpha.h): mask [N,H,W] uint8, non-zero = transparent.  A
    transparent pixel becomes `fill`, receives no error and hands none on; its hidden colour is never looked at.  With an all-zero
    mask the result is idiff()'s."""
    dx, dy, wt = _idiff_taps(taps, divisor, strength256)
    fl = _rgb_triple(fill, "fill")
    if pal.K > 256:
        raise ValueError(f"integer error diffusion supports at most 256 colours, the palette has {pal.K}")
    f, k, out = _masked_inputs(frames, mask, out, "integer error diffusion")
    n, h, w, _ = f.shape
    _check_palette_device(pal, f)
    L = _lib.load()
    ws_bytes = L.dp_idiff_workspace_bytes(n, h, w)
    with torch.cuda.device(f.device), _Launch(f.device, ws_bytes) as ws:
        args = _lib.AlphaIdiffArgs(C.sizeof(_lib.AlphaIdiffArgs), f.data_ptr(), k.data_ptr(), out.data_ptr(), n, h, w, pal._h, dx.ctypes.data,
                                   dy.ctypes.data, wt.ctypes.data, len(dx), int(divisor), int(strength256), fl, ws.data_ptr(), ws.numel(),
                                   _stream().value)
        check(L.dp_alpha_idiff_u8(C.byref(args)))
    return out.view(frames.shape)


def dotdiff_masked(frames, mask, pal: Palette, classes, strength256, fill=(0, 0, 0), out=None):
    """dotdiff() under a mask (dp_alpha_dotdiff_u8): a transparent pixel becomes `fill` and hands on nothing, and an opaque pixel
    shares its error among its OPAQUE neighbours of a higher class.  With an all-zero mask the result is dotdiff()'s."""
    c = _dotdiff_classes(classes)
    fl = _rgb_triple(fill, "fill")
    if not (isinstance(strength256, (int, np.integer)) and 0 <= strength256 <= 256):
        raise ValueError(f"dot diffusion strength256 must be an integer in 0 .. 256, not {strength256!r}")
    if pal.K > 256:
        raise ValueError(f"dot diffusion supports at most 256 colours, the palette has {pal.K}")
    reach = dotdiff_reach(c)
    if reach > DOTDIFF_MAX_REACH:
        raise ValueError(f"dot diffusion: the class matrix has reach {reach}, at most {DOTDIFF_MAX_REACH} is supported")
    f, k, out = _masked_inputs(frames, mask, out, "dot diffusion")
    n, h, w, _ = f.shape
    _check_palette_device(pal, f)
    L = _lib.load()
    with torch.cuda.device(f.device), _Launch(f.device, None):
        args = _lib.AlphaDotdiffArgs(C.sizeof(_lib.AlphaDotdiffArgs), f.data_ptr(), k.data_ptr(), out.data_ptr(), n, h, w, pal._h, c.ctypes.data,
                                     int(c.shape[0]), int(strength256), fl, _stream().value)
        check(L.dp_alpha_dotdiff_u8(C.byref(args)))
    return out.view(frames.shape)


def gif_lzw_stride(h, w, chunk_px=None):
    """The bytes dp_gif_lzw_encode_u8 may write per frame (dp_gif_lzw_bound_bytes): the row length of gif_lzw's payload."""
    return int(_lib.load().dp_gif_lzw_bound_bytes(int(h), int(w), int(chunk_px or GIF_CHUNK_PX)))


def gif_lzw(planes, min_code_size, chunk_px=None):
    """The GIF image data of one-byte index planes (dp_gif_lzw_encode_u8): uint8 CUDA planes [N,H,W] -> (payload [N, stride]
    uint8, sizes [N] int64), both on the device.  payload[f, :sizes[f]] is frame f's min_code_size byte, LZW sub-blocks and
    terminator, to be written verbatim behind an image descriptor; the bytes past sizes[f] are unspecified.  An index
    >= 1 << min_code_size is the caller's error (it is encoded by its low bits).  chunk_px: pixels a wave compresses on its
    own (default GIF_CHUNK_PX).  The device encoder is the only one here: the host statement is gif_lzw_host, by name.
    Asynchronous on the current stream."""
    p = _planes_u8(planes)
    mcs, chunk = int(min_code_size), int(GIF_CHUNK_PX if chunk_px is None else chunk_px)
    if not 2 <= mcs <= 8:
        raise ValueError(f"min_code_size must be in 2 ... 8, not {min_code_size!r}")
    if chunk < 1:
        raise ValueError(f"chunk_px must be >= 1, not {chunk_px!r}")
    n, h, w = p.shape
    L = _lib.load()
    stride = int(L.dp_gif_lzw_bound_bytes(h, w, chunk))
    if stride == 0:
        raise ValueError(f"planes of {h} x {w} are more than the encoder takes (h * w < 2^31)")
    payload = torch.empty((n, stride), dtype=torch.uint8, device=p.device)
    sizes = torch.empty(n, dtype=torch.int64, device=p.device)
    with torch.cuda.device(p.device):
        for a in range(0, n, GIF_MAX_FRAMES):
            b = min(n, a + GIF_MAX_FRAMES)
            need = int(L.dp_gif_lzw_workspace_bytes(b - a, h, w, chunk))
            with _Launch(p.device, need) as ws:
                check(L.dp_gif_lzw_encode_u8(p[a:b].data_ptr(), b - a, h, w, mcs, chunk, payload[a:b].data_ptr(), stride, sizes[a:b].data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream()))
    return payload, sizes


def gif_lzw_host(planes, min_code_size, chunk_px=None):
    """The same bytes from the host statement (dp_gif_lzw_host_u8), no device involved: numpy uint8 planes [N,H,W] ->
    [bytes per frame].  What the device encoder is tested against, and what GifWriter runs on when asked to (encoder="host")."""
    p = np.ascontiguousarray(planes, dtype=np.uint8)
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3 or p.shape[1] < 1 or p.shape[2] < 1:
        raise ValueError("planes must be [N,H,W] or [H,W] with at least one pixel")
    mcs, chunk = int(min_code_size), int(GIF_CHUNK_PX if chunk_px is None else chunk_px)
    n, h, w = p.shape
    if n == 0:
        return []
    L = _lib.load()
    stride = int(L.dp_gif_lzw_bound_bytes(h, w, max(chunk, 1)))
    out = np.empty((n, max(stride, 1)), np.uint8)
    sizes = np.zeros(n, np.int64)
    check(L.dp_gif_lzw_host_u8(_np_ptr(p), n, h, w, mcs, chunk, _np_ptr(out), stride, _np_ptr(sizes)))
    return [out[f, :int(sizes[f])].tobytes() for f in range(n)]


PNG_MAX_FRAMES = 65535      # dp_png_deflate_encode_u8: frames per call
PNG_SEG_BYTES = 8192        # the default segment of dp_png_deflate_encode_u8 (file size against parallelism)
PNG_DEPTHS = (1, 2, 4, 8)
PNG_BLOCKS = ("fixed", "dynamic")   # block types beside stored: "dynamic" adds dynamic-Huffman blocks (ditherpie_hip_png_dyn.h)
PNG_CODE_MAX_COUNT = 1 << 20        # dp_png_code_lengths_*: the largest count of a histogram


def png_depth(k):
    """The smallest PNG bit depth that holds the indices of a k-colour palette."""
    k = int(k)
    if k < 1 or k > 256:
        raise ValueError(f"a PNG palette holds 1 ... 256 colours, not {k}")
    return 1 if k <= 2 else 2 if k <= 4 else 4 if k <= 16 else 8


def _png_args(depth, seg_bytes):
    d, seg = int(depth), int(PNG_SEG_BYTES if seg_bytes is None else seg_bytes)
    if d not in PNG_DEPTHS:
        raise ValueError(f"depth must be one of {PNG_DEPTHS}, not {depth!r}")
    if not 256 <= seg <= 32768:
        raise ValueError(f"seg_bytes must be in 256 ... 32768, not {seg_bytes!r}")
    return d, seg


def _png_blocks(blocks):
    if blocks not in PNG_BLOCKS:
        raise ValueError(f"blocks must be one of {PNG_BLOCKS}, not {blocks!r}")
    return blocks == "dynamic"


def png_deflate_stride(h, w, depth, seg_bytes=None):
    """The bytes dp_png_deflate_encode_u8 may write per frame (dp_png_deflate_bound_bytes): the row length of png_deflate's
    payload."""
    d, seg = _png_args(depth, seg_bytes)
    return int(_lib.load().dp_png_deflate_bound_bytes(int(h), int(w), d, seg))


def png_deflate(planes, depth, seg_bytes=None, blocks="fixed"):
    """The zlib stream (the contents of a PNG's IDAT chunks) of one-byte index planes at bit depth `depth`, filter 0 on every
    row (dp_png_deflate_encode_u8): uint8 CUDA planes [N,H,W] -> (payload [N, stride] uint8, sizes [N] int64), both on the
    device.  payload[f, :sizes[f]] is frame f's stream; the bytes past sizes[f] are unspecified.  An index >= 1 << depth is
    the caller's error (it is encoded by its low bits).  seg_bytes: filtered bytes a wave compresses on its own (default
    PNG_SEG_BYTES).  blocks: "fixed" writes stored and fixed-Huffman blocks, "dynamic" dynamic-Huffman blocks as well
    (dp_png_deflate_dyn_encode_u8: smaller streams, a larger workspace).  The device encoder is the only one here: the host
    statement is png_deflate_host, by name.  Asynchronous on the current stream."""
    dyn = _png_blocks(blocks)
    p = _planes_u8(planes)
    d, seg = _png_args(depth, seg_bytes)
    n, h, w = p.shape
    L = _lib.load()
    ws_bytes, encode = ((L.dp_png_deflate_dyn_workspace_bytes, L.dp_png_deflate_dyn_encode_u8) if dyn else
                        (L.dp_png_deflate_workspace_bytes, L.dp_png_deflate_encode_u8))
    stride = int(L.dp_png_deflate_bound_bytes(h, w, d, seg))
    if stride == 0:
        raise ValueError(f"planes of {h} x {w} are more than the encoder takes (filtered bytes < 2^31)")
    payload = torch.empty((n, stride), dtype=torch.uint8, device=p.device)
    sizes = torch.empty(n, dtype=torch.int64, device=p.device)
    with torch.cuda.device(p.device):
        for a in range(0, n, PNG_MAX_FRAMES):
            b = min(n, a + PNG_MAX_FRAMES)
            need = int(ws_bytes(b - a, h, w, d, seg))
            with _Launch(p.device, need) as ws:
                check(encode(p[a:b].data_ptr(), b - a, h, w, d, seg, payload[a:b].data_ptr(), stride, sizes[a:b].data_ptr(), ws.data_ptr(),
                             ws.numel(), _stream()))
    return payload, sizes


def png_deflate_host(planes, depth, seg_bytes=None, blocks="fixed"):
    """The same bytes from the host statement (dp_png_deflate_host_u8, or dp_png_deflate_dyn_host_u8 for blocks="dynamic"), no
    device involved: numpy uint8 planes [N,H,W] -> [bytes per frame].  What the device encoder is tested against, and what
    png.encode_png runs on when asked to (encoder="host")."""
    dyn = _png_blocks(blocks)
    p = np.ascontiguousarray(planes, dtype=np.uint8)
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3 or p.shape[1] < 1 or p.shape[2] < 1:
        raise ValueError("planes must be [N,H,W] or [H,W] with at least one pixel")
    d, seg = _png_args(depth, seg_bytes)
    n, h, w = p.shape
    if n == 0:
        return []
    L = _lib.load()
    stride = int(L.dp_png_deflate_bound_bytes(h, w, d, seg))
    if stride == 0:
        raise ValueError(f"planes of {h} x {w} are more than the encoder takes (filtered bytes < 2^31)")
    out = np.empty((n, stride), np.uint8)
    sizes = np.zeros(n, np.int64)
    host = L.dp_png_deflate_dyn_host_u8 if dyn else L.dp_png_deflate_host_u8
    check(host(_np_ptr(p), n, h, w, d, seg, _np_ptr(out), stride, _np_ptr(sizes)))
    return [out[f, :int(sizes[f])].tobytes() for f in range(n)]


def _code_length_args(shape, max_len):
    L = int(max_len)
    if len(shape) != 2 or not 2 <= shape[1] <= 286:
        raise ValueError("counts must be [n_alphabets, n_symbols] with 2 ... 286 symbols")
    if not 1 <= L <= 15 or (1 << L) < shape[1]:
        raise ValueError(f"max_len must be in 1 ... 15 with 2^max_len >= {shape[1]} symbols, not {max_len!r}")
    return L


def png_code_lengths(counts, max_len):
    """Length-limited Huffman code lengths as the PNG encoder builds them (dp_png_code_lengths_u8, one wave per histogram):
    CUDA counts [A, M] (or [M]) of integers 0 ... PNG_CODE_MAX_COUNT -> uint8 lengths of the same shape, on the device.  A
    count outside that range is the caller's error.  Asynchronous on the current stream."""
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype.is_floating_point:
        raise ValueError("counts must be a CUDA tensor of integers")
    one = counts.ndim == 1
    c = (counts[None] if one else counts).to(torch.int32).contiguous()
    L = _code_length_args(tuple(c.shape), max_len)
    out = torch.empty(c.shape, dtype=torch.uint8, device=c.device)
    if c.shape[0] == 0:                                                 # (an empty tensor has no address to pass)
        return out
    with torch.cuda.device(c.device):
        check(_lib.load().dp_png_code_lengths_u8(c.data_ptr(), c.shape[0], c.shape[1], L, out.data_ptr(), _stream()))
    return out[0] if one else out


def png_code_lengths_host(counts, max_len):
    """The same from the host statement (dp_png_code_lengths_host): array-like counts [A, M] (or [M]) -> numpy uint8 lengths."""
    c = np.asarray(counts)
    one = c.ndim == 1
    c = c[None] if one else c
    L = _code_length_args(c.shape, max_len)
    if c.size and (c.min() < 0 or c.max() > PNG_CODE_MAX_COUNT):
        raise ValueError(f"counts must be in 0 ... {PNG_CODE_MAX_COUNT}")
    c = np.ascontiguousarray(c, dtype=np.uint32)
    out = np.zeros(c.shape, np.uint8)
    if c.shape[0]:
        check(_lib.load().dp_png_code_lengths_host(_np_ptr(c), c.shape[0], c.shape[1], L, _np_ptr(out)))
    return out[0] if one else out


PNG_CRC_PIECE_BYTES = 64    # DP_PNG_CRC_PIECE_BYTES: what one lane of dp_png_crc32_u8 runs the register over
PNG_CRC_SPAN_BYTES = 16384  # DP_PNG_CRC_SPAN_BYTES: what one workgroup covers in one step (256 pieces)
PNG_FILE_MAX_PRE = 4096     # dp_png_file_assemble_u8: bytes in front of a frame's chunk
PNG_FILE_MAX_POST = 64      # ... and behind it


def _runs_host(data, sizes):
    d = np.ascontiguousarray(data, dtype=np.uint8)
    if d.ndim == 1:
        d = d[None]
    if d.ndim != 2:
        raise ValueError("data must be [R, stride] (or [stride]) bytes")
    z = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64).reshape(-1))
    if z.shape[0] != d.shape[0]:
        raise ValueError(f"{d.shape[0]} runs and {z.shape[0]} sizes")
    return d, z


def png_crc32(data, sizes):
    """CRC-32 (zlib.crc32) of byte runs on the device (dp_png_crc32_u8): contiguous uint8 CUDA data [R, stride] (or [stride], one
    run) and sizes [R] (a CUDA int64 tensor, or host integers) -> uint32 CUDA tensor [R]; run r is data[r, :sizes[r]].  A size
    outside 0 ... stride is the caller's error (it is clamped).  Asynchronous on the current stream."""
    if not (isinstance(data, torch.Tensor) and data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()):
        raise TypeError("data must be a contiguous CUDA uint8 tensor")
    d = data if data.dim() == 2 else data.unsqueeze(0)
    if d.dim() != 2:
        raise ValueError("data must be [R, stride] (or [stride]) bytes")
    r, stride = d.shape
    z = (sizes if isinstance(sizes, torch.Tensor) else torch.as_tensor(np.asarray(sizes, dtype=np.int64).reshape(-1))).to(d.device, torch.int64).contiguous()
    if z.dim() != 1 or z.shape[0] != r:
        raise ValueError(f"{r} runs and {tuple(z.shape)} sizes")
    out = torch.empty(r, dtype=torch.uint32, device=d.device)
    if r == 0:
        return out
    L = _lib.load()
    with torch.cuda.device(d.device):
        for a in range(0, r, PNG_MAX_FRAMES):
            b = min(r, a + PNG_MAX_FRAMES)
            need = int(L.dp_png_crc32_workspace_bytes(b - a, stride))
            with _Launch(d.device, need) as ws:
                check(L.dp_png_crc32_u8(d[a:b].data_ptr(), stride, z[a:b].data_ptr(), b - a, out[a:b].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return out


def png_crc32_host(data, sizes):
    """The same from the host statement (dp_png_crc32_host_u8): array-like bytes [R, stride] (or [stride]) and sizes [R] -> numpy
    uint32 [R]."""
    d, z = _runs_host(data, sizes)
    out = np.zeros(d.shape[0], np.uint32)
    if d.shape[0]:
        keep = d if d.size else np.zeros(1, np.uint8)                   # (an empty array has no address to pass)
        check(_lib.load().dp_png_crc32_host_u8(_np_ptr(keep), d.shape[1], _np_ptr(z), d.shape[0], _np_ptr(out)))
    return out


def png_crc32_combine_host(crc_a, crc_b, len_b):
    """The CRC-32 of A + B from the CRC-32 of A, of B, and the length of B (dp_png_crc32_combine_host)."""
    if int(len_b) < 0:
        raise ValueError("len_b must be >= 0")
    return int(_lib.load().dp_png_crc32_combine_host(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b)))


def _file_args(n, pre, post, n_idat, seq0, seq_step):
    """-> (pre as numpy [rows, pre_bytes] or None, per_frame, post as numpy or None, n_idat, seq0, seq_step)"""
    per_frame = False
    if pre is not None and not isinstance(pre, torch.Tensor):
        pre = np.frombuffer(bytes(pre), np.uint8) if isinstance(pre, (bytes, bytearray, memoryview)) else np.ascontiguousarray(pre, dtype=np.uint8)
    if pre is not None:
        if pre.ndim == 2:
            per_frame = True
            if pre.shape[0] != n:
                raise ValueError(f"{pre.shape[0]} prefixes for {n} frames")
        elif pre.ndim != 1:
            raise ValueError("pre must be bytes, [pre_bytes] or [N, pre_bytes]")
        if pre.shape[-1] > PNG_FILE_MAX_PRE:
            raise ValueError(f"a prefix holds at most {PNG_FILE_MAX_PRE} bytes, not {pre.shape[-1]}")
        if pre.shape[-1] == 0:
            pre, per_frame = None, False
    if post is not None:
        post = np.frombuffer(bytes(post), np.uint8)
        if post.size > PNG_FILE_MAX_POST:
            raise ValueError(f"a suffix holds at most {PNG_FILE_MAX_POST} bytes, not {post.size}")
        if post.size == 0:
            post = None
    n_idat = n if n_idat is None else int(n_idat)
    if not 0 <= n_idat <= n:
        raise ValueError(f"n_idat must be in 0 ... {n}, not {n_idat}")
    s0, st = int(seq0), int(seq_step)
    if not (0 <= s0 < 2 ** 32 and 0 <= st < 2 ** 32):
        raise ValueError("seq0 and seq_step must be in 0 ... 2^32 - 1")
    return pre, per_frame, post, n_idat, s0, st


def png_file_assemble(payload, sizes, pre=None, post=None, n_idat=None, seq0=0, seq_step=2):
    """Finished PNG chunks from the encoder's output, on the device (dp_png_file_assemble_u8): payload [N, stride] uint8 and
    sizes [N] int64 as png_deflate returns them -> (out uint8 [N * bound], offsets int64 [N + 1]), both on the device.  Frame f
    is out[offsets[f]:offsets[f + 1]]: its prefix, ONE chunk -- IDAT for f < n_idat (default: all), else fdAT with the
    sequence number seq0 + (f - n_idat) * seq_step -- with its CRC-32, the suffix; the frames are packed back to back and
    out[offsets[N]:] is unspecified.  pre: bytes or [pre_bytes] (shared by all frames) or [N, pre_bytes] (one per frame), a
    host array or a CUDA tensor, at most PNG_FILE_MAX_PRE bytes; post: bytes, at most PNG_FILE_MAX_POST.  At most
    PNG_MAX_FRAMES frames per call.  Asynchronous on the current stream, like png_deflate: read offsets back, then copy
    out[:offsets[-1]] once."""
    if not (isinstance(payload, torch.Tensor) and payload.is_cuda and payload.dtype == torch.uint8 and payload.dim() == 2 and payload.is_contiguous()):
        raise TypeError("payload must be a contiguous CUDA uint8 tensor [N, stride]")
    if not (isinstance(sizes, torch.Tensor) and sizes.device == payload.device and sizes.dtype == torch.int64 and sizes.dim() == 1
            and sizes.shape[0] == payload.shape[0] and sizes.is_contiguous()):
        raise TypeError("sizes must be a contiguous int64 tensor [N] on the payload's device")
    n, stride = payload.shape
    if n > PNG_MAX_FRAMES:
        raise ValueError(f"at most {PNG_MAX_FRAMES} frames per call, not {n}: cut the batch")
    pre, per_frame, post, n_idat, s0, st = _file_args(n, pre, post, n_idat, seq0, seq_step)
    dev = payload.device
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), offsets
    L = _lib.load()
    pre_bytes, post_bytes = (0 if pre is None else int(pre.shape[-1])), (0 if post is None else int(post.size))
    bound = int(L.dp_png_file_bound_bytes(stride, pre_bytes, post_bytes))
    if bound == 0:
        raise ValueError(f"a stride of {stride} bytes is more than a chunk takes (below 2^31 - 16)")
    with torch.cuda.device(dev):
        pre_t = None if pre is None else (pre if isinstance(pre, torch.Tensor) else torch.from_numpy(pre.copy())).to(dev, torch.uint8).contiguous()
        post_t = None if post is None else torch.from_numpy(post.copy()).to(dev)
        out = torch.empty(n * bound, dtype=torch.uint8, device=dev)
        need = int(L.dp_png_file_workspace_bytes(n, stride))
        with _Launch(dev, need) as ws:
            check(L.dp_png_file_assemble_u8(payload.data_ptr(), stride, sizes.data_ptr(), n, n_idat, s0, st,
                                            None if pre_t is None else pre_t.data_ptr(), pre_bytes if per_frame else 0, pre_bytes,
                                            None if post_t is None else post_t.data_ptr(), post_bytes, out.data_ptr(), out.numel(), offsets.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _stream()))
        for t in (pre_t, post_t):                                       # uploaded here, read by kernels that may not have run yet
            if t is not None:
                t.record_stream(torch.cuda.current_stream(dev))
    return out, offsets


def png_file_assemble_host(streams, pre=None, post=None, n_idat=None, seq0=0, seq_step=2):
    """The same bytes from the host statement (dp_png_file_assemble_host_u8), no device involved: [bytes per frame] (what
    png_deflate_host returns) -> (bytes, [offsets]); frame f is bytes[offsets[f]:offsets[f + 1]]."""
    streams = [bytes(s) for s in streams]
    n = len(streams)
    if n > PNG_MAX_FRAMES:
        raise ValueError(f"at most {PNG_MAX_FRAMES} frames per call, not {n}: cut the batch")
    if isinstance(pre, torch.Tensor):
        pre = pre.detach().cpu().numpy()
    pre, per_frame, post, n_idat, s0, st = _file_args(n, pre, post, n_idat, seq0, seq_step)
    if n == 0:
        return b"", [0]
    stride = max(max(len(s) for s in streams), 1)
    data = np.zeros((n, stride), np.uint8)
    for f, s in enumerate(streams):
        data[f, :len(s)] = np.frombuffer(s, np.uint8)
    sizes = np.array([len(s) for s in streams], np.int64)
    L = _lib.load()
    pre_bytes, post_bytes = (0 if pre is None else int(pre.shape[-1])), (0 if post is None else int(post.size))
    bound = int(L.dp_png_file_bound_bytes(stride, pre_bytes, post_bytes))
    if bound == 0:
        raise ValueError(f"a stream of {stride} bytes is more than a chunk takes (below 2^31 - 16)")
    pre = None if pre is None else np.ascontiguousarray(pre)
    out = np.empty(n * bound, np.uint8)
    offsets = np.zeros(n + 1, np.int64)
    check(L.dp_png_file_assemble_host_u8(_np_ptr(data), stride, _np_ptr(sizes), n, n_idat, s0, st, _np_ptr(pre), pre_bytes if per_frame else 0, pre_bytes,
                                         _np_ptr(post), post_bytes, _np_ptr(out), out.size, _np_ptr(offsets)))
    return out[:int(offsets[-1])].tobytes(), offsets.tolist()


def profile_enable(on=True):
    check(_lib.load().dp_profile_enable(1 if on else 0))


def profile_read():
    """-> (main kernel ms, fix-up ms, launches) accumulated since the last read (HIP events on the
    launch stream)."""
    a, b, n = C.c_double(), C.c_double(), C.c_int64()
    check(_lib.load().dp_profile_read(C.byref(a), C.byref(b), C.byref(n)))
    return a.value, b.value, n.value
