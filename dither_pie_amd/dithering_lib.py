"""Drop-in counterpart of dither_pie's `dithering_lib` for the hot path, on MI355X.

Same public names, constructor arguments, parameter metadata and error behaviour as the reference
module (reference lines cited per item), so `from dither_pie_amd.dithering_lib import ImageDitherer,
DitherMode, ColorReducer` can replace `from dithering_lib import ...` in dither_cli.py /
dither_pie_gui.py / video_processor.py.  Pixel work happens in libditherpie_hip.so on the GPU; this
file is host plumbing only (palette preparation, parameter handling, tensor hand-off).  There is no
CPU fallback: without the shared library or a HIP device the calls raise DitherPieError.

In scope: none, bayer, blue_noise, IGN, error_diffusion, riemersma, polka_dot, perceptual,
hybrid, adaptive_variance, ostromoukhov; k-means / uniform / median-cut palettes.  HalftoneDitherStrategy and
WaveletDitherStrategy run on the GPU as classes (drop-ins for the reference's), not through ImageDitherer.  The other DitherMode members exist for configuration compatibility and raise
NotImplementedError when used.

Extras that the reference does not have (all optional): ImageDitherer.apply_dithering_frames() for
batches of frames already resident in HBM, and tile offsets (y0, x0) for row-band sharding.
"""
from __future__ import annotations

import os

import math
from collections import OrderedDict
from enum import Enum
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _tables

_staging = None  # threading.local(): .bufs = {nbytes: (pinned in, pinned out)}


def _pinned_pair(nbytes: int):
    """Two page-locked uint8 host buffers of `nbytes` for the calling thread (kept: at most 4 sizes per thread)."""
    import threading
    import torch
    global _staging
    if _staging is None:
        _staging = threading.local()
    bufs = getattr(_staging, "bufs", None)
    if bufs is None:
        bufs = _staging.bufs = OrderedDict()
    pair = bufs.get(nbytes)
    if pair is None:
        pair = (torch.empty(nbytes, dtype=torch.uint8, pin_memory=True),
                torch.empty(nbytes, dtype=torch.uint8, pin_memory=True))
        bufs[nbytes] = pair
        while len(bufs) > 4:
            bufs.popitem(last=False)
    else:
        bufs.move_to_end(nbytes)
    return pair

def _pil_rgbx_into(rgb, host_u8, rawmode="RGBX") -> bool:
    """The pixels of a PIL 'RGB' image in Pillow's own four-bytes-per-pixel layout, written into `host_u8` (a uint8 numpy view of
    h * w * 4 bytes) in pieces, with no intermediate bytes object of the whole image: what Image.tobytes("raw", "RGBX") does,
    minus its b"".join and the caller's copy.  False when the (private, long-stable) encoder interface is not there.
    rawmode="RGBA" does the same for an 'RGBA' image (the alpha paths)."""
    try:
        from PIL import Image
        rgb.load()
        enc = Image._getencoder(rgb.mode, "raw", rawmode)
        enc.setimage(rgb.im, (0, 0) + rgb.size)
        pos, total = 0, host_u8.shape[0]
        piece = max(1 << 20, rgb.size[0] * 4)   # (the raw encoder emits whole rows: RawEncode.c)
        while True:
            _, errcode, data = enc.encode(piece)
            n = len(data)
            if pos + n > total:
                return False
            host_u8[pos:pos + n] = np.frombuffer(data, dtype=np.uint8)
            pos += n
            if errcode:
                break
        return errcode > 0 and pos == total
    except Exception:  # noqa: BLE001 - any surprise: the packed path
        return False


__all__ = [
    "DitherMode", "PixelizeMethod", "PaletteSource", "ImageDitherer", "ColorReducer", "DitherUtils",
    "BaseDitherStrategy", "ErrorDiffusionKernel", "NoDitherStrategy", "MatrixDitherStrategy",
    "BayerDitherStrategy", "BlueNoiseDitherStrategy", "InterleavedGradientNoiseDitherStrategy",
    "ErrorDiffusionDitherStrategy", "PolkaDotDitherStrategy", "PerceptualDitherStrategy", "HybridDitherStrategy",
    "AdaptiveVarianceDitherStrategy", "OstromoukhovDitherStrategy", "RiemersmaDitherStrategy", "HalftoneDitherStrategy",
    "WaveletDitherStrategy", "PatternDitherStrategy", "DotDiffusionDitherStrategy", "CellPaletteDitherStrategy",
    "IntegerErrorDiffusionDitherStrategy", "AlphaMode",
    "generate_blue_noise", "generate_void_and_cluster", "VoidAndClusterDitherStrategy",
]


# ------------------------------------------------------------------------------------- enums
class DitherMode(Enum):
    """dithering_lib.py:61-75 (same member names and string values, incl. the upper-case "IGN")."""
    NONE = "none"
    BAYER = "bayer"
    ERROR_DIFFUSION = "error_diffusion"
    RIEMERSMA = "riemersma"
    BLUE_NOISE = "blue_noise"
    INTERLEAVED_GRADIENT_NOISE = "IGN"
    POLKA_DOT = "polka_dot"
    WAVELET = "wavelet"
    ADAPTIVE_VARIANCE = "adaptive_variance"
    PERCEPTUAL = "perceptual"
    HYBRID = "hybrid"
    HALFTONE = "halftone"
    OSTROMOUKHOV = "ostromoukhov"


class PixelizeMethod(Enum):
    """dithering_lib.py:78-82"""
    NONE = "none"
    REGULAR = "regular"
    NEURAL = "neural"


class PaletteSource(Enum):
    """dithering_lib.py:85-91"""
    MEDIAN_CUT = "median_cut"
    KMEANS = "kmeans"
    UNIFORM = "uniform"
    CUSTOM = "custom"
    FROM_FILE = "file"


_OUT_OF_SCOPE = {DitherMode.WAVELET, DitherMode.HALFTONE}
# per-pixel independent given global coordinates: these shard by row bands / tiles (sharding.dither_band); the diffusers do not
ORDERED_MODES = {DitherMode.NONE, DitherMode.BAYER, DitherMode.BLUE_NOISE, DitherMode.INTERLEAVED_GRADIENT_NOISE, DitherMode.POLKA_DOT}


# ------------------------------------------------------------------------------------- tap tables
def _kernel(taps, divisor, description, rows):
    return {"weights": taps, "divisor": divisor, "description": description, "rows": rows}


class ErrorDiffusionKernel:
    """Error-diffusion tap tables: (dx, dy, weight) lists and divisors (dithering_lib.py:96-209)."""

    FLOYD_STEINBERG = _kernel([(1, 0, 7), (-1, 1, 3), (0, 1, 5), (1, 1, 1)], 16,
                              "Classic Floyd-Steinberg (4 neighbors)", 2)
    JJN = _kernel([(1, 0, 7), (2, 0, 5)]
                  + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (3, 5, 7, 5, 3))]
                  + [(dx, 2, wt) for dx, wt in zip(range(-2, 3), (1, 3, 5, 3, 1))], 48,
                  "Jarvis-Judice-Ninke (12 neighbors, smooth gradients)", 3)
    STUCKI = _kernel([(1, 0, 8), (2, 0, 4)]
                     + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (2, 4, 8, 4, 2))]
                     + [(dx, 2, wt) for dx, wt in zip(range(-2, 3), (1, 2, 4, 2, 1))], 42,
                     "Stucki (12 neighbors, photographic quality)", 3)
    BURKES = _kernel([(1, 0, 8), (2, 0, 4)]
                     + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (2, 4, 8, 4, 2))], 32,
                     "Burkes (7 neighbors, fast)", 2)
    ATKINSON = _kernel([(1, 0, 1), (2, 0, 1), (-1, 1, 1), (0, 1, 1), (1, 1, 1), (0, 2, 1)], 8,
                       "Atkinson (6 neighbors, classic Mac look)", 3)
    SIERRA = _kernel([(1, 0, 5), (2, 0, 3)]
                     + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (2, 4, 5, 4, 2))]
                     + [(dx, 2, wt) for dx, wt in zip(range(-1, 2), (2, 3, 2))], 32,
                     "Sierra Full (10 neighbors, high quality)", 3)
    SIERRA_TWO_ROW = _kernel([(1, 0, 4), (2, 0, 3)]
                             + [(dx, 1, wt) for dx, wt in zip(range(-2, 3), (1, 2, 3, 2, 1))], 16,
                             "Sierra Two-Row (8 neighbors, balanced)", 2)
    SIERRA_LITE = _kernel([(1, 0, 2), (-1, 1, 1), (0, 1, 1)], 4, "Sierra Lite (4 neighbors, fastest)", 2)

    _NAMES = ("floyd_steinberg", "jjn", "stucki", "burkes", "atkinson", "sierra", "sierra_two_row",
              "sierra_lite")

    @classmethod
    def get_kernel(cls, name: str) -> Dict[str, Any]:
        """Unknown names fall back to Floyd-Steinberg (dithering_lib.py:203)."""
        if name in cls._NAMES:
            return getattr(cls, name.upper())
        return cls.FLOYD_STEINBERG

    @classmethod
    def list_kernels(cls) -> List[str]:
        return list(cls._NAMES)


# ------------------------------------------------------------------------------------- threshold tables
def _table(den, rows):
    return (np.array(rows, dtype=np.float64) / den).astype(np.float32)


class DitherUtils:
    """Threshold tables (stored as integer numerators over a power of two; the float32 values equal
    dithering_lib.py:1705-1768 bit for bit, including the two non-canonical entries at the end of
    BAYER8x8 row 3) and the gamma helpers (dithering_lib.py:1788-1802)."""

    BAYER2x2 = _table(4, [[1, 3], [4, 2]])
    BAYER4x4 = _table(32, [[1, 17, 5, 21], [25, 9, 29, 13], [7, 23, 3, 19], [31, 15, 27, 11]])
    BAYER8x8 = _table(64, [
        [1, 33, 9, 41, 3, 35, 11, 43], [49, 17, 57, 25, 51, 19, 59, 27],
        [13, 45, 5, 37, 15, 47, 7, 39], [61, 29, 53, 21, 63, 31, 54, 22],
        [4, 36, 12, 44, 2, 34, 10, 42], [52, 20, 60, 28, 50, 18, 58, 26],
        [16, 48, 8, 40, 14, 46, 6, 38], [64, 32, 56, 24, 62, 30, 54, 22]])
    BAYER16x16 = _table(256, [
        [1, 129, 33, 161, 9, 137, 41, 169, 3, 131, 35, 163, 11, 139, 43, 171],
        [193, 65, 225, 97, 201, 73, 233, 105, 195, 67, 227, 99, 203, 75, 235, 107],
        [49, 177, 17, 145, 57, 185, 25, 153, 51, 179, 19, 147, 59, 187, 27, 155],
        [241, 113, 209, 81, 249, 121, 217, 89, 243, 115, 211, 83, 251, 123, 219, 91],
        [13, 141, 45, 173, 5, 133, 37, 165, 15, 143, 47, 175, 7, 135, 39, 167],
        [205, 77, 237, 109, 197, 69, 229, 101, 207, 79, 239, 111, 199, 71, 231, 103],
        [61, 189, 29, 157, 53, 181, 21, 149, 63, 191, 31, 159, 55, 183, 23, 151],
        [253, 125, 221, 93, 245, 117, 213, 85, 255, 127, 223, 95, 247, 119, 215, 87],
        [4, 132, 36, 164, 12, 140, 44, 172, 2, 130, 34, 162, 10, 138, 42, 170],
        [196, 68, 228, 100, 204, 76, 236, 108, 194, 66, 226, 98, 202, 74, 234, 106],
        [52, 180, 20, 148, 60, 188, 28, 156, 50, 178, 18, 146, 58, 186, 26, 154],
        [244, 116, 212, 84, 252, 124, 220, 92, 242, 114, 210, 82, 250, 122, 218, 90],
        [16, 144, 48, 176, 8, 136, 40, 168, 14, 142, 46, 174, 6, 134, 38, 166],
        [208, 80, 240, 112, 200, 72, 232, 104, 206, 78, 238, 110, 198, 70, 230, 102],
        [64, 192, 32, 160, 56, 184, 24, 152, 62, 190, 30, 158, 54, 182, 22, 150],
        [256, 128, 224, 96, 248, 120, 216, 88, 254, 126, 222, 94, 246, 118, 214, 86]])
    PSX4x4 = _table(16, [[1, 9, 3, 11], [13, 5, 15, 7], [3, 11, 1, 9], [15, 7, 13, 5]])

    _BY_SIZE = {"2x2": "BAYER2x2", "4x4": "BAYER4x4", "8x8": "BAYER8x8", "16x16": "BAYER16x16",
                "psx4x4": "PSX4x4", "psx": "PSX4x4"}

    @staticmethod
    def get_threshold_matrix(mode: DitherMode, size: str = "4x4") -> np.ndarray:
        """dithering_lib.py:1770-1786"""
        if mode == DitherMode.NONE:
            return np.ones((1, 1), dtype=np.float32)
        if mode == DitherMode.BAYER:
            return getattr(DitherUtils, DitherUtils._BY_SIZE.get(size, "BAYER4x4"))
        raise ValueError(f"Unsupported matrix mode: {mode}")

    @staticmethod
    def srgb_to_linear(c: np.ndarray) -> np.ndarray:
        """dithering_lib.py:1788-1794"""
        c = np.asarray(c)
        out = np.empty_like(c, dtype=np.float32)
        lo = c <= 0.04045
        out[lo] = c[lo] / 12.92
        out[~lo] = ((c[~lo] + 0.055) / 1.055) ** 2.4
        return out

    @staticmethod
    def linear_to_srgb(c: np.ndarray) -> np.ndarray:
        """dithering_lib.py:1796-1802"""
        c = np.asarray(c)
        out = np.empty_like(c, dtype=np.float32)
        lo = c <= 0.0031308
        out[lo] = c[lo] * 12.92
        out[~lo] = 1.055 * (c[~lo] ** (1.0 / 2.4)) - 0.055
        return out


# ------------------------------------------------------------------------------------- device-object caches
class _LRU(OrderedDict):
    """Small LRU of device objects; get_or_make is atomic (the GUI calls the ditherer from several threads)."""

    def __init__(self, cap):
        super().__init__()
        self.cap = cap
        import threading
        self._lock = threading.RLock()

    def get_or_make(self, key, make):
        with self._lock:
            if key in self:
                self.move_to_end(key)
                return self[key]
            val = make()
            self[key] = val
            while len(self) > self.cap:
                self.popitem(last=False)
            return val


# device handles are process-local and never stored on the (picklable) ditherer objects
_PALETTES = _LRU(32)
_THRESHOLDS = _LRU(32)
_INDEX_MAPS = _LRU(32)


def drop_device_caches():
    """Forget every cached device palette / threshold matrix (they are re-created on demand)."""
    with _PALETTES._lock:
        _PALETTES.clear()
    with _THRESHOLDS._lock:
        _THRESHOLDS.clear()
    with _INDEX_MAPS._lock:
        _INDEX_MAPS.clear()
    OstromoukhovDitherStrategy._coef_cache.clear()


def _device_index():
    import torch
    return torch.cuda.current_device() if torch.cuda.is_available() else -1


METRICS = ("rgb", "oklab")   # ImageDitherer(metric=...): how "nearest" is measured (include/ditherpie_hip_metric.h)
PALETTE_FITS = ("median_cut", "oklab")   # ImageDitherer(palette_fit=...): how palette=None is fitted (include/ditherpie_hip_okfit.h)


def _device_palette(pal_f32, out_colors, lut_in, metric="rgb"):
    from . import backend
    key = (_device_index(), pal_f32.tobytes(), out_colors.tobytes(), None if lut_in is None else lut_in.tobytes(), metric)
    return _PALETTES.get_or_make(key, lambda: backend.Palette(pal_f32, out_colors, lut_in, metric=metric))


def _device_index_map(out_colors):
    """The index map of a palette's output colours (backend.IndexMap), per device and colour list."""
    from . import backend
    key = (_device_index(), out_colors.tobytes())
    return _INDEX_MAPS.get_or_make(key, lambda: backend.IndexMap(out_colors))


def _indexed(frames_rgb, palette, use_gamma, out):
    """Dithered RGB frames in HBM -> (index planes, palette_u8 [K,3]) on the frames' stream: the colours are the
    out_colors prepare_palette yields, which is what every mode writes."""
    from . import backend
    out_colors = prepare_palette(palette, use_gamma)[1]
    planes = backend.to_indices(frames_rgb, _device_index_map(out_colors), out=out)
    return planes, out_colors.copy()


def _device_thresholds_matrix(matrix):
    from . import backend
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    key = (_device_index(), "m", m.shape, m.tobytes())
    return _THRESHOLDS.get_or_make(key, lambda: backend.Thresholds.from_matrix(m))


def _device_thresholds_blue(size, seed):
    from . import backend
    key = (_device_index(), "bn", int(size), int(seed))
    return _THRESHOLDS.get_or_make(key, lambda: backend.Thresholds.blue_noise(size, seed))


def _device_thresholds_vac(h, w, seed, sigma256):
    from . import backend
    key = (_device_index(), "vac", int(h), int(w), int(seed), int(sigma256))
    return _THRESHOLDS.get_or_make(key, lambda: backend.Thresholds.void_cluster(h, w, seed, sigma256 / 256.0))


def prepare_palette(palette, use_gamma):
    """Host-side palette conversion of ImageDitherer.apply_dithering.

    -> (pal_f32 [K,3]: what the nearest-colour search sees (dithering_lib.py:1970-1974),
        out_colors [K,3] uint8: the bytes a chosen entry becomes (:1984-1990),
        lut_in: uint8[256] applied to the image first (:1957-1959), or None)"""
    pal = np.array(palette, dtype=np.float32).reshape(-1, 3)
    if not use_gamma:
        return np.ascontiguousarray(pal), np.ascontiguousarray(pal.astype(np.uint8)), None
    ints = pal.astype(np.int64)
    if np.array_equal(ints.astype(np.float32), pal) and ints.min() >= 0 and ints.max() <= 255:
        pal_lin = _tables.PAL_LIN[ints]
    else:  # values outside the uint8 grid: evaluate the reference's formula directly
        pal_lin = np.clip(DitherUtils.srgb_to_linear(pal / 255.0) * 255.0, 0, 255).astype(np.float32)
    out_colors = _tables.LUT_OUT[pal_lin.astype(np.uint8)]
    return np.ascontiguousarray(pal_lin, dtype=np.float32), np.ascontiguousarray(out_colors), _tables.LUT_IN


def _index_palette(palette_arr):
    """A device palette whose output bytes encode the chosen index (for the strategy-level API)."""
    pal = np.ascontiguousarray(palette_arr, dtype=np.float32).reshape(-1, 3)
    K = pal.shape[0]
    idx = np.arange(K)
    enc = np.stack([idx & 255, idx >> 8, np.zeros_like(idx)], axis=1).astype(np.uint8)
    return _device_palette(pal, enc, None)


def _pixels_to_frame(pixels, image_size):
    import torch
    h, w = image_size
    px = np.asarray(pixels)
    if px.shape != (h * w, 3):
        raise ValueError(f"pixels must have shape ({h * w}, 3)")
    u8 = px.astype(np.uint8)
    if not np.array_equal(u8.astype(px.dtype), px):
        raise ValueError("the MI355X backend dithers uint8 images: pixel values must be integers in [0, 255]")
    return torch.from_numpy(np.ascontiguousarray(u8.reshape(h, w, 3))).cuda()


def _decode(out_frame, palette_arr):
    o = out_frame.cpu().numpy().reshape(-1, 3)
    idx = o[:, 0].astype(np.int64) | (o[:, 1].astype(np.int64) << 8)
    return np.asarray(palette_arr)[idx, :]


# ------------------------------------------------------------------------------------- strategies
class BaseDitherStrategy:
    """dithering_lib.py:313-330: dither(pixels [N,3] f32, palette_arr [K,3] f32, (h, w)) -> [N,3].  This strategy-level
    call is the reference's and always searches in RGB; a colour metric is a property of ImageDitherer (metric="oklab")."""

    def dither(self, pixels: np.ndarray, palette_arr: np.ndarray, image_size: Tuple[int, int]) -> np.ndarray:
        raise NotImplementedError

    @staticmethod
    def get_parameter_info() -> Optional[Dict[str, Any]]:
        return None

    def get_current_parameters(self) -> Dict[str, Any]:
        return {}

    # device-level entry used by ImageDitherer: uint8 frames in HBM -> uint8 frames in HBM
    def _run(self, frames, pal, y0=0, x0=0, out=None):
        raise NotImplementedError


class NoDitherStrategy(BaseDitherStrategy):
    """Nearest palette colour (dithering_lib.py:333-341)."""

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        return backend.ordered(frames, pal, backend.MODE_NEAREST, y0=y0, x0=x0, out=out)

    def dither(self, pixels, palette_arr, image_size):
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)


class MatrixDitherStrategy(BaseDitherStrategy):
    """Threshold-matrix dithering between the two nearest colours (dithering_lib.py:346-378)."""

    def __init__(self, threshold_matrix: np.ndarray):
        self.threshold_matrix = threshold_matrix

    def _thresholds(self):
        return _device_thresholds_matrix(self.threshold_matrix)

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        return backend.ordered(frames, pal, backend.MODE_MATRIX, thr=self._thresholds(), y0=y0, x0=x0, out=out)

    def dither(self, pixels, palette_arr, image_size):
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)


def generate_blue_noise(size: int = 64, seed: int = 42) -> np.ndarray:
    """Void-filling blue-noise matrix (dithering_lib.py:381-399), generated on the GPU."""
    return _device_thresholds_blue(size, seed).numpy()


class BayerDitherStrategy(MatrixDitherStrategy):
    """dithering_lib.py:402-448"""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "size": {
                "type": "choice",
                "default": "4x4",
                "choices": ["2x2", "4x4", "8x8", "16x16", "psx4x4"],
                "label": "Matrix",
                "description": "Bayer matrix size or PSX 4x4 variant (larger = finer patterns)",
            }
        }

    def __init__(self, size: str = "4x4"):
        self.size = size
        super().__init__(DitherUtils.get_threshold_matrix(DitherMode.BAYER, size))

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"size": self.size}


class BlueNoiseDitherStrategy(MatrixDitherStrategy):
    """dithering_lib.py:451-499 (the matrix is generated and cached on the device per (size, seed))."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "size": {
                "type": "int", "default": 64, "min": 32, "max": 128, "label": "Matrix Size",
                "description": "Size of the blue noise matrix (larger = more detail but slower)",
            },
            "seed": {
                "type": "int", "default": 42, "min": 0, "max": 9999, "label": "Random Seed",
                "description": "Seed for noise generation (different seeds = different patterns)",
            },
        }

    def __init__(self, size: int = 64, seed: int = 42):
        self.size = size
        self.seed = seed
        self._matrix = None

    @property
    def threshold_matrix(self):
        if self._matrix is None:
            self._matrix = generate_blue_noise(self.size, self.seed)
        return self._matrix

    def _thresholds(self):
        return _device_thresholds_blue(self.size, self.seed)

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"size": self.size, "seed": self.seed}

    def __getstate__(self):
        return {"size": self.size, "seed": self.seed, "_matrix": None}


def _vac_settings(size, seed, sigma):
    """(size, seed, sigma) as given to generate_void_and_cluster -> (h, w, seed, sigma256); ValueError outside the ranges."""
    from . import backend
    hw = (size, size) if isinstance(size, (int, np.integer)) else tuple(size) if isinstance(size, (tuple, list)) else None
    if hw is None or len(hw) != 2:
        raise ValueError(f"void-and-cluster: size must be an integer or (h, w), not {size!r}")
    if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool):
        raise ValueError(f"void-and-cluster: seed must be an integer, not {seed!r}")
    h, w, s256 = backend._void_cluster_args(hw[0], hw[1], sigma)
    return h, w, int(seed) & 0xFFFFFFFF, s256


def generate_void_and_cluster(size=64, seed: int = 42, sigma: float = 1.5) -> np.ndarray:
    """A void-and-cluster threshold matrix (Ulichney 1993 on a torus; include/ditherpie_hip_voidcluster.h), float32 [h, w]:
    blue noise at every grey level, and it tiles.  size is an int or (h, w), each 8 .. 128; sigma 1.0 .. 3.0.  Generated on
    the device when there is one, by the library's host statement otherwise: the bytes are the same either way."""
    import torch
    from . import backend
    h, w, seed, s256 = _vac_settings(size, seed, sigma)
    if torch.cuda.is_available():
        return _device_thresholds_vac(h, w, seed, s256).numpy()
    return backend.void_cluster_thresholds(backend.void_cluster_ranks_host(h, w, seed, s256 / 256.0))


class VoidAndClusterDitherStrategy(MatrixDitherStrategy):
    """Ordered dithering with a void-and-cluster matrix generated and cached on the device per (size, seed, sigma).  Not in
    the reference: given to ImageDitherer as dither_mode=<instance>.  Position-only like every matrix mode, so bands, tiles,
    indexed output and the file writers take it as they take blue noise."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "size": {
                "type": "int", "default": 64, "min": 8, "max": 128, "label": "Matrix Size",
                "description": "Size of the void-and-cluster matrix (an integer, or (h, w) in code)",
            },
            "seed": {
                "type": "int", "default": 42, "min": 0, "max": 9999, "label": "Random Seed",
                "description": "Seed of the initial pattern (different seeds = different matrices)",
            },
            "sigma": {
                "type": "float", "default": 1.5, "min": 1.0, "max": 3.0, "step": 0.1, "label": "Sigma",
                "description": "Width of the Gaussian that measures voids and clusters, in pixels",
            },
        }

    def __init__(self, size=64, seed: int = 42, sigma: float = 1.5):
        _vac_settings(size, seed, sigma)
        self.size = size
        self.seed = seed
        self.sigma = sigma
        self._matrix = None

    @property
    def threshold_matrix(self):
        if self._matrix is None:
            self._matrix = generate_void_and_cluster(self.size, self.seed, self.sigma)
        return self._matrix

    def _thresholds(self):
        return _device_thresholds_vac(*_vac_settings(self.size, self.seed, self.sigma))

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"size": self.size, "seed": self.seed, "sigma": self.sigma}

    def __getstate__(self):
        return {"size": self.size, "seed": self.seed, "sigma": self.sigma, "_matrix": None}


class PolkaDotDitherStrategy(MatrixDitherStrategy):
    """Circular-dot threshold tile (dithering_lib.py:695-766): the decision rule is MatrixDitherStrategy's,
    only the tile differs; the tile_size x tile_size matrix is host setup exactly as in the reference."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "tile_size": {
                "type": "int", "default": 8, "min": 4, "max": 32, "label": "Tile Size",
                "description": "Size of the repeating dot pattern",
            },
            "gamma": {
                "type": "float", "default": 1.5, "min": 0.5, "max": 3.0, "step": 0.1, "label": "Gamma",
                "description": "Controls dot shape curve (higher = sharper edges)",
            },
        }

    def __init__(self, tile_size: int = 8, gamma: float = 1.5):
        self.tile_size = tile_size
        self.gamma = gamma
        super().__init__(self._generate_polka_dot_matrix(tile_size, gamma))

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"tile_size": self.tile_size, "gamma": self.gamma}

    @staticmethod
    def _generate_polka_dot_matrix(tile_size: int, gamma: float) -> np.ndarray:
        """1 - (distance to the tile centre / corner distance)^gamma, float64 then float32
        (dithering_lib.py:733-743)."""
        c = (tile_size - 1) / 2
        xv, yv = np.meshgrid(np.arange(tile_size), np.arange(tile_size))
        norm = np.sqrt((xv - c) ** 2 + (yv - c) ** 2) / (np.sqrt(c ** 2 + c ** 2) + 1e-9)
        return np.clip(1.0 - norm ** gamma, 0, 1).astype(np.float32)


class InterleavedGradientNoiseDitherStrategy(BaseDitherStrategy):
    """dithering_lib.py:502-571"""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "scale": {
                "type": "float", "default": 1.0, "min": 0.1, "max": 10.0, "step": 0.1, "label": "Scale",
                "description": "Noise frequency (lower = larger pattern, higher = finer grain)",
            },
            "seed": {
                "type": "int", "default": 0, "min": 0, "max": 9999, "label": "Seed",
                "description": "Deterministic offset to shift the pattern",
            },
        }

    def __init__(self, scale: float = 1.0, seed: int = 0):
        self.scale = float(scale)
        self.seed = int(seed)

    def _generate_thresholds(self, image_size: Tuple[int, int]) -> np.ndarray:
        from . import backend
        h, w = image_size
        return backend.ign_thresholds(h, w, self.scale, self.seed).cpu().numpy()

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        return backend.ordered(frames, pal, backend.MODE_IGN, ign_scale=self.scale, ign_seed=self.seed,
                               y0=y0, x0=x0, out=out)

    def dither(self, pixels, palette_arr, image_size):
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"scale": self.scale, "seed": self.seed}


# Which of the reference's two error-diffusion arithmetics to reproduce (dithering_lib.py:638-653 picks by whether numba
# imports): "python" -- the pure-Python loop (:655-690), what the reference runs in an environment without numba, pinned by
# the golden fixtures -- or "numba" -- _error_diffusion_numba (:213-308), typed per numba's unification rule: r / g / b are
# assigned a float32 element and float64 literals (:239-251), hence float64 -- a float64 linear scan with the first minimum
# winning, a float64 error, float64 products and sums with one rounding on the store.  Restated in the oracle; fixtures
# pending (no numba in the build image), so this branch is parity-unpinned.
ERROR_DIFFUSION_ARITHMETIC = os.environ.get("DITHER_PIE_ED_ARITHMETIC", "python")


class ErrorDiffusionDitherStrategy(BaseDitherStrategy):
    """dithering_lib.py:576-690 (by default the semantics of the pure-Python branch, which is what runs when numba is
    not installed -- see ERROR_DIFFUSION_ARITHMETIC; parameters are the reference's strings)."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "variant": {
                "type": "choice", "default": "atkinson", "choices": ErrorDiffusionKernel.list_kernels(),
                "label": "Algorithm", "description": "Error diffusion algorithm variant",
            },
            "serpentine": {
                "type": "choice", "default": "false", "choices": ["true", "false"], "label": "Serpentine Scan",
                "description": "Alternates direction each row to reduce artifacts",
            },
        }

    def __init__(self, variant: str = "atkinson", serpentine: str = "false"):
        self.variant = variant
        self.serpentine = (serpentine == "true")
        self._kernel = ErrorDiffusionKernel.get_kernel(variant)

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"variant": self.variant, "serpentine": "true" if self.serpentine else "false"}

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        if y0 or x0:
            raise ValueError("error diffusion carries state across the whole raster and cannot be tiled")
        return backend.error_diffusion(frames, pal, self._kernel["weights"], self._kernel["divisor"],
                                       self.serpentine, out=out, arithmetic=ERROR_DIFFUSION_ARITHMETIC)

    def dither(self, pixels, palette_arr, image_size):
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)


class _VariableDiffuser(BaseDitherStrategy):
    """Floyd-Steinberg-shaped scans whose coefficients depend on the source pixel."""

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        if y0 or x0:
            raise ValueError("error diffusion carries state across the whole raster and cannot be tiled")
        return self._diffuse(frames, pal, out)

    def dither(self, pixels, palette_arr, image_size):
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)


class PerceptualDitherStrategy(_VariableDiffuser):
    """Floyd-Steinberg weights scaled by 0.5 + 0.5*luminance/255 of the diffusing pixel (dithering_lib.py:1030-1066;
    the reference's optional base_weights argument is not exposed by any caller and is not supported)."""

    def _diffuse(self, frames, pal, out):
        from . import backend
        return backend.variable_diffusion(frames, pal, backend.DIFFUSER_PERCEPTUAL, out=out)


class HybridDitherStrategy(_VariableDiffuser):
    """Luminance part of the error diffused at lum_factor, colour part at col_factor (dithering_lib.py:1071-1155).  By default
    the pure-Python branch (:1127-1152), which is what runs without numba and is pinned by reference fixtures; with
    ERROR_DIFFUSION_ARITHMETIC = "numba" the strategy's numba branch (_hybrid_numba, :1396-1494, dispatched at :1114-1125),
    which clamps, scans the palette in float64 and keeps a float64 error -- typed per numba's unification rule, unpinned."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "lum_factor": {
                "type": "float", "default": 1.0, "min": 0.0, "max": 2.0, "step": 0.1, "label": "Luminance Factor",
                "description": "Strength of luminance error diffusion (1.0 = full, 0.0 = none)",
            },
            "col_factor": {
                "type": "float", "default": 0.2, "min": 0.0, "max": 2.0, "step": 0.1, "label": "Color Factor",
                "description": "Strength of color error diffusion (lower = less color noise)",
            },
        }

    def __init__(self, lum_factor: float = 1.0, col_factor: float = 0.2):
        self.lum_factor = lum_factor
        self.col_factor = col_factor
        self.fs_offsets = [(1, 0, 7 / 16), (-1, 1, 3 / 16), (0, 1, 5 / 16), (1, 1, 1 / 16)]

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"lum_factor": self.lum_factor, "col_factor": self.col_factor}

    def _diffuse(self, frames, pal, out):
        from . import backend
        if ERROR_DIFFUSION_ARITHMETIC == "numba":
            return backend.hybrid_numba(frames, pal, self.lum_factor, self.col_factor, out=out)
        return backend.variable_diffusion(frames, pal, backend.DIFFUSER_HYBRID, self.lum_factor, self.col_factor, out=out)


class AdaptiveVarianceDitherStrategy(_VariableDiffuser):
    """Floyd-Steinberg diffusion only from pixels whose local grayscale variance reaches var_threshold
    (dithering_lib.py:946-1025); the variance map reproduces scipy.ndimage.uniform_filter on the device."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "var_threshold": {
                "type": "float", "default": 300.0, "min": 0.0, "max": 1000.0, "step": 10.0, "label": "Variance Threshold",
                "description": "Threshold for local variance to trigger error diffusion",
            },
            "window_radius": {
                "type": "int", "default": 1, "min": 1, "max": 5, "label": "Window Radius",
                "description": "Radius of window for computing local variance",
            },
        }

    def __init__(self, var_threshold: float = 300.0, window_radius: int = 1):
        self.var_threshold = var_threshold
        self.window_radius = window_radius

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"var_threshold": self.var_threshold, "window_radius": self.window_radius}

    def _diffuse(self, frames, pal, out):
        from . import backend
        gate = backend.variance_gate(frames, pal, self.var_threshold, self.window_radius)
        return backend.variable_diffusion(frames, pal, backend.DIFFUSER_ADAPTIVE_VARIANCE, gate=gate, out=out)


class OstromoukhovDitherStrategy(_VariableDiffuser):
    """Ostromoukhov's intensity-dependent three-tap diffusion (dithering_lib.py:1160-1269)."""

    COEFFS_TABLE = [tuple(int(v) for v in row) for row in _tables.OSTROMOUKHOV]
    _coef_cache: Dict[int, Any] = {}

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            "serpentine": {
                "type": "choice", "default": "false", "choices": ["true", "false"], "label": "Serpentine Scan",
                "description": "Alternates direction each row to reduce artifacts",
            }
        }

    def __init__(self, serpentine: str = "false"):
        self.serpentine = (serpentine == "true")

    def get_current_parameters(self) -> Dict[str, Any]:
        return {"serpentine": "true" if self.serpentine else "false"}

    def _diffuse(self, frames, pal, out):
        import torch
        from . import backend
        dev = _device_index()
        coef = OstromoukhovDitherStrategy._coef_cache.get(dev)
        if coef is None:
            t = _tables.OSTROMOUKHOV
            coef = torch.from_numpy((t / t.sum(1, keepdims=True)).astype(np.float32)).cuda()  # f32(c_k / divisor)
            OstromoukhovDitherStrategy._coef_cache[dev] = coef
        return backend.variable_diffusion(frames, pal, backend.DIFFUSER_OSTROMOUKHOV, serpentine=self.serpentine,
                                          coef=coef, out=out)


# ------------------------------------------------------------------------------------- palettes
class ColorReducer:
    """Palette producers (dithering_lib.py:1807-1872).  Median cut and k-means cut and cluster in RGB whatever metric the ditherer
    that uses the palette has (ImageDitherer(metric="oklab") changes the search, not the palette); generate_oklab_palette (an
    addition to the reference's interface) clusters in the integer Oklab of that metric."""

    @staticmethod
    def find_dominant_channel(colors: List[Tuple[int, int, int]]) -> int:
        spans = [max(c[ch] for c in colors) - min(c[ch] for c in colors) for ch in range(3)]
        return spans.index(max(spans))

    @staticmethod
    def median_cut(colors: List[Tuple[int, int, int]], depth: int) -> List[Tuple[int, int, int]]:
        """dithering_lib.py:1822-1833: stable sort on the widest channel, split at len//2, bucket mean
        truncated per channel; an empty bucket yields (0, 0, 0)."""
        if not colors:
            return [(0, 0, 0)]
        if depth == 0:
            n = len(colors)
            return [tuple(int(sum(col) / n) for col in zip(*colors))]
        ch = ColorReducer.find_dominant_channel(colors)
        colors.sort(key=lambda c: c[ch])
        half = len(colors) // 2
        return ColorReducer.median_cut(colors[:half], depth - 1) + ColorReducer.median_cut(colors[half:], depth - 1)

    @staticmethod
    def _median_cut_arrays(colors: np.ndarray, depth: int) -> List[Tuple[int, int, int]]:
        """median_cut on an [n,3] integer array holding the colours in list order: same channel choice (first widest),
        same stable sort, same split, same truncated float mean -- numpy instead of Python lists of tuples."""
        if len(colors) == 0:
            return [(0, 0, 0)]
        if depth == 0:
            n = len(colors)
            sums = colors.sum(axis=0, dtype=np.int64)
            return [tuple(int(int(v) / n) for v in sums)]
        spans = colors.max(axis=0).astype(np.int64) - colors.min(axis=0).astype(np.int64)  # colors: uint8 rows
        ch = int(np.argmax(spans))  # the first of equal spans, like list.index(max(...))
        colors = colors[np.argsort(colors[:, ch], kind="stable")]
        half = len(colors) // 2
        return (ColorReducer._median_cut_arrays(colors[:half], depth - 1) +
                ColorReducer._median_cut_arrays(colors[half:], depth - 1))

    @staticmethod
    def _distinct_in_order(arr: np.ndarray) -> np.ndarray:
        """The distinct rows of an [n,3] uint8 array in order of first occurrence.  Images of 100 000 pixels and more go
        through the device (dp_distinct_first_u8: a 2^24-entry first-index table filled by atomic minima, the first
        occurrences compacted in pixel order; pinned staging buffer up, only the distinct colours down); smaller ones are
        host plumbing (numpy: the PCIe round trip would cost more than the work)."""
        n = len(arr)
        try:
            import torch
            use_gpu = n >= 100_000 and torch.cuda.is_available()
        except ImportError:
            use_gpu = False
        if use_gpu:
            from . import backend
            h_in, _ = _pinned_pair(3 * n)
            np.copyto(h_in.numpy()[:3 * n].reshape(n, 3), arr)   # (arr may be a read-only view of PIL's bytes)
            t = h_in[:3 * n].cuda(non_blocking=True).view(n, 3)
            return backend.distinct_first(t).cpu().numpy()
        packed = (arr[:, 0].astype(np.uint32) << 16) | (arr[:, 1].astype(np.uint32) << 8) | arr[:, 2].astype(np.uint32)
        _, first = np.unique(packed, return_index=True)
        return arr[np.sort(first)]

    @staticmethod
    def _distinct_of_image(rgb):
        """_distinct_in_order for a big PIL 'RGB' image without packing it on the host first: Pillow's four-bytes-per-pixel rows go
        straight into the pinned buffer (_pil_rgbx_into: 2.0 ms for a 4K image where tobytes() + the copy into the buffer took
        5.4), the fourth byte is dropped on the GPU.  None: not applicable (small image, no GPU, no raw encoder) -- the caller packs."""
        n = rgb.size[0] * rgb.size[1]
        try:
            import torch
            if n < 100_000 or not torch.cuda.is_available():
                return None
        except ImportError:
            return None
        from . import backend
        h_in, _ = _pinned_pair(4 * n)
        if not _pil_rgbx_into(rgb, h_in.numpy()[:4 * n]):
            return None
        t = h_in[:4 * n].view(n, 4).cuda(non_blocking=True)[:, :3].contiguous()
        return backend.distinct_first(t).cpu().numpy()

    _replay_ok = None  # does dp_pyset_order_host reproduce THIS interpreter's set order?  (checked once per process)

    @staticmethod
    def _pyset_replay_ok() -> bool:
        """The native median cut replays CPython's set (tuple hash, probing, growth) to obtain the order in which the
        reference's `list(set(image.getdata()))` yields the colours.  That is an implementation detail of the interpreter:
        before relying on it, compare the replay with a real set of this interpreter once -- 70 000 colours, enough to
        cross every growth step incl. the change of policy at 50 000 entries; on any difference (another Python
        implementation or a future CPython) reduce_colors keeps building real sets."""
        if ColorReducer._replay_ok is None:
            ok = False
            try:
                import ctypes as C
                from . import _lib
                L = _lib.load()
                rs = np.random.RandomState(20240607)
                probe = np.ascontiguousarray(rs.randint(0, 256, (70000, 3)).astype(np.uint8))
                probe[:5000] = probe[5000:10000] // 16          # plenty of duplicates and small values as well
                order = np.empty(len(probe), np.uint32)
                nd = C.c_int64(0)
                if L.dp_pyset_order_host(probe.ctypes.data, len(probe), order.ctypes.data, C.byref(nd)) == 0:
                    real = list(set(zip(probe[:, 0].tolist(), probe[:, 1].tolist(), probe[:, 2].tolist())))
                    mine = probe[order[:nd.value]]
                    ok = nd.value == len(real) and np.array_equal(mine, np.array(real, np.uint8).reshape(-1, 3))
            except Exception:  # noqa: BLE001 - library not built, or anything else: the Python path is always right
                ok = False
            ColorReducer._replay_ok = ok
        return ColorReducer._replay_ok

    @staticmethod
    def reduce_colors(image, num_colors: int) -> List[Tuple[int, int, int]]:
        """Median cut over the image's unique colours; returns 2**int(log2(n)) entries
        (dithering_lib.py:1835-1843).  Host-side, and bit-identical to the reference's
        `median_cut(list(set(image.getdata())), depth)`: the stable sort makes the iteration order of that Python set
        observable.  The distinct colours are taken in order of first occurrence (on the GPU for big images; adding a
        colour that is already in a set changes nothing, so the set ends up in the same state); then
        dp_median_cut_host replays CPython's set to get its iteration order and cuts with counting sorts -- a 4K
        photograph with 1.2 M distinct colours: ~0.1 s instead of ~1.5 s with a real set and numpy sorts (reference: ~9 s).
        Should the replay not match this interpreter's sets (_pyset_replay_ok), the set is built by Python as before."""
        rgb = image if image.mode == "RGB" else image.convert("RGB")   # (no copy of an image that is RGB already)
        distinct = ColorReducer._distinct_of_image(rgb)
        if distinct is None:
            distinct = ColorReducer._distinct_in_order(np.frombuffer(rgb.tobytes(), dtype=np.uint8).reshape(-1, 3))
        return ColorReducer._median_cut_of_distinct(distinct, num_colors)

    @staticmethod
    def _median_cut_of_distinct(distinct: np.ndarray, num_colors: int) -> List[Tuple[int, int, int]]:
        """The tail of reduce_colors: `distinct` holds the image's distinct colours ([n,3] uint8) in order of first
        occurrence -- the order they enter the reference's set -- however they were found (one image, or a clip's frames
        streamed through backend.DistinctStream)."""
        distinct = np.ascontiguousarray(distinct)
        n = max(int(num_colors), 1)
        depth = int(math.log2(n)) if n > 1 else 0
        if depth <= 10 and ColorReducer._pyset_replay_ok():
            import ctypes as C
            from . import _lib
            out = np.zeros((1 << depth, 3), np.int32)
            n_out = C.c_int(0)
            _lib.check(_lib.load().dp_median_cut_host(distinct.ctypes.data, len(distinct), depth, out.ctypes.data, C.byref(n_out)))
            return [tuple(int(v) for v in c) for c in out[:n_out.value]]
        import itertools
        unique = list(set(zip(distinct[:, 0].tolist(), distinct[:, 1].tolist(), distinct[:, 2].tolist())))
        colors = np.fromiter(itertools.chain.from_iterable(unique), dtype=np.uint8, count=3 * len(unique)).reshape(-1, 3)
        return ColorReducer._median_cut_arrays(colors, depth)

    @staticmethod
    def generate_kmeans_palette(img, num_colors: int, random_state=42) -> List[Tuple[int, int, int]]:
        """k-means palette (dithering_lib.py:1845-1857).  Images of at most 10 000 pixels, where the reference is
        deterministic: the reference's palette (sklearn's seeds, sklearn's labelling of equidistant pixels; 11 reference
        fixtures) -- except that a cluster mean that is an exact integer comes out as that integer, where the reference
        returns it or one less depending on its thread scheduling.  Larger images: the reference fits on an UNSEEDED random
        sample of 10 000 pixels and is not reproducible; here Lloyd runs on the GPU over every pixel (over the colour
        histogram) with exact integer sums, seeded from `random_state` (dither_pie_amd/kmeans.py: parity definition)."""
        from .kmeans import kmeans_palette_from_image
        return kmeans_palette_from_image(img, num_colors, random_state)

    @staticmethod
    def reduce_colors_frames(frames, num_colors: int, use_gamma: bool = False, every: int = 1) -> List[Tuple[int, int, int]]:
        """reduce_colors over a CLIP that is resident on the GPU (uint8 CUDA tensor [N,H,W,3]): one palette fitted to every
        `every`-th frame.  Equal to the reference's reduce_colors(image, n) with `image` the taken frames stacked top to
        bottom (linearised first under use_gamma).  clip_palette.ClipPalette is the streaming form."""
        from .clip_palette import ClipPalette
        return ClipPalette(use_gamma=use_gamma, device=frames.device).add(frames, every=every).median_cut(num_colors)

    @staticmethod
    def generate_kmeans_palette_frames(frames, num_colors: int, random_state=42, use_gamma: bool = False,
                                       every: int = 1) -> List[Tuple[int, int, int]]:
        """A k-means palette of a CLIP that is resident on the GPU: a pure function of the colour multiset of every
        `every`-th frame (clip_palette.ClipPalette.kmeans: seeds by pixel rank in histogram order, Lloyd over the
        histogram)."""
        from .clip_palette import ClipPalette
        return ClipPalette(use_gamma=use_gamma, device=frames.device).add(frames, every=every).kmeans(num_colors, random_state)

    @staticmethod
    def generate_oklab_palette(img, num_colors: int, max_iter: int = 100) -> List[Tuple[int, int, int]]:
        """A palette fitted in the integer Oklab (include/ditherpie_hip_okfit.h): a weighted k-means over the image's colour
        histogram on the GPU, all integer and exact -- a pure function of the image's colour multiset, no random numbers; every
        entry is a colour of the image (the member of its cluster nearest to the cluster's mean), so duplicates appear when the
        image has fewer distinct colours than num_colors.  At most 256 colours."""
        import torch
        from . import backend
        backend._okfit_args(num_colors, max_iter)
        rgb = img if img.mode == "RGB" else img.convert("RGB")
        frame = torch.from_numpy(np.asarray(rgb, dtype=np.uint8).copy()).cuda()
        return ColorReducer.generate_oklab_palette_frames(frame, num_colors, 1, max_iter)

    @staticmethod
    def generate_oklab_palette_frames(frames, num_colors: int, every: int = 1, max_iter: int = 100) -> List[Tuple[int, int, int]]:
        """generate_oklab_palette of a CLIP that is resident on the GPU (uint8 CUDA tensor [N,H,W,3] or [H,W,3]): one palette
        fitted to the colour multiset of every `every`-th frame (clip_palette.ClipPalette.oklab is the streaming form)."""
        from .clip_palette import ClipPalette
        from . import backend
        backend._okfit_args(num_colors, max_iter)
        return ClipPalette(device=frames.device).add(frames, every=every).oklab(num_colors, max_iter)

    @staticmethod
    def generate_uniform_palette(num_colors: int) -> List[Tuple[int, int, int]]:
        """dithering_lib.py:1859-1872: the first n points of a ceil(n^(1/3))^3 grid, r slowest."""
        side = int(math.ceil(num_colors ** (1 / 3)))
        if side <= 1:
            return [(128, 128, 128)][:num_colors]
        levels = [int(v * 255 / (side - 1)) for v in range(side)]
        grid = [(r, g, b) for r in levels for g in levels for b in levels]
        return grid[:num_colors]


# ------------------------------------------------------------------------------------- Riemersma
def _hilbert_order(n: int) -> np.ndarray:
    """The path of the Riemersma ditherer over an n x n square, n = 2^k (dithering_lib.py:771-805): int32 [n*n, 2] of
    (row, col) = (y, x) per path index, where (x, y) comes from the reference's hilbert_xy level loop (evaluated here for all
    indices at once)."""
    bits = int(math.log2(n))
    t = np.arange(n * n, dtype=np.int64)
    x = np.zeros_like(t)
    y = np.zeros_like(t)
    for lvl in range(bits):
        s = 1 << lvl
        rx = 1 & (t >> 1)
        ry = 1 & (t ^ rx)
        flip = (ry == 0) & (rx == 1)
        x = np.where(flip, s - 1 - x, x)
        y = np.where(flip, s - 1 - y, y)
        x, y = np.where(ry == 0, y, x), np.where(ry == 0, x, y)
        x += s * rx
        y += s * ry
        t >>= 2
    return np.stack([y, x], axis=1).astype(np.int32)


def _next_power_of_two(x: int) -> int:
    """Smallest power of two >= x; 1 for x <= 1 (dithering_lib.py:808-809)."""
    return 1 << (int(x) - 1).bit_length() if x > 0 else 1


class RiemersmaDitherStrategy(BaseDitherStrategy):
    """Error diffusion along a Hilbert curve (dithering_lib.py:812-841): the in-image indices of the path over the next
    power-of-two square each push their error into the next four path indices (7/16, 1/16, 5/16, 3/16).  No parameters."""

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        if y0 or x0:
            raise ValueError("Riemersma dithering carries state along the whole path and cannot be tiled")
        return backend.riemersma(frames, pal, out=out)

    def dither(self, pixels: np.ndarray, palette_arr: np.ndarray, image_size: Tuple[int, int]) -> np.ndarray:
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)


# ------------------------------------------------------------------------------------- Halftone
class HalftoneDitherStrategy(BaseDitherStrategy):
    """Newspaper-style halftone (dithering_lib.py:1498-1695): a screen of cells rotated by `angle`, each cell's mean colour
    mapped to its nearest entry, a pixel inked with that entry when its darkness exceeds the screen threshold, the paper
    (brightest) entry otherwise.  GPU kernels in halftone.hip; frames are independent, a frame cannot be tiled.

    Drop-in for the reference's class (same constructor, metadata, dither() contract).  Not dispatched by ImageDitherer:
    DitherMode.HALFTONE still raises NotImplementedError there; dither_frames() is the device-batch entry.  Divergence:
    cell_size <= 0, a dot_gain that is not a finite number > 0, and an empty image raise ValueError at dither time (the
    reference crashes or computes NaN-driven output)."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            'cell_size': {'type': 'int', 'default': 8, 'min': 2, 'max': 32, 'label': 'Cell Size',
                          'description': 'Distance between dot centers (smaller = finer detail)'},
            'angle': {'type': 'float', 'default': 45.0, 'min': 0.0, 'max': 90.0, 'label': 'Screen Angle',
                      'description': 'Rotation angle in degrees (45\u00b0 is classic newspaper)'},
            'dot_gain': {'type': 'float', 'default': 1.0, 'min': 0.5, 'max': 3.0, 'step': 0.1, 'label': 'Dot Gain',
                         'description': 'Controls dot growth (1.0 = linear, higher = more contrast)'},
            'min_dot_size': {'type': 'float', 'default': 0.0, 'min': 0.0, 'max': 0.5, 'step': 0.05, 'label': 'Min Dot Size',
                             'description': 'Minimum dot threshold (0 = pure white possible)'},
            'max_dot_size': {'type': 'float', 'default': 1.0, 'min': 0.5, 'max': 1.0, 'step': 0.05, 'label': 'Max Dot Size',
                             'description': 'Maximum dot threshold (1.0 = pure black possible)'},
            'shape': {'type': 'choice', 'default': 'circle', 'choices': ['circle', 'square', 'diamond'], 'label': 'Dot Shape',
                      'description': 'Shape of halftone dots'},
            'sharpness': {'type': 'float', 'default': 1.5, 'min': 0.5, 'max': 4.0, 'step': 0.1, 'label': 'Sharpness',
                          'description': 'Edge sharpness (higher = crisper dots)'},
        }

    def __init__(self, cell_size: int = 8, angle: float = 45.0, dot_gain: float = 1.0, min_dot_size: float = 0.0,
                 max_dot_size: float = 1.0, shape: str = "circle", sharpness: float = 1.5):
        self.cell_size = cell_size
        self.angle = angle
        self.dot_gain = dot_gain
        self.min_dot_size = min_dot_size
        self.max_dot_size = max_dot_size
        self.shape = shape
        self.sharpness = sharpness

    def get_current_parameters(self) -> Dict[str, Any]:
        return {'cell_size': self.cell_size, 'angle': self.angle, 'dot_gain': self.dot_gain,
                'min_dot_size': self.min_dot_size, 'max_dot_size': self.max_dot_size, 'shape': self.shape,
                'sharpness': self.sharpness}

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        if y0 or x0:
            raise ValueError("halftone cells average over the whole image: a frame cannot be tiled")
        return backend.halftone(frames, pal, self.get_current_parameters(), out=out)

    def dither(self, pixels: np.ndarray, palette_arr: np.ndarray, image_size: Tuple[int, int]) -> np.ndarray:
        h, w = image_size
        if h <= 0 or w <= 0:
            raise ValueError(f"halftone needs a non-empty image, not {h} x {w}")
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)

    def dither_frames(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """uint8 CUDA tensor [N,H,W,3] (or [H,W,3]) -> halftoned uint8 CUDA tensor of the same shape, each frame as
        ImageDitherer(..., palette, use_gamma).apply_dithering would halftone it (palette: the reference's list of RGB
        triples; use_gamma as there).  Frames stay in HBM."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            pal = _device_palette(*prepare_palette(palette, use_gamma))
            return self._run(frames_u8_cuda, pal, out=out)

    def dither_frames_indexed(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """dither_frames() as palette-index planes: -> (planes [N,H,W] (or [H,W]), palette_u8 [K,3]) with
        palette_u8[planes] == dither_frames(...); torch.uint8 up to 256 colours, torch.int16 above."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            return _indexed(self.dither_frames(frames_u8_cuda, palette, use_gamma), palette, use_gamma, out)


# ------------------------------------------------------------------------------------- Wavelet
class WaveletDitherStrategy(BaseDitherStrategy):
    """Wavelet dithering (dithering_lib.py:846-941): per channel a one-level 2-D DWT (pywt.dwt2, 'symmetric'), each subband
    quantised to subband_quant levels with uniform noise, the inverse DWT, crop and clip; then per pixel the nearest or the
    second-nearest palette entry, chosen by a uniform threshold.  GPU kernels in wavelet.hip (the transforms restate
    PyWavelets 1.x in float32 to the last bit; no pywt needed at run time); frames are independent, a frame cannot be
    tiled.  The random stream (numpy's RandomState(seed)) is generated on the host once per geometry and kept on the
    device.

    Drop-in for the reference's class (same constructor, metadata, dither() contract).  Not dispatched by ImageDitherer:
    DitherMode.WAVELET still raises NotImplementedError there; dither_frames() is the device-batch entry.  Divergences: a
    wavelet outside the nine of the metadata, a subband_quant that is not an int in [1, 2^31 - 1], a seed outside
    [0, 2^32) and an empty image raise ValueError at dither time (the reference needs pywt for other wavelets, or crashes)."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            'wavelet': {'type': 'choice', 'default': 'haar',
                        'choices': ['haar', 'db1', 'db2', 'db4', 'sym2', 'sym4', 'coif1', 'bior1.3', 'bior2.2'],
                        'label': 'Wavelet Type', 'description': 'Type of wavelet basis function'},
            'subband_quant': {'type': 'int', 'default': 8, 'min': 2, 'max': 32, 'label': 'Subband Quantization',
                              'description': 'Number of quantization levels for wavelet subbands'},
            'seed': {'type': 'int', 'default': 42, 'min': 0, 'max': 9999, 'label': 'Random Seed',
                     'description': 'Seed for random threshold generation (same seed = same output)'},
        }

    def __init__(self, wavelet: str = 'haar', subband_quant: int = 8, seed: int = 42):
        self.wavelet = wavelet
        self.subband_quant = subband_quant
        self.seed = seed

    def get_current_parameters(self) -> Dict[str, Any]:
        return {'wavelet': self.wavelet, 'subband_quant': self.subband_quant, 'seed': self.seed}

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        if y0 or x0:
            raise ValueError("wavelet subbands are quantised over the whole image: a frame cannot be tiled")
        return backend.wavelet(frames, pal, self.get_current_parameters(), out=out)

    def dither(self, pixels: np.ndarray, palette_arr: np.ndarray, image_size: Tuple[int, int]) -> np.ndarray:
        from . import backend
        h, w = image_size
        if h <= 0 or w <= 0:
            raise ValueError(f"wavelet needs a non-empty image, not {h} x {w}")
        backend.wavelet_check(**self.get_current_parameters())
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)

    def dither_frames(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """uint8 CUDA tensor [N,H,W,3] (or [H,W,3]) -> dithered uint8 CUDA tensor of the same shape, each frame as
        ImageDitherer(..., palette, use_gamma).apply_dithering would dither it (palette: the reference's list of RGB
        triples; use_gamma as there).  Frames stay in HBM."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            pal = _device_palette(*prepare_palette(palette, use_gamma))
            return self._run(frames_u8_cuda, pal, out=out)

    def dither_frames_indexed(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """dither_frames() as palette-index planes: -> (planes [N,H,W] (or [H,W]), palette_u8 [K,3]) with
        palette_u8[planes] == dither_frames(...); torch.uint8 up to 256 colours, torch.int16 above."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            return _indexed(self.dither_frames(frames_u8_cuda, palette, use_gamma), palette, use_gamma, out)


# ------------------------------------------------------------------------------------- Pattern (Knoll)
class PatternDitherStrategy(BaseDitherStrategy):
    """Pattern dithering (Thomas Knoll's; Yliluoma's "algorithm 2"), an ordered dither for arbitrary palettes: per pixel a
    list of n = m * m palette entries whose mean approximates the pixel (n nearest-colour searches, each steered by
    `strength` times the error accumulated so far), sorted by luminance; the m x m Bayer rank matrix picks one by position.
    Where the two-nearest ordered modes can only mix two entries, this mixes up to n.  Position-only, hence stable from
    frame to frame and tileable: _run takes (y0, x0).  GPU kernel and the per-palette 2^24-entry search table in
    pattern.hip (include/ditherpie_hip_pattern.h has the integer definition); at most 256 colours.

    Not in the reference and not a DitherMode member: pass an instance as ImageDitherer(dither_mode=...), or use
    dither_frames().  strength256 = round(strength * 256); a strength outside [0, 1], an unknown matrix and a palette of
    more than 256 colours raise ValueError at dither time."""

    _MATRICES = {"2x2": 2, "4x4": 4, "8x8": 8}

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            'matrix': {'type': 'choice', 'default': '4x4', 'choices': ['2x2', '4x4', '8x8'], 'label': 'Pattern Size',
                       'description': 'Rank matrix size (larger = more colours mixed per pixel, coarser pattern)'},
            'strength': {'type': 'float', 'default': 0.5, 'min': 0.0, 'max': 1.0, 'step': 0.05, 'label': 'Strength',
                         'description': 'Share of the accumulated error that steers the next candidate (0 = nearest colour)'},
        }

    def __init__(self, matrix: str = "4x4", strength: float = 0.5):
        self.matrix = matrix
        self.strength = strength

    def get_current_parameters(self) -> Dict[str, Any]:
        return {'matrix': self.matrix, 'strength': self.strength}

    def _settings(self):
        m = self._MATRICES.get(self.matrix)
        if m is None:
            raise ValueError(f"pattern matrix must be one of {sorted(self._MATRICES)}, not {self.matrix!r}")
        try:
            s256 = int(round(float(self.strength) * 256))
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"pattern strength must be a number in [0, 1], not {self.strength!r}") from None
        if not 0 <= s256 <= 256:
            raise ValueError(f"pattern strength must lie in [0, 1], not {self.strength!r}")
        return m, s256

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        m, s256 = self._settings()
        return backend.pattern(frames, pal, m, s256, y0=y0, x0=x0, out=out)

    def dither(self, pixels: np.ndarray, palette_arr: np.ndarray, image_size: Tuple[int, int]) -> np.ndarray:
        h, w = image_size
        if h <= 0 or w <= 0:
            raise ValueError(f"pattern dithering needs a non-empty image, not {h} x {w}")
        self._settings()
        if len(palette_arr) > 256:
            raise ValueError(f"pattern dithering supports at most 256 colours, the palette has {len(palette_arr)}")
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)

    def dither_frames(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None, y0: int = 0, x0: int = 0):
        """uint8 CUDA tensor [N,H,W,3] (or [H,W,3]) -> dithered uint8 CUDA tensor of the same shape, each frame as
        ImageDitherer(dither_mode=self, palette=palette, use_gamma=use_gamma).apply_dithering would dither it (palette:
        the reference's list of RGB triples).  Frames stay in HBM; (y0, x0): the tile's place in a larger image."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            pal = _device_palette(*prepare_palette(palette, use_gamma))
            return self._run(frames_u8_cuda, pal, y0=y0, x0=x0, out=out)

    def dither_frames_indexed(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """dither_frames() as palette-index planes: -> (planes [N,H,W] (or [H,W]), palette_u8 [K,3]) with
        palette_u8[planes] == dither_frames(...); torch.uint8 (at most 256 colours)."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            return _indexed(self.dither_frames(frames_u8_cuda, palette, use_gamma), palette, use_gamma, out)


# ------------------------------------------------------------------------------------- Dot diffusion (Knuth)
class DotDiffusionDitherStrategy(BaseDitherStrategy):
    """Dot diffusion (Knuth 1987): error diffusion without a scan.  Every pixel has a class from a small tiled class matrix,
    pixels are quantised in class order and a pixel's error goes to its neighbours of a higher class only (weight 2
    orthogonally, 1 diagonally).  Dependencies are local, so the GPU diffuses tiles independently and exactly
    (dotdiff.hip; include/ditherpie_hip_dotdiff.h has the integer definition): the look of diffusion at a small multiple of the
    cost of an ordered mode.  Errors cross every tile a caller could cut, so _run refuses (y0, x0) as the scans do.

    matrix: a name of MATRICES ("knuth": Knuth's 8 x 8 matrix, the default) or an m x m array (m = 2, 4, 8, 16) that is a
    permutation of 0 .. m*m-1 and whose reach (backend.dotdiff_reach) is at most 16.  strength256 = round(strength * 256).
    Not in the reference and not a DitherMode member: pass an instance as ImageDitherer(dither_mode=...), or use
    dither_frames().  A bad matrix, a strength outside [0, 1] and a palette of more than 256 colours raise ValueError at
    dither time."""

    MATRICES = {
        "knuth": ((34, 48, 40, 32, 29, 15, 23, 31), (42, 58, 56, 53, 21, 5, 7, 10), (50, 62, 61, 45, 13, 1, 2, 18),
                  (38, 46, 54, 37, 25, 17, 9, 26), (28, 14, 22, 30, 35, 49, 41, 33), (20, 4, 6, 11, 43, 59, 57, 52),
                  (12, 0, 3, 19, 51, 63, 60, 44), (24, 16, 8, 27, 39, 47, 55, 36)),
    }

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            'matrix': {'type': 'choice', 'default': 'knuth', 'choices': ['knuth'], 'label': 'Class Matrix',
                       'description': 'Order in which the pixels of a tile are quantised (an m x m array is taken too)'},
            'strength': {'type': 'float', 'default': 1.0, 'min': 0.0, 'max': 1.0, 'step': 0.05, 'label': 'Strength',
                         'description': 'Share of a pixel\'s error handed to its neighbours (0 = nearest colour)'},
        }

    def __init__(self, matrix="knuth", strength: float = 1.0):
        self.matrix = matrix
        self.strength = strength

    def get_current_parameters(self) -> Dict[str, Any]:
        return {'matrix': self.matrix, 'strength': self.strength}

    def _settings(self):
        """-> (the class matrix as a uint8 array, strength256)."""
        from . import backend
        matrix = self.matrix
        if isinstance(matrix, str):
            if matrix not in self.MATRICES:
                raise ValueError(f"dot diffusion matrix must be one of {sorted(self.MATRICES)} or an array, not {matrix!r}")
            matrix = self.MATRICES[matrix]
        classes = backend._dotdiff_classes(matrix)
        try:
            s256 = int(round(float(self.strength) * 256))
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"dot diffusion strength must be a number in [0, 1], not {self.strength!r}") from None
        if not 0 <= s256 <= 256:
            raise ValueError(f"dot diffusion strength must lie in [0, 1], not {self.strength!r}")
        return classes, s256

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        if y0 or x0:
            raise ValueError("dot diffusion hands errors across every tile edge and cannot be tiled by the caller")
        classes, s256 = self._settings()
        return backend.dotdiff(frames, pal, classes, s256, out=out)

    def _run_masked(self, frames, mask, pal, fill, out=None):
        """_run under a mask (backend.dotdiff_masked): transparent pixels become `fill` and take no part in the diffusion."""
        from . import backend
        classes, s256 = self._settings()
        return backend.dotdiff_masked(frames, mask, pal, classes, s256, fill=fill, out=out)

    def dither(self, pixels: np.ndarray, palette_arr: np.ndarray, image_size: Tuple[int, int]) -> np.ndarray:
        h, w = image_size
        if h <= 0 or w <= 0:
            raise ValueError(f"dot diffusion needs a non-empty image, not {h} x {w}")
        self._settings()
        if len(palette_arr) > 256:
            raise ValueError(f"dot diffusion supports at most 256 colours, the palette has {len(palette_arr)}")
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)

    def dither_frames(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """uint8 CUDA tensor [N,H,W,3] (or [H,W,3]) -> dithered uint8 CUDA tensor of the same shape, each frame as
        ImageDitherer(dither_mode=self, palette=palette, use_gamma=use_gamma).apply_dithering would dither it (palette:
        the reference's list of RGB triples).  Frames stay in HBM; `out` must not be the frames."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            pal = _device_palette(*prepare_palette(palette, use_gamma))
            return self._run(frames_u8_cuda, pal, out=out)

    def dither_frames_indexed(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """dither_frames() as palette-index planes: -> (planes [N,H,W] (or [H,W]), palette_u8 [K,3]) with
        palette_u8[planes] == dither_frames(...); torch.uint8 (at most 256 colours)."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            return _indexed(self.dither_frames(frames_u8_cuda, palette, use_gamma), palette, use_gamma, out)


# ------------------------------------------------------------------------------------- Integer error diffusion (table scans)
class IntegerErrorDiffusionDitherStrategy(BaseDitherStrategy):
    """The classical raster-scan error diffusers (ErrorDiffusionKernel's eight tap sets) in integer arithmetic: values in
    sixteenths, every share truncated on its own, the nearest colour from the palette's exact 2^24-entry table (idiff.hip;
    include/ditherpie_hip_idiff.h has the definition).  The search costs the same for 2 and for 256 colours, and because the
    table serves either metric this is the scan for ImageDitherer(metric="oklab") -- "Floyd-Steinberg, but perceptual".
    DitherMode.ERROR_DIFFUSION stays the reference's float scan, bit for bit; this mode is close to it, not identical, and has
    no serpentine.  Errors cross every band a caller could cut, so _run refuses (y0, x0) as the scans do.

    variant: a name of ErrorDiffusionKernel (an unknown name falls back to Floyd-Steinberg as in the reference; anything but
    a string is a ValueError).  strength256 = round(strength * 256).  Not in the reference and not a DitherMode member: pass
    an instance as ImageDitherer(dither_mode=...), or use dither_frames().  A strength outside [0, 1] and a palette of more
    than 256 colours raise ValueError at dither time."""

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        return {
            'variant': {'type': 'choice', 'default': 'floyd_steinberg', 'choices': ErrorDiffusionKernel.list_kernels(),
                        'label': 'Algorithm', 'description': 'Error diffusion algorithm variant'},
            'strength': {'type': 'float', 'default': 1.0, 'min': 0.0, 'max': 1.0, 'step': 0.05, 'label': 'Strength',
                         'description': 'Share of a pixel\'s error handed to its neighbours (0 = nearest colour)'},
        }

    def __init__(self, variant: str = "floyd_steinberg", strength: float = 1.0):
        self.variant = variant
        self.strength = strength

    def get_current_parameters(self) -> Dict[str, Any]:
        return {'variant': self.variant, 'strength': self.strength}

    def _settings(self):
        """-> (taps [(dx, dy, weight)], divisor, strength256)."""
        if not isinstance(self.variant, str):
            raise ValueError(f"integer error diffusion variant must be a name of {ErrorDiffusionKernel.list_kernels()}, "
                             f"not {self.variant!r}")
        kernel = ErrorDiffusionKernel.get_kernel(self.variant)
        try:
            s256 = int(round(float(self.strength) * 256))
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"integer error diffusion strength must be a number in [0, 1], not {self.strength!r}") from None
        if not 0 <= s256 <= 256:
            raise ValueError(f"integer error diffusion strength must lie in [0, 1], not {self.strength!r}")
        return [tuple(int(v) for v in t) for t in kernel["weights"]], int(kernel["divisor"]), s256

    def _run(self, frames, pal, y0=0, x0=0, out=None):
        from . import backend
        if y0 or x0:
            raise ValueError("integer error diffusion hands errors across every band edge and cannot be tiled by the caller")
        taps, divisor, s256 = self._settings()
        return backend.idiff(frames, pal, taps, divisor, s256, out=out)

    def _run_masked(self, frames, mask, pal, fill, out=None):
        """_run under a mask (backend.idiff_masked): transparent pixels become `fill` and take no part in the diffusion."""
        from . import backend
        taps, divisor, s256 = self._settings()
        return backend.idiff_masked(frames, mask, pal, taps, divisor, s256, fill=fill, out=out)

    def dither(self, pixels: np.ndarray, palette_arr: np.ndarray, image_size: Tuple[int, int]) -> np.ndarray:
        h, w = image_size
        if h <= 0 or w <= 0:
            raise ValueError(f"integer error diffusion needs a non-empty image, not {h} x {w}")
        self._settings()
        if len(palette_arr) > 256:
            raise ValueError(f"integer error diffusion supports at most 256 colours, the palette has {len(palette_arr)}")
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)

    def dither_frames(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """uint8 CUDA tensor [N,H,W,3] (or [H,W,3]) -> dithered uint8 CUDA tensor of the same shape, each frame as
        ImageDitherer(dither_mode=self, palette=palette, use_gamma=use_gamma).apply_dithering would dither it (palette:
        the reference's list of RGB triples).  Frames stay in HBM; `out` must not be the frames."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            pal = _device_palette(*prepare_palette(palette, use_gamma))
            return self._run(frames_u8_cuda, pal, out=out)

    def dither_frames_indexed(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """dither_frames() as palette-index planes: -> (planes [N,H,W] (or [H,W]), palette_u8 [K,3]) with
        palette_u8[planes] == dither_frames(...); torch.uint8 (at most 256 colours)."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            return _indexed(self.dither_frames(frames_u8_cuda, palette, use_gamma), palette, use_gamma, out)


# ------------------------------------------------------------------------------------- Cell palettes (k colours per cell)
class CellPaletteDitherStrategy(BaseDitherStrategy):
    """Cell-palette dithering: the picture is cut into small cells and every cell may show only a few of the palette's
    colours -- the colour constraint of the 8-bit home computers.  Per cell EVERY allowed set of colours is tried on the
    pixels, perturbed by a Bayer matrix, and the set of least total squared error is taken (cells.hip;
    include/ditherpie_hip_cells.h has the integer definition), so there is no attribute clash to repair.

    cell: "WxH" or a pair (width, height), each of 4, 8, 16.  colours: how many entries a cell chooses, 1 .. 4.  matrix:
    "2x2", "4x4", "8x8" (or 2, 4, 8), spread 0 .. 255: the perturbation.  shared: palette indices every cell owns besides
    its choice.  groups: an iterable of iterables of indices; the chosen entries of a cell all come from one group (None:
    one group of the whole palette).  At most 16 colours.
      C64 hires:        CellPaletteDitherStrategy() with the caller's 16-colour palette (8 x 8 cells, two colours each)
      C64 multicolour:  CellPaletteDitherStrategy(cell="4x8", colours=3, shared=(background,))
      ZX Spectrum:      CellPaletteDitherStrategy.zx_spectrum() with ZX_SPECTRUM_PALETTE (two colours of one brightness)
    Not in the reference and not a DitherMode member: pass an instance as ImageDitherer(dither_mode=...), or use
    dither_frames().  Cells are anchored at the frame's first pixel, so _run refuses (y0, x0): a band edge would split
    cells.  Bad settings and a palette of more than 16 colours raise ValueError at dither time."""

    _ZX = ((0, 0, 1), (1, 0, 0), (1, 0, 1), (0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1))   # blue red magenta green cyan yellow white
    ZX_SPECTRUM_PALETTE = ([(0, 0, 0)] + [tuple(215 * c for c in t) for t in _ZX] + [tuple(255 * c for c in t) for t in _ZX])
    ZX_SPECTRUM_GROUPS = ((0, 1, 2, 3, 4, 5, 6, 7), (0, 8, 9, 10, 11, 12, 13, 14))

    @staticmethod
    def get_parameter_info() -> Dict[str, Any]:
        sizes = [f"{a}x{b}" for a in (4, 8, 16) for b in (4, 8, 16)]
        return {
            'cell': {'type': 'choice', 'default': '8x8', 'choices': sizes, 'label': 'Cell Size',
                     'description': 'Width x height of the cells that share a small set of colours'},
            'colours': {'type': 'int', 'default': 2, 'min': 1, 'max': 4, 'label': 'Colours per Cell',
                        'description': 'Palette entries a cell chooses (besides the shared ones)'},
            'matrix': {'type': 'choice', 'default': '4x4', 'choices': ['2x2', '4x4', '8x8'], 'label': 'Matrix Size',
                       'description': 'Bayer matrix that perturbs the pixels before the search'},
            'spread': {'type': 'int', 'default': 64, 'min': 0, 'max': 255, 'label': 'Spread',
                       'description': 'Amplitude of the perturbation (0 = nearest colour of the cell\'s set)'},
        }

    def __init__(self, cell="8x8", colours: int = 2, matrix="4x4", spread: int = 64, shared=(), groups=None):
        self.cell = cell
        self.colours = colours
        self.matrix = matrix
        self.spread = spread
        self.shared = shared
        self.groups = groups

    @classmethod
    def zx_spectrum(cls, matrix="4x4", spread: int = 64):
        """The ZX Spectrum's rule for ZX_SPECTRUM_PALETTE: 8 x 8 cells, two colours of one brightness level (black is in both)."""
        return cls(cell="8x8", colours=2, matrix=matrix, spread=spread, groups=cls.ZX_SPECTRUM_GROUPS)

    def get_current_parameters(self) -> Dict[str, Any]:
        return {'cell': self.cell, 'colours': self.colours, 'matrix': self.matrix, 'spread': self.spread,
                'shared': self.shared, 'groups': self.groups}

    @staticmethod
    def _mask(indices, what):
        try:
            idx = [i for i in indices]
        except TypeError:
            raise ValueError(f"cell-palette {what} must be an iterable of palette indices, not {indices!r}") from None
        mask = 0
        for i in idx:
            if not (isinstance(i, (int, np.integer)) and 0 <= i < 16):
                raise ValueError(f"cell-palette {what} must hold palette indices in 0 .. 15, not {i!r}")
            mask |= 1 << int(i)
        return mask

    def _settings(self):
        """-> ((cw, ch), colours, matrix size, spread, fixed mask, group masks or None)."""
        from . import backend
        cell = self.cell
        if isinstance(cell, str):
            parts = cell.lower().split("x")
            if len(parts) != 2 or not all(p.strip().isdigit() for p in parts):
                raise ValueError(f"cell must be 'WxH' with W, H in {backend.CELL_SIZES}, not {self.cell!r}")
            cell = (int(parts[0]), int(parts[1]))
        try:
            cw, ch = cell
        except (TypeError, ValueError):
            raise ValueError(f"cell must be 'WxH' or a pair with W, H in {backend.CELL_SIZES}, not {self.cell!r}") from None
        if cw not in backend.CELL_SIZES or ch not in backend.CELL_SIZES:
            raise ValueError(f"cell must be 'WxH' or a pair with W, H in {backend.CELL_SIZES}, not {self.cell!r}")
        if not (isinstance(self.colours, (int, np.integer)) and 1 <= self.colours <= backend.CELL_MAX_CHOSEN):
            raise ValueError(f"colours per cell must be an integer in 1 .. {backend.CELL_MAX_CHOSEN}, not {self.colours!r}")
        m = self.matrix
        if isinstance(m, str):
            m = {"2x2": 2, "4x4": 4, "8x8": 8}.get(m)
        if m not in backend.CELL_MATRICES:
            raise ValueError(f"cell-palette matrix must be '2x2', '4x4' or '8x8', not {self.matrix!r}")
        if not (isinstance(self.spread, (int, np.integer)) and 0 <= self.spread <= 255):
            raise ValueError(f"cell-palette spread must be an integer in 0 .. 255, not {self.spread!r}")
        fixed = self._mask(self.shared, "shared")
        groups = None
        if self.groups is not None:
            try:
                groups = [self._mask(g, "groups") for g in self.groups]
            except TypeError:
                raise ValueError(f"cell-palette groups must be an iterable of iterables of indices, not {self.groups!r}") from None
        return (int(cw), int(ch)), int(self.colours), int(m), int(self.spread), fixed, groups

    def _run(self, frames, pal, y0=0, x0=0, out=None, sets=None):
        from . import backend
        if y0 or x0:
            raise ValueError("cell-palette dithering anchors its cells at the frame's first pixel and cannot be tiled by the caller")
        cell, colours, m, spread, fixed, groups = self._settings()
        if pal.K > backend.CELL_MAX_COLOURS:
            raise ValueError(f"cell-palette dithering supports at most {backend.CELL_MAX_COLOURS} colours, the palette has {pal.K}")
        return backend.cells(frames, pal, cell, colours, m, spread, fixed_mask=fixed, groups=groups, out=out, sets=sets)

    def dither(self, pixels: np.ndarray, palette_arr: np.ndarray, image_size: Tuple[int, int]) -> np.ndarray:
        from . import backend
        h, w = image_size
        if h <= 0 or w <= 0:
            raise ValueError(f"cell-palette dithering needs a non-empty image, not {h} x {w}")
        _, colours, _, _, fixed, groups = self._settings()
        if len(palette_arr) > backend.CELL_MAX_COLOURS:
            raise ValueError(f"cell-palette dithering supports at most {backend.CELL_MAX_COLOURS} colours, "
                             f"the palette has {len(palette_arr)}")
        backend._cell_masks(len(palette_arr), colours, fixed, groups)
        out = self._run(_pixels_to_frame(pixels, image_size), _index_palette(palette_arr))
        return _decode(out, palette_arr)

    def dither_frames(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None, return_sets: bool = False):
        """uint8 CUDA tensor [N,H,W,3] (or [H,W,3]) -> dithered uint8 CUDA tensor of the same shape, each frame as
        ImageDitherer(dither_mode=self, palette=palette, use_gamma=use_gamma).apply_dithering would dither it (palette:
        the reference's list of RGB triples).  Frames stay in HBM; `out` may be the frames.  return_sets: -> (frames, sets),
        sets a uint16 CUDA tensor [N, ceil(H/ch), ceil(W/cw)] (or without N): the mask of the entries each cell took."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            pal = _device_palette(*prepare_palette(palette, use_gamma))
            return self._run(frames_u8_cuda, pal, out=out, sets=True if return_sets else None)

    def dither_frames_indexed(self, frames_u8_cuda, palette, use_gamma: bool = False, out=None):
        """dither_frames() as palette-index planes: -> (planes [N,H,W] (or [H,W]), palette_u8 [K,3]) with
        palette_u8[planes] == dither_frames(...); torch.uint8."""
        import torch
        with torch.cuda.device(frames_u8_cuda.device):
            return _indexed(self.dither_frames(frames_u8_cuda, palette, use_gamma), palette, use_gamma, out)


# strategy instances (ImageDitherer(dither_mode=<instance>)) that are per-pixel independent given global coordinates, as
# ORDERED_MODES are among the enum members: these shard by row bands / tiles (sharding.dither_band)
ORDERED_STRATEGIES = (NoDitherStrategy, MatrixDitherStrategy, InterleavedGradientNoiseDitherStrategy, PatternDitherStrategy)
# ... and the strategies that run on a palette with a colour metric (ImageDitherer(metric="oklab")): those whose searches go
# through the palette's top-2 table (backend.ordered in nearest and matrix mode) or its rank table (pattern, dotdiff, idiff)
_METRIC_STRATEGIES = (NoDitherStrategy, MatrixDitherStrategy, PatternDitherStrategy, DotDiffusionDitherStrategy,
                      IntegerErrorDiffusionDitherStrategy)


# ------------------------------------------------------------------------------------- Transparency
# which strategies take an alpha mask: the position-only ones are dithered as always and masked afterwards, the two table
# diffusions run their masked kernels (_run_masked); nothing else does, and nothing falls back to ignoring the mask
_ALPHA_POSITION_STRATEGIES = (NoDitherStrategy, MatrixDitherStrategy, InterleavedGradientNoiseDitherStrategy, PatternDitherStrategy)
_ALPHA_MASKED_STRATEGIES = (IntegerErrorDiffusionDitherStrategy, DotDiffusionDitherStrategy)


class AlphaMode:
    """How the alpha channel of an RGBA source becomes the one-bit transparency of a palettised result
    (include/ditherpie_hip_alpha.h has the integer definitions).  Asked for per call (ImageDitherer.apply_dithering_rgba,
    apply_dithering_indexed_alpha, apply_dithering_png(alpha=...), apply_dithering_frames_alpha): the ditherer itself has no alpha
    setting.

    mode       "threshold": a pixel is transparent where alpha < threshold (0 .. 256); "ordered": the alpha channel is itself
               dithered with the Bayer matrix `matrix` ("2x2", "4x4", "8x8"), so a soft edge becomes a stipple
    matte      None, or the colour the RGB is composited over before dithering: what half-transparent pixels that end up opaque
               are blended with
    fill       the colour bytes under a transparent pixel in the output (palette entry K of the indexed results)
    Transparent pixels take no part: the palette (palette=None) is fitted to the opaque pixels, and the diffusion modes neither
    read their hidden colour nor push error across them.  Not in the reference."""

    MODES = ("threshold", "ordered")
    MATRICES = ("2x2", "4x4", "8x8")

    def __init__(self, mode: str = "threshold", threshold: int = 128, matrix: str = "4x4", matte=None, fill=(0, 0, 0)):
        self.mode = mode
        self.threshold = threshold
        self.matrix = matrix
        self.matte = matte
        self.fill = fill

    def __repr__(self):
        return f"AlphaMode(mode={self.mode!r}, threshold={self.threshold!r}, matrix={self.matrix!r}, matte={self.matte!r}, fill={self.fill!r})"

    def _settings(self):
        """-> (mode, threshold, m, matte or None, fill) checked; ValueError otherwise (no device needed)."""
        if self.mode not in self.MODES:
            raise ValueError(f"alpha mode must be one of {self.MODES}, not {self.mode!r}")
        if isinstance(self.threshold, bool) or not isinstance(self.threshold, (int, np.integer)) or not 0 <= self.threshold <= 256:
            raise ValueError(f"alpha threshold must be an integer in 0 .. 256, not {self.threshold!r}")
        if self.matrix not in self.MATRICES:
            raise ValueError(f"alpha matrix must be one of {self.MATRICES}, not {self.matrix!r}")

        def colour(c, what):
            try:
                t = tuple(int(v) for v in c)
                ok = len(t) == 3 and all(a == b for a, b in zip(t, c)) and all(0 <= v <= 255 for v in t)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"alpha {what} must be three integers in 0 .. 255, not {c!r}")
            return t
        matte = None if self.matte is None else colour(self.matte, "matte")
        return self.mode, int(self.threshold), int(self.matrix.split("x")[0]), matte, colour(self.fill, "fill")


# ------------------------------------------------------------------------------------- ImageDitherer
class ImageDitherer:
    """dithering_lib.py:1877-1992.  Plain attributes only, so instances pickle like the reference's
    (video_processor.py:312-322 ships them to worker processes)."""

    _STRATEGIES = {
        DitherMode.NONE: NoDitherStrategy,
        DitherMode.BAYER: BayerDitherStrategy,
        DitherMode.BLUE_NOISE: BlueNoiseDitherStrategy,
        DitherMode.INTERLEAVED_GRADIENT_NOISE: InterleavedGradientNoiseDitherStrategy,
        DitherMode.ERROR_DIFFUSION: ErrorDiffusionDitherStrategy,
        DitherMode.POLKA_DOT: PolkaDotDitherStrategy,
        DitherMode.PERCEPTUAL: PerceptualDitherStrategy,
        DitherMode.HYBRID: HybridDitherStrategy,
        DitherMode.ADAPTIVE_VARIANCE: AdaptiveVarianceDitherStrategy,
        DitherMode.OSTROMOUKHOV: OstromoukhovDitherStrategy,
        DitherMode.RIEMERSMA: RiemersmaDitherStrategy,
    }

    metric = "rgb"   # (the class default: an object pickled before the attribute existed reads as "rgb")
    palette_fit = "median_cut"   # (likewise: what palette=None meant before the attribute existed)

    def __init__(self, num_colors: int = 16, dither_mode: Optional[DitherMode] = DitherMode.BAYER,
                 palette: Optional[List[Tuple[int, int, int]]] = None, use_gamma: bool = False,
                 dither_params: Optional[Dict[str, Any]] = None, palette_fit: str = "median_cut", metric: str = "rgb"):
        """metric (an addition to the reference's interface): "rgb", the reference's squared Euclidean RGB distance, or "oklab",
        the integer Oklab of include/ditherpie_hip_metric.h -- for NONE, BAYER, BLUE_NOISE, POLKA_DOT, any MatrixDitherStrategy
        instance, PatternDitherStrategy, DotDiffusionDitherStrategy and IntegerErrorDiffusionDitherStrategy; every other mode, and use_gamma=True (Oklab linearises
        by itself), raise ValueError with it.  The strategy-level dither(pixels, palette_arr, size) stays RGB.
        palette_fit (another addition, independent of metric; pass both by keyword): what palette=None means -- "median_cut", the
        reference's RGB median cut of the first frame, or "oklab", ColorReducer.generate_oklab_palette of it (at most 256
        colours; ValueError together with use_gamma=True)."""
        self.num_colors = num_colors
        self.dither_mode = dither_mode
        self.palette = palette
        self.use_gamma = use_gamma
        self.dither_params = dither_params or {}
        self.palette_fit = palette_fit
        self.metric = metric
        self._check_metric(None)
        self._check_palette_fit()

    @staticmethod
    def get_mode_parameters(mode: DitherMode) -> Optional[Dict[str, Any]]:
        """Parameter metadata for the GUI/CLI (dithering_lib.py:1893-1911); None for modes without
        parameters and for the modes this backend does not implement."""
        cls = ImageDitherer._STRATEGIES.get(mode)
        if cls is None or cls in (NoDitherStrategy, PerceptualDitherStrategy):
            return None  # the reference lists no parameters for these modes either
        return cls.get_parameter_info()

    @staticmethod
    def mode_has_parameters(mode: DitherMode) -> bool:
        return ImageDitherer.get_mode_parameters(mode) is not None

    def _get_dither_strategy(self, mode: DitherMode) -> BaseDitherStrategy:
        """Defaults from get_parameter_info() overlaid by dither_params (dithering_lib.py:1918-1950);
        unknown mode -> ValueError, unknown parameter -> TypeError from the constructor.  An addition to the reference's
        interface: a BaseDitherStrategy INSTANCE as the mode is returned as it is (dither_params do not apply to it) --
        how modes without a DitherMode member (PatternDitherStrategy, DotDiffusionDitherStrategy, IntegerErrorDiffusionDitherStrategy,
        CellPaletteDitherStrategy, VoidAndClusterDitherStrategy, HalftoneDitherStrategy, WaveletDitherStrategy) reach every ImageDitherer / VideoProcessor path."""
        if isinstance(mode, BaseDitherStrategy):
            return mode
        if mode in _OUT_OF_SCOPE:
            raise NotImplementedError(
                f"dither mode {mode.value!r} is outside the MI355X backend's scope "
                "(none, bayer, blue_noise, IGN, polka_dot, error_diffusion, riemersma, perceptual, hybrid, "
                "adaptive_variance, ostromoukhov)")
        cls = self._STRATEGIES.get(mode)
        if cls is None:
            raise ValueError(f"Unrecognized DitherMode: {mode}")
        info = cls.get_parameter_info()
        if not info:
            return cls()
        settings = {name: meta["default"] for name, meta in info.items()}
        settings.update(self.dither_params)
        return cls(**settings)

    def _check_metric(self, strategy):
        """The metric of this ditherer, checked against use_gamma and (when given) the strategy: before any launch."""
        metric = self.metric
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
        if metric == "rgb":
            return metric
        if self.use_gamma:
            raise ValueError(f"use_gamma=True cannot be combined with the {metric!r} metric: Oklab linearises by itself")
        if strategy is not None and not isinstance(strategy, _METRIC_STRATEGIES):
            name = self.dither_mode.value if isinstance(self.dither_mode, DitherMode) else type(strategy).__name__
            raise ValueError(f"dither mode {name!r} does not support the {metric!r} metric (supported: none, bayer, blue_noise, "
                             "polka_dot, MatrixDitherStrategy instances, PatternDitherStrategy, DotDiffusionDitherStrategy, "
                             "IntegerErrorDiffusionDitherStrategy)")
        return metric

    def _check_palette_fit(self):
        """How palette=None is fitted, checked against use_gamma: before any launch."""
        fit = self.palette_fit
        if fit not in PALETTE_FITS:
            raise ValueError(f"palette_fit must be one of {PALETTE_FITS}, not {fit!r}")
        if fit == "oklab" and self.use_gamma:
            raise ValueError("use_gamma=True cannot be combined with the 'oklab' palette fit: Oklab linearises by itself")
        return fit

    def _palette_on_device(self, strategy=None):
        metric = self._check_metric(strategy)
        return _device_palette(*prepare_palette(self.palette, self.use_gamma), metric)

    # -- host plumbing ------------------------------------------------------------------------
    def _ensure_palette(self, first_frame_u8: np.ndarray):
        """palette=None: median cut of the (linearised, when gamma is on) image, kept on the object
        (dithering_lib.py:1960-1966); with palette_fit="oklab" the Oklab fit of the image instead."""
        if self.palette is None and self._check_palette_fit() == "oklab":
            from PIL import Image
            self.palette = ColorReducer.generate_oklab_palette(Image.fromarray(first_frame_u8, "RGB"), self.num_colors)
        if self.palette is None:
            from PIL import Image
            src = _tables.LUT_IN[first_frame_u8] if self.use_gamma else first_frame_u8
            self.palette = ColorReducer.reduce_colors(Image.fromarray(src, "RGB"), self.num_colors)

    def apply_dithering_frames(self, frames, y0: int = 0, x0: int = 0, out=None):
        """uint8 CUDA tensor [N,H,W,3] (or [H,W,3]) -> dithered uint8 CUDA tensor of the same shape.
        Frames stay in HBM; (y0, x0) are the global coordinates of each frame's first pixel when the
        frames are row bands / tiles of a larger image (ordered modes only)."""
        if not self.dither_mode:
            self.dither_mode = DitherMode.NONE
        if self.palette is None:
            first = frames if frames.dim() == 3 else frames[0]
            self._ensure_palette(first.cpu().numpy())
        strategy = self._get_dither_strategy(self.dither_mode)
        self._check_metric(strategy)
        import torch
        with torch.cuda.device(frames.device):  # palette, thresholds and launches on the device that holds the frames
            pal = self._palette_on_device(strategy)
            return strategy._run(frames, pal, y0=y0, x0=x0, out=out)

    def apply_dithering_frames_indexed(self, frames, y0: int = 0, x0: int = 0, out=None):
        """apply_dithering_frames() as palette-index planes: uint8 CUDA tensor [N,H,W,3] (or [H,W,3]) -> (planes [N,H,W]
        (or [H,W]), palette_u8 [K,3] numpy) with palette_u8[planes] == apply_dithering_frames(frames).  One byte per
        pixel (torch.uint8) up to 256 colours, two (torch.int16) above.  palette_u8 is the out_colors of
        prepare_palette: under use_gamma the sRGB bytes the RGB output carries, so two entries may be equal; a pixel
        then gets the lowest of the equal indices.  The dither and the index pass run on the same stream, frames stay
        in HBM; `out` receives the planes."""
        import torch
        rgb = self.apply_dithering_frames(frames, y0=y0, x0=x0)
        with torch.cuda.device(frames.device):
            return _indexed(rgb, self.palette, self.use_gamma, out)

    def apply_dithering_indexed(self, image):
        """PIL image -> PIL 'P' image whose palette is the out_colors of this ditherer's palette and whose
        convert("RGB") equals apply_dithering(image): what PNG-8 / GIF are saved from, without Pillow re-quantising an
        image whose indices the GPU already knew.  Host-in as apply_dithering (Pillow's own four-byte layout into the
        pinned buffer); the way back is one byte per pixel -- a 'P' image's own layout -- into a reused pinned buffer,
        copied once into storage the image owns (the staging buffer is overwritten by the next call).  ValueError above
        256 colours (a 'P' image holds 256 entries; apply_dithering_frames_indexed serves those)."""
        import torch
        from PIL import Image
        rgb = image if image.mode == "RGB" else image.convert("RGB")
        w, h = rgb.size
        if self.palette is None:
            self._ensure_palette(np.asarray(rgb))
        if len(self.palette) > 256:
            raise ValueError(f"a 'P' image holds at most 256 colours, the palette has {len(self.palette)}: "
                             "use apply_dithering_frames_indexed")
        pin_in, pin_out = _pinned_pair(h * w * 4)
        if w > 0 and h > 0 and _pil_rgbx_into(rgb, pin_in.numpy()):
            dev_in = pin_in.view(h, w, 4).cuda(non_blocking=True)[..., :3].contiguous()
        else:
            host_in = pin_in[:h * w * 3]
            np.copyto(host_in.numpy(), np.frombuffer(rgb.tobytes(), dtype=np.uint8))
            dev_in = host_in.view(h, w, 3).cuda(non_blocking=True)
        planes, colours = self.apply_dithering_frames_indexed(dev_in)
        host_out = pin_out[:h * w]
        host_out.view(h, w).copy_(planes, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out = Image.frombytes("P", (w, h), host_out.numpy())   # (a copy into the image's own storage)
        out.putpalette(colours.reshape(-1).tolist(), "RGB")
        return out

    # -- transparency (include/ditherpie_hip_alpha.h) ------------------------------------------
    def _alpha_strategy(self):
        """The strategy of this ditherer if it takes a mask, ValueError naming the supported ones otherwise: before any launch."""
        if not self.dither_mode:
            self.dither_mode = DitherMode.NONE
        strategy = self._get_dither_strategy(self.dither_mode)
        if not isinstance(strategy, _ALPHA_POSITION_STRATEGIES + _ALPHA_MASKED_STRATEGIES):
            name = self.dither_mode.value if isinstance(self.dither_mode, DitherMode) else type(strategy).__name__
            raise ValueError(f"dither mode {name!r} does not take an alpha mask (supported: none, bayer, blue_noise, polka_dot, IGN, "
                             "MatrixDitherStrategy instances, PatternDitherStrategy, IntegerErrorDiffusionDitherStrategy, "
                             "DotDiffusionDitherStrategy)")
        self._check_metric(strategy)
        return strategy

    def _dither_alpha(self, frames_rgba, alpha, y0, x0, kernel_fill):
        """-> (dithered rgb [N,H,W,3], mask [N,H,W], colour under the masked pixels of the diffusions).  kernel_fill: None for
        alpha.fill, "first" for the palette's first output colour (the indexed paths: to_indices then meets no missing colour)."""
        import torch
        from . import backend
        if not isinstance(alpha, AlphaMode):
            raise ValueError(f"alpha must be an AlphaMode, not {alpha!r}")
        mode, threshold, m, matte, fill = alpha._settings()
        strategy = self._alpha_strategy()
        if not (isinstance(frames_rgba, torch.Tensor) and frames_rgba.is_cuda and frames_rgba.dtype == torch.uint8
                and frames_rgba.dim() in (3, 4) and frames_rgba.shape[-1] == 4):
            raise ValueError("frames must be a CUDA uint8 tensor [N,H,W,4] or [H,W,4]")
        with torch.cuda.device(frames_rgba.device):
            rgb, mask, _ = backend.alpha_split(frames_rgba, mode, threshold, m, matte, y0 if mode == "ordered" else 0,
                                               x0 if mode == "ordered" else 0)
            if self.palette is None:
                first_rgb, first_mask = (rgb, mask) if rgb.dim() == 3 else (rgb[0], mask[0])
                seen = first_rgb[first_mask == 0]                      # the opaque pixels of the first frame after the matte, raster order
                if seen.shape[0] == 0:
                    raise ValueError("the first frame has no opaque pixel: there is nothing to fit a palette to")
                self._ensure_palette(np.ascontiguousarray(seen.cpu().numpy().reshape(1, -1, 3)))
            pal = self._palette_on_device(strategy)
            if kernel_fill == "first":
                fill = tuple(int(v) for v in prepare_palette(self.palette, self.use_gamma)[1][0])
            if isinstance(strategy, _ALPHA_MASKED_STRATEGIES):
                if y0 or x0:
                    raise ValueError("the diffusion modes hand errors across every edge a caller could cut: no (y0, x0)")
                return strategy._run_masked(rgb, mask, pal, fill), mask, fill
            return strategy._run(rgb, pal, y0=y0, x0=x0), mask, fill

    def apply_dithering_frames_alpha(self, frames_rgba, alpha, y0: int = 0, x0: int = 0):
        """uint8 CUDA tensor [N,H,W,4] (or [H,W,4]) -> (rgb [N,H,W,3] dithered, mask [N,H,W] with 1 at the transparent pixels), both in
        HBM.  The RGB under a transparent pixel is not specified (alpha.fill in the diffusion modes, the dither of the hidden colour
        in the position-only ones): backend.alpha_join(rgb, mask, alpha.fill) makes the RGBA frame.  palette=None is fitted to the
        opaque pixels of the first frame after the matte (ValueError when there is none).  The position-only modes (none, the
        threshold matrices, IGN, PatternDitherStrategy) dither as always and are masked afterwards; IntegerErrorDiffusionDitherStrategy
        and DotDiffusionDitherStrategy run their masked kernels; every other mode is a ValueError before any launch.  (y0, x0): the
        global coordinates of the frames' first pixel, for the position-only modes and the ordered alpha matrix."""
        rgb, mask, _ = self._dither_alpha(frames_rgba, alpha, y0, x0, None)
        return rgb, mask

    def _check_alpha_colours(self):
        if self.palette is not None and len(self.palette) > 255:
            raise ValueError(f"an indexed result with a transparent key holds at most 255 colours, the palette has {len(self.palette)}")

    def apply_dithering_frames_indexed_alpha(self, frames_rgba, alpha, y0: int = 0, x0: int = 0):
        """apply_dithering_frames_alpha() as index planes: -> (planes [N,H,W] uint8, palette_u8 [K + 1, 3] numpy, key) with key = K, the
        index of every transparent pixel, palette_u8[K] = alpha.fill and palette_u8[planes] the RGB result at the opaque pixels.
        ValueError above 255 colours (the key needs an entry of its own, as the GIF / APNG writers' does)."""
        import torch
        from . import backend
        if isinstance(alpha, AlphaMode):
            alpha._settings()
        self._alpha_strategy()
        if self.palette is None and self.num_colors > 255:
            raise ValueError(f"an indexed result with a transparent key holds at most 255 colours, not {self.num_colors}")
        self._check_alpha_colours()
        rgb, mask, _ = self._dither_alpha(frames_rgba, alpha, y0, x0, "first")
        self._check_alpha_colours()
        with torch.cuda.device(rgb.device):
            planes, colours = _indexed(rgb, self.palette, self.use_gamma, None)
            key = colours.shape[0]
            backend.alpha_key(planes, mask, key, out=planes)
        return planes, np.concatenate([colours, np.asarray(alpha.fill, np.uint8).reshape(1, 3)]), key

    @staticmethod
    def _rgba_on_device(image):
        """PIL image -> its pixels as a uint8 CUDA tensor [H,W,4] (an image without an alpha channel is fully opaque): Pillow's raw
        'RGBA' encoder into the pinned four-byte buffer the RGB path uses."""
        rgba = image if image.mode == "RGBA" else image.convert("RGBA")
        w, h = rgba.size
        if w < 1 or h < 1:
            raise ValueError("the image has no pixel")
        pin_in, pin_out = _pinned_pair(h * w * 4)
        if not _pil_rgbx_into(rgba, pin_in.numpy(), "RGBA"):
            np.copyto(pin_in.numpy(), np.frombuffer(rgba.tobytes(), dtype=np.uint8))
        return pin_in.view(h, w, 4).cuda(non_blocking=True), pin_out

    def apply_dithering_rgba(self, image, alpha=None):
        """PIL image (any mode; 'RGBA' is what it is for) -> PIL 'RGBA' image: the dither of the opaque pixels with alpha 255, alpha.fill
        with alpha 0 at the transparent ones (alpha: an AlphaMode, default AlphaMode())."""
        import torch
        from PIL import Image
        from . import backend
        alpha = AlphaMode() if alpha is None else alpha
        dev, pin_out = self._rgba_on_device(image)
        h, w, _ = dev.shape
        rgb, mask = self.apply_dithering_frames_alpha(dev, alpha)
        out = backend.alpha_join(rgb, mask, alpha._settings()[4])
        pin_out.view(h, w, 4).copy_(out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return Image.frombytes("RGBA", (w, h), pin_out.numpy())       # (a copy into the image's own storage)

    def apply_dithering_indexed_alpha(self, image, alpha=None):
        """PIL image -> PIL 'P' image with info["transparency"] = K: entries 0 .. K-1 are the palette's out_colors, entry K is
        alpha.fill and is the index of every transparent pixel; convert("RGBA") equals apply_dithering_rgba(image, alpha)."""
        import torch
        from PIL import Image
        alpha = AlphaMode() if alpha is None else alpha
        dev, pin_out = self._rgba_on_device(image)
        h, w, _ = dev.shape
        planes, colours, key = self.apply_dithering_frames_indexed_alpha(dev, alpha)
        host_out = pin_out[:h * w]
        host_out.view(h, w).copy_(planes, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out = Image.frombytes("P", (w, h), host_out.numpy())
        out.putpalette(colours.reshape(-1).tolist(), "RGB")
        out.info["transparency"] = key
        return out

    def _apply_dithering_png_alpha(self, image, alpha, seg_bytes, blocks, assemble) -> bytes:
        from . import png
        dev, _ = self._rgba_on_device(image)
        planes, colours, key = self.apply_dithering_frames_indexed_alpha(dev, alpha)
        return png.encode_png(planes, colours, seg_bytes, blocks=blocks, assemble=assemble, transparent=key)[0]

    def apply_dithering_png(self, image, seg_bytes=None, blocks="fixed", assemble="host", *, alpha=None) -> bytes:
        """PIL image -> the bytes of a PNG-8 file whose decoding equals apply_dithering(image), exactly.  Host-in as
        apply_dithering_indexed; the index plane never comes back: it is compressed where it lies (png.encode_png: the
        zlib stream on the device, the container and its CRCs in Python) and only the compressed stream crosses to the
        host.  assemble="device": the container and its CRCs on the device as well (png.encode_png).  ValueError above
        256 colours.  alpha=AlphaMode(...) (keyword only): the image's alpha channel is honoured -- a PNG-8 with a tRNS chunk whose
        decoding equals apply_dithering_rgba(image, alpha) (at most 255 colours); without it the alpha channel is dropped as before."""
        from . import png
        if alpha is not None:
            return self._apply_dithering_png_alpha(image, alpha, seg_bytes, blocks, assemble)
        rgb = image if image.mode == "RGB" else image.convert("RGB")
        w, h = rgb.size
        if w < 1 or h < 1:
            raise ValueError("a PNG has at least one pixel")
        if self.palette is None:
            self._ensure_palette(np.asarray(rgb))
        if len(self.palette) > 256:
            raise ValueError(f"a PNG palette holds at most 256 colours, the palette has {len(self.palette)}")
        pin_in, _ = _pinned_pair(h * w * 4)
        if _pil_rgbx_into(rgb, pin_in.numpy()):
            dev_in = pin_in.view(h, w, 4).cuda(non_blocking=True)[..., :3].contiguous()
        else:
            host_in = pin_in[:h * w * 3]
            np.copyto(host_in.numpy(), np.frombuffer(rgb.tobytes(), dtype=np.uint8))
            dev_in = host_in.view(h, w, 3).cuda(non_blocking=True)
        planes, colours = self.apply_dithering_frames_indexed(dev_in)
        return png.encode_png(planes, colours, seg_bytes, blocks=blocks, assemble=assemble)[0]

    def prepare(self, device=None, accel=True):
        """Create the device-side palette now (and, with accel=True, its search accelerator: ~3.5 ms once) instead of on
        first use / once enough pixels have been served -- for long-running jobs (a video) that know what is coming.
        An addition to the reference's interface; nothing is stored on the (picklable) object."""
        import torch
        if self.palette is None:
            raise ValueError("prepare() needs an explicit palette")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(dev):
            pal = self._palette_on_device()
            if accel and pal.metric != "rgb":
                pal.metric_prepare()   # a metric palette's table is its accelerator
            elif accel:
                pal.build_accel()
        return self

    def apply_dithering(self, image):
        """PIL image -> PIL 'RGB' image (dithering_lib.py:1952-1992).  Host <-> device copies go through per-thread pinned
        staging buffers that are reused from call to call (the GUI calls this from worker threads).

        Pillow stores an 'RGB' image as FOUR bytes per pixel; packing it to three (tobytes: encode in 64 KB pieces, join them, and
        here one more copy into the pinned buffer) was the largest part of a call (7.6 ms for a 4K image with a 0.02 ms kernel).  So the host side stays in Pillow's own layout: the raw 'RGBX' encoder -- a row memcpy -- writes straight
        into the pinned buffer (2.0 ms instead of 5.4) and the fourth byte is dropped on the GPU; the result comes back packed
        and is unpacked by Image.fromarray (2.5 ms; see below why not mapped).  tools/bench_scripts/pil_probe2.py, pil_probe3.py.
        If Pillow's encoder interface is not what it has been for a decade, the packed path of rounds 1-4 runs instead."""
        import torch
        from PIL import Image
        rgb = image if image.mode == "RGB" else image.convert("RGB")
        w, h = rgb.size
        if self.palette is None:
            self._ensure_palette(np.asarray(rgb))
        n4 = h * w * 4
        pin_in, pin_out = _pinned_pair(n4)
        if w > 0 and h > 0 and _pil_rgbx_into(rgb, pin_in.numpy()):
            dev4 = pin_in.view(h, w, 4).cuda(non_blocking=True)
            dev_out = self.apply_dithering_frames(dev4[..., :3].contiguous())
            out3 = pin_out[:h * w * 3]
            out3.view(h, w, 3).copy_(dev_out.view(h, w, 3), non_blocking=True)
            torch.cuda.current_stream().synchronize()
            # The way back stays packed: an image mapped onto a four-byte buffer carries the raw mode's name ('RGBX'), and
            # convert('RGB') from it is a per-pixel loop (3.5 ms) -- slower than unpacking packed RGB into storage of the image's
            # own (2.5 ms), which also makes the image own its pixels (the staging buffer is overwritten by the next call;
            # tests/test_cabi_and_host.py checks that).  tools/bench_scripts/pil_probe3.py
            return Image.fromarray(out3.numpy().reshape(h, w, 3), "RGB")
        pin_in, pin_out = _pinned_pair(h * w * 3)
        host_in = pin_in.numpy().reshape(h, w, 3)
        np.copyto(host_in.reshape(-1), np.frombuffer(rgb.tobytes(), dtype=np.uint8))
        dev_in = pin_in.view(h, w, 3).cuda(non_blocking=True)
        dev_out = self.apply_dithering_frames(dev_in)
        pin_out.view(h, w, 3).copy_(dev_out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return Image.fromarray(pin_out.numpy().reshape(h, w, 3), "RGB")
