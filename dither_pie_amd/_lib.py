"""ctypes binding of libditherpie_hip.so (C ABI: include/ditherpie_hip.h).

The library is the product: there is no CPU fallback.  If the shared object is missing or a
call fails, a DitherPieError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# Two builds of the same sources (csrc/Makefile): libditherpie_hip.so -- the product, which reads no environment variable --
# and libditherpie_hip_exp.so (-DDP_EXPERIMENTS), in which the DP_* switches that force a table / kernel / schedule are
# compiled in.  The product library is what load() returns unless DITHER_PIE_EXPERIMENTS=1 is set (tools/bench_scripts) or
# select(True) was called (the `switches` fixture of tests/conftest.py: only the tests that set a DP_* switch run on the
# twin; every other test, golden and fuzzer runs on the library that ships).
# DP_LIB_PATH: another build altogether (A/B measurements of kernel variants: tools/bench_scripts/ab_kernel.py)
PRODUCT_PATH = os.path.join(_HERE, "libditherpie_hip.so")
EXPERIMENTS_PATH = os.path.join(_HERE, "libditherpie_hip_exp.so")
EXPERIMENTS = os.environ.get("DITHER_PIE_EXPERIMENTS", "") not in ("", "0")
LIB_PATH = os.environ.get("DP_LIB_PATH") or (EXPERIMENTS_PATH if EXPERIMENTS else PRODUCT_PATH)
CSRC = os.path.join(_HERE, "csrc")
# the ABI revision this binding was written against (include/ditherpie_hip.h: DP_ABI_VERSION); load() refuses a library
# that reports another one -- a stale build bound through DP_LIB_PATH would otherwise read K as a pointer
ABI_VERSION = 103

DP_OK, DP_EINVAL, DP_EUNSUPPORTED, DP_EHIP, DP_ENOMEM, DP_EWORKSPACE = range(6)
DP_MAX_COLORS = 1024
MODE_NEAREST, MODE_MATRIX, MODE_IGN = 0, 1, 2


class DitherPieError(RuntimeError):
    """A libditherpie_hip call failed (the message is dp_last_error())."""

    def __init__(self, code, msg):
        super().__init__(f"libditherpie_hip error {code}: {msg}")
        self.code = code


_lock = threading.Lock()
_lib = None
_loaded = {}   # path -> CDLL (both builds may be mapped in one process; their device records have the same layout)

_vp, _i, _i64, _sz, _f = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float
_SIGS = {
    "dp_version": (C.c_int, []),
    "dp_last_error": (C.c_char_p, []),
    "dp_device_info": (_i, [C.POINTER(C.c_int), C.c_char_p, _sz]),
    "dp_palette_create": (_i, [_vp, _vp, _i, _vp, C.POINTER(_vp)]),
    "dp_palette_destroy": (None, [_vp]),
    "dp_palette_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "dp_palette_build_accel": (_i, [_vp]),
    "dp_palette_accel_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "dp_kdtree_build_host": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i)]),
    "dp_thresholds_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "dp_thresholds_blue_noise": (_i, [_i, C.c_uint32, _vp, C.POINTER(_vp)]),
    "dp_thresholds_shape": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "dp_thresholds_download": (_i, [_vp, _vp]),
    "dp_thresholds_destroy": (None, [_vp]),
    "dp_ign_thresholds": (_i, [_vp, _i, _i, _i, _i, _f, _i, _vp]),
    "dp_ordered_workspace_bytes": (_sz, [_i64, _i, _i]),
    "dp_ordered_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _i, _vp, _f, _i, _vp, _sz, _vp]),
    "dp_error_diffusion_workspace_bytes": (_sz, [_i64, _i, _i]),
    "dp_error_diffusion_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "dp_error_diffusion_numba_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, C.c_double, _i, _i, _vp, _sz, _vp]),
    "dp_hybrid_numba_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, C.c_double, C.c_double, _vp, _sz, _vp]),
    "dp_variable_diffusion_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i, _f, _f, _i, _vp, _vp, _vp, _sz, _vp]),
    "dp_riemersma_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp]),
    "dp_halftone_workspace_bytes": (_sz, [_i64, _i, _i, _vp]),
    "dp_halftone_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dp_halftone_pow_flags": (_i, [_i, _i, _vp, _vp, _i64, _vp, _vp]),
    "dp_wavelet_uniforms_needed": (_i64, [_i, _i, _i]),
    "dp_wavelet_workspace_bytes": (_sz, [_i64, _i, _i, _vp]),
    "dp_wavelet_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dp_variance_gate_workspace_bytes": (_sz, [_i64, _i, _i]),
    "dp_variance_gate_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _f, _i, _vp, _sz, _vp]),
    "dp_kmeans_step_u8": (_i, [_vp, _i64, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "dp_kmeans_hist_bytes": (_sz, []),
    "dp_kmeans_hist_workspace_bytes": (_sz, [_i64]),
    "dp_kmeans_hist_build_u8": (_i, [_vp, _i64, _vp, _i, _vp, _sz, _vp]),
    "dp_kmeans_hist_step": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "dp_kmeans_hist_iterate": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, C.c_double, _i, _i, _vp]),
    "dp_kmeans_update": (_i, [_vp, _vp, _vp, _vp, _i, C.c_double, _i, _vp]),
    "dp_kmeans_plusplus_u8": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "dp_resize_nearest_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp]),
    "dp_distinct_first_workspace_bytes": (_sz, [_i64]),
    "dp_distinct_first_u8": (_i, [_vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "dp_pyset_order_host": (_i, [_vp, _i64, _vp, C.POINTER(_i64)]),
    "dp_median_cut_host": (_i, [_vp, _i64, _i, _vp, C.POINTER(_i)]),
    "dp_profile_enable": (_i, [_i]),
    "dp_profile_read": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i64)]),
}
EXPORTS = tuple(_SIGS)
# include/ditherpie_hip_indexed.h: the indexed-output extension (index planes beside packed RGB).  A table of its own
# because the suite pins EXPORTS to the functions of ditherpie_hip.h; load() resolves both.
_SIGS_INDEXED = {
    "dp_index_map_create": (_i, [_vp, _i, C.POINTER(_vp)]),
    "dp_index_map_destroy": (None, [_vp]),
    "dp_index_map_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "dp_index_from_rgb_u8": (_i, [_vp, _vp, _i64, _vp, _i, _vp, _vp]),
    "dp_rgb_from_index_u8": (_i, [_vp, _vp, _i64, _vp, _i, _vp, _vp]),
    "dp_resize_nearest_plane_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _vp]),
}
EXPORTS_INDEXED = tuple(_SIGS_INDEXED)
# include/ditherpie_hip_clip.h: clip-wide palettes (distinct colours over a stream of buffers, rank sample of a histogram);
# a table of its own for the same reason.
_SIGS_CLIP = {
    "dp_distinct_stream_state_bytes": (_sz, []),
    "dp_distinct_stream_workspace_bytes": (_sz, [_i64]),
    "dp_distinct_stream_reset": (_i, [_vp, _vp, _vp]),
    "dp_distinct_stream_add_u8": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dp_hist_sample_workspace_bytes": (_sz, []),
    "dp_hist_sample_u8": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
}
EXPORTS_CLIP = tuple(_SIGS_CLIP)
# include/ditherpie_hip_scene.h: scene-cut detection (frame signatures and their distances); a table of its own for the same
# reason.
_SIGS_SCENE = {
    "dp_frame_signatures_u8": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "dp_signature_distances": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
}
EXPORTS_SCENE = tuple(_SIGS_SCENE)
# include/ditherpie_hip_gif.h: animated GIF output (inter-frame deltas, LZW image data on the device and its host statement);
# a table of its own for the same reason.
_SIGS_GIF = {
    "dp_index_delta_u8": (_i, [_vp, _i, _i64, _vp, _i, _i, _vp, _vp, _vp]),
    "dp_gif_lzw_bound_bytes": (_sz, [_i, _i, _i64]),
    "dp_gif_lzw_workspace_bytes": (_sz, [_i, _i, _i, _i64]),
    "dp_gif_lzw_encode_u8": (_i, [_vp, _i, _i, _i, _i, _i64, _vp, _i64, _vp, _vp, _sz, _vp]),
    "dp_gif_lzw_host_u8": (_i, [_vp, _i, _i, _i, _i, _i64, _vp, _i64, _vp]),
}
EXPORTS_GIF = tuple(_SIGS_GIF)
# include/ditherpie_hip_png.h: PNG-8 output (the zlib stream of index planes on the device and its host statement); a table
# of its own for the same reason.
_SIGS_PNG = {
    "dp_png_filtered_bytes": (_sz, [_i, _i, _i]),
    "dp_png_deflate_bound_bytes": (_sz, [_i, _i, _i, _i]),
    "dp_png_deflate_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "dp_png_deflate_encode_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _sz, _vp]),
    "dp_png_deflate_host_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
}
EXPORTS_PNG = tuple(_SIGS_PNG)
# include/ditherpie_hip_png_dyn.h: dynamic-Huffman blocks for the PNG-8 output and the code construction on its own; a table of
# its own for the same reason.
_SIGS_PNG_DYN = {
    "dp_png_deflate_dyn_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "dp_png_deflate_dyn_encode_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _sz, _vp]),
    "dp_png_deflate_dyn_host_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i64, _vp]),
    "dp_png_code_lengths_u8": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "dp_png_code_lengths_host": (_i, [_vp, _i, _i, _i, _vp]),
}
EXPORTS_PNG_DYN = tuple(_SIGS_PNG_DYN)
# include/ditherpie_hip_pattern.h: pattern (Knoll) dithering and its per-palette search table; a table of its own for the
# same reason.
_SIGS_PATTERN = {
    "dp_pattern_prepare": (_i, [_vp]),
    "dp_pattern_table_bytes": (_sz, [_vp]),
    "dp_pattern_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _i, _i, _vp]),
}
EXPORTS_PATTERN = tuple(_SIGS_PATTERN)
# include/ditherpie_hip_png_file.h: CRC-32 on the device and finished IDAT / fdAT chunks packed back to back (what png.py's
# assemble="device" and apng.py are built on), with their host statements; a table of its own for the same reason.
_u32 = C.c_uint32
_SIGS_PNG_FILE = {
    "dp_png_crc32_workspace_bytes": (_sz, [_i, _i64]),
    "dp_png_crc32_u8": (_i, [_vp, _i64, _vp, _i, _vp, _vp, _sz, _vp]),
    "dp_png_crc32_host_u8": (_i, [_vp, _i64, _vp, _i, _vp]),
    "dp_png_crc32_combine_host": (_u32, [_u32, _u32, _i64]),
    "dp_png_file_bound_bytes": (_sz, [_i64, _i, _i]),
    "dp_png_file_workspace_bytes": (_sz, [_i, _i64]),
    "dp_png_file_assemble_u8": (_i, [_vp, _i64, _vp, _i, _i, _u32, _u32, _vp, _i64, _i, _vp, _i, _vp, _sz, _vp, _vp, _sz, _vp]),
    "dp_png_file_assemble_host_u8": (_i, [_vp, _i64, _vp, _i, _i, _u32, _u32, _vp, _i64, _i, _vp, _i, _vp, _sz, _vp]),
}
EXPORTS_PNG_FILE = tuple(_SIGS_PNG_FILE)
# include/ditherpie_hip_dotdiff.h: dot diffusion (error diffusion in class-matrix order, tiled); a table of its own for the
# same reason.
_SIGS_DOTDIFF = {
    "dp_dotdiff_reach": (_i, [_vp, _i]),
    "dp_dotdiff_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _i, _i, _vp]),
}
EXPORTS_DOTDIFF = tuple(_SIGS_DOTDIFF)
# include/ditherpie_hip_cells.h: cell-palette dithering (k colours per cell, every allowed set searched); a table of its own
# for the same reason.
_SIGS_CELLS = {
    "dp_cells_candidates": (_i, [_i, _i, _u32, _vp, _i]),
    "dp_cells_u8": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _i, _i, _i, _u32, _vp, _i, _i, _i, _vp]),
}
EXPORTS_CELLS = tuple(_SIGS_CELLS)
# include/ditherpie_hip_voidcluster.h: void-and-cluster rank matrices (blue-noise masks that tile, generated on the device)
# and the thresholds made of one; a table of its own for the same reason.
_SIGS_VOIDCLUSTER = {
    "dp_void_cluster_u16": (_i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    "dp_void_cluster_host": (_i, [_vp, _i, _i, _u32, _i]),
    "dp_thresholds_void_cluster": (_i, [_i, _i, _u32, _i, _vp, C.POINTER(_vp)]),
}
EXPORTS_VOIDCLUSTER = tuple(_SIGS_VOIDCLUSTER)
# include/ditherpie_hip_metric.h: palettes with a colour metric (an integer Oklab), their top-2 table, ordered dithering
# through it and the host statements; a table of its own for the same reason.
METRIC_RGB, METRIC_OKLAB = 0, 1
_SIGS_METRIC = {
    "dp_palette_create_metric": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "dp_palette_metric": (_i, [_vp]),
    "dp_metric_prepare": (_i, [_vp]),
    "dp_metric_table_bytes": (_sz, [_vp]),
    "dp_metric_ordered_u8": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "dp_metric_lab_u8": (_i, [_vp, _vp, _i64, _vp]),
    "dp_metric_lab_host": (_i, [_vp, _i64, _vp]),
    "dp_metric_top2_host": (_i, [_vp, _i64, _vp, _i, _i, _vp, _vp]),
}
EXPORTS_METRIC = tuple(_SIGS_METRIC)
# include/ditherpie_hip_idiff.h: integer error diffusion (the classical scans in sixteenths, searched through the palette's
# nearest table under either metric); a table of its own for the same reason.
_SIGS_IDIFF = {
    "dp_idiff_workspace_bytes": (_sz, [_i64, _i, _i]),
    "dp_idiff_u8": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
}
EXPORTS_IDIFF = tuple(_SIGS_IDIFF)
# include/ditherpie_hip_okfit.h: palettes fitted in the integer Oklab (point records of a colour histogram, the weighted k-means
# over them and its host statement); a table of its own for the same reason.
OKFIT_MAX_COLORS, OKFIT_MAX_ITER, OKFIT_MAX_POINTS, OKFIT_POINT_BYTES = 256, 10000, 1 << 24, 16
_SIGS_OKFIT = {
    "dp_okfit_hist_workspace_bytes": (_sz, []),
    "dp_okfit_hist_count": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "dp_okfit_hist_points": (_i, [_vp, _vp, _i64, _vp, _vp, _sz, _vp]),
    "dp_okfit_points_u32": (_i, [_vp, _vp, _i64, _vp, _vp]),
    "dp_okfit_workspace_bytes": (_sz, [_i64, _i]),
    "dp_okfit_fit": (_i, [_vp, _i64, _i, _i, _vp, _vp, _vp, C.POINTER(_i), _vp, _sz, _vp]),
    "dp_okfit_host": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, C.POINTER(_i), C.POINTER(C.c_uint64)]),
}
EXPORTS_OKFIT = tuple(_SIGS_OKFIT)
# include/ditherpie_hip_resample.h: filtered resize (Pillow's BOX / BILINEAR / HAMMING / BICUBIC / LANCZOS, bit for bit) and its
# host statement; a table of its own for the same reason.  dp_resample_u8 takes its arguments, the stream among them, in a
# descriptor whose first field is its own size.
RESAMPLE_FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")   # DP_RESAMPLE_* order
RESAMPLE_MAX_SIZE = 16384


class ResampleArgs(C.Structure):
    """dp_resample_args"""
    _fields_ = [("struct_size", C.c_size_t), ("in_dev", C.c_void_p), ("out_dev", C.c_void_p), ("n_frames", C.c_int64),
                ("plan", C.c_void_p), ("workspace_dev", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


_SIGS_RESAMPLE = {
    "dp_resample_plan_create": (_i, [_i, _i, _i, _i, _i, C.POINTER(_vp)]),
    "dp_resample_plan_destroy": (None, [_vp]),
    "dp_resample_workspace_bytes": (_sz, [_vp, _i64]),
    "dp_resample_u8": (_i, [C.POINTER(ResampleArgs)]),
    "dp_resample_host": (_i, [_i, _vp, _vp, _i64, _i, _i, _i, _i]),
}
EXPORTS_RESAMPLE = tuple(_SIGS_RESAMPLE)
# include/ditherpie_hip_hold.h: the temporal hold for video (cells whose source has not moved keep their indices) and its host
# statement; a table of its own for the same reason.  dp_hold_u8 and dp_hold_host_u8 take a descriptor, as dp_resample_u8 does.
HOLD_CELLS = (1, 2, 4, 8, 16)
HOLD_MAX_FRAMES = 65535     # DP_HOLD_MAX_FRAMES: frames per call


class HoldArgs(C.Structure):
    """dp_hold_args"""
    _fields_ = [("struct_size", C.c_size_t), ("src_dev", C.c_void_p), ("planes_dev", C.c_void_p), ("n_frames", C.c_int64),
                ("h", C.c_int), ("w", C.c_int), ("cell", C.c_int), ("tol", C.c_int), ("share256", C.c_int),
                ("anchor_dev", C.c_void_p), ("held_dev", C.c_void_p), ("has_state", C.c_int), ("out_dev", C.c_void_p),
                ("refreshed_dev", C.c_void_p), ("stream", C.c_void_p)]


_SIGS_HOLD = {
    "dp_hold_u8": (_i, [C.POINTER(HoldArgs)]),
    "dp_hold_host_u8": (_i, [C.POINTER(HoldArgs)]),
    "dp_hold_state_bytes": (_i, [_i, _i, C.POINTER(_sz), C.POINTER(_sz)]),
}
EXPORTS_HOLD = tuple(_SIGS_HOLD)
# include/ditherpie_hip_alpha.h: transparency (RGBA split, key index, RGBA join and their host statements; the masked integer
# error diffusion and the masked dot diffusion); a table of its own for the same reason.  Every entry point takes a descriptor.
ALPHA_MODES = ("threshold", "ordered")   # DP_ALPHA_THRESHOLD, DP_ALPHA_ORDERED
ALPHA_MATRICES = (2, 4, 8)
ALPHA_MAX_FRAMES = 65535                 # DP_ALPHA_MAX_FRAMES: frames per call of split, key and join
ALPHA_MAX_ORIGIN = 1 << 30               # DP_ALPHA_MAX_ORIGIN
_rgb3 = C.c_uint8 * 3


class AlphaSplitArgs(C.Structure):
    """dp_alpha_split_args"""
    _fields_ = [("struct_size", C.c_size_t), ("rgba_dev", C.c_void_p), ("n_frames", C.c_int64), ("h", C.c_int), ("w", C.c_int),
                ("mode", C.c_int), ("threshold", C.c_int), ("m", C.c_int), ("y0", C.c_int), ("x0", C.c_int), ("has_matte", C.c_int),
                ("matte", _rgb3), ("rgb_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("masked_dev", C.c_void_p), ("stream", C.c_void_p)]


class AlphaKeyArgs(C.Structure):
    """dp_alpha_key_args"""
    _fields_ = [("struct_size", C.c_size_t), ("planes_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("n_frames", C.c_int64), ("h", C.c_int),
                ("w", C.c_int), ("key", C.c_int), ("out_dev", C.c_void_p), ("stream", C.c_void_p)]


class AlphaJoinArgs(C.Structure):
    """dp_alpha_join_args"""
    _fields_ = [("struct_size", C.c_size_t), ("rgb_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("n_frames", C.c_int64), ("h", C.c_int),
                ("w", C.c_int), ("fill", _rgb3), ("rgba_dev", C.c_void_p), ("stream", C.c_void_p)]


class AlphaIdiffArgs(C.Structure):
    """dp_alpha_idiff_args"""
    _fields_ = [("struct_size", C.c_size_t), ("in_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("out_dev", C.c_void_p), ("n_frames", C.c_int64),
                ("h", C.c_int), ("w", C.c_int), ("pal", C.c_void_p), ("dx", C.c_void_p), ("dy", C.c_void_p), ("weight", C.c_void_p),
                ("n_taps", C.c_int), ("divisor", C.c_int), ("strength256", C.c_int), ("fill", _rgb3), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class AlphaDotdiffArgs(C.Structure):
    """dp_alpha_dotdiff_args"""
    _fields_ = [("struct_size", C.c_size_t), ("in_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("out_dev", C.c_void_p), ("n_frames", C.c_int64),
                ("h", C.c_int), ("w", C.c_int), ("pal", C.c_void_p), ("classes_host", C.c_void_p), ("m", C.c_int), ("strength256", C.c_int),
                ("fill", _rgb3), ("stream", C.c_void_p)]


_SIGS_ALPHA = {
    "dp_alpha_split_u8": (_i, [C.POINTER(AlphaSplitArgs)]),
    "dp_alpha_split_host_u8": (_i, [C.POINTER(AlphaSplitArgs)]),
    "dp_alpha_key_u8": (_i, [C.POINTER(AlphaKeyArgs)]),
    "dp_alpha_key_host_u8": (_i, [C.POINTER(AlphaKeyArgs)]),
    "dp_alpha_join_u8": (_i, [C.POINTER(AlphaJoinArgs)]),
    "dp_alpha_join_host_u8": (_i, [C.POINTER(AlphaJoinArgs)]),
    "dp_alpha_idiff_u8": (_i, [C.POINTER(AlphaIdiffArgs)]),
    "dp_alpha_dotdiff_u8": (_i, [C.POINTER(AlphaDotdiffArgs)]),
}
EXPORTS_ALPHA = tuple(_SIGS_ALPHA)


def build(force=False):
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC])
    return LIB_PATH


def load():
    """Return the loaded library; raises DitherPieError when it is not built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise DitherPieError(-1, f"{LIB_PATH} is missing: build it with "
                                         f"`make -C {CSRC}` (or dither_pie_amd.build()); there is no CPU fallback")
            # The library shares the process's HIP runtime with PyTorch (device memory and streams are torch's).
            # torch ships its own libamdhip64: import it first so that ours binds to that copy -- loading the
            # system runtime before torch's leaves two runtimes in the process and this one without a device.
            try:
                import torch  # noqa: F401
            except ImportError:  # host-only use (dp_kdtree_build_host, symbol checks)
                pass
            L = _loaded.get(LIB_PATH)
            if L is None:
                L = C.CDLL(LIB_PATH)
                # the version first, bound alone: a stale library may lack entry points of _SIGS altogether, and the
                # message a user needs is "rebuild it", not an AttributeError out of the signature loop
                try:
                    ver = L.dp_version
                except AttributeError:
                    raise DitherPieError(-1, f"{LIB_PATH} exports no dp_version: not a libditherpie_hip build; rebuild it "
                                             f"with `make -C {CSRC}`") from None
                ver.restype, ver.argtypes = C.c_int, []
                got = ver()
                if got != ABI_VERSION:
                    raise DitherPieError(-1, f"{LIB_PATH} reports ABI version {got}, this binding was written for "
                                             f"{ABI_VERSION}: rebuild it with `make -C {CSRC}`")
                for name, (res, args) in (list(_SIGS.items()) + list(_SIGS_INDEXED.items()) + list(_SIGS_CLIP.items())
                                          + list(_SIGS_SCENE.items()) + list(_SIGS_GIF.items()) + list(_SIGS_PNG.items())
                                          + list(_SIGS_PNG_DYN.items()) + list(_SIGS_PATTERN.items())
                                          + list(_SIGS_PNG_FILE.items()) + list(_SIGS_DOTDIFF.items())
                                          + list(_SIGS_CELLS.items()) + list(_SIGS_VOIDCLUSTER.items())
                                          + list(_SIGS_METRIC.items()) + list(_SIGS_IDIFF.items())
                                          + list(_SIGS_OKFIT.items()) + list(_SIGS_RESAMPLE.items())
                                          + list(_SIGS_HOLD.items()) + list(_SIGS_ALPHA.items())):
                    try:
                        fn = getattr(L, name)
                    except AttributeError:
                        raise DitherPieError(-1, f"{LIB_PATH} (ABI {got}) does not export {name}: rebuild it with "
                                                 f"`make -C {CSRC}`") from None
                    fn.restype = res
                    fn.argtypes = args
                _loaded[LIB_PATH] = L
            _lib = L
    return _lib


def select(experiments):
    """Make load() return the product library (False) or its -DDP_EXPERIMENTS twin (True) from now on; returns the previous
    choice.  Device objects (palettes, thresholds) made through one library must not be handed to the other: callers drop
    their caches (dithering_lib.drop_device_caches) around a switch.  Test infrastructure; the product never calls it."""
    global _lib, EXPERIMENTS, LIB_PATH
    with _lock:
        prev = EXPERIMENTS
        EXPERIMENTS = bool(experiments)
        LIB_PATH = EXPERIMENTS_PATH if EXPERIMENTS else PRODUCT_PATH
        _lib = None
    return prev


def check(rc):
    if rc != DP_OK:
        msg = load().dp_last_error()
        raise DitherPieError(rc, msg.decode("utf-8", "replace") if msg else "unknown error")


def device_info():
    n = C.c_int(0)
    buf = C.create_string_buffer(128)
    check(load().dp_device_info(C.byref(n), buf, 128))
    return n.value, buf.value.decode()
