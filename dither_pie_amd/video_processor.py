"""Drop-in counterpart of dither_pie's `video_processor` for the frame path, on MI355X.

Same public names and call signatures as the reference module (video_processor.py:27-46, 98, 172-178,
393-475, 547-577).  What changes is where frames are processed: the reference forks a
multiprocessing.Pool of <= 4 workers per 15-frame batch and pickles the ditherer into each
(video_processor.py:304-346); a HIP context must not cross fork(), and frames are independent, so here
frames are processed IN PROCESS in batches that stay resident in HBM between the stages
(NEAREST down-scale -> dither -> NEAREST up-scale, all through libditherpie_hip.so).
ffmpeg/ffprobe remain external subprocesses as in the reference (same libx264 re-encode with audio/subtitle
copy), but frames travel as rawvideo rgb24 through pipes into pinned host buffers instead of PNG files on
disk (PNG encode/decode dominates a processed frame in the reference); the PNG-file
exchange of the reference remains available (`use_pipes=False`).  Both keep the reference's failure policy
(video_processor.py:325-336, 53-96): a batch that fails is retried frame by frame (three attempts each), a frame that
still fails is replaced by the nearest good output frame (the previous one first) and the video goes on; the call
returns False only when ffmpeg fails or no frame could be processed.  progress_callback(fraction, message) gets the
same milestones (0.0, 0.05, 0.1 ... 0.9, 1.0).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile
from multiprocessing import cpu_count
from pathlib import Path
from typing import Callable, Optional, Tuple

import numpy as np
from PIL import Image

from .dithering_lib import ImageDitherer, PixelizeMethod

__all__ = ["VideoProcessor", "pixelize_regular", "NeuralPixelizer", "process_frames", "process_frames_indexed"]


def _even_dimensions(orig_w: int, orig_h: int, max_size: int) -> Tuple[int, int]:
    """video_processor.py:547-560: the smaller side becomes max_size (made even), the other keeps the
    aspect ratio, rounded and made even."""
    small = max_size if max_size % 2 == 0 else max_size - 1
    if orig_w >= orig_h:
        other = int(round((orig_w / orig_h) * small))
        return other + (other % 2), small
    other = int(round((orig_h / orig_w) * small))
    return small, other + (other % 2)


class NeuralPixelizer:
    """The GAN pixelizer (video_processor.py:478-545) is a separate model-inference workload whose
    weights are not part of the repository; only the dimension helper is provided."""

    _compute_even_dimensions = staticmethod(_even_dimensions)

    def __init__(self, *a, **k):
        raise NotImplementedError("neural pixelization is outside the MI355X backend's scope")


def _downscale_filter(name) -> str:
    """The `resample` / `downscale_filter` keyword: ValueError (listing the accepted names) for anything else."""
    from . import backend
    return backend._resample_filter(name)


def _downscale(x, th: int, tw: int, downscale_filter: str):
    """The pixelization down-scale of frames in HBM: NEAREST as in the reference, or one of Pillow's averaging filters
    (backend.resample: bit-identical to Image.resize)."""
    from . import backend
    if downscale_filter == "nearest":
        return backend.resize_nearest(x, th, tw)
    return backend.resample(x, th, tw, downscale_filter)


def pixelize_regular(image: Image.Image, max_size: int, resample: str = "nearest") -> Image.Image:
    """Down-scale to even dimensions (video_processor.py:563-577), on the GPU: NEAREST as in the reference, or with
    resample = "box", "bilinear", "hamming", "bicubic" or "lanczos" what image.resize gives with that filter."""
    import torch
    resample = _downscale_filter(resample)
    tw, th = _even_dimensions(image.size[0], image.size[1], max_size)
    arr = np.array(image.convert("RGB"), dtype=np.uint8)
    out = _downscale(torch.from_numpy(arr).cuda(), th, tw, resample)
    return Image.fromarray(out.cpu().numpy(), "RGB")


def _final_size(w: int, h: int, multiplier: int) -> Tuple[int, int]:
    """video_processor.py:408-415: integer multiple, bumped to even for yuv420p."""
    nw, nh = w * multiplier, h * multiplier
    return nw + (nw % 2), nh + (nh % 2)


def output_size(h: int, w: int, pixelize_method: Optional[str] = None, max_size: int = 64,
                final_resize_multiplier: Optional[int] = None) -> Tuple[int, int]:
    """(H', W') of process_frames() for frames of h x w: the geometry of video_processor.py:423-475 without running it."""
    if pixelize_method in (PixelizeMethod.REGULAR.value, "regular"):
        w, h = _even_dimensions(w, h, max_size)
    if final_resize_multiplier:
        w, h = _final_size(w, h, final_resize_multiplier)
    return h, w


def _apply_final_resize_to_frame(image: Image.Image, multiplier: int) -> Image.Image:
    """video_processor.py:393-420"""
    import torch
    from . import backend
    nw, nh = _final_size(image.size[0], image.size[1], multiplier)
    arr = np.array(image.convert("RGB"), dtype=np.uint8)
    out = backend.resize_nearest(torch.from_numpy(arr).cuda(), nh, nw)
    return Image.fromarray(out.cpu().numpy(), "RGB")


def process_frames(frames, ditherer: ImageDitherer, pixelize_method: Optional[str] = None, max_size: int = 64,
                   final_resize_multiplier: Optional[int] = None, downscale_filter: str = "nearest"):
    """The per-frame pipeline of _process_single_frame (video_processor.py:423-475) for a batch of
    equally sized frames resident in HBM: uint8 CUDA tensor [N,H,W,3] -> uint8 CUDA tensor [N,H',W',3].
    downscale_filter: the filter of the pixelization down-scale ("nearest": the reference's; "box" ... "lanczos": Pillow's
    averaging filters, backend.resample).  The final up-scale stays NEAREST: a pixel-art enlargement must not blur."""
    from . import backend
    downscale_filter = _downscale_filter(downscale_filter)
    if pixelize_method in (PixelizeMethod.NEURAL.value, "neural"):
        raise NotImplementedError("neural pixelization is outside the MI355X backend's scope")
    x = frames
    if pixelize_method in (PixelizeMethod.REGULAR.value, "regular"):
        tw, th = _even_dimensions(x.shape[2], x.shape[1], max_size)
        x = _downscale(x, th, tw, downscale_filter)
    x = ditherer.apply_dithering_frames(x)
    if final_resize_multiplier:
        nw, nh = _final_size(x.shape[2], x.shape[1], final_resize_multiplier)
        x = backend.resize_nearest(x, nh, nw)
    return x


def process_frames_indexed(frames, ditherer: ImageDitherer, pixelize_method: Optional[str] = None, max_size: int = 64,
                           final_resize_multiplier: Optional[int] = None, hold=None, downscale_filter: str = "nearest"):
    """process_frames() as palette-index planes: uint8 CUDA tensor [N,H,W,3] -> (planes [N,H',W'], palette_u8 [K,3]) with
    palette_u8[planes] == process_frames(...).  The final up-scale runs on the index plane (the same NEAREST coordinates),
    so the index pass looks up the small frames only.  downscale_filter: as for process_frames.
    hold (an addition, in front of downscale_filter, which stays the last parameter: pass both by keyword; None leaves every byte
    as it was): a backend.HoldStream, or the settings (cell, tol, share) of a new one that lives for this call.  The temporal hold then runs on the small planes, between the dither and the final up-scale, with
    the frames as handed to the ditherer as its source: cells whose source has not moved keep the indices of an earlier frame, so
    the planes are no longer process_frames() of each frame on its own.  The stream is reset() when the palette is not the one
    its indices belong to (a palette fitted per call); two-byte planes (more than 256 colours) are refused with a ValueError."""
    from . import backend
    downscale_filter = _downscale_filter(downscale_filter)
    if pixelize_method in (PixelizeMethod.NEURAL.value, "neural"):
        raise NotImplementedError("neural pixelization is outside the MI355X backend's scope")
    x = frames
    if pixelize_method in (PixelizeMethod.REGULAR.value, "regular"):
        tw, th = _even_dimensions(x.shape[2], x.shape[1], max_size)
        x = _downscale(x, th, tw, downscale_filter)
    planes, colours = ditherer.apply_dithering_frames_indexed(x)
    if hold is not None:
        stream = backend.as_hold_stream(hold, x.device)
        if len(colours) > 256:
            raise ValueError(f"the temporal hold takes one-byte planes: at most 256 colours, the palette has {len(colours)}")
        pal = np.ascontiguousarray(colours, dtype=np.uint8)
        if stream.palette is None or stream.palette.shape != pal.shape or not np.array_equal(stream.palette, pal):
            stream.reset()   # held indices of another palette mean other colours
        planes, _ = stream.add(x, planes)
        stream.palette = pal
    if final_resize_multiplier:
        nw, nh = _final_size(planes.shape[2], planes.shape[1], final_resize_multiplier)
        planes = backend.resize_nearest_plane(planes, nh, nw)
    return planes, colours


def process_frames_png(frames, ditherer: ImageDitherer, pixelize_method: Optional[str] = None, max_size: int = 64,
                       final_resize_multiplier: Optional[int] = None, seg_bytes: Optional[int] = None, blocks: str = "fixed",
                       assemble: str = "host", downscale_filter: str = "nearest"):
    """process_frames() as PNG-8 files: uint8 CUDA tensor [N,H,W,3] -> [bytes of one PNG file per frame]; decoding file i
    gives process_frames(...)[i], exactly.  process_frames_indexed, then png.encode_png: the planes are compressed on the
    device and only the compressed streams come back (assemble="device": the finished files, png.encode_png).  ValueError above
    256 colours."""
    from . import png
    planes, colours = process_frames_indexed(frames, ditherer, pixelize_method, max_size, final_resize_multiplier, downscale_filter=downscale_filter)
    return png.encode_png(planes, colours, seg_bytes, blocks=blocks, assemble=assemble)


def _process_single_frame(frame_path: Path, ditherer: ImageDitherer, pixelize_method: Optional[str] = None,
                          max_size: int = 64, final_resize_multiplier: Optional[int] = None, downscale_filter: str = "nearest") -> bool:
    """One PNG in place; True on success, False (with a message on stderr) on any error
    (video_processor.py:423-475)."""
    try:
        import torch
        frame_path = Path(frame_path)
        arr = np.array(Image.open(frame_path).convert("RGB"), dtype=np.uint8)
        out = process_frames(torch.from_numpy(arr).cuda().unsqueeze(0), ditherer, pixelize_method, max_size,
                             final_resize_multiplier, downscale_filter)
        Image.fromarray(out[0].cpu().numpy(), "RGB").save(frame_path)
        if not frame_path.exists() or frame_path.stat().st_size == 0:
            raise ValueError(f"Frame {frame_path} not saved properly")
        return True
    except Exception as e:  # noqa: BLE001 - the reference swallows everything here too
        print(f"Error processing frame {frame_path}: {e}", file=sys.stderr)
        return False


def _check_oklab_source(num_colors, use_gamma):
    """What ClipPalette.oklab would refuse, before a frame is decoded."""
    from . import backend
    backend._okfit_args(num_colors, 100)
    if use_gamma:
        raise ValueError("use_gamma=True cannot be combined with the 'oklab' palette fit: Oklab linearises by itself")


def _fit_clip(clip, source, num_colors, random_state):
    """The palette of a clip_palette.ClipPalette for a scan's `source`."""
    if source == "median_cut":
        return clip.median_cut(num_colors)
    if source == "oklab":
        return clip.oklab(num_colors)
    return clip.kmeans(num_colors, random_state)


class _PipeSplicer:
    """vmsplice(2) of a buffer's pages into a pipe: the kernel takes references to the pages instead of copying them into pipe
    buffers of its own -- no copy and no page allocation on the writing side, which on the bench box also speeds the READER of
    the other pipe up by a third (the two kernel-side copies contend; tools/bench_scripts/pipe_vmsplice.py: writer 650 -> 1890
    fps, concurrent reader 620 -> 800).  The pages stay referenced until the pipe's reader has consumed them, so the CALLER must
    not overwrite the buffer before that (the overlapped pipe path holds a slot back until consumed_bytes() has passed it).
    Linux only; anything unexpected turns it off and the caller writes as before."""

    def __init__(self):
        self.ok = False
        try:
            import ctypes
            import ctypes.util
            libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6", use_errno=True)

            class IoVec(ctypes.Structure):
                _fields_ = [("base", ctypes.c_void_p), ("len", ctypes.c_size_t)]

            libc.vmsplice.argtypes = [ctypes.c_int, ctypes.POINTER(IoVec), ctypes.c_ulong, ctypes.c_uint]
            libc.vmsplice.restype = ctypes.c_ssize_t
            self._ct, self._libc, self._IoVec = ctypes, libc, IoVec
            self.ok = sys.platform.startswith("linux")
        except Exception:  # noqa: BLE001
            pass

    def splice_all(self, fd: int, addr: int, nbytes: int) -> bool:
        """All nbytes at addr into the pipe fd.  True: done.  False: not available here (nothing was written: the caller
        falls back to write()).  Raises BrokenPipeError when the reader is gone."""
        import errno
        ct = self._ct
        off = 0
        while off < nbytes:
            iov = self._IoVec(addr + off, nbytes - off)
            n = self._libc.vmsplice(fd, ct.byref(iov), 1, 0)
            if n < 0:
                e = ct.get_errno()
                if e == errno.EINTR:
                    continue
                if e == errno.EPIPE:
                    raise BrokenPipeError(e, "vmsplice: the encoder closed its pipe")
                if off == 0:
                    self.ok = False   # EINVAL / EFAULT / ENOSYS: not here
                    return False
                raise OSError(e, "vmsplice failed in the middle of a batch")
            off += n
        return True

    @staticmethod
    def unread_bytes(fd: int) -> int:
        import array
        import fcntl
        import termios
        buf = array.array("i", [0])
        fcntl.ioctl(fd, termios.FIONREAD, buf)
        return int(buf[0])


class VideoProcessor:
    """video_processor.py:27-390"""

    def __init__(self, num_workers: Optional[int] = None,
                 progress_callback: Optional[Callable[[float, str], None]] = None, devices=None):
        if num_workers is None:
            num_workers = min(4, max(1, cpu_count() - 1))
        self.num_workers = num_workers  # kept for interface compatibility; frames batch on the GPU instead
        self.progress_callback = progress_callback
        # an addition: the GPUs the frame batches are spread over (contiguous blocks, one worker thread and stream per
        # device -- the reference's Pool over frames, video_processor.py:304-346).  None = every visible device.
        self.devices = devices

    def _devices(self):
        from . import sharding
        return sharding.visible_devices() if self.devices is None else list(self.devices)

    def _report_progress(self, fraction: float, message: str):
        if self.progress_callback:
            self.progress_callback(fraction, message)

    def _fix_failed_frames(self, failed_frames: list, all_frames: list):
        """Copy the nearest good frame (previous first, then next) over each failed one
        (video_processor.py:53-96)."""
        bad = set(failed_frames)
        for f in failed_frames:
            if f not in all_frames:
                print(f"Could not find index for {f.name}", file=sys.stderr)
                continue
            i = all_frames.index(f)
            order = list(range(i - 1, -1, -1)) + list(range(i + 1, len(all_frames)))
            src = next((all_frames[j] for j in order if all_frames[j] not in bad and all_frames[j].exists()), None)
            if src is None:
                print(f"ERROR: Could not find any successful frame to copy for {f.name}", file=sys.stderr)
                continue
            try:
                shutil.copy2(src, f)
                print(f"Fixed {f.name} by copying from {src.name}", file=sys.stderr)
            except Exception as e:  # noqa: BLE001
                print(f"Failed to copy frame {src.name} to {f.name}: {e}", file=sys.stderr)

    def get_video_info(self, video_path: str) -> dict:
        """fps / width / height / duration / frame_count via ffprobe, with the reference's defaults when
        probing fails (video_processor.py:98-170)."""
        def probe(entries):
            r = subprocess.run(["ffprobe", "-v", "error", "-select_streams", "v:0", "-show_entries",
                                f"stream={entries}", "-of", "default=nokey=1:noprint_wrappers=1", video_path],
                               capture_output=True, text=True, check=True)
            return r.stdout.strip()
        try:
            rate = probe("r_frame_rate")
            if "/" in rate:
                a, b = rate.split("/")
                fps = float(a) / float(b)
            else:
                fps = float(rate) if rate else 30.0
            dims = probe("width,height").split("\n")
            width = int(dims[0]) if len(dims) > 0 else 1920
            height = int(dims[1]) if len(dims) > 1 else 1080
            duration = frame_count = None
            for line in probe("duration,nb_frames").split("\n"):
                if line and line != "N/A":
                    try:
                        v = float(line)
                    except ValueError:
                        continue
                    if v > 100:
                        frame_count = int(v)
                    else:
                        duration = v
            if frame_count is None and duration is not None:
                frame_count = int(duration * fps)
            self._probe_ok = True
            return {"fps": fps, "width": width, "height": height, "duration": duration, "frame_count": frame_count}
        except Exception as e:  # noqa: BLE001
            print(f"Warning: Could not get video info: {e}", file=sys.stderr)
            # the reference's defaults (video_processor.py:164-170); _probe_ok tells the pipe path that width and
            # height are guesses it must not slice a byte stream with
            self._probe_ok = False
            return {"fps": 30.0, "width": 1920, "height": 1080, "duration": None, "frame_count": None}

    def _process_batch(self, files, ditherer, pixelize_method, max_size, final_resize_multiplier, downscale_filter="nearest"):
        """One batch of PNG files through the GPU; returns the list of files that failed."""
        import torch
        try:
            arrs = [np.array(Image.open(f).convert("RGB"), dtype=np.uint8) for f in files]
            if len({a.shape for a in arrs}) != 1:
                raise ValueError("frames of one batch differ in size")
            out = process_frames(torch.from_numpy(np.stack(arrs)).cuda(), ditherer, pixelize_method, max_size,
                                 final_resize_multiplier, downscale_filter).cpu().numpy()
            for f, o in zip(files, out):
                Image.fromarray(o, "RGB").save(f)
                if not f.exists() or f.stat().st_size == 0:
                    raise ValueError(f"Frame {f} not saved properly")
            return []
        except Exception as e:  # noqa: BLE001
            print(f"Batch failed ({e}); retrying frame by frame", file=sys.stderr)
        failed = []
        for f in files:
            if not any(_process_single_frame(f, ditherer, pixelize_method, max_size, final_resize_multiplier, downscale_filter)
                       for _ in range(3)):
                failed.append(f)
        return failed

    ATTEMPTS = 3  # the first try plus the reference's two retries (video_processor.py:325-336)

    @staticmethod
    def _device_is_gone(e: BaseException) -> bool:
        """A failure of the DEVICE, not of a frame: the library's DP_EHIP / DP_ENOMEM, or a HIP / out-of-memory error out of
        torch.  The reference's per-frame retry policy is about PNG and I/O failures; retrying on a faulted or exhausted GPU
        only makes 3 x batch doomed launches and would fill the rest of the video with copies of the last good frame."""
        from ._lib import DP_EHIP, DP_ENOMEM, DitherPieError
        if isinstance(e, DitherPieError):
            return e.code in (DP_EHIP, DP_ENOMEM)
        try:
            import torch
            if isinstance(e, torch.cuda.OutOfMemoryError):
                return True
        except Exception:  # noqa: BLE001
            pass
        text = str(e)
        return isinstance(e, RuntimeError) and any(k in text for k in ("HIP error", "CUDA error", "hipError", "out of memory"))

    def _batch_with_retries(self, host_frames, run, to_host=None, first_index=None):
        """The reference's failure policy for one batch (video_processor.py:304-346): the whole batch in one go; if that
        raises, every frame on its own, up to ATTEMPTS times; a frame that keeps failing is reported as None and the
        caller substitutes a neighbour.  run(frames [k,H,W,3]) -> [k,H',W',3]; to_host(frame tensor) -> host tensor (the
        default is .cpu() on the current stream; a caller whose run() works on a stream of its own passes its own).
        first_index: the stream index of host_frames[0] for a batch function that needs to know where in the stream it is
        (scene palettes): run is then called as run(frames, first=...), frame i of a retried batch with first_index + i --
        stated with every call, so that retries cannot desynchronise it.
        -> (out tensor [n,...] or None, per-frame list or None): exactly one of the two is set."""
        if to_host is None:
            def to_host(t):
                return t.cpu()
        def call(frames, i):
            return run(frames) if first_index is None else run(frames, first=first_index + i)
        try:
            return call(host_frames, 0), None
        except Exception as e:  # noqa: BLE001 - "a frame that errors must not abort the video"
            if self._device_is_gone(e):
                raise   # not a frame's fault: process_video_streaming reports failure instead of substituting frames
            print(f"Batch failed ({e}); retrying frame by frame", file=sys.stderr)
        outs = []
        for i in range(host_frames.shape[0]):
            o = None
            for attempt in range(self.ATTEMPTS):
                try:
                    o = to_host(call(host_frames[i:i + 1], i)[0])
                    break
                except Exception as e:  # noqa: BLE001
                    if self._device_is_gone(e):
                        raise
                    print(f"Error processing frame {i} of the batch (attempt {attempt + 1}): {e}", file=sys.stderr)
            outs.append(o)
        return None, outs

    def _probe_rotation(self, video_path: str) -> int:
        """Display rotation of the first video stream in degrees (0 when there is none): ffmpeg auto-rotates while
        decoding - the reference's plain `ffmpeg -i input frame_%05d.png` (video_processor.py:208-217) does - so the
        piped frames have the ROTATED geometry."""
        try:
            r = subprocess.run(["ffprobe", "-v", "error", "-select_streams", "v:0", "-show_entries",
                                "stream_tags=rotate:stream_side_data=rotation", "-of",
                                "default=nokey=1:noprint_wrappers=1", video_path], capture_output=True, text=True, check=True)
            for line in r.stdout.split("\n"):
                try:
                    return int(round(float(line.strip()))) % 360
                except ValueError:
                    continue
        except Exception as e:  # noqa: BLE001
            print(f"Warning: Could not probe rotation: {e}", file=sys.stderr)
        return 0

    PIPE_SLOTS = 4            # rotating pinned batch slots of the overlapped pipe path (reader, GPU, writer; the writer keeps a
                              # spliced slot until the encoder has consumed it)
    PIPE_ZERO_COPY = True     # vmsplice the output slots into the encoder pipe (see _PipeSplicer)
    PIPE_SLOT_BYTES = 128 << 20   # pinned bytes of a slot's input (or output) buffer at most
    PIPE_BYTES = 1 << 20      # requested pipe capacity (F_SETPIPE_SZ; the kernel default is 64 KiB = one syscall per 64 KiB)

    @staticmethod
    def _widen_pipe(fileobj):
        """Best effort: a 1 MiB pipe instead of 64 KiB, so that a 6 MB frame is ~6 reads / writes instead of ~95."""
        try:
            import fcntl
            fcntl.fcntl(fileobj.fileno(), getattr(fcntl, "F_SETPIPE_SZ", 1031), VideoProcessor.PIPE_BYTES)
        except Exception:  # noqa: BLE001 - not Linux, or above /proc/sys/fs/pipe-max-size
            pass

    @staticmethod
    def _write_all(f, buf):
        """The whole buffer into an unbuffered pipe (a raw write may be partial when a signal arrives)."""
        mv = memoryview(buf).cast("B")
        while len(mv):
            n = f.write(mv)
            mv = mv[len(mv) if n is None else n:]

    def _open_decoder(self, input_path, w, h):
        """The decode half of the pipes path: ffmpeg writing rgb24 frames of exactly w x h to a (widened) pipe.  The byte
        stream is sliced into frames of that size, so the decoder's output size is made explicit."""
        dec = subprocess.Popen(["ffmpeg", "-v", "error", "-i", input_path, "-f", "rawvideo", "-pix_fmt",
                                "rgb24", "-s", f"{w}x{h}", "pipe:1"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                               bufsize=0)
        self._widen_pipe(dec.stdout)
        return dec

    @staticmethod
    def _decoder_reader(dec, batch_size, frame_bytes, w, h, stats, max_frames=None):
        """The reader stage's work: read_batch(view) -> (whole frames read, bytes read) fills `view` from the decoder until it
        holds a batch or the stream ends.  max_frames: stop after that many frames of the stream (the last batch comes out
        short, which ends the stage as the end of the stream does)."""
        import time
        left = {"frames": None if max_frames is None else max(int(max_frames), 0)}

        def read_batch(view):
            t0 = time.perf_counter()
            got, want = 0, batch_size * frame_bytes
            if left["frames"] is not None:
                want = min(want, left["frames"] * frame_bytes)
            while got < want:  # a pipe read returns at most the pipe's capacity at a time
                n = dec.stdout.readinto(view[got:want])
                if not n:
                    break
                got += n
            stats["read_s"] += time.perf_counter() - t0
            if got % frame_bytes:
                raise RuntimeError(f"decoder stream is not a whole number of {w}x{h} rgb24 frames "
                                   f"({got % frame_bytes} bytes left over)")
            if left["frames"] is not None:
                left["frames"] -= got // frame_bytes
            return got // frame_bytes, got
        return read_batch

    def _scan_decoded(self, video_path, max_frames, setup, what, noun, indexed=False):
        """The DECODE half of the rawvideo pipes path, shared by scan_palette and scan_scenes: the same decoder command line,
        reader thread, rotating pinned slots and failure policy as _stream_through_pipes, no encoder.  setup(dev, gpu_stream,
        h, w, stats) -> feed(frames_on_device, first): called once on the scan's device and stream, it makes the
        accumulators; feed then gets every batch (or, after a failed batch, every frame on its own) on that stream, with
        the stream index of its first frame when `indexed` and None otherwise.  -> (frames decoded, device); fills
        self.last_scan_stats.  A frame that keeps failing is counted in stats["skipped"]; a device failure, a malformed
        stream or a decoder that exits with an error raises."""
        import time
        import torch
        self._report_progress(0.0, f"Initializing the {what}...")
        info = self.get_video_info(video_path)
        if not getattr(self, "_probe_ok", True):
            raise RuntimeError("could not probe the video's frame size: the decoder stream cannot be sliced into frames")
        w, h = int(info["width"]), int(info["height"])
        if self._probe_rotation(video_path) in (90, 270):
            w, h = h, w
        frame_bytes = w * h * 3
        total_hint = info.get("frame_count") or 0
        if max_frames is not None:
            total_hint = min(total_hint, int(max_frames)) if total_hint else int(max_frames)
        dev = self._devices()[0]   # histograms add, but one accumulator lives on one device
        dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
        batch_size = max(1, min(15, self.PIPE_SLOT_BYTES // max(frame_bytes, 1)))
        stats = {"mode": "scan", "slots": self.PIPE_SLOTS, "batch_frames": batch_size, "read_s": 0.0, "gpu_submit_s": 0.0,
                 "gpu_wait_s": 0.0, "write_s": 0.0, "frames": 0}
        self.last_scan_stats = stats
        with torch.cuda.device(dev):
            gpu_stream = torch.cuda.Stream()
            with torch.cuda.stream(gpu_stream):
                feed = setup(dev, gpu_stream, h, w, stats)
        token = {}

        def run(x, first=None):
            # H2D and the accumulators on the scan's own stream; what comes back is one byte per frame, so that the
            # stages downstream (D2H behind the kernels, one event per slot, the slot's way back to the reader) run unchanged
            with torch.cuda.device(dev), torch.cuda.stream(gpu_stream):
                feed(x.cuda(non_blocking=True), first)
                t = token.get("t")
                if t is None:
                    t = token["t"] = torch.zeros((batch_size, 1, 1, 1), dtype=torch.uint8, device=dev)
                return t[:x.shape[0]]

        def to_host(t):
            with torch.cuda.device(dev), torch.cuda.stream(gpu_stream):
                return t.cpu()

        state = {"skipped": 0}

        def emit(out_host, n_frames, per_frame, may_splice=False):
            if out_host is None:   # a batch that was retried frame by frame: the frames that kept failing are left out
                state["skipped"] += sum(1 for o in per_frame if o is None)
            return False

        def progress(done):
            frac = done / total_hint if total_hint else 0.5
            self._report_progress(0.05 + 0.85 * min(frac, 1.0), f"Scanned {done}/{total_hint or '?'} frames")

        def new_out(shape):
            return torch.empty((batch_size,) + tuple(shape), dtype=torch.uint8, pin_memory=True)

        self._report_progress(0.05, "Starting the decoder...")
        dec = self._open_decoder(video_path, w, h)
        read_batch = self._decoder_reader(dec, batch_size, frame_bytes, w, h, stats, max_frames)
        done, stopped_early = 0, False
        t_wall = time.perf_counter()
        try:
            done = self._pipe_overlapped(batch_size, frame_bytes, (h, w), (1, 1), run, to_host, gpu_stream, {"out": None}, read_batch,
                                         emit, progress, lambda shape: new_out((1, 1, 1)), stats, dec, lambda: 0, state,
                                         indexed_run=indexed)
            stopped_early = max_frames is not None and done >= int(max_frames)
        finally:
            if stopped_early:
                try:
                    dec.kill()   # the rest of the stream is not wanted
                except Exception:  # noqa: BLE001
                    pass
            if dec.stdout:
                dec.stdout.close()
            rc_dec = dec.wait()
            gpu_stream.synchronize()
            state.pop("slots", None)
            stats["frames"] = done
            stats["skipped"] = state["skipped"]
            stats["wall_s"] = time.perf_counter() - t_wall
        if rc_dec != 0 and not stopped_early:
            raise RuntimeError(f"ffmpeg failed (decoder {rc_dec})")
        if done == 0:
            raise ValueError("No frames extracted from video")
        if state["skipped"]:
            print(f"Left {state['skipped']} failed frames out of the {noun}", file=sys.stderr)
        return done, dev

    def scan_palette(self, video_path, source, num_colors, every=1, max_frames=None, use_gamma=False, random_state=42):
        """One palette fitted to the whole clip, ready for ImageDitherer(palette=...): the DECODE half of the rawvideo pipes
        path (the same decoder command line, reader thread, rotating pinned slots and failure policy as
        _stream_through_pipes; no encoder) feeding every `every`-th frame into a clip_palette.ClipPalette.
        source: "median_cut" (the reference's reduce_colors on the taken frames stacked top to bottom) or "kmeans" (a pure
        function of the clip's colour multiset; clip_palette's parity definitions) or "oklab" (ClipPalette.oklab: the integer
        Oklab fit, at most 256 colours, not with use_gamma).  max_frames: look at the first that
        many frames of the stream only.  Failure policy: a batch that fails is retried frame by frame and a frame that
        keeps failing is left out of the palette; a device failure, a malformed stream or a decoder that exits with an
        error raises, as in the pipes path.  Progress goes through progress_callback."""
        import torch
        from .clip_palette import ClipPalette
        if source not in ("median_cut", "kmeans", "oklab"):
            raise ValueError(f"source must be 'median_cut', 'kmeans' or 'oklab', not {source!r}")
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        if source == "oklab":
            _check_oklab_source(num_colors, use_gamma)
        made = {}

        def setup(dev, gpu_stream, h, w, stats):
            clip = made["clip"] = ClipPalette(use_gamma=use_gamma, device=dev)
            return lambda x, first: clip.add(x, every=every)

        done, dev = self._scan_decoded(video_path, max_frames, setup, "palette scan", "palette")
        clip = made["clip"]
        if clip.n_pixels == 0:
            raise RuntimeError("no frame of the video could be scanned")
        self._report_progress(0.9, "Fitting the palette...")
        self.last_clip_palette = clip
        with torch.cuda.device(dev):
            palette = _fit_clip(clip, source, num_colors, random_state)
        self._report_progress(1.0, "Palette scan complete!")
        return palette

    def scan_scenes(self, video_path, source=None, num_colors=16, threshold=0.4, min_scene_frames=8, every=1, max_frames=None,
                    use_gamma=False, random_state=42):
        """Where the clip cuts, and one palette per scene -> list of scenes.Scene(start, end, palette), in stream order and
        tiling frames 0 ... n-1; hand it to process_video_streaming(..., scene_palettes=...).  One decode-only pass built as
        scan_palette is (the same decoder line, reader thread, rotating slots, failure policy and progress milestones; it
        fills last_scan_stats too).  Per batch: the frames' colour signatures and the distances of consecutive signatures on
        the device (backend.SceneStream), the N distances read back -- one small synchronising copy per batch --,
        scenes.scene_cuts, the batch split at the cuts (scenes.split_at), every piece into ONE clip_palette.ClipPalette; at
        each cut the finished scene's palette is fitted and the accumulator reset.
        source: "median_cut" / "kmeans" / "oklab" as in scan_palette -- a scene's palette is what a fresh
        ClipPalette(use_gamma).add(frames[start:end], every) gives for that source; None: boundaries only, every palette is
        None and no accumulator is made.  every: every that-many-th frame of each scene, counted from the scene's first
        frame.  Frame i starts a scene when its distance exceeds threshold * 2 * H * W and the open scene holds at least
        min_scene_frames frames (scenes.scene_cuts).  threshold=0.4 and min_scene_frames=8 are design choices -- "two fifths
        of the pixels changed their 16^3 cell, and no scene shorter than a third of a second at 24 fps" -- NOT tuned
        values: there was no footage to tune them on.
        Failure policy: a frame that keeps failing stays in the scene that is open, does not update the carried signature
        and is left out of the palette (last_scan_stats["skipped"]); a scene of which no frame could be scanned has palette
        None.  last_scan_stats gains "signature_s" (signatures, distances and their read-back) and "palette_s" (the fits at
        the cuts), both part of gpu_submit_s, and "scenes"."""
        import time
        import torch
        from . import backend
        from .clip_palette import ClipPalette
        from .scenes import Scene, _check_cut_parameters, scene_cuts, split_at
        if source not in (None, "median_cut", "kmeans", "oklab"):
            raise ValueError(f"source must be None, 'median_cut', 'kmeans' or 'oklab', not {source!r}")
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        _check_cut_parameters(threshold, min_scene_frames)
        if int(every) < 1:
            raise ValueError("every must be >= 1")
        if source is not None and int(num_colors) < 1:
            raise ValueError("num_colors must be >= 1")
        if source == "kmeans" and int(num_colors) > backend.KMEANS_HIST_MAX_K:
            raise ValueError(f"a clip k-means palette has at most {backend.KMEANS_HIST_MAX_K} colours, not {num_colors}")
        if source == "oklab":
            _check_oklab_source(num_colors, use_gamma)
        scenes = []
        made = {"clip": None}
        cur = {"open": 0, "carry": 0, "starts": set()}

        def fit(clip):
            return _fit_clip(clip, source, num_colors, random_state)

        def close(end, stats):
            """the open scene ends in front of stream frame `end`"""
            clip, palette = made["clip"], None
            if clip is not None:
                if clip.n_pixels:
                    t0 = time.perf_counter()
                    palette = fit(clip)
                    stats["palette_s"] += time.perf_counter() - t0
                clip.reset()
            scenes.append(Scene(cur["open"], end, palette))
            cur["open"] = end

        def setup(dev, gpu_stream, h, w, stats):
            stats.update(signature_s=0.0, palette_s=0.0, scenes=0)
            made["stats"] = stats
            sig = backend.SceneStream(dev)
            clip = made["clip"] = ClipPalette(use_gamma=use_gamma, device=dev) if source is not None else None
            taken = {"first": 0, "n": 0}   # the batch whose distances were taken last: a retry of its frames must not take them again

            def feed(x, first):
                n = x.shape[0]
                if not (taken["first"] <= first and first + n <= taken["first"] + taken["n"]):
                    t0 = time.perf_counter()
                    dist = sig.add(x).cpu().tolist()
                    stats["signature_s"] += time.perf_counter() - t0
                    cuts, cur["carry"] = scene_cuts(dist, h * w, threshold, min_scene_frames, cur["carry"])
                    cur["starts"].update(first + c for c in cuts)
                    taken.update(first=first, n=n)
                for lo, hi in split_at(first, n, cur["starts"]):
                    if lo in cur["starts"] and lo != cur["open"]:
                        close(lo, stats)
                    if clip is not None:
                        clip.add(x[lo - first:hi - first], every=every)
            return feed

        done, dev = self._scan_decoded(video_path, max_frames, setup, "scene scan", "scene palettes", indexed=True)
        self._report_progress(0.9, "Fitting the last scene's palette...")
        with torch.cuda.device(dev):
            if done > cur["open"]:
                close(done, made["stats"])
        made["stats"]["scenes"] = len(scenes)
        if source is not None and all(s.palette is None for s in scenes):
            raise RuntimeError("no frame of the video could be scanned")
        self._report_progress(1.0, "Scene scan complete!")
        return scenes

    def process_video_gif(self, input_path, output_path, ditherer, pixelize_method=None, max_size=64, final_resize_multiplier=None,
                          scene_palettes=None, delta=True, max_frames=None, chunk_px=None, hold=None, downscale_filter="nearest") -> int:
        """The video as an animated GIF of palette indices (gif.GifWriter): decode -> GPU -> file, no encoder pipe and no RGB
        frames on the way out.  Built on the decode-only loop of scan_palette / scan_scenes (_scan_decoded: the same decoder
        line, reader thread and rotating pinned slots).  Per batch: process_frames_indexed -- piece by piece with each
        scene's palette when scene_palettes (the list scan_scenes returns) is given, as _stream_through_pipes cuts its
        batches --, the inter-frame delta and the LZW image data on the device, one copy of the compressed bytes to the host,
        the container in Python.  A scene's palette that is not the first one travels as a local colour table, and the
        delta starts over at every palette change.  Decoding a frame of the file gives process_frames of that frame (with
        its scene's palette), exactly.  The file plays at gif.delay_cs(fps) centiseconds per frame.
        hold (an addition; None leaves every byte as it was): a backend.HoldStream or the settings (cell, tol, share) of one --
        the temporal hold of process_frames_indexed over the whole file: cells whose source has not moved keep their indices, so
        the delta finds them equal and drops them.  Decoding a frame then gives the held planes, not process_frames of that
        frame alone.  The hold starts over wherever the palette changes: at every scene start under scene_palettes.
        One device: the first of `devices`; a list of several is refused (frames of one file are written in order by one
        writer).  Failure policy: a batch that fails RAISES -- the rawvideo path's substitution of the nearest good frame is
        not mirrored: a GIF with a silently substituted frame is worse than an error -- and so does a device failure, a
        malformed stream or a decoder that exits with an error; the partial file is left as it is.
        -> the number of frames written.  ValueError before the decoder starts: a bad scene list, several devices, a ditherer
        of more than 256 colours where that is known up front, max_frames or chunk_px < 1."""
        import copy
        from .gif import GIF_MAX_COLOURS, GifWriter
        downscale_filter = _downscale_filter(downscale_filter)   # (the filter of the pixelization down-scale, as for process_frames)
        if self.devices is not None and len(list(self.devices)) > 1:
            raise ValueError(f"process_video_gif runs on one device, not on {len(list(self.devices))}: a GIF's frames are "
                             "written in order by one writer; pass devices=[one]")
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        if chunk_px is not None and int(chunk_px) < 1:
            raise ValueError("chunk_px must be >= 1")
        pieces_of = None
        if scene_palettes is not None:
            from .scenes import check_scene_palettes, scene_of, split_at
            scene_list = check_scene_palettes(scene_palettes)
            for sc in scene_list:
                if len(sc.palette) > GIF_MAX_COLOURS:
                    raise ValueError(f"the scene at frame {sc.start} has {len(sc.palette)} colours: a GIF colour table holds {GIF_MAX_COLOURS}")
            cut_points = [int(sc.start) for sc in scene_list[1:]]
            scene_ditherers = []
            for sc in scene_list:
                d = copy.copy(ditherer)
                d.palette = [tuple(c) for c in sc.palette]
                scene_ditherers.append(d)

            def pieces_of(first, n):
                return [(lo - first, hi - first, scene_ditherers[scene_of(scene_list, lo)]) for lo, hi in split_at(first, n, cut_points)]
        if hold is not None:
            from . import backend
            backend.check_hold_argument(hold)
        info = self.get_video_info(input_path)
        fps = info.get("fps") or 25.0
        made = {}

        class _BatchFailed(BaseException):   # past _batch_with_retries' `except Exception`: no frame-by-frame retry here
            def __init__(self, error):
                super().__init__(str(error))
                self.error = error

        def setup(dev, gpu_stream, h, w, stats):
            from . import backend
            oh, ow = output_size(h, w, pixelize_method, max_size, final_resize_multiplier)
            writer = made["writer"] = GifWriter(made["file"], ow, oh, fps, 0, chunk_px)
            held = made["hold"] = backend.as_hold_stream(hold, dev)
            if held is not None:
                held.reset()   # a file is a stream of its own

            def feed(x, first):
                try:
                    pieces = pieces_of(first, x.shape[0]) if pieces_of else [(0, x.shape[0], ditherer)]
                    for a, b, d in pieces:
                        if held is not None and pieces_of and (first + a) in cut_points:
                            held.reset()   # a scene starts: its palette is another one (and were it equal, a cut refreshes everything)
                        planes, colours = process_frames_indexed(x[a:b], d, pixelize_method, max_size, final_resize_multiplier, hold=held,
                                                                 downscale_filter=downscale_filter)
                        writer.add(planes, colours, delta)
                except Exception as e:  # noqa: BLE001
                    raise _BatchFailed(e) from e
            return feed

        with open(output_path, "wb") as f:
            made["file"] = f
            try:
                done, _ = self._scan_decoded(input_path, max_frames, setup, "GIF encode", "GIF", indexed=True)
            except _BatchFailed as e:
                raise e.error
            finally:
                if "writer" in made:
                    made["writer"].close()
        self.last_gif_stats = dict(self.last_scan_stats, mode="gif", bytes=os.path.getsize(output_path))
        self._report_progress(1.0, "GIF complete!")
        return made["writer"].n_frames

    def process_video_apng(self, input_path, output_path, ditherer, pixelize_method=None, max_size=64, final_resize_multiplier=None,
                           delta=True, max_frames=None, seg_bytes=None, blocks="fixed", hold=None, downscale_filter="nearest") -> int:
        """The video as an animated PNG of palette indices (apng.ApngWriter): decode -> GPU -> file, no encoder pipe and no
        RGB frames on the way out.  Built on the decode-only loop of scan_palette / scan_scenes (_scan_decoded), exactly as
        process_video_gif is.  Per batch: process_frames_indexed, the inter-frame delta, the zlib streams, the chunk CRCs and
        the finished fcTL + IDAT / fdAT chunks on the device, one copy of exactly those bytes to the host, one write.
        Decoding frame i of the file gives process_frames of frame i, exactly; the file plays at apng.delay(fps), which is
        exact for every rate a fraction of two 16-bit numbers expresses (30000/1001 among them).
        One palette: an APNG has a single PLTE, so there is no scene_palettes argument, and a ditherer that fits its palette
        per frame is refused at the first frame whose colours differ from the file's.  A palette fitted to the whole clip
        (scan_palette) is the natural companion.
        hold (an addition; None leaves every byte as it was): as for process_video_gif -- the temporal hold over the whole file.
        One device: the first of `devices`; a list of several is refused.  Failure policy as process_video_gif: a batch that
        fails RAISES, and so does a device failure, a malformed stream or a decoder that exits with an error; the partial
        file is left as it is.
        -> the number of frames written.  ValueError before the decoder starts: several devices, a ditherer of more than 256
        colours where that is known up front, max_frames < 1, seg_bytes outside 256 ... 32768, a `blocks` that does not
        exist."""
        from .apng import APNG_MAX_COLOURS, ApngWriter
        downscale_filter = _downscale_filter(downscale_filter)   # (the filter of the pixelization down-scale, as for process_frames)
        if self.devices is not None and len(list(self.devices)) > 1:
            raise ValueError(f"process_video_apng runs on one device, not on {len(list(self.devices))}: an APNG's frames are "
                             "written in order by one writer; pass devices=[one]")
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        if seg_bytes is not None and not 256 <= int(seg_bytes) <= 32768:
            raise ValueError("seg_bytes must be in 256 ... 32768")
        if blocks not in ("fixed", "dynamic"):
            raise ValueError(f"blocks must be 'fixed' or 'dynamic', not {blocks!r}")
        if getattr(ditherer, "palette", None) is not None and len(ditherer.palette) > APNG_MAX_COLOURS:
            raise ValueError(f"the ditherer has {len(ditherer.palette)} colours: a PNG palette holds {APNG_MAX_COLOURS}")
        if hold is not None:
            from . import backend
            backend.check_hold_argument(hold)
        info = self.get_video_info(input_path)
        fps = info.get("fps") or 25.0
        made = {}

        class _BatchFailed(BaseException):   # past _batch_with_retries' `except Exception`: no frame-by-frame retry here
            def __init__(self, error):
                super().__init__(str(error))
                self.error = error

        def setup(dev, gpu_stream, h, w, stats):
            from . import backend
            oh, ow = output_size(h, w, pixelize_method, max_size, final_resize_multiplier)
            writer = made["writer"] = ApngWriter(made["file"], ow, oh, fps, 0, delta, seg_bytes, "device", blocks)
            held = made["hold"] = backend.as_hold_stream(hold, dev)
            if held is not None:
                held.reset()   # a file is a stream of its own

            def feed(x, first):
                try:
                    planes, colours = process_frames_indexed(x, ditherer, pixelize_method, max_size, final_resize_multiplier, hold=held,
                                                             downscale_filter=downscale_filter)
                    writer.add(planes, colours)
                except Exception as e:  # noqa: BLE001
                    raise _BatchFailed(e) from e
            return feed

        with open(output_path, "w+b") as f:
            made["file"] = f
            try:
                self._scan_decoded(input_path, max_frames, setup, "APNG encode", "APNG", indexed=True)
            except _BatchFailed as e:
                raise e.error
            finally:
                if "writer" in made:
                    made["writer"].close()
        self.last_apng_stats = dict(self.last_scan_stats, mode="apng", bytes=os.path.getsize(output_path))
        self._report_progress(1.0, "APNG complete!")
        return made["writer"].n_frames

    def process_video_pngs(self, input_path, out_pattern, ditherer, pixelize_method=None, max_size=64, final_resize_multiplier=None,
                           scene_palettes=None, max_frames=None, seg_bytes=None, start=1, blocks="fixed", assemble="host",
                           downscale_filter="nearest") -> int:
        """The video as a sequence of PNG-8 files out_pattern % start, out_pattern % (start + 1), ... (the 'frame_%05d.png'
        of a frame directory): decode -> GPU -> files, no encoder pipe and no RGB frames on the way out.  Built on the
        decode-only loop of scan_palette / scan_scenes (_scan_decoded), exactly as process_video_gif is.  Per batch:
        process_frames_indexed -- piece by piece with each scene's palette when scene_palettes (the list scan_scenes
        returns) is given --, the zlib streams on the device, one copy of the compressed bytes to the host, the containers
        in Python (assemble="device": the containers and their CRCs on the device too, png.encode_png).  Decoding file i
        gives process_frames of frame i (with its scene's palette), exactly.
        One device: the first of `devices`; a list of several is refused.  Failure policy as process_video_gif: a batch that
        fails RAISES, and so does a device failure, a malformed stream or a decoder that exits with an error; the files
        written so far are left as they are.
        -> the number of files written.  ValueError before the decoder starts: a bad scene list, several devices, a ditherer
        or scene of more than 256 colours where that is known up front, max_frames < 1, seg_bytes outside 256 ... 32768, a
        pattern that does not format an integer."""
        import copy
        from .png import PNG_MAX_COLOURS, encode_png
        downscale_filter = _downscale_filter(downscale_filter)   # (the filter of the pixelization down-scale, as for process_frames)
        if self.devices is not None and len(list(self.devices)) > 1:
            raise ValueError(f"process_video_pngs runs on one device, not on {len(list(self.devices))}: the files are "
                             "numbered in order by one writer; pass devices=[one]")
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1")
        if seg_bytes is not None and not 256 <= int(seg_bytes) <= 32768:
            raise ValueError("seg_bytes must be in 256 ... 32768")
        if blocks not in ("fixed", "dynamic"):
            raise ValueError(f"blocks must be 'fixed' or 'dynamic', not {blocks!r}")
        if assemble not in ("host", "device"):
            raise ValueError(f"assemble must be 'host' or 'device', not {assemble!r}")
        try:
            if str(out_pattern) % 1 == str(out_pattern) % 2:
                raise TypeError("no field")
        except (TypeError, ValueError):
            raise ValueError(f"out_pattern must format a frame number (as 'frame_%05d.png'), not {out_pattern!r}") from None
        if getattr(ditherer, "palette", None) is not None and len(ditherer.palette) > PNG_MAX_COLOURS:
            raise ValueError(f"the ditherer has {len(ditherer.palette)} colours: a PNG palette holds {PNG_MAX_COLOURS}")
        pieces_of = None
        if scene_palettes is not None:
            from .scenes import check_scene_palettes, scene_of, split_at
            scene_list = check_scene_palettes(scene_palettes)
            for sc in scene_list:
                if len(sc.palette) > PNG_MAX_COLOURS:
                    raise ValueError(f"the scene at frame {sc.start} has {len(sc.palette)} colours: a PNG palette holds {PNG_MAX_COLOURS}")
            cut_points = [int(sc.start) for sc in scene_list[1:]]
            scene_ditherers = []
            for sc in scene_list:
                d = copy.copy(ditherer)
                d.palette = [tuple(c) for c in sc.palette]
                scene_ditherers.append(d)

            def pieces_of(first, n):
                return [(lo - first, hi - first, scene_ditherers[scene_of(scene_list, lo)]) for lo, hi in split_at(first, n, cut_points)]
        made = {"written": 0, "bytes": 0}

        class _BatchFailed(BaseException):   # past _batch_with_retries' `except Exception`: no frame-by-frame retry here
            def __init__(self, error):
                super().__init__(str(error))
                self.error = error

        def setup(dev, gpu_stream, h, w, stats):
            def feed(x, first):
                try:
                    pieces = pieces_of(first, x.shape[0]) if pieces_of else [(0, x.shape[0], ditherer)]
                    for a, b, d in pieces:
                        planes, colours = process_frames_indexed(x[a:b], d, pixelize_method, max_size, final_resize_multiplier, downscale_filter=downscale_filter)
                        for k, data in enumerate(encode_png(planes, colours, seg_bytes, blocks=blocks, assemble=assemble)):
                            with open(str(out_pattern) % (int(start) + first + a + k), "wb") as f:
                                f.write(data)
                            made["written"] += 1
                            made["bytes"] += len(data)
                except Exception as e:  # noqa: BLE001
                    raise _BatchFailed(e) from e
            return feed

        try:
            self._scan_decoded(input_path, max_frames, setup, "PNG encode", "PNG sequence", indexed=True)
        except _BatchFailed as e:
            raise e.error
        self.last_png_stats = dict(self.last_scan_stats, mode="png", bytes=made["bytes"])
        self._report_progress(1.0, "PNG sequence complete!")
        return made["written"]

    def _stream_through_pipes(self, input_path, output_path, ditherer, method, max_size, batch_size,
                              final_resize_multiplier, info, run=None, overlap=True, scene_palettes=None,
                              downscale_filter="nearest") -> int:
        """decode -> GPU -> encode through two ffmpeg rawvideo pipes; returns the number of frames written.
        downscale_filter: the filter of the pixelization down-scale, as for process_frames.
        Failure policy as in the reference: a batch that fails is retried frame by frame, a frame that still fails is
        replaced by the nearest good output frame (the previous one first, video_processor.py:53-96) and the video goes
        on; the call fails only when ffmpeg does or when no frame at all could be processed.  `run` (tests): the batch
        function, default process_frames on the configured devices.

        overlap=True (the default): the three stages run CONCURRENTLY on PIPE_SLOTS rotating pinned batch slots -- a reader
        thread fills a slot from the decoder pipe, this thread submits it to the GPU on a stream of its own (H2D,
        process_frames, D2H into the slot's pinned output buffer, one event; it never waits for the device), a writer
        thread waits for the event, applies the substitution policy in frame order and feeds the encoder pipe -- so a
        video costs max(decode, GPU, encode) per batch instead of their sum (the reference overlaps nothing either: it
        extracts every PNG, then processes, then encodes, video_processor.py:204-217, 304-346, 361-382).
        overlap=False: the serial loop of rounds 2-4 (read -> H2D -> kernels -> D2H -> write per batch), kept as the
        byte-for-byte A/B partner of the overlapped path.  Both fill self.last_pipe_stats.

        scene_palettes (a list of scenes.Scene, from scan_scenes): every batch is cut at the scene starts that fall inside it
        (scenes.split_at) and each piece runs through process_frames with a shallow copy of `ditherer` that carries its
        scene's palette; the pieces' outputs go into one batch tensor, so the stages downstream see what they see without
        it.  The batch function is told the stream index of its first frame with every call (_batch_with_retries), also
        when a failed batch is retried frame by frame.  Frames past the last scene's end use the last scene's palette.
        ValueError before the decoder starts: scenes.check_scene_palettes, or a `run` of the caller's beside the list."""
        import time
        import torch
        downscale_filter = _downscale_filter(downscale_filter)
        scene_run = scene_palettes is not None
        if scene_run:
            import copy
            from .scenes import check_scene_palettes, scene_of, split_at
            if run is not None:
                raise ValueError("scene_palettes go with the product batch function, not with a run of the caller's")
            scene_list = check_scene_palettes(scene_palettes)
            cut_points = [int(sc.start) for sc in scene_list[1:]]
            scene_ditherers = []
            for sc in scene_list:
                d = copy.copy(ditherer)
                d.palette = [tuple(c) for c in sc.palette]
                scene_ditherers.append(d)
        w, h, fps = int(info["width"]), int(info["height"]), info["fps"]
        if self._probe_rotation(input_path) in (90, 270):
            w, h = h, w  # ffprobe reports the coded size; the decoder below rotates as the reference's extraction does
        frame_bytes = w * h * 3
        total_hint = info.get("frame_count") or 0
        devs = self._devices() if run is None else [None]
        batch_size = batch_size * len(devs)  # one batch per device in flight
        product_run = run is None
        pin = torch.cuda.is_available()
        out_geom = None   # (H', W') of the product path: known up front, so that the output slots are allocated once
        if product_run:
            # a slot is one batch of input + one of output, pinned; three of them rotate: keep a slot's larger half under
            # PIPE_SLOT_BYTES (4K frames: 5 per batch instead of the reference's 15 -- only the granularity of the retry
            # policy changes with it, not the result)
            oh_, ow_ = output_size(h, w, method, max_size, final_resize_multiplier)
            per_frame = max(frame_bytes, oh_ * ow_ * 3)
            batch_size = max(len(devs), min(batch_size, self.PIPE_SLOT_BYTES // max(per_frame, 1)))
        gpu_stream = None  # overlap, one device: the stream this call's H2D / kernels / D2H are queued on
        target = {"out": None}   # several devices: the pinned host tensor the workers write the current batch into
        if product_run:
            out_geom = output_size(h, w, method, max_size, final_resize_multiplier)
            if overlap and len(devs) == 1 and pin:
                with torch.cuda.device(devs[0]):
                    gpu_stream = torch.cuda.Stream()  # the caller's current stream is never blocked or waited on

            def run(x):  # noqa: F811 - the product batch function: frames stay in HBM between the stages
                if len(devs) > 1 and x.shape[0] > 1:
                    from . import sharding
                    out = target["out"]
                    return sharding.process_on_devices(
                        x, lambda y: process_frames(y, ditherer, method, max_size, final_resize_multiplier, downscale_filter), devs,
                        out=None if out is None else out[:x.shape[0]])
                with torch.cuda.device(devs[0]):
                    if gpu_stream is not None:
                        with torch.cuda.stream(gpu_stream):
                            return process_frames(x.cuda(non_blocking=True), ditherer, method, max_size, final_resize_multiplier, downscale_filter)
                    return process_frames(x.cuda(non_blocking=True), ditherer, method, max_size, final_resize_multiplier, downscale_filter)

            def one_palette(y, d):
                return process_frames(y, d, method, max_size, final_resize_multiplier, downscale_filter)

            def run_scenes(x, first=0):   # the same, piece by piece with the palette of the piece's scene
                n = x.shape[0]
                pieces = [(lo - first, hi - first, scene_ditherers[scene_of(scene_list, lo)]) for lo, hi in split_at(first, n, cut_points)]
                if len(devs) > 1 and n > 1:
                    from . import sharding
                    out = target["out"]
                    parts = [sharding.process_on_devices(x[a:b], lambda y, d=d: one_palette(y, d), devs,
                                                         out=None if out is None else out[a:b]) for a, b, d in pieces]
                    return out[:n] if out is not None else (parts[0] if len(parts) == 1 else torch.cat(parts))
                with torch.cuda.device(devs[0]), torch.cuda.stream(gpu_stream if gpu_stream is not None else torch.cuda.current_stream()):
                    xd = x.cuda(non_blocking=True)
                    if len(pieces) == 1:
                        return one_palette(xd, pieces[0][2])
                    out = None
                    for a, b, d in pieces:
                        y = one_palette(xd[a:b], d)
                        if out is None:
                            out = torch.empty((n,) + tuple(y.shape[1:]), dtype=y.dtype, device=y.device)
                        out[a:b] = y
                    return out

            if scene_run:
                run = run_scenes

        def to_host(t):
            if gpu_stream is not None and t.is_cuda:   # the copy goes behind the kernels, on their stream
                with torch.cuda.device(t.device), torch.cuda.stream(gpu_stream):
                    return t.cpu()
            return t.cpu()

        dec = self._open_decoder(input_path, w, h)
        state = {"enc": None, "last_good": None, "leading": 0, "substituted": 0, "written": 0, "piped": 0}
        stats = {"mode": "overlapped" if overlap else "serial", "slots": self.PIPE_SLOTS if overlap else 1, "batch_frames": batch_size,
                 "read_s": 0.0, "gpu_submit_s": 0.0, "gpu_wait_s": 0.0, "write_s": 0.0, "frames": 0}
        self.last_pipe_stats = stats

        def open_encoder(shape):
            oh, ow = int(shape[0]), int(shape[1])
            enc = subprocess.Popen(
                ["ffmpeg", "-y", "-v", "error", "-f", "rawvideo", "-pix_fmt", "rgb24", "-s", f"{ow}x{oh}",
                 "-framerate", f"{fps:.5f}", "-i", "pipe:0", "-i", input_path, "-map", "0:v:0", "-map", "1:a?",
                 "-map", "1:s?", "-c:v", "libx264", "-preset", "medium", "-crf", "18", "-pix_fmt", "yuv420p",
                 "-c:a", "copy", "-c:s", "copy", output_path],
                stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, bufsize=0)
            self._widen_pipe(enc.stdin)
            return enc

        read_batch = self._decoder_reader(dec, batch_size, frame_bytes, w, h, stats)

        splicer = _PipeSplicer() if (overlap and self.PIPE_ZERO_COPY) else None

        def emit(out_host, n_frames, per_frame, may_splice=False):
            """One batch to the encoder, in frame order, with the substitution policy (state: the encoder, the newest good
            output frame, frames that failed before any frame succeeded).  out_host: host tensor [>= n_frames, H', W', 3]
            of a batch that succeeded as a whole; per_frame: list of host tensors / None of one that was retried.
            may_splice: out_host is a slot's own buffer that the caller keeps untouched until the encoder has consumed it.
            -> True when the batch's pages were handed to the pipe by reference (state["piped"] = bytes piped so far)."""
            t0 = time.perf_counter()
            spliced = False
            if out_host is not None:  # the usual case: one write of the whole batch
                if state["enc"] is None:
                    state["enc"] = open_encoder(out_host.shape[1:])
                for _ in range(state["leading"]):
                    self._write_all(state["enc"].stdin, out_host[0].numpy())
                    state["piped"] += out_host[0].numel()
                state["leading"] = 0
                body = out_host[:n_frames]
                if may_splice and splicer is not None and splicer.ok and body.is_contiguous():
                    spliced = splicer.splice_all(state["enc"].stdin.fileno(), body.data_ptr(), body.numel())
                if not spliced:
                    self._write_all(state["enc"].stdin, body.numpy())
                state["piped"] += body.numel()
                # (numpy's single-threaded copy, not tensor.clone(): a torch CPU op wakes the OpenMP pool -- one thread per
                # visible core, 256 on the bench box -- whose idle spinning burns the container's CPU quota (16 cores) and
                # gets reader, writer and both ffmpeg processes throttled: measured as ~20 ms lost per batch)
                state["last_good"] = torch.from_numpy(out_host[n_frames - 1].numpy().copy())
            else:
                for i, o in enumerate(per_frame):
                    if o is not None:
                        state["last_good"] = o
                    else:
                        state["substituted"] += 1
                        if state["last_good"] is not None:
                            o = state["last_good"]  # the previous good frame first (video_processor.py:66-77)
                        else:  # nothing before it: the next good frame, of this batch or of a later one
                            o = next((q for q in per_frame[i + 1:] if q is not None), None)
                            if o is None:
                                state["leading"] += 1
                                continue
                    if state["enc"] is None:
                        state["enc"] = open_encoder(o.shape)
                    buf = np.ascontiguousarray(o.numpy())
                    for _ in range(state["leading"] + 1):
                        self._write_all(state["enc"].stdin, buf)
                        state["piped"] += buf.size
                    state["leading"] = 0
            state["written"] += n_frames
            stats["write_s"] += time.perf_counter() - t0
            if spliced:
                stats["spliced_batches"] = stats.get("spliced_batches", 0) + 1
            return spliced

        def consumed_bytes():
            """bytes of the encoder pipe's stream that its reader has taken out of the pipe so far"""
            if state["enc"] is None:
                return 0
            return state["piped"] - _PipeSplicer.unread_bytes(state["enc"].stdin.fileno())

        def progress(done):
            frac = done / total_hint if total_hint else 0.5
            self._report_progress(0.1 + 0.8 * min(frac, 1.0), f"Processed {done}/{total_hint or '?'} frames")

        def new_out(shape):
            return torch.empty((batch_size,) + tuple(shape), dtype=torch.uint8, pin_memory=pin)

        done = 0
        t_wall = time.perf_counter()
        try:
            if overlap:
                done = self._pipe_overlapped(batch_size, frame_bytes, (h, w), out_geom, run, to_host, gpu_stream, target, read_batch, emit,
                                             progress, new_out, stats, dec, consumed_bytes, state, indexed_run=scene_run)
            else:
                stage = torch.empty(batch_size * frame_bytes, dtype=torch.uint8, pin_memory=pin)
                view = memoryview(stage.numpy())
                out_host = new_out(tuple(out_geom) + (3,)) if out_geom is not None else None
                target["out"] = out_host
                while True:
                    n_frames, got = read_batch(view)
                    if n_frames == 0:
                        break
                    host_frames = stage[:n_frames * frame_bytes].view(n_frames, h, w, 3)
                    t0 = time.perf_counter()
                    out, per_frame = self._batch_with_retries(host_frames, run, to_host, done if scene_run else None)
                    if out is not None:  # one copy into the pinned buffer
                        if out_host is None:
                            out_host = new_out(out.shape[1:])
                        if out.is_cuda:
                            out_host[:n_frames].copy_(out, non_blocking=True)
                        elif out.data_ptr() != out_host.data_ptr():   # (a host tensor: numpy's copy, see emit())
                            np.copyto(out_host[:n_frames].numpy(), out.numpy())
                        if out.is_cuda:
                            torch.cuda.current_stream(out.device).synchronize()
                    stats["gpu_wait_s"] += time.perf_counter() - t0
                    emit(out_host if out is not None else None, n_frames, per_frame)   # (one buffer, reused at once: copied, not spliced)
                    done += n_frames
                    progress(done)
                    if got < batch_size * frame_bytes:
                        break
            if state["substituted"]:
                print(f"Fixed {state['substituted']} failed frames by copying from nearest frames", file=sys.stderr)
            self._report_progress(0.9, "Finishing the encode...")
        finally:
            if dec.stdout:
                dec.stdout.close()
            rc_dec = dec.wait()
            rc_enc = 0
            if state["enc"] is not None:
                t0 = time.perf_counter()
                try:
                    state["enc"].stdin.close()
                except BrokenPipeError:
                    pass
                rc_enc = state["enc"].wait()
                stats["encoder_drain_s"] = time.perf_counter() - t0
            state.pop("slots", None)   # (only now may the pinned slot buffers go back to the allocator)
            stats["frames"] = done
            stats["wall_s"] = time.perf_counter() - t_wall
        if rc_dec != 0 or rc_enc != 0:
            raise RuntimeError(f"ffmpeg failed (decoder {rc_dec}, encoder {rc_enc})")
        if done == 0:
            raise ValueError("No frames extracted from video")
        if state["last_good"] is None:
            raise RuntimeError("no frame of the video could be processed")
        return done

    def _pipe_overlapped(self, batch_size, frame_bytes, in_geom, out_geom, run, to_host, gpu_stream, target, read_batch, emit, progress,
                         new_out, stats, dec, consumed_bytes, state, indexed_run=False) -> int:
        """The three concurrent stages of _stream_through_pipes (see there).  Slots rotate free -> filled -> submitted ->
        free; every blocking queue operation polls an abort flag, so an error in any stage (a dead encoder, a device that
        is gone, a malformed stream) ends the other two instead of leaving them blocked on a queue.  indexed_run: run takes
        the stream index of its first frame (_batch_with_retries: first_index)."""
        import queue
        import threading
        import time
        import torch
        h, w = in_geom
        pin = torch.cuda.is_available()

        class Slot:
            def __init__(self):
                self.inp = torch.empty(batch_size * frame_bytes, dtype=torch.uint8, pin_memory=pin)
                self.view = memoryview(self.inp.numpy())
                self.out = new_out(tuple(out_geom) + (3,)) if out_geom is not None else None

        slots = [Slot() for _ in range(max(2, int(self.PIPE_SLOTS)))]
        # (the last spliced slot's pages may still sit in the encoder pipe when this function returns: the caller keeps the slots
        # -- and with them their pinned memory, out of the allocator's hands -- until the encoder has exited)
        state["slots"] = slots
        free_q, filled_q, write_q = queue.Queue(), queue.Queue(), queue.Queue()
        for s in slots:
            free_q.put(s)
        abort = threading.Event()
        errors = []   # (stage, exception) in the order they happened

        class _Abort(Exception):
            pass

        def take(q):
            while True:
                try:
                    return q.get(timeout=0.05)
                except queue.Empty:
                    if abort.is_set():
                        raise _Abort() from None

        def fail(stage, e):
            errors.append((stage, e))
            abort.set()

        def reader():
            try:
                while True:
                    slot = take(free_q)
                    n_frames, got = read_batch(slot.view)
                    filled_q.put((slot, n_frames, got))
                    if n_frames == 0 or got < batch_size * frame_bytes:
                        return
            except _Abort:
                pass
            except BaseException as e:  # noqa: BLE001 - handed to the submitting thread, which re-raises it
                fail("reader", e)

        def writer():
            held = []   # [(slot, stream offset at which its spliced pages end)]: back to the reader once the encoder is past them
            try:
                while True:
                    item = take(write_q)
                    if item is None:
                        return
                    slot, n_frames, out_host, per_frame, event = item
                    if event is not None:
                        t0 = time.perf_counter()
                        event.synchronize()
                        stats["gpu_wait_s"] += time.perf_counter() - t0
                    own = out_host is not None and slot.out is not None and out_host.data_ptr() == slot.out.data_ptr()
                    if emit(out_host, n_frames, per_frame, may_splice=own):
                        held.append((slot, state["piped"]))
                    else:
                        free_q.put(slot)
                    # a spliced slot's pages are referenced by the pipe until read: with the next batch behind them in a
                    # pipe of at most 1 MiB they always are by now, but it is checked, not assumed (a stalled encoder)
                    if held:
                        seen = consumed_bytes()
                        while held and held[0][1] <= seen:
                            free_q.put(held.pop(0)[0])
                        while len(held) > 1:   # never sit on more than one: wait for the encoder instead of starving the reader
                            if abort.is_set():
                                raise _Abort()
                            time.sleep(0.0005)
                            seen = consumed_bytes()
                            while held and held[0][1] <= seen:
                                free_q.put(held.pop(0)[0])
            except _Abort:
                pass
            except BaseException as e:  # noqa: BLE001
                fail("writer", e)

        t_read = threading.Thread(target=reader, name="dp-pipe-reader", daemon=True)
        t_write = threading.Thread(target=writer, name="dp-pipe-writer", daemon=True)
        t_read.start()
        t_write.start()
        done = 0
        try:
            while True:
                slot, n_frames, got = take(filled_q)
                if n_frames == 0:
                    break
                host_frames = slot.inp[:n_frames * frame_bytes].view(n_frames, h, w, 3)
                t0 = time.perf_counter()
                target["out"] = slot.out
                out, per_frame = self._batch_with_retries(host_frames, run, to_host, done if indexed_run else None)
                event, out_host = None, None
                if out is not None and out.is_cuda:
                    # D2H into the slot's pinned buffer behind the kernels, on their stream; one event, no host wait
                    if slot.out is None or tuple(slot.out.shape[1:]) != tuple(out.shape[1:]):
                        slot.out = new_out(out.shape[1:])
                    with torch.cuda.device(out.device):
                        st = gpu_stream if gpu_stream is not None else torch.cuda.current_stream()
                        with torch.cuda.stream(st):
                            slot.out[:n_frames].copy_(out, non_blocking=True)
                            event = torch.cuda.Event()
                            event.record(st)
                    out_host = slot.out
                elif out is not None:
                    out_host = out   # on the host already (several devices: the workers wrote it into slot.out)
                stats["gpu_submit_s"] += time.perf_counter() - t0
                write_q.put((slot, n_frames, out_host, per_frame, event))
                done += n_frames
                progress(done)
                if got < batch_size * frame_bytes:
                    break
            write_q.put(None)
            while t_write.is_alive() and not abort.is_set():
                t_write.join(0.05)
        except _Abort:
            pass
        except BaseException:
            abort.set()
            raise
        finally:
            if abort.is_set():
                try:
                    dec.kill()   # a reader blocked in read() wakes up on the end of the stream
                except Exception:  # noqa: BLE001
                    pass
            t_read.join(5.0)
            t_write.join(5.0)
        if errors:
            raise errors[0][1]
        return done

    def process_video_streaming(self, input_path: str, output_path: str, ditherer: ImageDitherer,
                                pixelize_func=None, batch_size: int = 15,
                                final_resize_multiplier: Optional[int] = None, use_pipes: bool = True,
                                scene_palettes=None, downscale_filter: str = "nearest") -> bool:
        """video_processor.py:172-390; pixelize_func is the reference's tuple (method_str, max_size) or None.
        downscale_filter (an addition): the filter of the pixelization down-scale, as for process_frames; ValueError for an
        unknown name before anything is started.
        use_pipes (an addition): rawvideo pipes instead of the reference's PNG files on disk.
        scene_palettes (an addition; pipes path only): the list scan_scenes returns -- the palette switches at the scene
        boundaries (_stream_through_pipes).  None: one palette, the ditherer's, as ever.  ValueError, before anything is
        started: an empty list, overlapping scenes, a scene whose palette is None, use_pipes=False."""
        downscale_filter = _downscale_filter(downscale_filter)
        if scene_palettes is not None:
            from .scenes import check_scene_palettes
            if not use_pipes:
                raise ValueError("scene_palettes need the pipes path (use_pipes=True)")
            scene_palettes = check_scene_palettes(scene_palettes)
        if use_pipes:
            info = self.get_video_info(input_path)
            if not getattr(self, "_probe_ok", True):
                use_pipes = False  # frame size unknown: the PNG-file exchange below does not depend on it
                if scene_palettes is not None:
                    self._report_progress(1.0, "Error: could not probe the video's frame size")
                    print("Video processing error: scene palettes need the pipes path, and the frame size could not be probed",
                          file=sys.stderr)
                    return False
        if use_pipes:
            try:
                # the reference's milestones (0.0, 0.05, 0.1 ... 0.9, 1.0; video_processor.py:199-384) with messages that
                # say what this path does at them: decode, processing and encode run concurrently through the pipes
                self._report_progress(0.0, "Initializing video processing...")
                self._report_progress(0.05, "Starting the decoder...")
                method, max_size = (None, 64) if pixelize_func is None else pixelize_func
                self._report_progress(0.1, "Processing frames...")
                self._stream_through_pipes(input_path, output_path, ditherer, method, max_size, max(1, batch_size),
                                           final_resize_multiplier, info,   # reports 0.9 before it waits for the encoder
                                           scene_palettes=scene_palettes, downscale_filter=downscale_filter)
                self._report_progress(1.0, "Video processing complete!")
                return True
            except Exception as e:  # noqa: BLE001
                self._report_progress(1.0, f"Error: {str(e)}")
                print(f"Video processing error: {e}", file=sys.stderr)
                return False
        try:
            info = self.get_video_info(input_path)
            fps = info["fps"]
            self._report_progress(0.0, "Initializing video processing...")
            with tempfile.TemporaryDirectory() as tmp:
                tmp_dir = Path(tmp)
                self._report_progress(0.05, "Extracting frames...")
                pattern = str(tmp_dir / "frame_%05d.png")
                subprocess.run(["ffmpeg", "-i", input_path, "-qscale:v", "2", pattern], stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, check=True)
                frames = sorted(tmp_dir.glob("frame_*.png"))
                total = len(frames)
                if total == 0:
                    raise ValueError("No frames extracted from video")
                self._report_progress(0.1, f"Processing {total} frames...")
                method, max_size = (None, 64) if pixelize_func is None else pixelize_func
                failed, done = [], 0
                for lo in range(0, total, batch_size):
                    batch = frames[lo:lo + batch_size]
                    failed += self._process_batch(batch, ditherer, method, max_size, final_resize_multiplier, downscale_filter)
                    done += len(batch)
                    self._report_progress(0.1 + 0.8 * (done / total), f"Processed {done}/{total} frames")
                if failed:
                    print(f"Fixing {len(failed)} failed frames by copying from nearest frames...", file=sys.stderr)
                    self._fix_failed_frames(failed, frames)
                self._report_progress(0.9, "Encoding final video...")
                subprocess.run(["ffmpeg", "-y", "-framerate", f"{fps:.5f}", "-i", pattern, "-i", input_path,
                                "-map", "0:v:0", "-map", "1:a?", "-map", "1:s?", "-c:v", "libx264", "-preset",
                                "medium", "-crf", "18", "-pix_fmt", "yuv420p", "-vframes", str(total), "-c:a", "copy",
                                "-c:s", "copy", output_path], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                               check=True)
                self._report_progress(1.0, "Video processing complete!")
                return True
        except Exception as e:  # noqa: BLE001
            self._report_progress(1.0, f"Error: {str(e)}")
            print(f"Video processing error: {e}", file=sys.stderr)
            return False
