"""Per-scene palettes for video: where a clip cuts, and which palette each scene gets.

A 16- or 32-colour palette fitted to a clip that cuts between a dark interior and a bright exterior serves neither scene.
VideoProcessor.scan_scenes finds the cuts on the device while the decoded frames are resident in HBM anyway
(backend.SceneStream: a 4096-bin colour signature per frame, the L1 distance between consecutive signatures), fits one
clip_palette.ClipPalette per scene and returns a list of Scene; process_video_streaming(..., scene_palettes=scenes) switches
palettes at the boundaries.  This module holds the host side of that: the Scene record and two pure functions.

Parity definitions: there is no counterpart in the reference.  A signature is np.bincount of the cell
ids (r>>4)<<8 | (g>>4)<<4 | (b>>4) of a frame, a distance the int64 L1 of consecutive signatures, a scene's palette what a
fresh ClipPalette(use_gamma).add(frames[start:end], every) gives, streaming output process_frames run scene by scene.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple


class Scene(NamedTuple):
    """Frames start ... end-1 of the stream and the palette fitted to them (a list of (r, g, b) tuples, or None)."""
    start: int
    end: int
    palette: Optional[List[Tuple[int, int, int]]]


def _check_cut_parameters(threshold, min_scene_frames):
    if not 0.0 < float(threshold) <= 1.0:
        raise ValueError(f"threshold must be in (0, 1], not {threshold!r}")
    if int(min_scene_frames) != min_scene_frames or int(min_scene_frames) < 1:
        raise ValueError(f"min_scene_frames must be an integer >= 1, not {min_scene_frames!r}")


def scene_cuts(distances, n_px, threshold, min_scene_frames, carry=0):
    """Which frames of a batch start a new scene -> (starts, carry): `starts` the indices i into `distances` (ascending),
    `carry` the number of frames the scene that is open after the batch holds so far -- hand it to the call for the next
    batch of the same stream; any cutting of a stream into batches then gives the starts of one call over the whole stream.

    distances[i]: the signature distance of frame i to the frame before it (backend.SceneStream.add, read back), an integer
    in 0 ... 2 * n_px.  Frame i starts a scene when int(distances[i]) > threshold * 2 * n_px -- a Python int against a Python
    float product, strictly: equality is not a cut -- and the open scene already holds at least min_scene_frames frames.
    carry = 0 is the start of the stream: its first frame opens the first scene and is never reported as a cut.
    ValueError: threshold outside (0, 1], min_scene_frames < 1, n_px < 1, carry < 0."""
    _check_cut_parameters(threshold, min_scene_frames)
    if int(n_px) < 1:
        raise ValueError(f"n_px must be >= 1, not {n_px!r}")
    if int(carry) < 0:
        raise ValueError(f"carry must be >= 0, not {carry!r}")
    bar = float(threshold) * 2 * int(n_px)
    need, held = int(min_scene_frames), int(carry)
    starts = []
    for i, d in enumerate(distances):
        if int(d) > bar and held >= need:
            starts.append(i)
            held = 0
        held += 1
    return starts, held


def split_at(first, n, starts):
    """The pieces of the batch of stream frames [first, first + n) cut at the scene starts that fall inside it: yields
    (lo, hi) stream-index pairs in order, lo < hi, that tile the batch; every piece lies within one scene.  A start at
    `first` itself, or outside the batch, cuts nothing."""
    first, end = int(first), int(first) + int(n)
    lo = first
    for s in sorted({int(s) for s in starts}):
        if lo < s < end:
            yield lo, s
            lo = s
    if lo < end:
        yield lo, end


def check_scene_palettes(scenes):
    """What process_video_streaming asks of its scene_palettes -> the list as Scene records.  ValueError: an empty list, a
    scene that is empty or starts before its predecessor ends, a scene without a palette."""
    scenes = [Scene(*s) for s in (scenes or [])]
    if not scenes:
        raise ValueError("scene_palettes is empty: pass None for one palette over the whole clip")
    at = None
    for k, s in enumerate(scenes):
        if int(s.start) < 0 or int(s.end) <= int(s.start):
            raise ValueError(f"scene {k} covers no frame: [{s.start}, {s.end})")
        if at is not None and int(s.start) < at:
            raise ValueError(f"scene {k} starts at frame {s.start}, inside or before its predecessor (which ends at {at}): "
                             "scenes must be in stream order and must not overlap")
        if not s.palette:
            raise ValueError(f"scene {k} has no palette (scan_scenes(source=None) returns boundaries only)")
        at = int(s.end)
    return scenes


def scene_of(scenes, frame):
    """Index of the scene whose palette stream frame `frame` takes: the last scene that starts at or before it (so frames
    past the last scene's end, and frames in a gap, use the scene before them), the first scene for earlier frames."""
    k = 0
    for j, s in enumerate(scenes):
        if int(s.start) <= frame:
            k = j
    return k
