"""One palette fitted to a whole clip: streaming median cut and k-means over frames.

The video path otherwise takes its palette the way a single image does -- ImageDitherer(palette=None) cuts the FIRST frame,
as the reference's CLI and GUI do with reduce_colors(first_frame) / generate_kmeans_palette(first_frame) -- so a clip that
opens on a fade-in, a title card or a dark shot is dithered end to end with a palette that knows nothing of the rest.
ClipPalette accumulates frames batch by batch (they need not be resident together, nor of one geometry) into
  * backend.DistinctStream   the distinct colours in order of first occurrence over the stream (dp_distinct_stream_add_u8), and
  * backend.ColourHistogram  count[colour] over all 2^24 colours (dp_kmeans_hist_build_u8, accumulate = 1),
and fits either palette from them at any time; a fit does not consume the accumulator, more frames may follow.

Parity definitions.
  median cut  equal to the reference's ColorReducer.reduce_colors(image, n) where `image` is the taken frames stacked top to
              bottom (linearised first under use_gamma): `set(image.getdata())` of the stack inserts the colours in stream
              order, which is the order DistinctStream keeps.  Independent of how the stream was batched.
  k-means     a pure function of the clip's colour MULTISET: it does not depend on batching, on frame order or on how frames
              were split over add() calls.  The k-means++ seeds are drawn from the pixels at ranks
              RandomState(random_state).randint(0, n_pixels, 10000) (all pixels when there are at most 10 000) with the
              clip's pixels laid out in HISTOGRAM order (ColourHistogram.sample), then Lloyd runs over the histogram exactly
              as kmeans.fit_palette runs it.  This is deliberately not fit_palette's raster-index sample (the image path is
              untouched): above 10 000 pixels the reference samples unseeded and has no single answer, so there is nothing
              tighter to match.
  oklab       the integer Oklab fit of include/ditherpie_hip_okfit.h over the histogram's occupied colours: all integer, no
              random numbers, a pure function of the clip's colour multiset by construction (the points are the distinct
              colours in code order, every sum is an integer sum); its entries are colours of the clip.  Not with use_gamma.
"""
from __future__ import annotations

import numpy as np

from . import _tables

_LUT_CHUNK = 1 << 22   # bytes linearised per indexing step under use_gamma (the index tensor is 8 bytes per byte)


class ClipPalette:
    """ClipPalette(use_gamma=False, device=None).add(frames).add(more)...  then .median_cut(n), .kmeans(n) and / or .oklab(n)."""

    def __init__(self, use_gamma=False, device=None):
        import torch
        from . import backend
        backend.require_gpu()
        dev = torch.device(device or "cuda")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.use_gamma = bool(use_gamma)
        self._distinct = backend.DistinctStream(dev)
        self._hist = backend.ColourHistogram(device=dev)
        self._seen_frames = 0    # frames offered so far, taken or not: `every` counts across calls
        self._taken_frames = 0
        self._lut = None

    def _linear(self, f):
        import torch
        if self._lut is None:
            self._lut = torch.from_numpy(np.ascontiguousarray(_tables.LUT_IN)).to(self.device)
        flat = f.reshape(-1)
        out = torch.empty_like(flat)
        for a in range(0, flat.numel(), _LUT_CHUNK):
            out[a:a + _LUT_CHUNK] = self._lut[flat[a:a + _LUT_CHUNK].long()]
        return out.view(f.shape)

    def add(self, frames, every=1):
        """frames: uint8 CUDA tensor [N,H,W,3] or [H,W,3] on this object's device.  Takes every `every`-th frame of the
        STREAM (counted across calls: frames 0, every, 2 every, ... of everything offered so far), linearises the taken
        frames through _tables.LUT_IN under use_gamma (as ImageDitherer._ensure_palette does) and feeds them to the
        distinct stream and to the histogram.  Geometry may differ from call to call.  Returns self."""
        import torch
        from . import backend
        f = backend._frames(frames)
        if f.device != self.device:
            raise ValueError(f"the clip palette lives on {self.device}, frames on {f.device}")
        every = int(every)
        if every < 1:
            raise ValueError("every must be >= 1")
        n = f.shape[0]
        first = (-self._seen_frames) % every   # the first frame of this call that the stream's stride lands on
        self._seen_frames += n
        if first >= n or f[0].numel() == 0:
            return self
        take = f[first::every] if (every > 1 or first) else f
        with torch.cuda.device(self.device):
            px = take.contiguous()
            if self.use_gamma:
                px = self._linear(px)
            px = px.view(-1, 3)
            if self._hist.n + px.shape[0] >= 1 << 32:
                raise ValueError("a clip palette holds fewer than 2^32 pixels: sample the clip with `every`")
            self._distinct.add(px)
            if self._hist.n == 0:
                self._hist.add(px, accumulate=False)   # (the first build defines every slice of the table)
            else:
                self._hist.add(px, accumulate=True)
        self._taken_frames += take.shape[0]
        return self

    def reset(self):
        """Forget every frame: the distinct stream is cleared (dp_distinct_stream_reset), the histogram starts over with the
        next add (its first build defines every slice of the table) and the frame counters -- `every` counts from the next
        frame offered -- go back to zero.  The object then behaves as a fresh one; its 114 MB of device buffers are kept.
        Runs on the caller's current stream, as add() does.  Returns self."""
        import torch
        with torch.cuda.device(self.device):
            self._distinct.reset()
        self._hist.n = 0
        self._seen_frames = 0
        self._taken_frames = 0
        return self

    @property
    def n_pixels(self):
        return self._hist.n

    @property
    def n_frames(self):
        return self._taken_frames

    @property
    def n_distinct(self):
        return len(self._distinct)

    def colours(self):
        """The clip's distinct colours in stream order -> uint8 tensor [n_distinct, 3] on the device."""
        return self._distinct.colours()

    def median_cut(self, num_colors):
        """Median cut over the clip's distinct colours -> list of 2**int(log2(num_colors)) (r, g, b) tuples: the
        reference's reduce_colors on the taken frames stacked top to bottom (module docstring).  The list comes down to
        the host; dp_median_cut_host replays the reference's set order and cuts, with reduce_colors' own fallback."""
        from .dithering_lib import ColorReducer
        if self.n_pixels == 0:
            raise ValueError("the clip palette holds no pixels yet")
        return ColorReducer._median_cut_of_distinct(self.colours().cpu().numpy(), num_colors)

    def seed_ranks(self, random_state=42):
        """The pixel ranks (histogram order) the k-means seeding looks at."""
        from .kmeans import SAMPLE
        n = self.n_pixels
        if n <= SAMPLE:
            return np.arange(n, dtype=np.int64)
        return np.random.RandomState(random_state).randint(0, n, SAMPLE).astype(np.int64)

    def kmeans_fit(self, num_colors, random_state=42, max_iter=300, tol=1e-4):
        """-> (palette list, centres float64 [K,3], inertia, n_iter), as kmeans.fit_palette returns them."""
        import torch
        from . import backend, kmeans
        K = int(num_colors)
        if K > backend.KMEANS_HIST_MAX_K:
            raise ValueError(f"a clip k-means palette has at most {backend.KMEANS_HIST_MAX_K} colours, not {K}")
        if K < 1:
            raise ValueError("num_colors must be >= 1")
        if self.n_pixels == 0:
            raise ValueError("the clip palette holds no pixels yet")
        with torch.cuda.device(self.device):
            sample = self._hist.sample(self.seed_ranks(random_state))
            init = kmeans.kmeans_plusplus_device(sample, K, np.random.RandomState(random_state))
            centers, inertia, n_iter = kmeans.lloyd(None, init, max_iter=max_iter, tol=tol, hist=self._hist, centres_are_data_points=True)
        palette = [tuple(int(v) for v in c) for c in centers.astype(int)]
        return palette, centers, inertia, n_iter

    def kmeans(self, num_colors, random_state=42, max_iter=300, tol=1e-4):
        """A k-means palette of the clip -> list of num_colors (r, g, b) tuples; a pure function of the clip's colour
        multiset (module docstring).  ValueError above backend.KMEANS_HIST_MAX_K colours and for an empty clip."""
        return self.kmeans_fit(num_colors, random_state, max_iter, tol)[0]

    def oklab_fit(self, num_colors, max_iter=100):
        """-> (palette list, centres int32 [K,3] in the integer Oklab, n_iter, distortion) of backend.okfit over the clip's
        histogram.  ValueError above backend.OKFIT_MAX_COLORS colours, for an empty clip and with use_gamma=True."""
        import torch
        from . import backend
        K, max_iter = backend._okfit_args(num_colors, max_iter)
        if self.use_gamma:
            raise ValueError("use_gamma=True cannot be combined with the 'oklab' palette fit: Oklab linearises by itself")
        if self.n_pixels == 0:
            raise ValueError("the clip palette holds no pixels yet")
        with torch.cuda.device(self.device):
            pal, centres, n_iter, distortion = backend.okfit(self._hist, K, max_iter)
        return [tuple(int(v) for v in c) for c in pal], centres, n_iter, distortion

    def oklab(self, num_colors, max_iter=100):
        """An Oklab-fitted palette of the clip -> list of num_colors (r, g, b) tuples, each a colour of the clip; a pure
        function of the clip's colour multiset (module docstring)."""
        return self.oklab_fit(num_colors, max_iter)[0]
