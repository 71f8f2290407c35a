"""Frames of the clip fixtures (tests/golden/clip.json) from their specifications: seeded formulas of oracle/oracle.py plus
three clip-specific kinds, so that any machine regenerates the inputs."""
import numpy as np

from oracle.oracle import grad, imgl, rnd


def clip_frames(specs):
    frames = []
    for s in specs:
        kind = s[0]
        if kind == "rnd":
            f = rnd(s[1], s[2], s[3])
        elif kind == "imgl":
            f = imgl(s[1], s[2], s[3], s[4])
        elif kind == "grad":
            f = grad(s[1], s[2])
        elif kind == "flat":
            f = np.empty((s[1], s[2], 3), np.uint8)
            f[:] = np.array(s[3], np.uint8)
        elif kind == "few":      # h x w pixels drawn from n random colours
            rs = np.random.RandomState(s[4])
            cols = rs.randint(0, 256, (s[3], 3)).astype(np.uint8)
            f = cols[rs.randint(0, s[3], (s[1], s[2]))]
        elif kind == "sub":      # h x w pixels drawn from an earlier frame's pixels: no new colour
            src = frames[s[3]].reshape(-1, 3)
            f = src[np.random.RandomState(s[4]).randint(0, len(src), (s[1], s[2]))]
        else:
            raise ValueError(s)
        frames.append(np.ascontiguousarray(f, np.uint8))
    return frames
