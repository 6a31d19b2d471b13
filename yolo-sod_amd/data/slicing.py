"""Tile planner for sliced inference: a large frame is cut into overlapping tiles at native resolution, the model runs
on every tile (and, optionally, on the whole frame), and all candidates meet in one NMS in frame coordinates
(``engine/predictor.py`` ``SlicedPredictor``, ``csrc/tile_merge.hip``).

The reference has no slicing; the rule here is this project's own definition. Per axis with extent ``n``, requested
tile size ``s`` and overlap ratio ``0 <= r < 1``:

* ``t = min(s, n)``; ``step = t - floor(r * t)`` (the floor of the double product), refused below 1;
* starts ``0, step, 2 step, ...`` while ``start + t < n``, then the last start ``n - t``, flush with the far border
  (dropped if it equals the previous start).

So every tile is exactly ``t_y x t_x``, the tiles cover the frame, neighbours overlap by at least ``floor(r * t)`` and
an axis with ``n <= s`` has one tile. Tiles are listed row-major (y outer, x inner). Only host arithmetic on shapes
lives here."""
from __future__ import annotations

import math
from dataclasses import dataclass

from .augment import LetterBox


def _pair(v, name):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"slice_grid: {name} must be a number or a (y, x) pair, got {v!r}")
        return v[0], v[1]
    return v, v


def axis_starts(n: int, s: int, r: float):
    """``(t, starts)`` of one axis (module docstring)."""
    n, s = int(n), int(s)
    if n < 1 or s < 1:
        raise ValueError(f"slice_grid: extent {n} / tile size {s} must be >= 1")
    if not 0 <= r < 1:
        raise ValueError(f"slice_grid: overlap ratio {r} outside [0, 1)")
    t = min(s, n)
    step = t - int(math.floor(r * t))
    if step < 1:
        raise ValueError(f"slice_grid: overlap {r} of a {t}-pixel tile leaves a step of {step}")
    starts = list(range(0, max(n - t, 0), step))  # start + t < n
    if not starts or starts[-1] != n - t:
        starts.append(n - t)
    return t, starts


def slice_grid(shape, slice=640, overlap=0.2):
    """Tiles ``(y0, x0, y1, x1)`` (integers, end exclusive) of a frame ``(H, W)``, row-major."""
    H, W = int(shape[0]), int(shape[1])
    sh, sw = _pair(slice, "slice")
    rh, rw = _pair(overlap, "overlap")
    th, ys = axis_starts(H, sh, rh)
    tw, xs = axis_starts(W, sw, rw)
    return [(y0, x0, y0 + th, x0 + tw) for y0 in ys for x0 in xs]


def way_back(canvas, shape):
    """``(gain, pad_x, pad_y)`` that take canvas coordinates back to a letterboxed ``(h, w)`` image's own pixels:
    ``scale_boxes``' own rule (ratio_pad=None, ops.py:92-105), as ``DetectionPredictor.ingest`` puts it in ``geom``."""
    h0, w0 = int(shape[0]), int(shape[1])
    gain = min(canvas[0] / h0, canvas[1] / w0)
    return gain, round((canvas[1] - w0 * gain) / 2 - 0.1), round((canvas[0] - h0 * gain) / 2 - 0.1)


@dataclass(frozen=True)
class Slot:
    """One model input of a frame: the rectangle ``rect`` = (y0, x0, y1, x1) it shows (the whole frame for the
    full-frame slot), its letterbox ``geometry`` on the canvas (``LetterBox.geometry``), the way back (``gain``,
    ``pad_x``, ``pad_y``) and which of its edges are ``interior`` to the frame: (left, right, top, bottom)."""

    rect: tuple
    geometry: tuple
    gain: float
    pad_x: int
    pad_y: int
    interior: tuple
    full: bool = False

    @property
    def shape(self):
        return self.rect[2] - self.rect[0], self.rect[3] - self.rect[1]


class SlicePlan:
    """The slots of a batch of frames. ``slots[f]`` lists frame f's slots: the whole frame first when ``full_frame``,
    then its tiles in grid order. ``S`` is the largest slot count of the batch (the slot axis of the merged tensor),
    ``order`` the flat list of ``(frame, slot)`` in the order the tiles go through the model, ``canvas`` the one
    canvas every slot is letterboxed onto."""

    def __init__(self, shapes, slice=640, overlap=0.2, full_frame=True, imgsz=640, stride=32):
        self.shapes = [(int(s[0]), int(s[1])) for s in shapes]
        if not self.shapes:
            raise ValueError("SlicePlan: no frames")
        self.imgsz = (imgsz, imgsz) if isinstance(imgsz, int) else (int(imgsz[0]), int(imgsz[1]))
        self.slice, self.overlap, self.full_frame = slice, overlap, bool(full_frame)
        lb = LetterBox(self.imgsz, auto=False, stride=stride)
        self.pad_value = lb.pad_value
        self.canvas = self.imgsz
        self.slots = []
        for H, W in self.shapes:
            rects = [(0, 0, H, W)] if self.full_frame else []
            rects += slice_grid((H, W), slice, overlap)
            row = []
            for k, (y0, x0, y1, x1) in enumerate(rects):
                full = self.full_frame and k == 0
                geometry = lb.geometry((y1 - y0, x1 - x0))
                assert tuple(geometry[4:]) == self.canvas
                gain, px, py = way_back(self.canvas, (y1 - y0, x1 - x0))
                interior = (False,) * 4 if full else (x0 > 0, x1 < W, y0 > 0, y1 < H)
                row.append(Slot((y0, x0, y1, x1), tuple(geometry), gain, px, py, interior, full))
            self.slots.append(row)
        self.S = max(len(r) for r in self.slots)
        self.order = [(f, k) for f, row in enumerate(self.slots) for k in range(len(row))]

    def __len__(self):
        return len(self.order)

    def slot(self, frame, slot) -> Slot:
        return self.slots[frame][slot]

    def chunks(self, batch):
        """``[lo, hi)`` ranges of ``order`` of at most ``batch`` tiles each."""
        n = len(self.order)
        return [(lo, min(lo + batch, n)) for lo in range(0, n, batch)]

    def merge_rows(self, lo, hi):
        """The descriptor rows (``_hip.tile_merge``) of the model call that ran ``order[lo:hi]``: row i of its output is
        tile ``order[lo + i]``. The empty slots of a frame with fewer than ``S`` slots ride along with the call that
        holds the frame's last tile, as ``src = -1`` rows, so that over the calls of one batch every (frame, slot) of
        the merged tensor is named exactly once."""
        rows = []
        for i in range(lo, hi):
            f, k = self.order[i]
            s = self.slots[f][k]
            y0, x0, y1, x1 = s.rect
            rows.append((i - lo, f, k, s.gain, s.pad_x, s.pad_y, x0, y0, x1 - x0, y1 - y0, s.interior))
            if k == len(self.slots[f]) - 1:
                rows += [(-1, f, e, 1.0, 0, 0, 0, 0, 0, 0, (False,) * 4) for e in range(k + 1, self.S)]
        return rows
