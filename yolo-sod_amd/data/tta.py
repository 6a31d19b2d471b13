"""Test-time augmentation, host side: the geometry of ``DetectionModel._predict_augment`` (the reference's
``nn/tasks.py:381-418`` with ``scale_img``, ``utils/torch_utils.py:423-432``) as integers, for the two HIP launches
around the model calls (``csrc/tta.hip``: ``_hip.tta_views``, ``_hip.tta_merge``). Host arithmetic only.

A branch is one model call: the batch scaled by ``scale`` (bilinear, to ``(int(h * r), int(w * r))``), flipped
(None, 2 up-down, 3 left-right) and padded with 0.447 to ``ceil(v * r / gs) * gs`` with ``gs`` the largest stride; a
scale of exactly 1 is not resized or padded (``scale_img`` returns its input), and with no flip either the model runs on
the batch itself. Of the first branch's anchors the last ``(A // g) * 1`` are dropped and of the last branch's the
first ``(A // g) * 4 ** (nl - 1)``, ``g = sum(4 ** k for k in range(nl))`` (``_clip_augmented``); what is kept is
concatenated along the anchor axis in branch order."""
from __future__ import annotations

import math
from dataclasses import dataclass

DEFAULT_SCALES = (1, 0.83, 0.67)
DEFAULT_FLIPS = (None, 3, None)


@dataclass(frozen=True)
class TTABranch:
    """One model call: ``view`` = (flip, sh, sw, ph, pw) as ``_hip.tta_views`` takes it (None: the batch itself),
    ``A`` its anchor count, and its kept anchors [src_lo, src_lo + n) placed at [dst, dst + n) of the concatenation."""

    scale: float
    flip: int | None
    resized: tuple
    padded: tuple
    view: tuple | None
    A: int
    src_lo: int
    n: int
    dst: int


def _level_extent(n: int, stride: int) -> int:
    """Extent of the feature map of this stride over n pixels: one ceil(n / 2) per stride-2 stage."""
    if stride & (stride - 1):
        return -(-n // stride)
    while stride > 1:
        n, stride = (n + 1) // 2, stride // 2
    return n


class TTAPlan:
    def __init__(self, shape, scales=DEFAULT_SCALES, flips=DEFAULT_FLIPS, *, stride, nl):
        """``shape`` = (h, w) of the batch; ``stride``: the largest stride (levels of stride, stride / 2, ...: ``nl``
        of them) or the strides of all levels; ``nl``: the number of detection levels."""
        h, w = int(shape[0]), int(shape[1])
        if h < 1 or w < 1:
            raise ValueError(f"TTAPlan: shape {tuple(shape)}")
        scales, flips = tuple(scales), tuple(flips)
        if not scales or len(scales) != len(flips):
            raise ValueError(f"TTAPlan: {len(scales)} scales with {len(flips)} flips")
        nl = int(nl)
        if nl < 1:
            raise ValueError(f"TTAPlan: nl={nl}")
        if isinstance(stride, (int, float)):
            strides = [int(stride) >> k for k in range(nl)]
        else:
            strides = [int(s) for s in stride]
        if len(strides) != nl or min(strides) < 1:
            raise ValueError(f"TTAPlan: strides {strides} for {nl} levels")
        gs = max(strides)
        self.shape, self.scales, self.flips, self.nl, self.gs = (h, w), scales, flips, nl, gs
        self.strides = tuple(strides)
        geo = []
        for r, f in zip(scales, flips):
            if f not in (None, 2, 3):
                raise ValueError(f"TTAPlan: flip {f} (None, 2 up-down or 3 left-right)")
            if not (r > 0 and r < float("inf")):
                raise ValueError(f"TTAPlan: scale {r}")
            if r == 1.0:  # scale_img returns its input
                resized = padded = (h, w)
            else:
                resized = (int(h * r), int(w * r))
                padded = tuple(math.ceil(v * r / gs) * gs for v in (h, w))
            if min(resized) < 1 or resized[0] > padded[0] or resized[1] > padded[1]:
                raise ValueError(f"TTAPlan: scale {r} of {h}x{w} gives {resized} in {padded}")
            A = sum(_level_extent(padded[0], s) * _level_extent(padded[1], s) for s in strides)
            geo.append((r, f, resized, padded, A))
        # _clip_augmented: the tail of the first branch, the head of the last
        g = sum(4 ** k for k in range(nl))
        lo = [0] * len(geo)
        hi = [b[4] for b in geo]
        cut_first = (geo[0][4] // g) * 1
        cut_last = (geo[-1][4] // g) * 4 ** (nl - 1)
        if cut_first < 1:
            raise ValueError(f"TTAPlan: {geo[0][4]} anchors in the first branch, fewer than {g}")
        hi[0] -= cut_first
        lo[-1] += cut_last
        self.branches = []
        dst = 0
        for (r, f, resized, padded, A), a, b in zip(geo, lo, hi):
            if b - a < 1:
                raise ValueError(f"TTAPlan: branch of scale {r} keeps no anchor")
            view = None if (r == 1.0 and f is None) else (f, *resized, *padded)
            self.branches.append(TTABranch(float(r), f, resized, padded, view, A, a, b - a, dst))
            dst += b - a
        self.A_tot = dst
        self.views = [b.view for b in self.branches if b.view is not None]
        self._desc = {}  # _hip.tta_views' uploaded descriptor tables

    def __len__(self):
        return len(self.branches)

    def locate(self, index: int):
        """(branch, anchor of that branch's own output) of an index into the concatenation, as NMS returns it."""
        index = int(index)
        if not 0 <= index < self.A_tot:
            raise IndexError(f"TTAPlan.locate: {index} outside [0, {self.A_tot})")
        for k, b in enumerate(self.branches):
            if index < b.dst + b.n:
                return k, b.src_lo + index - b.dst
        raise AssertionError

    def index(self, branch: int, anchor: int):
        """Inverse of :meth:`locate`; None for an anchor that the clip drops."""
        b = self.branches[branch]
        if not b.src_lo <= anchor < b.src_lo + b.n:
            return None
        return b.dst + anchor - b.src_lo

    def make_views(self, x):
        """The model's input of every branch (the batch itself for an unflipped scale of 1): one ``_hip.tta_views``
        launch for all the others."""
        from .. import _hip
        made = iter(_hip.tta_views(x, self.views, cache=self._desc)) if self.views else iter(())
        return [x if b.view is None else next(made) for b in self.branches]

    def merge(self, k: int, y, cat):
        """Branch k's output into ``cat`` [B, 4+nc, A_tot]: one ``_hip.tta_merge`` launch."""
        from .. import _hip
        b = self.branches[k]
        if int(y.shape[-1]) != b.A:
            raise RuntimeError(f"TTAPlan: branch {k} ({b.padded[0]}x{b.padded[1]}) has {int(y.shape[-1])} anchors, "
                               f"{b.A} planned (strides {self.strides})")
        return _hip.tta_merge(y, cat, b.src_lo, b.n, b.dst, b.scale, b.flip, self.shape)
