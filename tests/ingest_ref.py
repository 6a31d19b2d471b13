"""Test helper: the CPU restatement of the fused ingest (``csrc/ingest.hip``) in numpy int64 - the integer bilinear
resize (cv2 INTER_LINEAR geometry, 11-bit coefficients, one rounding), the 114 border, BGR -> RGB, HWC -> CHW and
uint8 -> float / 255 on the CPU. The product has no CPU path; this file is the definition the kernel is tested against.

Per axis (source extent n, destination extent m, destination index d):
    num = (2d + 1) n - m, den = 2m;  num < 0: s = 0, a = 0;  else s = num // den, a = ((num % den) * 2048 + m) // den
    s >= n - 1: s = n - 1, a = 0;  s1 = min(s + 1, n - 1)
    q = ((2048-ax)(2048-ay) p[y][x] + ax (2048-ay) p[y][x1] + (2048-ax) ay p[y1][x] + ax ay p[y1][x1] + 2^21) >> 22
"""
from __future__ import annotations

import numpy as np
import torch


def axis_map(n: int, m: int):
    """(s, s1, a) int64 arrays of length m."""
    d = np.arange(m, dtype=np.int64)
    num = (2 * d + 1) * n - m
    den = 2 * m
    neg = num < 0
    nn = np.where(neg, 0, num)
    s = np.where(neg, 0, nn // den)
    a = np.where(neg, 0, ((nn % den) * 2048 + m) // den)
    edge = s >= n - 1
    s = np.where(edge, n - 1, s)
    a = np.where(edge, 0, a)
    return s, np.minimum(s + 1, n - 1), a


def resize_u8(img: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """[h, w, C] uint8 -> [new_h, new_w, C] uint8."""
    h, w = img.shape[:2]
    p = img.astype(np.int64)
    sy, sy1, ay = axis_map(h, new_h)
    sx, sx1, ax = axis_map(w, new_w)
    ay, ax = ay[:, None, None], ax[None, :, None]
    q = ((2048 - ax) * (2048 - ay) * p[sy][:, sx] + ax * (2048 - ay) * p[sy][:, sx1]
         + (2048 - ax) * ay * p[sy1][:, sx] + ax * ay * p[sy1][:, sx1] + (1 << 21)) >> 22
    assert q.min() >= 0 and q.max() <= 255
    return q.astype(np.uint8)


def canvas_u8(frame_bgr: np.ndarray, geom, pad: int = 114) -> np.ndarray:
    """The letterboxed frame as uint8 [out_h, out_w, 3], still BGR; geom = (new_h, new_w, top, left, out_h, out_w)."""
    new_h, new_w, top, left, out_h, out_w = (int(v) for v in geom)
    c = np.full((out_h, out_w, 3), pad, dtype=np.uint8)
    c[top:top + new_h, left:left + new_w] = resize_u8(np.asarray(frame_bgr), new_h, new_w)
    return c


def ingest_ref(frames, geoms, pad: int = 114) -> torch.Tensor:
    """[B, 3, out_h, out_w] float32 on the CPU: RGB planes, uint8 -> .float() / 255 (torch's CPU division)."""
    cs = [torch.from_numpy(np.ascontiguousarray(canvas_u8(f, g, pad)[:, :, ::-1].transpose(2, 0, 1)))
          for f, g in zip(frames, geoms)]
    return torch.stack(cs).float() / 255
