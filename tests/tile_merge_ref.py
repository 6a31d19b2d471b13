"""Test helper: the CPU restatement of the tile merge (``csrc/tile_merge.hip``) in numpy float32. The product has no
CPU path; this file is the definition the kernel is tested against, bit for bit.

Per anchor of source row ``src`` going to ``merged[frame][:, slot*A : (slot+1)*A]`` (every operation rounds to fp32;
numpy never contracts a multiply and an add, and 0.5 * b is exact, so contraction could not change the result):
    bx = (x - pad_x) / gain;  by = (y - pad_y) / gain;  bw = w / gain;  bh = h / gain
    cut = cut_margin >= 0 and ((left  and bx - 0.5 bw <= cut_margin) or (right  and bx + 0.5 bw >= tile_w - cut_margin)
                            or (top   and by - 0.5 bh <= cut_margin) or (bottom and by + 0.5 bh >= tile_h - cut_margin))
    box = bx + off_x, by + off_y, bw, bh;  score_c = 0 if cut else score_c
``src = -1`` writes zeros. Rows are ``SlicePlan.merge_rows``' tuples."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def tile_merge_ref(y: np.ndarray, rows, merged: np.ndarray, A: int, cut_margin=None) -> np.ndarray:
    """``y`` [n, 4+nc, A] float32, ``merged`` [F, 4+nc, S*A] float32 (written in place, only the named slots)."""
    assert y.dtype == np.float32 and merged.dtype == np.float32 and y.shape[2] == A and merged.shape[2] % A == 0
    cm = f32(-1.0 if cut_margin is None else cut_margin)
    half = f32(0.5)
    for src, frame, slot, gain, pad_x, pad_y, off_x, off_y, tile_w, tile_h, interior in rows:
        dst = merged[frame, :, slot * A:(slot + 1) * A]
        if src < 0:
            dst[:] = 0
            continue
        gain, pad_x, pad_y, off_x, off_y = f32(gain), f32(pad_x), f32(pad_y), f32(off_x), f32(off_y)
        tile_w, tile_h = f32(tile_w), f32(tile_h)
        x, yy, w, h = y[src, 0], y[src, 1], y[src, 2], y[src, 3]
        with np.errstate(all="ignore"):
            bx, by, bw, bh = (x - pad_x) / gain, (yy - pad_y) / gain, w / gain, h / gain
            assert bx.dtype == np.float32
            cut = np.zeros(A, dtype=bool)
            if cm >= 0:
                left, right, top, bottom = (bool(v) for v in interior)
                if left:
                    cut |= bx - half * bw <= cm
                if right:
                    cut |= bx + half * bw >= tile_w - cm
                if top:
                    cut |= by - half * bh <= cm
                if bottom:
                    cut |= by + half * bh >= tile_h - cm
            dst[0], dst[1], dst[2], dst[3] = bx + off_x, by + off_y, bw, bh
        dst[4:] = np.where(cut[None], f32(0), y[src, 4:])
    return merged
