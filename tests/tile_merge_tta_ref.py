"""Test helper: the CPU restatement of the fused branch merge of sliced inference with test-time augmentation
(``csrc/tile_merge_tta.hip``) in numpy float32. The product has no CPU path; this file is the definition the kernel is
tested against, bit for bit. It is written out on its own, not as calls of ``tta_merge_ref`` and ``tile_merge_ref``:
tests/test_sliced_tta_cpu.py checks that it equals that chain.

Anchors [src_lo, src_lo + n) of source row ``src`` of branch output ``y`` [rows, 4+nc, A_k] go to
``merged[frame][:, slot*A_tot + dst : slot*A_tot + dst + n]``. Per anchor (every operation rounds to fp32; numpy never
contracts a multiply and an add):
    x, y, w, h = each / float32(scale);  x = float32(img_w) - x (flip 3)  or  y = float32(img_h) - y (flip 2)
    bx = (x - pad_x) / gain;  by = (y - pad_y) / gain;  bw = w / gain;  bh = h / gain
    cut = cut_margin >= 0 and ((left  and bx - 0.5 bw <= cut_margin) or (right  and bx + 0.5 bw >= tile_w - cut_margin)
                            or (top   and by - 0.5 bh <= cut_margin) or (bottom and by + 0.5 bh >= tile_h - cut_margin))
    box = bx + off_x, by + off_y, bw, bh;  score_c = 0 if cut else score_c
``src = -1`` writes zeros to the same range. Rows are ``SlicePlan.merge_rows``' tuples; ``branch`` is a ``TTABranch`` or
``(src_lo, n, dst, scale, flip)`` with flip None / 0 (none), 2 (up-down) or 3 (left-right)."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def branch_terms(branch):
    if hasattr(branch, "src_lo"):
        return branch.src_lo, branch.n, branch.dst, branch.scale, branch.flip
    src_lo, n, dst, scale, flip = branch
    return src_lo, n, dst, scale, flip


def tile_merge_tta_ref(y: np.ndarray, rows, merged: np.ndarray, A_tot: int, branch, canvas_hw,
                       cut_margin=None) -> np.ndarray:
    """``y`` [n, 4+nc, A_k] float32, ``merged`` [F, 4+nc, S*A_tot] float32 (written in place, only the branch's range
    of the named slots)."""
    assert y.dtype == np.float32 and merged.dtype == np.float32 and merged.shape[2] % A_tot == 0
    src_lo, n, dst, scale, flip = branch_terms(branch)
    assert 0 <= src_lo and n >= 1 and src_lo + n <= y.shape[2] and 0 <= dst and dst + n <= A_tot
    assert flip in (None, 0, 2, 3)
    scale, img_h, img_w = f32(scale), f32(canvas_hw[0]), f32(canvas_hw[1])
    cm = f32(-1.0 if cut_margin is None else cut_margin)
    half = f32(0.5)
    for src, frame, slot, gain, pad_x, pad_y, off_x, off_y, tile_w, tile_h, interior in rows:
        out = merged[frame, :, slot * A_tot + dst:slot * A_tot + dst + n]
        if src < 0:
            out[:] = 0
            continue
        gain, pad_x, pad_y, off_x, off_y = f32(gain), f32(pad_x), f32(pad_y), f32(off_x), f32(off_y)
        tile_w, tile_h = f32(tile_w), f32(tile_h)
        s = y[src, :, src_lo:src_lo + n]
        with np.errstate(all="ignore"):
            x, yy, w, h = s[0] / scale, s[1] / scale, s[2] / scale, s[3] / scale
            if flip == 3:
                x = img_w - x
            elif flip == 2:
                yy = img_h - yy
            bx, by, bw, bh = (x - pad_x) / gain, (yy - pad_y) / gain, w / gain, h / gain
            assert bx.dtype == np.float32 and by.dtype == np.float32 and bw.dtype == np.float32
            cut = np.zeros(n, dtype=bool)
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
            out[0], out[1], out[2], out[3] = bx + off_x, by + off_y, bw, bh
        out[4:] = np.where(cut[None], f32(0), s[4:])
    return merged
