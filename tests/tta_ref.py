"""Test helper: the CPU restatement of test-time augmentation's two kernels (``csrc/tta.hip``) in numpy float32, and
the whole flow on a CPU model. The product has no CPU path (its wrappers refuse CPU tensors); this is what the kernels
are compared with bit for bit, itself checked against the reference's recorded ``scale_img`` / ``_descale_pred`` /
``predict(augment=True)`` outputs (tests/test_tta_cpu.py). Every product and sum below is one float32 operation, as in
the kernels (built with -ffp-contract=off)."""
from __future__ import annotations

import numpy as np
import torch

F32 = np.float32
PAD = F32(0.447)
FLIPS = {None: 0, 0: 0, 2: 2, 3: 3}


def bf16_round(a: np.ndarray) -> np.ndarray:
    """float32 values rounded to bfloat16 (nearest even), back in float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).float().numpy()


def axis_ref(n_in: int, n_out: int, flip: bool):
    """(i0, i1, l0, l1) of every destination index of one axis."""
    scale = F32(n_in) / F32(n_out)
    d = np.arange(n_out, dtype=F32)
    src = np.maximum(scale * (d + F32(0.5)) - F32(0.5), F32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(F32)
    l0 = F32(1) - l1
    assert src.dtype == F32 and l1.dtype == F32 and l0.dtype == F32
    if flip:
        i0, i1 = n_in - 1 - i0, n_in - 1 - i1
    return i0, i1, l0, l1


def tta_view_ref(x: np.ndarray, view, bf16: bool = False) -> np.ndarray:
    """One view of x [B, C, H, W] (float32; with ``bf16`` its values are bf16 values and so is the result):
    ``view`` = (flip, sh, sw, ph, pw)."""
    flip, sh, sw, ph, pw = view
    flip = FLIPS[flip]
    x = np.ascontiguousarray(x, dtype=F32)
    B, C, H, W = x.shape
    y0, y1, ly0, ly1 = axis_ref(H, sh, flip == 2)
    x0, x1, lx0, lx1 = axis_ref(W, sw, flip == 3)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    a, b = x[:, :, y0][:, :, :, x0], x[:, :, y0][:, :, :, x1]
    c, d = x[:, :, y1][:, :, :, x0], x[:, :, y1][:, :, :, x1]
    top = lx0 * a + lx1 * b
    bot = lx0 * c + lx1 * d
    val = ly0 * top + ly1 * bot
    assert val.dtype == F32
    out = np.full((B, C, ph, pw), PAD, dtype=F32)
    out[:, :, :sh, :sw] = val
    return bf16_round(out) if bf16 else out


def tta_merge_ref(y: np.ndarray, cat: np.ndarray, src_lo: int, n: int, dst: int, scale, flip, img_hw) -> np.ndarray:
    """Anchors [src_lo, src_lo + n) of y [B, 4+nc, A] into anchors [dst, dst + n) of cat, in place."""
    y = np.asarray(y, dtype=F32)
    s = y[:, :, src_lo:src_lo + n]
    box = s[:, :4] / F32(scale)
    assert box.dtype == F32
    if FLIPS[flip] == 3:
        box[:, 0] = F32(img_hw[1]) - box[:, 0]
    elif FLIPS[flip] == 2:
        box[:, 1] = F32(img_hw[0]) - box[:, 1]
    cat[:, :4, dst:dst + n] = box
    cat[:, 4:, dst:dst + n] = s[:, 4:]
    return cat


def predict_augment_ref(model, x: torch.Tensor, plan, bf16: bool = False):
    """The flow of ``DetectionModel._predict_augment`` on a CPU model: (cat, views, branch outputs)."""
    xn = x.float().numpy()
    views, ys = [], []
    cat = None
    for k, b in enumerate(plan.branches):
        xi = x if b.view is None else torch.from_numpy(tta_view_ref(xn, b.view, bf16)).to(x.dtype)
        with torch.inference_mode():
            yi = model(xi)
        yi = (yi[0] if isinstance(yi, (list, tuple)) else yi).float().numpy()
        assert yi.shape[-1] == b.A, (k, yi.shape, b.A)
        if cat is None:
            cat = np.full((yi.shape[0], yi.shape[1], plan.A_tot), np.nan, dtype=F32)
        tta_merge_ref(yi, cat, b.src_lo, b.n, b.dst, b.scale, b.flip, plan.shape)
        views.append(xi)
        ys.append(yi)
    return cat, views, ys
