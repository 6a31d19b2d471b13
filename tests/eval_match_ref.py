"""Test helper: the CPU restatement of the evaluator's matching kernel (``csrc/eval_match.hip``) in numpy float32, and
the seeded crowds it is tested on. The product has no CPU path for ``update_padded``; this file is the definition the
kernel is tested against, bit for bit, and tests/test_eval_match_cpu.py checks it against the reference's own result.

One image, labels l = 0..L-1 (cls, x1, y1, x2, y2) and detections d = 0..n-1 (x1, y1, x2, y2, conf, cls) in NMS order
(every operation rounds to fp32; numpy never contracts a multiply and an add):
    w = max(min(x2_l, x2_d) - max(x1_l, x1_d), 0), h likewise;  inter = w * h
    iou[l][d] = inter / (((a_l + a_d) - inter) + 1e-7), 0 where cls_l != cls_d (and where it is not > 0)
    bi[d] = max_l iou[l][d];  best[d] = the highest l that attains it, none if bi[d] == 0
    m[d]  = max{ bi[d'] : d' < d, best[d'] == best[d] }, 0 if there is none
    tp[d][t] = bi[d] >= thr_t and thr_t > m[d]
This is what the reference's threshold-by-threshold greedy matching (nonzero, argsort by IoU, np.unique over detections,
np.unique over labels) computes: after the IoU sort and the first np.unique every detection holds its best label, rows
in detection order; the second keeps, per label, the first detection that claimed it at that threshold."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def iou_ref(labels: np.ndarray, det: np.ndarray) -> np.ndarray:
    """[L, n] float32: box_iou's operation order, class mismatches and non-positive values (NaN included) as 0."""
    lab, det = np.asarray(labels, dtype=f32).reshape(-1, 5), np.asarray(det, dtype=f32).reshape(-1, 6)
    a, b = lab[:, None, 1:5], det[None, :, 0:4]
    with np.errstate(all="ignore"):
        w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), f32(0))
        h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), f32(0))
        inter = w * h
        a_l = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        a_d = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        iou = inter / (((a_l + a_d) - inter) + f32(1e-7))
        assert iou.dtype == np.float32
        same = lab[:, None, 0] == det[None, :, 5]
        return np.where(same & (iou > 0), iou, f32(0))


def match_ref(labels: np.ndarray, det: np.ndarray, iouv) -> np.ndarray:
    """uint8 [n, T] for one image: ``labels`` [L, 5], ``det`` [n, 6], thresholds ``iouv`` (> 0, compared as fp32)."""
    thr = np.asarray(iouv, dtype=f32).reshape(-1)
    assert (thr > 0).all()
    det = np.asarray(det, dtype=f32).reshape(-1, 6)
    n, L = len(det), len(np.asarray(labels).reshape(-1, 5))
    if n == 0 or L == 0:
        return np.zeros((n, len(thr)), dtype=np.uint8)
    iou = iou_ref(labels, det)
    bi = iou.max(0)
    best = np.where(bi > 0, L - 1 - iou[::-1].argmax(0), -1)  # the highest label index among equal maxima
    m = np.zeros(n, dtype=f32)
    claimed = {}
    for d in range(n):
        if best[d] >= 0:
            m[d] = claimed.get(best[d], f32(0))
            claimed[best[d]] = max(m[d], bi[d])
    return ((bi[:, None] >= thr[None]) & (thr[None] > m[:, None])).astype(np.uint8)


def match_batch_ref(out: np.ndarray, counts, targets, iouv) -> np.ndarray:
    """uint8 [B, D, T] for padded rows ``out`` [B, D, 6]: rows >= counts[b] are 0. ``targets``: (cls, boxes) per
    image."""
    B, D = out.shape[:2]
    T = len(np.asarray(iouv).reshape(-1))
    tp = np.zeros((B, D, T), dtype=np.uint8)
    for b, (cls, boxes) in enumerate(targets):
        n = int(counts[b])
        lab = np.concatenate([np.asarray(cls, dtype=f32).reshape(-1, 1),
                              np.asarray(boxes, dtype=f32).reshape(-1, 4)], 1)
        tp[b, :n] = match_ref(lab, out[b, :n], iouv)
    return tp


def assert_no_ties(labels: np.ndarray, det: np.ndarray) -> None:
    """No detection has two labels at an equal, non-zero, class-matched maximum IoU (numpy's order for such ties is
    unspecified for long lists, so the reference's own result is not defined there)."""
    if len(labels) == 0 or len(det) == 0:
        return
    iou = iou_ref(labels, det)
    bi = iou.max(0)
    at_max = ((iou == bi[None]) & (bi[None] > 0)).sum(0)
    assert int(at_max.max()) <= 1, f"a detection ties {int(at_max.max())} labels"


def crowd(seed: int, n_labels=None, n_det=None, img: float = 640.0):
    """A seeded crowd of small objects: (cls [L] fp32, boxes [L, 4] fp32 xyxy, det [n, 6] fp32). 1..399 labels (or
    ``n_labels``, 0 allowed) of 4..40 px in 1..3 classes; 1..299 detections (or ``n_det``), each a label's box plus
    N(0, 1.5) jitter with the class flipped 10 % of the time (random boxes when there is no label), in descending
    confidence as NMS leaves them. Asserts that no detection ties two labels."""
    rng = np.random.default_rng(seed)
    L = int(rng.integers(1, 400)) if n_labels is None else int(n_labels)
    n = int(rng.integers(1, 300)) if n_det is None else int(n_det)
    nc = int(rng.integers(1, 4))
    cls = rng.integers(0, nc, L).astype(f32)
    wh = rng.uniform(4, 40, (L, 2))
    xy = rng.uniform(0, img - 40, (L, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(f32)
    if L:
        src = rng.integers(0, L, n)
        dbox = boxes[src] + rng.normal(0, 1.5, (n, 4))
        dcls = cls[src].copy()
    else:
        xy0 = rng.uniform(0, img - 40, (n, 2))
        dbox = np.concatenate([xy0, xy0 + rng.uniform(4, 40, (n, 2))], 1)
        dcls = np.zeros(n, dtype=f32)
    flip = rng.uniform(size=n) < 0.1
    dcls[flip] = rng.integers(0, nc, int(flip.sum())).astype(f32)
    conf = np.sort(rng.uniform(0.001, 1.0, n))[::-1]
    det = np.concatenate([dbox, conf[:, None], dcls[:, None]], 1).astype(f32)
    assert_no_ties(np.concatenate([cls[:, None], boxes], 1), det)
    return cls, boxes, det
