"""Test helper: the CPU restatement of the confusion-matrix kernel (``csrc/eval_confusion.hip``) in numpy float32, and
the seeded crowds it is tested on. This file is the definition the kernel is tested against, bit for bit;
tests/test_confusion_cpu.py checks it against the reference's own matrices (tests/golden/confusion_eval.npz) and against
the host class ``utils.metrics.ConfusionMatrix``, which walks the reference's steps.

One image, labels l = 0..L-1 (cls, x1, y1, x2, y2) and rows d = 0..n-1 (x1, y1, x2, y2, conf, cls) in NMS order (every
operation rounds to fp32; numpy never contracts a multiply and an add):
    kept(d)   = conf[d] > conf_thr                               (fp32; NaN is not kept)
    dc, gc    = the class truncated to int
    iou[l][d] = inter / (((a_l + a_d) - inter) + 1e-7), class-agnostic (tests/eval_match_ref.py's box arithmetic)
    v[d]      = max_l iou[l][d] over iou[l][d] > iou_thr (strict); bl[d] = the highest l that attains it, or none
    win(d)    = bl[d] exists and no kept e != d has bl[e] == bl[d] with v[e] > v[d], or v[e] == v[d] and e > d
    M[dc[d]][gc[bl[d]]] += 1 for kept d with win(d);  M[dc[d]][nc] += 1 for kept d without;
    M[nc][gc[l]] += 1 for every label l that no winner claims
A row or label whose class is NaN or truncates outside [0, nc) is counted nowhere; it still takes part in the matching
(such a row can take a label; the winner of such a label is counted nowhere and the label is not missed).

This is what the reference computes: it sorts the pairs above the threshold by IoU, np.unique over detections leaves each
detection its best label, the second sort and np.unique over labels leave each label its best claimant, and a detection
that lost its label is background. numpy's order among equal IoUs is unspecified for long lists, so a comparison with
the reference (or with the host class) is only meaningful where ``ties`` is 0."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def iou_all(labels: np.ndarray, det: np.ndarray) -> np.ndarray:
    """[L, n] float32: box_iou's operation order, whatever the classes (NaN where the reference has NaN)."""
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
    return iou


def class_index(c, nc: int) -> np.ndarray:
    """The truncated class where it lies in [0, nc), else -1 (NaN included)."""
    c = np.asarray(c, dtype=f32).reshape(-1)
    with np.errstate(all="ignore"):
        ok = (c > f32(-1)) & (c < f32(nc))
        return np.where(ok, np.trunc(np.where(ok, c, 0)), -1).astype(np.int64)


def confusion_ref(labels: np.ndarray, det: np.ndarray, nc: int, conf=0.25, iou_thres=0.45):
    """(M int64 [nc + 1, nc + 1], ties) for one image: ``labels`` [L, 5], ``det`` [n, 6]. ``ties`` counts the places
    where one of the two "highest index" rules decided: kept rows whose maximum is attained by two labels or more, and
    claimed labels whose best IoU is held by two kept rows or more."""
    lab, det = np.asarray(labels, dtype=f32).reshape(-1, 5), np.asarray(det, dtype=f32).reshape(-1, 6)
    L, n = len(lab), len(det)
    M = np.zeros((nc + 1, nc + 1), dtype=np.int64)
    gc, dc = class_index(lab[:, 0], nc), class_index(det[:, 5], nc)
    with np.errstate(all="ignore"):
        kept = det[:, 4] > f32(conf)
    ties = 0
    bl = np.full(n, -1, dtype=np.int64)
    v = np.zeros(n, dtype=f32)
    if L and n:
        iou = iou_all(lab, det)
        with np.errstate(all="ignore"):
            ok = (iou > f32(iou_thres)) & kept[None]
        masked = np.where(ok, iou, f32(-1))
        v = masked.max(0)
        has = ok.any(0)
        bl = np.where(has, L - 1 - masked[::-1].argmax(0), -1)  # the highest label index among equal maxima
        ties += int(((ok & (masked == v[None])).sum(0)[has] > 1).sum())
    claimed = np.zeros(L, dtype=bool)
    for l in np.unique(bl[bl >= 0]):
        rows = np.nonzero(bl == l)[0]
        top = v[rows].max()
        best = rows[v[rows] == top]
        ties += int(len(best) > 1)
        d = best.max()  # the highest row among equal IoUs
        claimed[l] = True
        if dc[d] >= 0 and gc[l] >= 0:
            M[dc[d], gc[l]] += 1
        bl[rows[rows != d]] = -1  # the losers are background
    for d in np.nonzero(kept & (bl < 0))[0]:
        if dc[d] >= 0:
            M[dc[d], nc] += 1
    for l in np.nonzero(~claimed)[0]:
        if gc[l] >= 0:
            M[nc, gc[l]] += 1
    return M, ties


def lab5(cls, boxes) -> np.ndarray:
    return np.concatenate([np.asarray(cls, f32).reshape(-1, 1), np.asarray(boxes, f32).reshape(-1, 4)], 1)


def confusion_batch_ref(out: np.ndarray, counts, targets, nc: int, conf=0.25, iou_thres=0.45):
    """(int64 [B, nc + 1, nc + 1], ties) for padded rows ``out`` [B, D, 6]; ``targets``: (cls, boxes) per image."""
    cms, ties = [], 0
    for b, (cls, boxes) in enumerate(targets):
        n = min(max(int(counts[b]), 0), out.shape[1])
        M, t = confusion_ref(lab5(cls, boxes), out[b, :n], nc, conf, iou_thres)
        cms.append(M)
        ties += t
    return np.stack(cms), ties


def conserved(M: np.ndarray, labels: np.ndarray, det: np.ndarray, nc: int, conf=0.25) -> bool:
    """Column sums over the true classes are the labels per class, row sums the kept rows per class (true where every
    class lies in [0, nc); classes outside are left out on both sides, so it holds as long as no such row wins and no
    such label is won)."""
    lab, det = np.asarray(labels, dtype=f32).reshape(-1, 5), np.asarray(det, dtype=f32).reshape(-1, 6)
    gc, dc = class_index(lab[:, 0], nc), class_index(det[:, 5], nc)
    with np.errstate(all="ignore"):
        kept = det[:, 4] > f32(conf)
    cols = np.bincount(gc[gc >= 0], minlength=nc)
    rows = np.bincount(dc[kept & (dc >= 0)], minlength=nc)
    return bool((M[:, :nc].sum(0) == cols).all() and (M[:nc].sum(1) == rows).all())


def fixture_sets():
    """tests/golden/confusion_eval.npz as {"a": (nc, [(cls, boxes, det) per image], cm [24, nc+1, nc+1]), "b": ...}:
    set (a)'s inputs are ``recipes.synthetic_eval_set(21)``, set (b)'s are stored in the fixture."""
    import recipes
    from conftest import golden
    z = golden("confusion_eval")
    assert float(z["conf"]) == 0.25 and float(z["iou_thres"]) == 0.45

    def split(flat, n):
        at = np.cumsum(np.r_[0, n])
        return [flat[at[i]:at[i + 1]] for i in range(len(n))]

    gt, preds = recipes.synthetic_eval_set(21)
    a = [(c, b, p) for (c, b), p in zip(gt, preds)]
    b = list(zip(split(z["b_gt_cls"], z["b_gt_n"]), split(z["b_gt_boxes"], z["b_gt_n"]),
                 split(z["b_pred"], z["b_pred_n"])))
    return {"a": (int(z["a_nc"]), a, z["a_cm"]), "b": (int(z["b_nc"]), b, z["b_cm"])}


def crowd(seed: int, n_labels=None, n_det=None, nc: int = 10, img: float = 640.0):
    """A seeded crowd of small objects: (cls [L] fp32, boxes [L, 4] fp32 xyxy, det [n, 6] fp32). 0..399 labels (or
    ``n_labels``) of 4..40 px in ``nc`` classes; 0..299 rows (or ``n_det``): about three in four a label's box plus
    N(0, 1.5) jitter with the class wrong 30 % of the time, the rest clutter (random boxes, random classes; all of them
    where there is no label); confidences in (0.001, 1) descending as NMS leaves them, so roughly a quarter lies below
    0.25."""
    rng = np.random.default_rng(seed)
    L = int(rng.integers(0, 400)) if n_labels is None else int(n_labels)
    n = int(rng.integers(0, 300)) if n_det is None else int(n_det)
    cls = rng.integers(0, nc, L).astype(f32)
    wh = rng.uniform(4, 40, (L, 2))
    xy = rng.uniform(0, img - 40, (L, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(f32)
    xy0 = rng.uniform(0, img - 40, (n, 2))
    dbox = np.concatenate([xy0, xy0 + rng.uniform(4, 40, (n, 2))], 1)
    dcls = rng.integers(0, nc, n).astype(f32)
    if L and n:
        src = rng.integers(0, L, n)
        on = rng.uniform(size=n) < 0.75
        dbox[on] = (boxes[src] + rng.normal(0, 1.5, (n, 4)))[on]
        right = on & (rng.uniform(size=n) >= 0.3)
        dcls[right] = cls[src][right]
    conf = np.sort(rng.uniform(0.001, 1.0, n))[::-1]
    det = np.concatenate([dbox, conf[:, None], dcls[:, None]], 1).astype(f32).reshape(n, 6)
    return cls, boxes, det
