"""Test helper: the CPU restatement of merge-NMS (``nms_merge_kernel`` in ``csrc/nms.hip``; the definition is the
comment on ``yolosod_nms_merged`` in ``include/yolosod_hip.h``). The product has no CPU path; this file is what the
kernel is tested against. The kept rows come from the oracle's NMS (``oracle.nms.non_max_suppression_ref``).

Per image and kept row k = (x1, y1, x2, y2, conf, cls) with anchor a_k:
    candidates   every (anchor, class) with score > conf_thres that passes the class filter: the best class of an anchor,
                 or with multi_label every class above conf_thres. All of them: no max_nms cut.
    member_j     IoU(k, j) > iou_thres, torchvision's formula in fp32 on the class-offset boxes (box + cls * max_wh):
                 inter / ((area_k + area_j) - inter), compared as a double; or j is k's own candidate (a_k, cls).
    merged c     sum_j (double)score_j * (double)c_j / sum_j (double)score_j on the plain xyxy boxes, rounded once to fp32.
    n_merged     the number of members.
The fp64 sums here run in numpy's order and the kernel's in its own: the two may differ by the final rounding, one
fp32 ulp (:func:`ulp_diff`)."""
from __future__ import annotations

import numpy as np

from oracle.nms import non_max_suppression_ref, xywh2xyxy_np

f32 = np.float32


def candidates_ref(pred_b: np.ndarray, conf_thres, classes=None, multi_label=False):
    """One image [4+nc, A] xywh: (xyxy boxes [n, 4] f32, scores [n] f32, classes [n] int64, anchors [n] int64) in
    (anchor, class) order."""
    nc = pred_b.shape[0] - 4
    box = xywh2xyxy_np(np.ascontiguousarray(pred_b[:4].T))
    sc = np.ascontiguousarray(pred_b[4:].T)  # [A, nc]
    conf32 = f32(conf_thres)
    if multi_label and nc > 1:
        a, j = np.nonzero(sc > conf32)
    else:
        j = sc.argmax(1)
        a = np.nonzero(sc[np.arange(sc.shape[0]), j] > conf32)[0]
        j = j[a]
    if classes is not None:
        m = np.isin(j, np.asarray(classes))
        a, j = a[m], j[m]
    return box[a], sc[a, j], j.astype(np.int64), a.astype(np.int64)


def members_ref(krow, kanchor, boxes, cls, anchors, iou_thres, agnostic, max_wh):
    """bool [n]: the candidates in kept row ``krow``'s cluster."""
    off = f32(0 if agnostic else max_wh)
    ob = (boxes + (cls.astype(f32) * off)[:, None]).astype(f32)
    kb = (krow[:4] + krow[5] * off).astype(f32)
    with np.errstate(all="ignore"):
        aj = (ob[:, 2] - ob[:, 0]) * (ob[:, 3] - ob[:, 1])
        ak = (kb[2] - kb[0]) * (kb[3] - kb[1])
        w = np.maximum(f32(0), np.minimum(kb[2], ob[:, 2]) - np.maximum(kb[0], ob[:, 0]))
        h = np.maximum(f32(0), np.minimum(kb[3], ob[:, 3]) - np.maximum(kb[1], ob[:, 1]))
        inter = w * h
        ovr = inter / ((ak + aj) - inter)
        assert ovr.dtype == np.float32
        hit = ovr.astype(np.float64) > float(iou_thres)
    return hit | ((anchors == int(kanchor)) & (cls == int(krow[5])))


def nms_merge_ref(prediction: np.ndarray, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False,
                  multi_label=False, max_det=300, max_nms=30000, max_wh=7680):
    """``prediction`` [B, 4+nc, A] xywh (not modified). Returns per image (lists of length B): the kept rows of plain
    NMS [n_i, 6] f32, their anchors [n_i], the merged rows [n_i, 6] f32, the merged boxes before the final rounding
    [n_i, 4] f64, and n_merged [n_i] int64."""
    rows, idx = non_max_suppression_ref(prediction.copy(), conf_thres, iou_thres, classes=classes, agnostic=agnostic,
                                        multi_label=multi_label, max_det=max_det, max_nms=max_nms, max_wh=max_wh)
    merged, merged64, nmer = [], [], []
    for b in range(prediction.shape[0]):
        boxes, scores, cls, anchors = candidates_ref(prediction[b], conf_thres, classes, multi_label)
        m = rows[b].copy()
        m64 = np.zeros((len(m), 4), np.float64)
        cn = np.zeros(len(m), np.int64)
        w = scores.astype(np.float64)
        b64 = boxes.astype(np.float64)
        for k in range(len(m)):
            mem = members_ref(rows[b][k], idx[b][k], boxes, cls, anchors, iou_thres, agnostic, max_wh)
            cn[k] = int(mem.sum())
            m64[k] = (w[mem, None] * b64[mem]).sum(0) / w[mem].sum()
        m[:, :4] = m64.astype(f32)
        merged.append(m)
        merged64.append(m64)
        nmer.append(cn)
    return rows, idx, merged, merged64, nmer


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """|a - b| in units of the last place of fp32 (finite values; +0 and -0 are 0 apart)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
