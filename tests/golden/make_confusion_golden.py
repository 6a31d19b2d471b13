"""Generate the confusion-matrix fixture by running the REFERENCE (``make_golden.import_reference``):
``python tests/golden/make_confusion_golden.py``. Data only - inputs and recorded matrices:

  tests/golden/confusion_eval.npz   ``ConfusionMatrix(nc, conf=0.25, iou_thres=0.45).process_batch`` of
                                    ultralytics/utils/metrics.py:326-382, one fresh matrix per image, called the way
                                    detect/val.py:140-159 calls it (``detections=None`` for an image with labels and no
                                    rows, no call for an image with neither), for
      a_*   ``recipes.synthetic_eval_set(21)``, the inputs of metrics_eval.npz (nc 6, 24 images): ``a_cm`` only
      b_*   ``confusion_ref.crowd(SEED_B + i, ...)``, nc 10, 24 images with the sizes of ``SIZES_B``: the inputs
            (``b_gt_cls``, ``b_gt_boxes``, ``b_gt_n``, ``b_pred``, ``b_pred_n``) and ``b_cm``

Asserted here: no image holds an exact IoU tie among the pairs above the threshold (numpy's order there is unspecified,
so the reference's own result would not be defined), the restatement tests/confusion_ref.py gives the same matrices,
and set (b) fills off-diagonal cells, the background row and the background column.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from make_golden import HERE, import_reference

sys.path.insert(0, str(HERE.parent))
import recipes  # noqa: E402
from confusion_ref import confusion_ref, crowd, lab5  # noqa: E402

CONF, IOU = 0.25, 0.45
NC_A, NC_B, SEED_B = 6, 10, 4100
# (labels, rows) per image of set (b): both empty sides, a single pair, more labels than a staging chunk, a full 300
SIZES_B = [(0, 0), (0, 37), (29, 0), (1, 1), (260, 300), (150, 299), (3, 120), (90, 12)] + [(None, None)] * 16


def crowd_b(i: int):
    nl, nd = SIZES_B[i]
    if nl is None:
        rng = np.random.default_rng(SEED_B + 1000 + i)
        nl, nd = int(rng.integers(1, 150)), int(rng.integers(1, 300))
    return crowd(SEED_B + i, n_labels=nl, n_det=nd, nc=NC_B)


def reference_matrix(RM, nc, cls, boxes, pred):
    cm = RM.ConfusionMatrix(nc=nc, conf=CONF, iou_thres=IOU)
    cls_t, box_t, pred_t = torch.from_numpy(cls), torch.from_numpy(boxes), torch.from_numpy(pred)
    if len(pred_t) == 0:
        if len(cls_t):
            cm.process_batch(detections=None, gt_bboxes=box_t, gt_cls=cls_t)
    else:
        cm.process_batch(pred_t, box_t, cls_t)
    m = cm.matrix
    assert m.shape == (nc + 1, nc + 1) and (m == np.round(m)).all()
    return m.astype(np.int64)


def run_set(RM, nc, images):
    cms = []
    for i, (cls, boxes, pred) in enumerate(images):
        m = reference_matrix(RM, nc, cls, boxes, pred)
        mine, ties = confusion_ref(lab5(cls, boxes), pred, nc, CONF, IOU)
        assert ties == 0, f"image {i} holds {ties} exact IoU ties"
        assert np.array_equal(mine, m), f"image {i}: the restatement differs from the reference"
        cms.append(m)
    return np.stack(cms)


def main():
    import_reference()
    import ultralytics.utils.metrics as RM

    gt, preds = recipes.synthetic_eval_set(21)
    a_cm = run_set(RM, NC_A, [(c, b, p) for (c, b), p in zip(gt, preds)])
    images = [crowd_b(i) for i in range(len(SIZES_B))]
    b_cm = run_set(RM, NC_B, images)
    tot = b_cm.sum(0)
    off = tot[:NC_B, :NC_B] - np.diag(np.diag(tot[:NC_B, :NC_B]))
    assert off.sum() > 0 and tot[NC_B, :NC_B].sum() > 0 and tot[:NC_B, NC_B].sum() > 0 and np.diag(tot).sum() > 0
    np.savez_compressed(
        HERE / "confusion_eval.npz", conf=np.array(CONF), iou_thres=np.array(IOU), a_nc=np.array(NC_A), a_cm=a_cm,
        b_nc=np.array(NC_B), b_cm=b_cm, b_gt_cls=np.concatenate([c for c, _, _ in images]),
        b_gt_boxes=np.concatenate([b for _, b, _ in images]), b_gt_n=np.array([len(c) for c, _, _ in images]),
        b_pred=np.concatenate([p for _, _, p in images]), b_pred_n=np.array([len(p) for _, _, p in images]))
    print("a: total", int(a_cm.sum()), "diagonal", int(np.trace(a_cm.sum(0))))
    print("b: total", int(tot.sum()), "diagonal", int(np.trace(tot)), "off-diagonal", int(off.sum()),
          "missed", int(tot[NC_B].sum()), "on background", int(tot[:, NC_B].sum()))


if __name__ == "__main__":
    main()
