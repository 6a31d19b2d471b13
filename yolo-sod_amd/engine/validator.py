"""Detection evaluator: accumulates per-image statistics and reports mAP like the reference's DetectionValidator.

Mirrors ultralytics/models/yolo/detect/val.py:125-187 (update_metrics, _process_batch, get_stats) for the tensor
path, where predictions and labels live in the same image space (scale_boxes with gain 1, pad 0: predict.py:39,
val.py:113-123), so no rescaling is applied. NMS for validation is the reference's val mode
(val.py:92-102: conf 0.001, iou 0.7, multi_label=True, max_det 300) and runs on the GPU via
``yolosod_amd.utils.ops.non_max_suppression``.

Two ways in, one way out. :meth:`DetectionEvaluator.update` takes per-image lists and matches on the host
(utils/metrics.py), one host sync per image. :meth:`DetectionEvaluator.update_padded` takes what ``predict_padded``
returns, matches the whole batch in one HIP launch (``_hip.match_predictions``, csrc/eval_match.hip) and only queues
the result: no host sync until :meth:`DetectionEvaluator.get_stats` fetches everything queued in one copy. Both feed
the same host-side AP arithmetic with the same arrays, so the metrics are equal, not merely close.
:func:`validate` is the loop over a predictor.

``DetectionEvaluator(nc, confusion=True)`` also keeps the reference's confusion matrix (val.py:83,145,159,177 over
utils/metrics.py:294-393): :meth:`~DetectionEvaluator.update` walks ``ConfusionMatrix.process_batch`` per image on the
host, :meth:`~DetectionEvaluator.update_padded` makes one more launch on the labels it has packed already
(``_hip.confusion_matrix``, csrc/eval_confusion.hip) and sums the batch's matrices into a device accumulator, which
``get_stats`` fetches in the same copy as the queued batches. Still no host sync before ``get_stats``.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _hip
from ..utils.metrics import IOU_THRESHOLDS, ConfusionMatrix, DetMetrics, box_iou, match_predictions

VAL_NMS = dict(conf_thres=0.001, iou_thres=0.7, multi_label=True, max_det=300)


def _host_targets(targets):
    """[(cls [m] fp32, boxes [m, 4] fp32)] as host tensors, converted the way :meth:`DetectionEvaluator.update` does."""
    return [(torch.as_tensor(cls).float().cpu().reshape(-1), torch.as_tensor(bbox).float().cpu().reshape(-1, 4))
            for cls, bbox in targets]


def pack_labels(targets, device):
    """The labels of a batch for ``_hip.match_predictions``: ``targets`` is a list of (cls [m_i], boxes_xyxy [m_i, 4])
    per image (numpy arrays or host tensors; an image may have none). Returns (labels [L, 5] fp32 = cls, x1, y1, x2,
    y2 of all images back to back, label_off [B + 1] int32 with label_off[0] = 0) on ``device``. Both go up through one
    pinned staging buffer as one non-blocking copy (as ``predictor.frames_to_device`` does for frames): no host sync."""
    return _pack(_host_targets(targets), device)


def _pack(host, device):
    for i, (cls, bbox) in enumerate(host):
        if len(cls) != len(bbox):
            raise ValueError(f"pack_labels: image {i}: {len(cls)} classes for {len(bbox)} boxes")
    B = len(host)
    off = np.zeros(B + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(cls) for cls, _ in host])
    L = int(off[-1])
    stage = torch.empty(L * 5 + B + 1, dtype=torch.float32)
    device = torch.device(device)
    if device.type == "cuda":
        stage = stage.pin_memory()
    rows = stage[:L * 5].view(L, 5)
    for (cls, bbox), lo, hi in zip(host, off[:-1], off[1:]):
        rows[lo:hi, 0] = cls
        rows[lo:hi, 1:] = bbox
    stage[L * 5:].view(torch.int32).copy_(torch.from_numpy(off))
    up = stage.to(device, non_blocking=True)
    return up[:L * 5].view(L, 5), up[L * 5:].view(torch.int32)


def _per_class(classes, nc):
    """[nc] int64: how often each class in [0, nc) occurs; NaN and classes outside are not counted (np.bincount alone
    would raise on a negative class and grow past nc on a large one)."""
    with np.errstate(invalid="ignore"):
        inside = classes[(classes >= 0) & (classes < nc)]
    return np.bincount(inside.astype(int), minlength=nc)[:nc].astype(np.int64)


class _Queued:
    """A batch that :meth:`DetectionEvaluator.update_padded` matched on the device and has not fetched yet. It stands
    in every list of ``stats`` at the batch's place in call order until ``get_stats`` replaces it by the per-image
    arrays."""

    __slots__ = ("tp", "cc", "counts", "cls", "rows")

    def __init__(self, tp, cc, counts, cls):
        # device [B, D, T] uint8, [B, D, 2] fp32 (conf, cls), [B] int32; the labels' classes per image on the host
        self.tp, self.cc, self.counts, self.cls = tp, cc, counts, cls
        self.rows = None  # per stats key, the arrays of this batch's images


class DetectionEvaluator:
    def __init__(self, nc: int, iouv: torch.Tensor = IOU_THRESHOLDS, confusion=False):
        """``confusion``: True for a ``ConfusionMatrix(nc)`` at the reference's thresholds (conf 0.25, IoU 0.45), or a
        ``ConfusionMatrix`` of the caller's; it is ``self.confusion_matrix`` and complete after :meth:`get_stats`.
        False: none is kept and nothing is launched for it."""
        if isinstance(confusion, ConfusionMatrix):
            if confusion.nc != nc:
                raise ValueError(f"DetectionEvaluator: a ConfusionMatrix of {confusion.nc} classes for nc={nc}")
            self.confusion_matrix = confusion
        else:
            self.confusion_matrix = ConfusionMatrix(nc) if confusion else None
        self._cm_dev = None  # [nc + 1, nc + 1] int64 on the device: the batches of update_padded not fetched yet
        self.nt_per_class, self.nt_per_image = np.zeros(nc, dtype=np.int64), np.zeros(nc, dtype=np.int64)
        self.nc = nc
        self.iouv = iouv
        self.niou = iouv.numel()
        self.seen = 0
        self.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])
        self.metrics = DetMetrics()

    def update(self, preds, targets):
        """preds: list of [n_i, 6] (x1, y1, x2, y2, conf, cls); targets: list of (cls [m_i], boxes_xyxy [m_i, 4])."""
        for pred, (cls, bbox) in zip(preds, targets):
            self.seen += 1
            pred = pred.detach().float().cpu()
            cls = torch.as_tensor(cls).float().cpu().reshape(-1)
            bbox = torch.as_tensor(bbox).float().cpu().reshape(-1, 4)
            npr, nl = len(pred), len(cls)
            stat = dict(conf=np.zeros(0, np.float32), pred_cls=np.zeros(0, np.float32),
                        tp=np.zeros((npr, self.niou), bool), target_cls=cls.numpy(), target_img=cls.unique().numpy())
            if npr == 0:
                if nl:
                    for k in self.stats:
                        self.stats[k].append(stat[k])
                    if self.confusion_matrix is not None:
                        self.confusion_matrix.process_batch(None, bbox, cls)
                continue
            stat["conf"] = pred[:, 4].numpy()
            stat["pred_cls"] = pred[:, 5].numpy()
            if nl:
                stat["tp"] = match_predictions(pred[:, 5], cls, box_iou(bbox, pred[:, :4]), self.iouv)
            if self.confusion_matrix is not None:
                self.confusion_matrix.process_batch(pred, bbox, cls)
            for k in self.stats:
                self.stats[k].append(stat[k])

    def update_padded(self, out, counts, targets):
        """The same bookkeeping for a batch as ``predict_padded`` returns it, without a host sync: ``out`` [B, D, 6]
        fp32 and ``counts`` [B] int32 on the GPU (boxes and labels in the same space: the frames' own pixels for a list
        of frames), ``targets`` one (cls [m_i], boxes_xyxy [m_i, 4]) per image on the host. The labels go up as one
        pinned copy (:func:`pack_labels`), one HIP launch matches the batch (``_hip.match_predictions``), and the
        true-positive matrix, the rows' (conf, cls) and the counts stay on the device until :meth:`get_stats`. With a
        confusion matrix, a second launch on the same packed labels (``_hip.confusion_matrix``) counts the batch's
        [B, nc + 1, nc + 1] matrices and a torch sum adds them to the device accumulator."""
        for t, name in ((out, "out"), (counts, "counts")):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"update_padded: {name}: expected a tensor")
            if t.device.type != "cuda":
                raise RuntimeError(f"update_padded: {name}: HIP kernel requires a GPU tensor (got device {t.device}); "
                                   "no CPU fallback - DetectionEvaluator.update takes host detections")
        targets = list(targets)
        if out.dim() != 3 or len(targets) != out.shape[0]:
            raise RuntimeError(f"update_padded: {len(targets)} targets for out {tuple(out.shape)}")
        host = _host_targets(targets)
        labels, label_off = _pack(host, out.device)
        tp = _hip.match_predictions(out, counts, labels, label_off, self.iouv)
        if self.confusion_matrix is not None:
            cm = _hip.confusion_matrix(out, counts, labels, label_off, self.nc, self.confusion_matrix.conf,
                                       self.confusion_matrix.iou_thres).sum(0)  # int64
            if self._cm_dev is None:
                self._cm_dev = cm
            elif self._cm_dev.device == cm.device:
                self._cm_dev += cm
            else:
                raise RuntimeError(f"update_padded: out on {cm.device}, earlier batches on {self._cm_dev.device}")
        # copies: the caller may reuse out / counts for the next batch
        q = _Queued(tp, out[..., 4:6].contiguous(), counts.clone(), [cls for cls, _ in host])
        self.seen += len(targets)
        for k in self.stats:
            self.stats[k].append(q)

    def _fetch(self):
        """Everything :meth:`update_padded` queued, in one device-to-host copy; each queued batch becomes the arrays
        :meth:`update` would have appended for the same images. The confusion accumulator rides in the same byte
        buffer and is folded into ``confusion_matrix.matrix``."""
        qs = [v for v in self.stats["tp"] if isinstance(v, _Queued)]
        if not qs:
            return
        # one byte buffer: the 8-byte part, then the 4-byte parts, so that every part starts aligned
        acc = self._cm_dev
        parts = [] if acc is None else [acc.view(-1).view(torch.uint8)]
        parts += [q.cc.view(-1).view(torch.uint8) for q in qs] + [q.counts.view(torch.uint8) for q in qs]
        parts += [q.tp.view(-1) for q in qs]
        buf = (torch.cat(parts) if len(parts) > 1 else parts[0]).cpu().numpy()
        pos = 0
        if acc is not None:
            self._cm_dev = None  # fetched: the next update_padded starts a new accumulator
            pos = acc.numel() * 8
            self.confusion_matrix.add(buf[:pos].view(np.int64).reshape(tuple(acc.shape)))

        def take(q_t, dtype):
            nonlocal pos
            n = q_t.numel() * q_t.element_size()
            a = buf[pos:pos + n].view(dtype).reshape(tuple(q_t.shape))
            pos += n
            return a

        ccs = [take(q.cc, np.float32) for q in qs]
        cnts = [take(q.counts, np.int32) for q in qs]
        tps = [take(q.tp, np.uint8) for q in qs]
        for q, cc, cnt, tp in zip(qs, ccs, cnts, tps):
            q.rows = {k: [] for k in self.stats}
            D = tp.shape[1]
            for i, cls in enumerate(q.cls):
                npr, nl = min(max(int(cnt[i]), 0), D), len(cls)
                if npr == 0 and not nl:
                    continue
                stat = dict(conf=cc[i, :npr, 0].copy(), pred_cls=cc[i, :npr, 1].copy(), tp=tp[i, :npr].astype(bool),
                            target_cls=cls.numpy(), target_img=cls.unique().numpy())
                for k in self.stats:
                    q.rows[k].append(stat[k])
        for k, vals in self.stats.items():
            flat = []
            for v in vals:
                if isinstance(v, _Queued):
                    flat.extend(v.rows[k])
                else:
                    flat.append(v)
            self.stats[k] = flat

    def get_stats(self):
        """Concatenate and score; same gate as the reference (metrics only when any prediction is a TP). Batches from
        :meth:`update_padded` are fetched here (the one host sync of a validation run) and take their place in call
        order among the images of :meth:`update`. Afterwards ``nt_per_class`` / ``nt_per_image`` hold the labels and
        the images per class (val.py:182-183; always [nc], a class that is NaN or outside [0, nc) is left out of them and
        goes on to the AP arithmetic as before), and ``confusion_matrix``, if one is kept, every batch of both ways in."""
        self._fetch()
        self.nt_per_class, self.nt_per_image = np.zeros(self.nc, np.int64), np.zeros(self.nc, np.int64)
        if not self.stats["tp"]:
            return self.metrics.results_dict
        st = {k: np.concatenate(v, 0) for k, v in self.stats.items()}
        self.nt_per_class = _per_class(st["target_cls"], self.nc)
        self.nt_per_image = _per_class(st.pop("target_img"), self.nc)
        if len(st) and st["tp"].any():
            self.metrics.process(st["tp"], st["conf"], st["pred_cls"], st["target_cls"])
        return self.metrics.results_dict


def validate(predictor, batches, nc: int, iouv: torch.Tensor = IOU_THRESHOLDS, evaluator=None) -> dict:
    """mAP of a predictor on labelled batches: ``batches`` yields (frames_or_tensor, targets) with ``targets`` one
    (cls [m_i], boxes_xyxy [m_i, 4]) per image on the host, in the space of the predictor's boxes (a tensor batch: the
    tensor's own pixels; a list of raw frames: each frame's pixels). ``predictor`` is anything whose
    ``predict_padded(batch)`` returns (out [B, D, 6], counts [B], index) on the GPU: ``DetectionPredictor``, or
    ``SlicedPredictor`` with the targets in frame pixels. Returns ``DetMetrics.results_dict``.

    The loop makes no host sync: a batch is the predictor's launches, one pinned copy of its labels and one matching
    launch (:meth:`DetectionEvaluator.update_padded`); the single sync is the fetch in ``get_stats`` at the end.

    The predictor's thresholds are used as they are. The reference validates in its val mode (val.py:92-102), which is
    ``DetectionPredictor(model, conf=0.001, iou=0.7, multi_label=True, max_det=300)`` - the values of ``VAL_NMS``; a
    predictor left at its predict-mode defaults (conf 0.25) scores a truncated precision-recall curve.

    ``evaluator``: a ``DetectionEvaluator`` of the caller's to feed instead of a fresh one, e.g.
    ``DetectionEvaluator(nc, confusion=True)``, whose ``confusion_matrix``, ``nt_per_class`` and ``metrics`` the caller
    reads afterwards; ``nc`` and ``iouv`` must be its own."""
    if evaluator is None:
        ev = DetectionEvaluator(nc, iouv)
    else:
        ev = evaluator
        if ev.nc != nc or not torch.equal(torch.as_tensor(ev.iouv), torch.as_tensor(iouv)):
            raise ValueError("validate: the evaluator was made for another nc or other thresholds")
    for batch, targets in batches:
        out, counts = predictor.predict_padded(batch)[:2]
        ev.update_padded(out, counts, targets)
    return ev.get_stats()
