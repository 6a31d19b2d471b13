"""Inference driver for tensor batches and for lists of raw frames (the reference's predictor hot loop; of the absent
``ultralytics/data`` only LetterBox's geometry is restated, ``data/augment.py``).

Reference flow (``engine/predictor.py:116-143, 219-304`` and ``models/yolo/detect/predict.py:23-41``):
``preprocess`` (tensor input: ``.to(device).float()``, no /255, no letterbox; list of uint8 HWC BGR frames: LetterBox,
RGB, CHW, /255) -> ``AutoBackend`` forward of the fused model -> ``postprocess`` = ``non_max_suppression`` +
``scale_boxes`` (same-shape tensor input: clip to the image; frames: back to each frame's pixels).

MI355X additions:
* :meth:`DetectionPredictor.predict_padded` never syncs the host: NMS returns fixed-shape ``[B, max_det, 6]``
  rows + counts, so a batch is one stream-ordered sequence of launches (graph-capturable). ``__call__`` (which syncs
  for the per-image lists anyway) also reads the split-range guard and redoes a batch whose operands left the fp16-split
  kernels' range on the exact fp32 kernels; predict_padded callers read ``_hip.split_range_flag()`` themselves.
* Data parallel inference: one process per GPU; :func:`shard_bounds` splits images across ranks (no data-path
  collective), :func:`gather_detections` is the single exchange step - ONE all-gather of a packed int32 buffer per
  image holding the padded detections, the kept anchor indices and the count (RCCL over xGMI with backend ``nccl``;
  ``gloo`` on CPU for tests): one collective latency instead of three, ~8.4 KB per image at max_det 300.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.distributed as dist

from .. import _hip
from ..data.augment import LetterBox
from ..data.nv12 import NV12Frame
from ..data.slicing import SlicePlan
from ..utils import ops


@dataclass
class Detections:
    """Per-image result: ``boxes`` [n, 6] = (x1, y1, x2, y2, conf, cls) clipped to the image, ``index`` anchors."""

    boxes: torch.Tensor
    index: torch.Tensor
    orig_shape: tuple


class Ingested:
    """A list of raw frames after :meth:`DetectionPredictor.preprocess`: the model's input tensor ``x``, each frame's
    ``(h, w)`` and the device tensor ``geom`` [B, 5] = (gain, pad_x, pad_y, w0, h0) that maps boxes back."""

    __slots__ = ("x", "shapes", "geom")

    def __init__(self, x, shapes, geom):
        self.x, self.shapes, self.geom = x, shapes, geom


def frames_to_device(frames, device, who="DetectionPredictor"):
    """A list of uint8 HWC BGR frames (numpy arrays or torch tensors, on the CPU or on the GPU, any sizes) as a list of
    uint8 [h, w, 3] tensors on the GPU. CPU frames go up as they are: packed into one pinned staging buffer (16-byte
    aligned slots), one H2D copy, no host sync; GPU frames pass through untouched.

    A list of :class:`NV12Frame` goes up the same way (:func:`_nv12_to_device`) and comes back as a list of NV12Frame
    on the GPU; a list that mixes the two kinds is refused."""
    if len(frames) == 0:
        raise ValueError(f"{who}: empty list of frames")
    nv12 = [isinstance(f, NV12Frame) for f in frames]
    if any(nv12):
        if not all(nv12):
            raise TypeError(f"{who}: the list mixes BGR arrays and NV12Frame (frame {nv12.index(False)} is no "
                            "NV12Frame); one kind per call")
        return _nv12_to_device(frames, device)
    ts = []
    for i, f in enumerate(frames):
        if not isinstance(f, torch.Tensor):
            import numpy as np
            f = np.asarray(f)
            if any(s < 0 for s in f.strides):
                f = np.ascontiguousarray(f)
            f = torch.from_numpy(f)
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            raise RuntimeError(f"{who}: frame {i} must be uint8 [h, w, 3] (BGR), got {f.dtype} "
                               f"{tuple(f.shape)}")
        ts.append(f)
    host = [i for i, t in enumerate(ts) if t.device.type == "cpu"]
    if host:
        offs, total = [], 0
        for i in host:
            offs.append(total)
            total += (ts[i].numel() + 15) // 16 * 16
        stage = torch.empty(total, dtype=torch.uint8).pin_memory()
        for i, o in zip(host, offs):
            stage[o:o + ts[i].numel()].view(ts[i].shape).copy_(ts[i])
        up = stage.to(device, non_blocking=True)
        for i, o in zip(host, offs):
            ts[i] = up[o:o + ts[i].numel()].view(ts[i].shape)
    return ts


def _nv12_to_device(frames, device):
    """NV12 frames on the GPU: the planes of CPU frames packed into one pinned staging buffer (16-byte aligned slots,
    every plane contiguous there), one H2D copy, no host sync; a frame whose planes are on the GPU passes through."""
    device = torch.device(device)
    planes = [(i, k, p) for i, f in enumerate(frames) for k, p in enumerate((f.y, f.uv)) if p.device.type == "cpu"]
    up = {}
    if planes:
        offs, total = [], 0
        for _, _, p in planes:
            offs.append(total)
            total += (p.numel() + 15) // 16 * 16
        stage = torch.empty(total, dtype=torch.uint8).pin_memory()
        for (_, _, p), o in zip(planes, offs):
            stage[o:o + p.numel()].view(p.shape).copy_(p)
        dev = stage.to(device, non_blocking=True)
        for (i, k, p), o in zip(planes, offs):
            up[i, k] = dev[o:o + p.numel()].view(p.shape)
    return [NV12Frame._view(up.get((i, 0), f.y), up.get((i, 1), f.uv), f.matrix, f.parity)
            for i, f in enumerate(frames)]


class DetectionPredictor:
    def __init__(self, model, conf=0.25, iou=0.7, max_det=300, classes=None, agnostic_nms=False,
                 multi_label=False, imgsz=640, rect=None, augment=False, merge_nms=False, tracker=None):
        self.model = model
        # track mode (engine/tracker.py): a ByteTracker whose streams are this predictor's batch; :meth:`track`
        self.tracker = tracker
        self.conf, self.iou, self.max_det = conf, iou, max_det
        # merge-NMS (ops.non_max_suppression_padded(merge=True)): kept boxes are their clusters' score-weighted means,
        # merged in canvas pixels before the boxes are mapped and clipped; ``n_merged`` [B, max_det] int32 of the last
        # batch (the clusters' sizes, a device tensor) stays on the predictor, None until then and without merge_nms
        self.merge_nms = bool(merge_nms)
        self.n_merged = None
        self.classes, self.agnostic, self.multi_label = classes, agnostic_nms, multi_label
        # test-time augmentation (DetectionModel._predict_augment: three views, one concatenated prediction tensor in
        # canvas pixels, so NMS and everything after it are the same; ``index`` then counts along that concatenation:
        # model.tta_plan(canvas).locate(index) gives the branch and its anchor)
        self.augment = bool(augment)
        p = next(model.parameters())
        self.device, self.dtype = p.device, p.dtype
        # list input (raw frames): the canvas, and whether same-shape batches take the minimal rectangle
        # (None: the reference's rule, predictor.py:155-160; True / False force it)
        self.imgsz = (imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)
        self.rect = rect
        self.stride = int(max(getattr(model, "stride", torch.tensor([32.0]))))  # LetterBox's `auto` modulus

    def preprocess(self, im):
        """predictor.py:116-134. Tensor branch: ``.to(device)``, ``.half()`` if the model is fp16 else ``.float()`` -
        here the model's dtype (bf16 in the bf16 config); no /255, no letterbox. List branch (raw frames): see
        :meth:`ingest`."""
        if isinstance(im, (list, tuple)):
            return self.ingest(im).x
        return im.to(self.device, non_blocking=True).to(self.dtype)

    def ingest(self, frames) -> Ingested:
        """predictor.py:116-134 non-tensor branch + pre_transform :145-161 for a list of uint8 HWC BGR frames (numpy
        arrays or torch tensors, on the CPU or on the GPU, any sizes): LetterBox, BGR -> RGB, HWC -> CHW, the model's
        dtype, / 255 - as one HIP launch on the raw bytes (``_hip.letterbox_ingest``). CPU frames go up as they are:
        packed into one pinned buffer, one H2D copy, no host resize. Everything else here is arithmetic on shapes:
        no host sync. A list of :class:`NV12Frame` (decoded video) takes the same path through
        ``_hip.letterbox_ingest_nv12``: the colour conversion is part of that launch, everything else is shared."""
        ts = frames_to_device(frames, self.device, "DetectionPredictor")
        nv12 = isinstance(ts[0], NV12Frame)
        shapes = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
        same = all(s == shapes[0] for s in shapes)
        auto = same if self.rect is None else bool(self.rect)
        if auto and not same:
            raise ValueError("DetectionPredictor(rect=True): frames of different shapes give different canvases")
        lb = LetterBox(self.imgsz, auto=auto, stride=self.stride)
        geoms = [lb.geometry(s) for s in shapes]
        canvas = geoms[0][4:]
        ingest = _hip.letterbox_ingest_nv12 if nv12 else _hip.letterbox_ingest
        x = ingest(ts, canvas, geoms, self.dtype, pad_value=lb.pad_value)
        # scale_boxes' own gain / pad (ratio_pad=None, ops.py:92-105), recomputed from the two shapes as it does
        rows = []
        for h0, w0 in shapes:
            gain = min(canvas[0] / h0, canvas[1] / w0)
            rows.append([gain, round((canvas[1] - w0 * gain) / 2 - 0.1), round((canvas[0] - h0 * gain) / 2 - 0.1),
                         w0, h0])
        geom = torch.tensor(rows, dtype=torch.float64).to(torch.float32).pin_memory().to(self.device, non_blocking=True)
        return Ingested(x, shapes, geom)

    def _forward(self, x):
        """The model's prediction tensor [B, 4+nc, A] for the input tensor x (A = the plan's A_tot with ``augment``)."""
        preds = self.model(x, augment=True) if self.augment else self.model(x)
        return preds[0] if isinstance(preds, (list, tuple)) else preds

    def _nms(self, y):
        """NMS of the prediction tensor y as this predictor is set up (in_place=False); with ``merge_nms`` the merged
        rows, ``n_merged`` kept on the predictor."""
        res = ops.non_max_suppression_padded(
            y, self.conf, self.iou, classes=self.classes, agnostic=self.agnostic, multi_label=self.multi_label,
            max_det=self.max_det, in_place=False, merge=self.merge_nms)
        if self.merge_nms:
            self.n_merged = res[3]
        return res[:3]

    def _predict_ingested(self, ing: Ingested):
        """The model, NMS and the boxes back in each frame's pixels (predict.py:23-41: scale_boxes(img.shape[2:], boxes,
        orig_img.shape) per image) as one more launch on the padded rows."""
        preds = self._forward(ing.x)
        y = preds[0] if isinstance(preds, (list, tuple)) else preds
        out, counts, index = self._nms(y)
        _hip.scale_boxes_padded(out, counts, ing.geom)
        return out, counts, index

    @torch.inference_mode()
    def predict_padded(self, im):
        """(out [B, max_det, 6] clipped, counts [B] int32, index [B, max_det] int32) without host sync. A list of raw
        frames (:meth:`ingest`) gives boxes in each frame's own pixels."""
        if isinstance(im, (list, tuple)):
            return self._predict_ingested(self.ingest(im))
        x = self.preprocess(im)
        y = self._forward(x)
        # in_place=False: the reference's postprocess rewrites preds[:, :4] to xyxy (ops.py:167, in_place=True) and
        # then drops preds; y is local here too, so the rewrite (17 MB at bs 32) is skipped - same detections
        out, counts, index = self._nms(y)
        ops.clip_boxes(out[..., :4], x.shape[2:])  # scale_boxes with gain 1 / pad 0 (same-shape tensor input)
        return out, counts, index

    def predict_padded_guarded(self, im: torch.Tensor):
        """:meth:`predict_padded`, then the split-range guard (reads one flag word: a host sync): a batch in which an
        operand left the fp16-split kernels' range (|v| > 65504, or NaN) is redone on the exact fp32 MFMA kernels."""
        if isinstance(im, (list, tuple)):
            return self._predict_list_guarded(im)[:3]
        out, counts, index = self.predict_padded(im)
        if self.dtype == torch.float32 and _hip.split_range_flag(reset=True, device=self.device):
            with _hip.exact_fp32_matrix():
                out, counts, index = self.predict_padded(im)
            _hip.split_range_flag(reset=True, device=self.device)
        return out, counts, index

    @torch.inference_mode()
    def _predict_list_guarded(self, frames):
        """The guarded step on raw frames: they are ingested once, and a redo reuses the ingested tensor."""
        ing = self.ingest(frames)
        out, counts, index = self._predict_ingested(ing)
        if self.dtype == torch.float32 and _hip.split_range_flag(reset=True, device=self.device):
            with _hip.exact_fp32_matrix():
                out, counts, index = self._predict_ingested(ing)
            _hip.split_range_flag(reset=True, device=self.device)
        return out, counts, index, ing.shapes

    @torch.inference_mode()
    def track_padded(self, frames, warps=None):
        """:meth:`predict_padded`, then the tracker's update on the rows (after ``scale_boxes_padded``: tracks live in
        each stream's own pixels): (rows [B, T, 8], n_tracks [B], out, counts, index), no host sync. ``frames[i]`` is
        the next frame of stream ``i``; the batch must be the tracker's ``streams``. The second-tier association only
        sees detections the NMS lets through: it needs ``conf <= track_low_thresh`` (the reference's track mode has
        the same trait; the default ``conf`` stays 0.25). ``warps`` [B, 2, 3], for a BoT-SORT tracker: every stream's
        camera motion since its previous frame, in that stream's own frame pixels (not the letterboxed ones)."""
        _require_tracker(self.tracker, len(frames), "DetectionPredictor", warps)
        out, counts, index = self.predict_padded(frames)
        rows, n_tracks = _tracker_update(self.tracker, out, counts, warps)
        return rows, n_tracks, out, counts, index

    def track(self, frames, warps=None):
        """Per stream :class:`~.tracker.Tracked` (boxes [n, 7] = xyxy, id, conf, cls; index; orig_shape); syncs for
        the per-stream lists."""
        from .tracker import tracked_lists
        rows, n_tracks, out, counts, index = self.track_padded(frames, warps)
        if isinstance(frames, (list, tuple)):
            shapes = [tuple(int(v) for v in f.shape[:2]) for f in frames]
        else:
            shapes = [tuple(frames.shape[2:])] * int(frames.shape[0])
        return tracked_lists(rows, n_tracks, index, shapes)

    def __call__(self, im):
        if isinstance(im, (list, tuple)):
            out, counts, index, shapes = self._predict_list_guarded(im)
            n = counts.cpu().tolist()
            return [Detections(out[i, : n[i]], index[i, : n[i]], shapes[i]) for i in range(len(n))]
        out, counts, index = self.predict_padded_guarded(im)
        n = counts.cpu().tolist()
        shape = tuple(im.shape[2:])
        return [Detections(out[i, : n[i]], index[i, : n[i]], shape) for i in range(len(n))]


class SlicedPredictor:
    """Sliced inference for frames much larger than the canvas (the project's own; the reference has none): every frame
    is cut into overlapping ``slice`` tiles at native resolution (``data/slicing.py``), the model runs on the tiles and,
    with ``full_frame``, on the whole frame too, and all candidates of a frame meet in ONE NMS in frame pixels.

    Takes a list of uint8 HWC BGR frames (numpy arrays, CPU or GPU tensors, any sizes) or a list of :class:`NV12Frame`
    (a tile is then ``frame.crop(*rect)``, ingested by ``_hip.letterbox_ingest_nv12``; all else is the same). Stages, each a method so that a
    test or a validator can check it on the same tensors: :meth:`plan` (host arithmetic) -> :meth:`forward_tiles`
    (tiles are views of the device frames, letterboxed onto the one canvas by ``_hip.letterbox_ingest`` straight from
    the frame's memory, ``batch`` tiles per model call, tiles of different frames share a call) -> :meth:`merge`
    (``_hip.tile_merge`` per call into merged [F, 4+nc, S*A], frame pixels) -> :meth:`postprocess` (NMS on merged,
    clip to the frame). ``index`` of a detection is ``slot * A + anchor``; ``plan.slot(frame, slot)`` is its tile.

    ``augment=True``: test-time augmentation on every tile (``scales`` / ``flips`` as ``DetectionModel.tta_plan`` takes
    them; None: the reference's three views). Every tile is letterboxed onto the same ``imgsz`` canvas, so one
    ``TTAPlan`` serves the batch; a model call is then K branches, :meth:`forward_tiles` gives per call the tuple of
    their outputs [n_i, 4+nc, A_k] (each in its own view's pixels), and :meth:`merge` puts every branch straight into
    merged [F, 4+nc, S*A_tot] with one ``_hip.tile_merge_tta`` launch: the concatenated tensor of
    ``model(x, augment=True)`` is never made. ``index`` is then ``slot * A_tot + j``, j along the plan's
    concatenation; :meth:`locate` takes it apart. Everything after ``merged`` is the same.

    ``cut_margin`` (tile pixels; None: off): a candidate whose box comes within it of a tile edge that is interior to
    the frame is dropped before NMS - the tile saw the object truncated, a neighbouring tile or the whole-frame slot
    sees it whole. ``merged`` takes F * (4+nc) * S * A * 4 bytes.

    ``merge_nms=True``: the one NMS is a merge-NMS (``ops.non_max_suppression_padded(merge=True)``): an object seen by
    several tiles, the whole frame and the augmented views gives one row whose box is the score-weighted mean of all of
    them, in frame pixels; the clusters' sizes of the last batch are ``n_merged`` [F, max_det] int32."""

    def __init__(self, model, slice=640, overlap=0.2, full_frame=True, cut_margin=None, batch=32, conf=0.25, iou=0.7,
                 max_det=300, classes=None, agnostic_nms=False, multi_label=False, imgsz=640, augment=False, scales=None,
                 flips=None, merge_nms=False, tracker=None):
        self.model = model
        self.tracker = tracker  # track mode, as DetectionPredictor's
        # merge-NMS in frame pixels, before the clip to the frame; ``n_merged`` [F, max_det] int32 of the last batch
        self.merge_nms = bool(merge_nms)
        self.n_merged = None
        self.augment = bool(augment)
        if not self.augment and (scales is not None or flips is not None):
            raise ValueError("SlicedPredictor: scales / flips are the views of augment=True")
        self.scales = None if scales is None else tuple(scales)
        self.flips = None if flips is None else tuple(flips)
        self.slice, self.overlap, self.full_frame = slice, overlap, bool(full_frame)
        self.cut_margin = None if cut_margin is None else float(cut_margin)
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"SlicedPredictor: batch={batch}")
        self.conf, self.iou, self.max_det = conf, iou, max_det
        self.classes, self.agnostic, self.multi_label = classes, agnostic_nms, multi_label
        p = next(model.parameters())
        self.device, self.dtype = p.device, p.dtype
        self.imgsz = (imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)
        self.stride = int(max(getattr(model, "stride", torch.tensor([32.0]))))

    def plan(self, shapes) -> SlicePlan:
        """The slots of frames of these ``(h, w)`` shapes."""
        return SlicePlan(shapes, self.slice, self.overlap, self.full_frame, self.imgsz, self.stride)

    def _views(self, ts, plan, lo, hi):
        views = []
        for f, k in plan.order[lo:hi]:
            y0, x0, y1, x1 = plan.slots[f][k].rect
            views.append(ts[f].crop(y0, x0, y1, x1) if isinstance(ts[f], NV12Frame) else ts[f][y0:y1, x0:x1])
        return views

    def ingest_tiles(self, frames, plan, lo=0, hi=None):
        """The model's input for tiles ``plan.order[lo:hi]``: [hi - lo, 3, *canvas], one launch on views of the frames."""
        ts = frames_to_device(frames, self.device, "SlicedPredictor")
        hi = len(plan) if hi is None else hi
        geoms = [plan.slots[f][k].geometry for f, k in plan.order[lo:hi]]
        ingest = _hip.letterbox_ingest_nv12 if isinstance(ts[0], NV12Frame) else _hip.letterbox_ingest
        return ingest(self._views(ts, plan, lo, hi), plan.canvas, geoms, self.dtype, pad_value=plan.pad_value)

    def tta_plan(self, plan):
        """The ``TTAPlan`` of the tiles of ``plan`` (``augment=True``): every tile is on the one canvas."""
        if not self.augment:
            raise RuntimeError("SlicedPredictor: tta_plan is for augment=True")
        return self.model.tta_plan(plan.canvas, self.scales, self.flips)

    def _calls(self, ts, plan):
        """The model calls in ``plan.order``, one at a time: yields ``(lo, y)``, y the Detect output [n_i, 4+nc, A] of
        tiles ``order[lo:lo + n_i]``, or with ``augment`` one branch of it, ``(lo, (k, y_k))``, K times per call."""
        tp = self.tta_plan(plan) if self.augment else None
        for lo, hi in plan.chunks(self.batch):
            x = self.ingest_tiles(ts, plan, lo, hi)
            if tp is None:
                preds = self.model(x)
                yield lo, preds[0] if isinstance(preds, (list, tuple)) else preds
            else:
                for k, y in self.model.augment_branches(x, tp):
                    yield lo, (k, y)

    @torch.inference_mode()
    def forward_tiles(self, frames, plan):
        """The Detect outputs [n_i, 4+nc, A] (fp32, canvas pixels) of the model calls, ``batch`` tiles at most each, in
        ``plan.order``; with ``augment`` per call the tuple of its K branch outputs [n_i, 4+nc, A_k], each in its own
        view's pixels (the views are ``_hip.tta_views`` of the ingested tiles). CPU frames go up once."""
        ts = frames_to_device(frames, self.device, "SlicedPredictor")
        if [tuple(t.shape[:2]) for t in ts] != plan.shapes:
            raise ValueError("SlicedPredictor: the plan was made for other frame shapes")
        ys = [y for _, y in self._calls(ts, plan)]
        if self.augment:
            K = len(self.tta_plan(plan))
            ys = [tuple(y for _, y in ys[i:i + K]) for i in range(0, len(ys), K)]
        return ys

    def _merge_into(self, merged, y, plan, lo):
        """One call's output (with ``augment`` one branch of it, ``(k, y_k)``) for tiles ``order[lo:lo + n]`` into
        ``merged`` (None: allocated here), one launch. Returns ``merged``."""
        k, y = y if self.augment else (None, y)
        tp = self.tta_plan(plan) if self.augment else None
        A = int(y.shape[2]) if tp is None else tp.A_tot
        if merged is None:
            merged = torch.empty((len(plan.shapes), int(y.shape[1]), plan.S * A), dtype=torch.float32, device=y.device)
        rows = plan.merge_rows(lo, lo + int(y.shape[0]))
        if tp is None:
            return _hip.tile_merge(y, rows, merged, A, self.cut_margin)
        return _hip.tile_merge_tta(y, rows, merged, A, tp.branches[k], plan.canvas, self.cut_margin)

    def merge(self, y_chunks, plan):
        """merged [F, 4+nc, S*A] in frame pixels from the model calls' outputs (any grouping of ``plan.order`` into
        consecutive calls): one ``_hip.tile_merge`` launch per call; every (frame, slot) is written exactly once. With
        ``augment`` a call is the tuple of its K branch outputs, A is the plan's A_tot and a call takes K
        ``_hip.tile_merge_tta`` launches, each writing its branch's range of every slot the call names."""
        y_chunks = list(y_chunks)
        for c in y_chunks:
            for y in (c if isinstance(c, (tuple, list)) else (c,)):
                if not isinstance(y, torch.Tensor) or y.device.type != "cuda":
                    raise RuntimeError("SlicedPredictor.merge: HIP kernel requires GPU tensors; no CPU fallback")
        if self.augment:
            K = len(self.tta_plan(plan))
            if any(not isinstance(c, (tuple, list)) or len(c) != K for c in y_chunks):
                raise ValueError(f"SlicedPredictor.merge: with augment a call is the tuple of its {K} branch outputs")
            if any(len({int(y.shape[0]) for y in c}) != 1 for c in y_chunks):
                raise ValueError("SlicedPredictor.merge: the branches of a call hold different numbers of tiles")
        first = [c[0] if self.augment else c for c in y_chunks]
        if not first or sum(int(y.shape[0]) for y in first) != len(plan):
            raise ValueError(f"SlicedPredictor.merge: the chunks hold {sum(int(y.shape[0]) for y in first)} tiles, "
                             f"the plan {len(plan)}")
        merged, lo = None, 0
        for c, y0 in zip(y_chunks, first):
            for y in (enumerate(c) if self.augment else (c,)):
                merged = self._merge_into(merged, y, plan, lo)
            lo += int(y0.shape[0])
        return merged

    def postprocess(self, merged, plan):
        """One NMS per frame over all its slots, boxes clipped to the frame: (out [F, max_det, 6], counts [F],
        index [F, max_det] = slot * A + anchor; with ``augment`` slot * A_tot + j, :meth:`locate`)."""
        res = ops.non_max_suppression_padded(
            merged, self.conf, self.iou, classes=self.classes, agnostic=self.agnostic, multi_label=self.multi_label,
            max_det=self.max_det, max_wh=max(7680, max(max(s) for s in plan.shapes)), in_place=False,
            merge=self.merge_nms)
        out, counts, index = res[:3]
        if self.merge_nms:
            self.n_merged = res[3]
        geom = torch.tensor([[1.0, 0.0, 0.0, w, h] for h, w in plan.shapes], dtype=torch.float32)
        _hip.scale_boxes_padded(out, counts, geom.pin_memory().to(out.device, non_blocking=True))
        return out, counts, index

    @torch.inference_mode()
    def _predict(self, ts, plan):
        """The stages with every call (every branch of it) merged as soon as it has run: one output is alive at a time."""
        merged = None
        for lo, y in self._calls(ts, plan):
            merged = self._merge_into(merged, y, plan, lo)
        return self.postprocess(merged, plan)

    def locate(self, index, plan):
        """``(slot, branch, anchor)`` of a detection's ``index``: ``plan.slot(frame, slot)`` is its tile, ``anchor`` counts
        along that branch's own output (branch 0 and the one output without ``augment``)."""
        if self.augment:
            tp = self.tta_plan(plan)
            A = tp.A_tot
        else:
            A = self.model.tta_plan(plan.canvas, (1,), (None,)).branches[0].A  # the canvas' anchor count
        index = int(index)
        if not 0 <= index < plan.S * A:
            raise IndexError(f"SlicedPredictor.locate: {index} outside [0, {plan.S} * {A})")
        slot, j = divmod(index, A)
        return (slot, *tp.locate(j)) if self.augment else (slot, 0, j)

    def index(self, slot, branch, anchor, plan):
        """Inverse of :meth:`locate`; None for an anchor that the augmentation's clip drops."""
        if not 0 <= slot < plan.S:
            raise IndexError(f"SlicedPredictor.index: slot {slot} outside [0, {plan.S})")
        if self.augment:
            tp = self.tta_plan(plan)
            j = tp.index(branch, anchor)
            return None if j is None else slot * tp.A_tot + j
        A = self.model.tta_plan(plan.canvas, (1,), (None,)).branches[0].A
        if branch != 0 or not 0 <= anchor < A:
            raise IndexError(f"SlicedPredictor.index: branch {branch}, anchor {anchor} (one branch of {A} anchors)")
        return slot * A + anchor

    def _start(self, frames):
        if not isinstance(frames, (list, tuple)):
            raise TypeError("SlicedPredictor: expected a list of uint8 [h, w, 3] frames")
        ts = frames_to_device(frames, self.device, "SlicedPredictor")
        return ts, self.plan([t.shape[:2] for t in ts])

    def predict_padded(self, frames):
        """(out [F, max_det, 6] in each frame's pixels, counts [F] int32, index [F, max_det] int32), no host sync."""
        ts, plan = self._start(frames)
        return self._predict(ts, plan)

    def _predict_guarded(self, frames):
        ts, plan = self._start(frames)
        res = self._predict(ts, plan)
        if self.dtype == torch.float32 and _hip.split_range_flag(reset=True, device=self.device):
            with _hip.exact_fp32_matrix():
                res = self._predict(ts, plan)
            _hip.split_range_flag(reset=True, device=self.device)
        return res, plan

    def predict_padded_guarded(self, frames):
        """:meth:`predict_padded`, then the split-range guard as ``DetectionPredictor.predict_padded_guarded``: the flag
        is read once (a host sync) and a batch that left the fp16-split kernels' range is redone on the exact fp32
        kernels (the frames are not uploaded again)."""
        return self._predict_guarded(frames)[0]

    def track_padded(self, frames, warps=None):
        """:meth:`predict_padded`, then the tracker's update on the rows in frame pixels: (rows [F, T, 8], n_tracks [F],
        out, counts, index), no host sync; as ``DetectionPredictor.track_padded`` (``conf <= track_low_thresh`` for a
        second tier; ``warps`` [F, 2, 3] in frame pixels for a BoT-SORT tracker)."""
        _require_tracker(self.tracker, len(frames), "SlicedPredictor", warps)
        out, counts, index = self.predict_padded(frames)
        rows, n_tracks = _tracker_update(self.tracker, out, counts, warps)
        return rows, n_tracks, out, counts, index

    def track(self, frames, warps=None):
        """Per stream :class:`~.tracker.Tracked`; ``index`` is ``slot * A + anchor`` (:meth:`locate`)."""
        from .tracker import tracked_lists
        rows, n_tracks, out, counts, index = self.track_padded(frames, warps)
        return tracked_lists(rows, n_tracks, index, [tuple(int(v) for v in f.shape[:2]) for f in frames])

    def __call__(self, frames):
        (out, counts, index), plan = self._predict_guarded(frames)
        n = counts.cpu().tolist()
        return [Detections(out[i, : n[i]], index[i, : n[i]], plan.shapes[i]) for i in range(len(n))]


def _require_tracker(tracker, batch, who, warps=None):
    if tracker is None:
        raise RuntimeError(f"{who}.track: constructed without a tracker (tracker=ByteTracker(streams=...))")
    if int(batch) != tracker.streams:
        raise ValueError(f"{who}.track: batch of {int(batch)} frames for a tracker of {tracker.streams} streams")
    if warps is not None:
        from .tracker import takes_warps
        if not takes_warps(tracker):
            raise ValueError(f"{who}.track: warps given, but the tracker is a {type(tracker).__name__}: ByteTrack has "
                             "no camera-motion step (tracker=BotSortTracker(streams=...))")


def _tracker_update(tracker, out, counts, warps):
    return tracker.update(out, counts) if warps is None else tracker.update(out, counts, warps)


def shard_bounds(n: int, rank: int, world: int):
    """Contiguous, balanced image shard [lo, hi) of rank ``rank``."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def pack_detections(out: torch.Tensor, counts: torch.Tensor, index: torch.Tensor | None = None) -> torch.Tensor:
    """One int32 row per image: the [D, 6] fp32 rows (bit patterns), then the [D] kept anchor indices (if given),
    then the count - [B, 6D (+ D) + 1], contiguous (the single buffer the exchange step all-gathers)."""
    B, D = out.shape[:2]
    parts = [out.float().reshape(B, D * 6).contiguous().view(torch.int32)]
    if index is not None:
        parts.append(index.to(torch.int32).reshape(B, D))
    parts.append(counts.to(torch.int32).reshape(B, 1))
    return torch.cat(parts, 1).contiguous()


def unpack_detections(packed: torch.Tensor, D: int, with_index: bool):
    """Inverse of :func:`pack_detections`: (out [B, D, 6] fp32, counts [B] int32[, index [B, D] int32])."""
    B = packed.shape[0]
    out = packed[:, : 6 * D].contiguous().view(torch.float32).reshape(B, D, 6)
    counts = packed[:, -1].contiguous()
    if not with_index:
        return out, counts
    return out, counts, packed[:, 6 * D: 7 * D].contiguous()


def gather_detections(out: torch.Tensor, counts: torch.Tensor, index: torch.Tensor | None = None, group=None):
    """All-gather padded detections of equal-size shards: [B_local, D, 6] + [B_local] (+ the kept anchor indices
    [B_local, D]) -> [world*B_local, ...] in rank order, as ONE collective on the packed buffer
    (:func:`pack_detections`). Returns (out, counts) or (out, counts, index)."""
    world = dist.get_world_size(group)
    packed = pack_detections(out, counts, index)
    g = torch.empty((world * packed.shape[0], packed.shape[1]), dtype=packed.dtype, device=packed.device)
    dist.all_gather_into_tensor(g, packed, group=group)
    return unpack_detections(g, out.shape[1], index is not None)


def sharded_predict(predict_padded, n_images: int, images, group=None, split_guard: bool = True):
    """Data-parallel inference over ``n_images`` global images, one process per GPU.

    ``images(lo, hi)`` returns this rank's shard (global images [lo, hi), ``shard_bounds``) - each rank
    materialises only its own images; ``predict_padded(x) -> (out [b, D, 6], counts [b], index [b, D])`` is the
    rank-local path (``DetectionPredictor.predict_padded``). Shards are padded to the largest shard (count 0,
    index -1) so one fixed-size all-gather serves uneven splits. Returns (out [n_images, D, 6], counts [n_images],
    index [n_images, D]) in global image order on every rank: the kept anchor indices of every image
    (``models/yolo/detect/predict.py:23-41`` per image) survive the exchange.

    ``split_guard``: after the rank-local step on a GPU, the split-range flag is read (a host sync) and a shard whose
    operands left the fp16-split kernels' range is redone on the exact fp32 kernels before the exchange, as
    :meth:`DetectionPredictor.__call__` does for one process."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    lo, hi = shard_bounds(n_images, rank, world)
    x = images(lo, hi)
    out, counts, index = predict_padded(x)[:3]
    model_dtype = getattr(getattr(predict_padded, "__self__", None), "dtype", torch.float32)  # bf16: no split kernels
    if split_guard and out.is_cuda and model_dtype == torch.float32 and _hip.split_range_flag(reset=True,
                                                                                              device=out.device):
        with _hip.exact_fp32_matrix():
            out, counts, index = predict_padded(x)[:3]
        _hip.split_range_flag(reset=True, device=out.device)
    smax = -(-n_images // world)
    if out.shape[0] < smax:
        pad = smax - out.shape[0]
        out = torch.cat([out, out.new_zeros((pad, *out.shape[1:]))])
        counts = torch.cat([counts, counts.new_zeros((pad,))])
        index = torch.cat([index, index.new_full((pad, *index.shape[1:]), -1)])
    g_out, g_cnt, g_idx = gather_detections(out, counts, index, group)
    if n_images % world:
        keep = torch.cat([torch.arange(r * smax, r * smax + (b - a)) for r in range(world)
                          for a, b in [shard_bounds(n_images, r, world)]])
        g_out, g_cnt, g_idx = (t[keep.to(t.device)] for t in (g_out, g_cnt, g_idx))
    return g_out, g_cnt, g_idx


def seeded_images(lo: int, hi: int, imgsz: int, seed: int = 1000, device=None) -> torch.Tensor:
    """Synthetic input batch of global images [lo, hi): image i = torch.rand(3, imgsz, imgsz) from a generator
    seeded ``seed + i``, so every rank's shard is a slice of one global batch whatever the world size."""
    x = torch.empty((hi - lo, 3, imgsz, imgsz))
    for k, i in enumerate(range(lo, hi)):
        x[k] = torch.rand(3, imgsz, imgsz, generator=torch.Generator().manual_seed(seed + i))
    return x if device is None else x.to(device)
