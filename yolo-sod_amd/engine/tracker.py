"""ByteTrack behind the predictors: track ids per video stream (the reference's ``mode="track"``:
``ultralytics/trackers/track.py`` hooks ``BYTETracker.update`` behind every predicted frame, default
``cfg/trackers/bytetrack.yaml``).

The batch dimension is the streams: ``out[i]`` / ``counts[i]`` of every :meth:`update` are the next frame of stream
``i``. :class:`ByteTracker` keeps every stream's tracks on the device and runs an update as ONE HIP launch, one
workgroup per stream, with no host sync (``_hip.track_update``, csrc/track.hip). :class:`ByteTrackerHost` has the same
interface on fetched detections - the CPU path, and the steps' one host implementation (``utils/bytetrack.py``, DESIGN
section 34).

:class:`BotSortTracker` / :class:`BotSortTrackerHost` are the reference's second tracker, BoT-SORT
(``trackers/bot_sort.py``, ``cfg/trackers/botsort.yaml``), for a moving camera: the XYWH Kalman filter and a 2x3
camera-motion warp per stream and update, applied to the tracks before the first association (the XYWH instantiation of
the same kernel; ``utils/botsort.py``). The warp is an input (``update(out, counts, warps=...)``):
estimating it (the reference's OpenCV ``GMC``) and ReID (a stub in the reference) are out of scope.
:func:`tracker_from_yaml` picks the class by the YAML's ``tracker_type`` and by the device.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from ..utils import botsort as bs
from ..utils import bytetrack as bt


class Tracks(NamedTuple):
    """``rows`` [B, T, 8] fp32 = (x1, y1, x2, y2, track_id, score, cls, idx) per activated tracked track, ascending
    ``track_id``, zero padded; ``counts`` [B] int32. ``idx`` is the row of the frame's padded detections."""

    rows: torch.Tensor
    counts: torch.Tensor


@dataclass
class Tracked:
    """Per-stream result: ``boxes`` [n, 7] = (x1, y1, x2, y2, track_id, conf, cls), ``index`` the anchors."""

    boxes: torch.Tensor
    index: torch.Tensor
    orig_shape: tuple


_YAML_KEYS = ("track_high_thresh", "track_low_thresh", "new_track_thresh", "track_buffer", "match_thresh", "fuse_score")
_BOTSORT_YAML_KEYS = ("gmc_method", "proximity_thresh", "appearance_thresh", "with_reid")


class _Base:
    def __init__(self, streams, capacity=256, track_high_thresh=0.25, track_low_thresh=0.1, new_track_thresh=0.25,
                 track_buffer=30, match_thresh=0.8, fuse_score=True, frame_rate=30):
        if isinstance(streams, bool) or not isinstance(streams, int) or streams < 1:
            raise ValueError(f"{type(self).__name__}: streams={streams!r} (an int >= 1)")
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not 64 <= capacity <= 1024 or capacity % 64:
            raise ValueError(f"{type(self).__name__}: capacity={capacity!r} (a multiple of 64 in 64..1024)")
        self.streams, self.capacity = streams, capacity
        self.args = dict(track_high_thresh=track_high_thresh, track_low_thresh=track_low_thresh,
                         new_track_thresh=new_track_thresh, track_buffer=track_buffer, match_thresh=match_thresh,
                         fuse_score=fuse_score, frame_rate=frame_rate)
        self.params = bt.params_vector(**self.args)

    @classmethod
    def from_yaml(cls, path, streams, capacity=256, frame_rate=30, **kw):
        """A tracker from the reference's tracker YAML (``cfg/trackers/bytetrack.yaml`` keys: tracker_type,
        track_high_thresh, track_low_thresh, new_track_thresh, track_buffer, match_thresh, fuse_score)."""
        import yaml
        with open(path) as f:
            cfg = yaml.safe_load(f) or {}
        kind = cfg.get("tracker_type", "bytetrack")
        if kind == "botsort":
            raise NotImplementedError(f"tracker_type botsort is not implemented by {cls.__name__}, a ByteTrack class: "
                                      "use BotSortTracker / BotSortTrackerHost.from_yaml or tracker_from_yaml")
        if kind != "bytetrack":
            raise ValueError(f"tracker_type {kind!r}: bytetrack (ByteTrack) and botsort (BoT-SORT) are implemented")
        args = {k: cfg[k] for k in _YAML_KEYS if k in cfg}
        return cls(streams=streams, capacity=capacity, frame_rate=frame_rate, **args, **kw)


class ByteTracker(_Base):
    """ByteTrack for ``streams`` video streams with ``capacity`` track slots each, state on ``device``. Second-tier
    association needs detections with ``track_low_thresh < conf < track_high_thresh``: the predictor's ``conf`` must be
    at most ``track_low_thresh`` for it to see any (the reference's track mode has the same trait)."""

    def __init__(self, streams, capacity=256, device="cuda", **kw):
        super().__init__(streams, capacity, **kw)
        from .. import _hip
        self._hip = _hip
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"ByteTracker: HIP kernel requires a GPU device (got {self.device}); no CPU fallback - "
                               "ByteTrackerHost is the host path")
        self.state = torch.zeros((streams, _hip.track_state_bytes(capacity)), dtype=torch.uint8, device=self.device)
        self._rows = torch.zeros((streams, capacity, 8), dtype=torch.float32, device=self.device)
        self._counts = torch.zeros((streams,), dtype=torch.int32, device=self.device)
        self._ws = None
        self.reset()

    _MODEL = "xyah"  # the filter's model of the launch (_hip.TRACK_MODELS)

    def reset(self, streams=None):
        """Restart all streams, or the listed ones (a sequence of ints or an int32 device tensor); no host sync."""
        if streams is not None and not isinstance(streams, torch.Tensor):
            ids = [int(s) for s in streams]
            if any(not 0 <= s < self.streams for s in ids):
                raise ValueError(f"{type(self).__name__}.reset: streams {ids} outside [0, {self.streams})")
            streams = torch.tensor(ids, dtype=torch.int32).to(self.device, non_blocking=True)
        self._hip.track_reset(self.state, self.capacity, streams)

    def update(self, out, counts, warps=None) -> Tracks:
        """The next frame of every stream: ``out`` [streams, D, 6] fp32 padded NMS rows and ``counts`` [streams] int32,
        on the device. One launch, no host sync. The returned tensors are the tracker's own and are rewritten by the
        next update. ByteTrack has no camera-motion step: ``warps`` other than None is refused (BotSortTracker takes
        them)."""
        if warps is not None:
            raise ValueError("ByteTracker.update: warps given, but ByteTrack has no camera-motion step; "
                             "BotSortTracker takes them")
        return self._update(out, counts, None)

    def _update(self, out, counts, warps) -> Tracks:
        who = type(self).__name__
        if isinstance(out, torch.Tensor) and out.dim() == 3 and int(out.shape[0]) != self.streams:
            raise ValueError(f"{who}.update: batch of {int(out.shape[0])} for a tracker of {self.streams} streams")
        if isinstance(out, torch.Tensor) and out.dim() == 3:  # anything else is track_update's to refuse
            need = int(self._hip.load_library().yolosod_track_workspace(self.streams, self.capacity, int(out.shape[1])))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        if self._MODEL == "xyah":
            self._hip.track_update(self.state, self.capacity, out, counts, self.params, self._rows, self._counts, self._ws)
        else:
            self._hip.track_update(self.state, self.capacity, out, counts, self.params, self._rows, self._counts, self._ws,
                                   model=self._MODEL, warps=warps)
        return Tracks(self._rows, self._counts)

    @property
    def overflow(self) -> torch.Tensor:
        """[streams] int32 on the device: births skipped so far because no slot was free."""
        return self.state[:, :64].view(torch.int32)[:, 2]

    def fetch_state(self):
        """Debug: the per-stream state as numpy arrays (``_hip.track_state_fetch``; a host sync)."""
        return self._hip.track_state_fetch(self.state, self.capacity)


class ByteTrackerHost(_Base):
    """The same interface on the host: ``update`` takes fetched detections (CPU tensors or numpy arrays) and runs
    ``utils.bytetrack.StreamTracker`` per stream."""

    _STREAM = bt.StreamTracker

    def __init__(self, streams, capacity=256, device="cpu", **kw):
        super().__init__(streams, capacity, **kw)
        self.device = torch.device("cpu")
        self.trackers = [self._STREAM(capacity=capacity, **self.args) for _ in range(streams)]

    def reset(self, streams=None):
        for s in (range(self.streams) if streams is None else [int(v) for v in streams]):
            self.trackers[s].reset()

    def update(self, out, counts, warps=None) -> Tracks:
        if warps is not None:
            raise ValueError("ByteTrackerHost.update: warps given, but ByteTrack has no camera-motion step; "
                             "BotSortTrackerHost takes them")
        return self._update(out, counts, None)

    def _update(self, out, counts, warps) -> Tracks:
        who = type(self).__name__
        out = np.asarray(out.detach().cpu() if isinstance(out, torch.Tensor) else out, dtype=np.float32)
        counts = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
        if out.ndim != 3 or out.shape[2] != 6 or out.shape[0] != self.streams or counts.shape != (self.streams,):
            raise ValueError(f"{who}.update: out {out.shape} / counts {counts.shape} for {self.streams} streams")
        rows = np.zeros((self.streams, self.capacity, 8), dtype=np.float32)
        n = np.zeros((self.streams,), dtype=np.int32)
        for s, t in enumerate(self.trackers):
            r = t.update(out[s], int(counts[s])) if warps is None else t.update(out[s], int(counts[s]), warps[s])
            rows[s, :len(r)] = r
            n[s] = len(r)
        return Tracks(torch.from_numpy(rows), torch.from_numpy(n))

    @property
    def overflow(self) -> torch.Tensor:
        return torch.tensor([t.overflow for t in self.trackers], dtype=torch.int32)


class _BotSortBase:
    """What the two BoT-SORT classes share: the constructor's extra arguments, the YAML route, the warps' checks."""

    def _botsort_args(self, gmc_method, proximity_thresh, appearance_thresh, with_reid):
        if with_reid:
            raise NotImplementedError(f"{type(self).__name__}: with_reid=True: the reference's ReID is a stub (its "
                                      "encoder is always None); only with_reid=False is implemented")
        # recorded, not acted on: the warp is an input of update(), and the two thresholds gate the ReID term only
        self.gmc_method = gmc_method
        self.proximity_thresh, self.appearance_thresh, self.with_reid = proximity_thresh, appearance_thresh, False

    @classmethod
    def from_yaml(cls, path, streams, capacity=256, frame_rate=30, **kw):
        """A tracker from the reference's ``cfg/trackers/botsort.yaml`` keys: ByteTrack's, plus gmc_method (recorded),
        proximity_thresh, appearance_thresh (accepted, ignored) and with_reid (False only)."""
        import yaml
        with open(path) as f:
            cfg = yaml.safe_load(f) or {}
        kind = cfg.get("tracker_type", "botsort")
        if kind == "bytetrack":
            raise ValueError(f"tracker_type bytetrack is not BoT-SORT ({cls.__name__}): use ByteTracker / "
                             "ByteTrackerHost.from_yaml or tracker_from_yaml")
        if kind != "botsort":
            raise ValueError(f"tracker_type {kind!r}: bytetrack (ByteTrack) and botsort (BoT-SORT) are implemented")
        args = {k: cfg[k] for k in _YAML_KEYS + _BOTSORT_YAML_KEYS if k in cfg}
        return cls(streams=streams, capacity=capacity, frame_rate=frame_rate, **{**args, **kw})

    def _warps(self, warps, to_device):
        """``warps`` [streams, 2, 3] fp32 or fp64 (a tensor or an array) -> fp64 where the tracker lives, no sync."""
        if warps is None:
            return None
        w = warps if isinstance(warps, torch.Tensor) else torch.as_tensor(np.asarray(warps))
        if tuple(w.shape) != (self.streams, 2, 3):
            raise ValueError(f"{type(self).__name__}.update: warps {tuple(w.shape)} for {self.streams} streams "
                             f"([{self.streams}, 2, 3] expected)")
        if w.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{type(self).__name__}.update: warps of {w.dtype} (fp32 or fp64 expected)")
        return w.to(device=to_device, dtype=torch.float64, non_blocking=True).contiguous()


class BotSortTracker(_BotSortBase, ByteTracker):
    """BoT-SORT for ``streams`` video streams, state on ``device``: :class:`ByteTracker` with the XYWH filter and
    ``update(out, counts, warps=None)``. ``warps`` [streams, 2, 3] (fp32 or fp64) is every stream's camera motion from
    its previous frame to this one, in the stream's own frame pixels (where the tracks live); ``None`` skips the step,
    as the reference's ``update(results, img=None)`` does. A warp with a non-finite entry is skipped for its stream and
    counted in :attr:`bad_warp`. ``gmc_method`` is recorded only: the warp is estimated elsewhere."""

    _MODEL = "xywh"

    def __init__(self, streams, capacity=256, device="cuda", gmc_method="none", proximity_thresh=0.5,
                 appearance_thresh=0.25, with_reid=False, **kw):
        self._botsort_args(gmc_method, proximity_thresh, appearance_thresh, with_reid)
        ByteTracker.__init__(self, streams, capacity, device, **kw)

    def update(self, out, counts, warps=None) -> Tracks:
        return self._update(out, counts, self._warps(warps, self.device))

    @property
    def bad_warp(self) -> torch.Tensor:
        """[streams] int32 on the device: warps skipped so far because an entry was not finite."""
        return self.state[:, :64].view(torch.int32)[:, 3]


class BotSortTrackerHost(_BotSortBase, ByteTrackerHost):
    """The same interface on the host: ``utils.botsort.BotSortStreamTracker`` per stream."""

    _STREAM = bs.BotSortStreamTracker

    def __init__(self, streams, capacity=256, device="cpu", gmc_method="none", proximity_thresh=0.5,
                 appearance_thresh=0.25, with_reid=False, **kw):
        self._botsort_args(gmc_method, proximity_thresh, appearance_thresh, with_reid)
        ByteTrackerHost.__init__(self, streams, capacity, device, **kw)

    def update(self, out, counts, warps=None) -> Tracks:
        w = self._warps(warps, "cpu")
        return self._update(out, counts, None if w is None else w.numpy())

    @property
    def bad_warp(self) -> torch.Tensor:
        return torch.tensor([t.bad_warp for t in self.trackers], dtype=torch.int32)


def tracker_from_yaml(path, streams, device="cuda", **kw):
    """The tracker a reference tracker YAML asks for: ``tracker_type`` bytetrack or botsort (the reference's default
    file is botsort.yaml's sibling bytetrack.yaml; a file without the key is ByteTrack), the device class on a GPU
    ``device`` and the host class on ``"cpu"``."""
    import yaml
    with open(path) as f:
        kind = (yaml.safe_load(f) or {}).get("tracker_type", "bytetrack")
    on_gpu = torch.device(device).type == "cuda"
    classes = {"bytetrack": (ByteTrackerHost, ByteTracker), "botsort": (BotSortTrackerHost, BotSortTracker)}
    if kind not in classes:
        raise ValueError(f"tracker_type {kind!r}: bytetrack (ByteTrack) and botsort (BoT-SORT) are implemented")
    return classes[kind][on_gpu].from_yaml(path, streams, device=device, **kw)


def takes_warps(tracker) -> bool:
    return isinstance(tracker, _BotSortBase)


def tracked_lists(rows, n_tracks, index, shapes):
    """Per-stream :class:`Tracked` from the padded results (a host sync on ``n_tracks``): boxes [n, 7] = xyxy, id,
    conf, cls, and ``index`` the anchor index gathered through the rows' ``idx``."""
    n = n_tracks.cpu().tolist()
    res = []
    for i, k in enumerate(n):
        r = rows[i, :k]
        idx = r[:, 7].to(torch.int64)
        res.append(Tracked(r[:, :7].clone(), index[i].to(r.device)[idx], shapes[i]))
    return res
