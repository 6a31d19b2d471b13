"""ByteTrack behind the predictors: track ids per video stream (the reference's ``mode="track"``:
``ultralytics/trackers/track.py`` hooks ``BYTETracker.update`` behind every predicted frame, default
``cfg/trackers/bytetrack.yaml``).

The batch dimension is the streams: ``out[i]`` / ``counts[i]`` of every :meth:`update` are the next frame of stream
``i``. :class:`ByteTracker` keeps every stream's tracks on the device and runs an update as ONE HIP launch, one
workgroup per stream, with no host sync (``_hip.track_update``, csrc/track.hip). :class:`ByteTrackerHost` has the same
interface on fetched detections - the CPU path, and the steps' one host implementation (``utils/bytetrack.py``, DESIGN
section 34). BoT-SORT (GMC, ReID) is out of scope.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

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
            raise NotImplementedError("tracker_type botsort (GMC, ReID) is not implemented; ByteTrack is: use "
                                      "tracker_type: bytetrack")
        if kind != "bytetrack":
            raise ValueError(f"tracker_type {kind!r}: only bytetrack (ByteTrack) is implemented")
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

    def reset(self, streams=None):
        """Restart all streams, or the listed ones (a sequence of ints or an int32 device tensor); no host sync."""
        if streams is not None and not isinstance(streams, torch.Tensor):
            ids = [int(s) for s in streams]
            if any(not 0 <= s < self.streams for s in ids):
                raise ValueError(f"ByteTracker.reset: streams {ids} outside [0, {self.streams})")
            streams = torch.tensor(ids, dtype=torch.int32).to(self.device, non_blocking=True)
        self._hip.track_reset(self.state, self.capacity, streams)

    def update(self, out, counts) -> Tracks:
        """The next frame of every stream: ``out`` [streams, D, 6] fp32 padded NMS rows and ``counts`` [streams] int32,
        on the device. One launch, no host sync. The returned tensors are the tracker's own and are rewritten by the
        next update."""
        if isinstance(out, torch.Tensor) and out.dim() == 3 and int(out.shape[0]) != self.streams:
            raise ValueError(f"ByteTracker.update: batch of {int(out.shape[0])} for a tracker of {self.streams} streams")
        if isinstance(out, torch.Tensor) and out.dim() == 3:  # anything else is track_update's to refuse
            need = int(self._hip.load_library().yolosod_track_workspace(self.streams, self.capacity, int(out.shape[1])))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        self._hip.track_update(self.state, self.capacity, out, counts, self.params, self._rows, self._counts, self._ws)
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

    def __init__(self, streams, capacity=256, device="cpu", **kw):
        super().__init__(streams, capacity, **kw)
        self.device = torch.device("cpu")
        self.trackers = [bt.StreamTracker(capacity=capacity, **self.args) for _ in range(streams)]

    def reset(self, streams=None):
        for s in (range(self.streams) if streams is None else [int(v) for v in streams]):
            self.trackers[s].reset()

    def update(self, out, counts) -> Tracks:
        out = np.asarray(out.detach().cpu() if isinstance(out, torch.Tensor) else out, dtype=np.float32)
        counts = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
        if out.ndim != 3 or out.shape[2] != 6 or out.shape[0] != self.streams or counts.shape != (self.streams,):
            raise ValueError(f"ByteTrackerHost.update: out {out.shape} / counts {counts.shape} for {self.streams} streams")
        rows = np.zeros((self.streams, self.capacity, 8), dtype=np.float32)
        n = np.zeros((self.streams,), dtype=np.int32)
        for s, t in enumerate(self.trackers):
            r = t.update(out[s], int(counts[s]))
            rows[s, :len(r)] = r
            n[s] = len(r)
        return Tracks(torch.from_numpy(rows), torch.from_numpy(n))

    @property
    def overflow(self) -> torch.Tensor:
        return torch.tensor([t.overflow for t in self.trackers], dtype=torch.int32)


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
