"""ByteTrack, one stream at a time, in numpy: the steps of the reference's ``BYTETracker.update`` on a fixed number of
track slots. This is the one host implementation of the steps: ``engine.tracker.ByteTrackerHost`` runs it on fetched
detections, ``tests/bytetrack_ref.py`` adds the decision margins and the scene generators, and the HIP kernel
(csrc/track.hip) is held to it.

Written from reading ``ultralytics/trackers/byte_tracker.py:293-405`` (update), ``basetrack.py`` (states, ids),
``utils/kalman_filter.py:65-236`` (KalmanFilterXYAH), ``utils/matching.py:20-157`` (linear_assignment, iou_distance,
fuse_score), ``utils/metrics.py:20-49`` (bbox_ioa) and ``utils/ops.py`` (xyxy2xywh, xywh2ltwh). Every dtype is spelled
out so nothing here depends on NumPy's promotion rules.

Assignment. The reference calls ``lap.lapjv(cost, extend_cost=True, cost_limit=thresh)`` (matching.py:45), which solves
the square problem of size N + M whose matrix is ``thresh / 2`` everywhere, 0 in the lower-right M x N block and
``cost`` in the upper-left N x M block; the matches are the pairs (i < N, j < M) of its optimum. A pair costs ``c_ij``,
an unmatched row and an unmatched column together cost ``thresh``: it is the partial matching that minimises
``sum over matched (c_ij - thresh)``. ``lap`` is not a dependency here: :func:`assign` solves the same extended matrix
with ``scipy.optimize.linear_sum_assignment`` in fp64. Where the optimum is unique both give the same matches; the
order of rows and columns is then immaterial, and the pool is taken in slot order, not in the reference's list order.
``match_thresh`` is taken as its fp32 value (the kernel's parameters are fp32); 0.5 and 0.7 are the reference's literals.

Slots. A stream holds at most ``T`` live tracks (tracked, unconfirmed, lost). A birth takes the lowest free slot; with
none free it is skipped and ``overflow`` counts it. The reference's ``removed_stracks`` list only matters through
``sub_stracks(lost, removed)`` (byte_tracker.py:399): a slot flag ``wasrem`` says the same, because ids are never
reused; the clip of that list at 1000 entries (byte_tracker.py:402) is not reproduced.

Invalid detections (a non-finite box or score, ``w <= 0`` or ``h <= 0``) would give the reference NaN or inf; here they
are in neither tier and keep their row index.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
F64 = np.float64

# slot states: basetrack.py TrackState has New 0, Tracked 1, Lost 2, Removed 3; 0 here is a free slot (a New track is
# never stored: activate() makes it Tracked at once, byte_tracker.py:129)
FREE, TRACKED, LOST, REMOVED = 0, 1, 2, 3

DEFAULTS = dict(track_high_thresh=0.25, track_low_thresh=0.1, new_track_thresh=0.25, track_buffer=30,
                match_thresh=0.8, fuse_score=True, frame_rate=30)
SECOND_THRESH = 0.5       # byte_tracker.py:354
UNCONFIRMED_THRESH = 0.7  # byte_tracker.py:373
DUPLICATE_DIST = 0.15     # byte_tracker.py:465


def max_time_lost(frame_rate, track_buffer) -> int:
    return int(frame_rate / 30.0 * track_buffer)  # byte_tracker.py:289


def params_vector(track_high_thresh, track_low_thresh, new_track_thresh, match_thresh, track_buffer, frame_rate,
                  fuse_score) -> np.ndarray:
    """The kernel's host parameter vector, fp32 [8]: high, low, new, match, second (0.5), unconfirmed (0.7) thresholds,
    max_time_lost, fuse."""
    return np.array([track_high_thresh, track_low_thresh, new_track_thresh, match_thresh, SECOND_THRESH,
                     UNCONFIRMED_THRESH, max_time_lost(frame_rate, track_buffer), 1.0 if fuse_score else 0.0], dtype=F32)


# ---- boxes (fp32) ----------------------------------------------------------------------------------------------------
def det_boxes(rows: np.ndarray):
    """rows fp32 [n, 6] -> (xyxy for IoU, xyah measurement, valid), all from fp32 arithmetic.
    xywh: ops.py xyxy2xywh; tlwh: xywh2ltwh (byte_tracker.py:70); xyxy: STrack.xyxy on _tlwh (byte_tracker.py:197-199);
    xyah: tlwh_to_xyah (byte_tracker.py:204-207)."""
    r = np.ascontiguousarray(rows, dtype=F32)
    x1, y1, x2, y2 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    two = F32(2)
    cx = (x1 + x2) / two
    cy = (y1 + y2) / two
    w = x2 - x1
    h = y2 - y1
    with np.errstate(all="ignore"):
        left = cx - w / two
        top = cy - h / two
        xyxy = np.stack([left, top, left + w, top + h], axis=1).astype(F32)
        valid = np.isfinite(r[:, :5]).all(axis=1) & (w > 0) & (h > 0)
        hs = np.where(valid, h, F32(1))
        xyah = np.stack([left + w / two, top + h / two, w / hs, h], axis=1).astype(F32)
    return xyxy, xyah, valid


def track_boxes(mean: np.ndarray) -> np.ndarray:
    """fp64 means [n, 8] -> xyxy fp32 [n, 4]: STrack.tlwh and .xyxy (byte_tracker.py:189-199) in fp64, one cast."""
    m = np.asarray(mean, dtype=F64).reshape(-1, 8)
    w = m[:, 2] * m[:, 3]
    h = m[:, 3]
    left = m[:, 0] - w / 2.0
    top = m[:, 1] - h / 2.0
    return np.stack([left, top, w + left, h + top], axis=1).astype(F32)


def iou_cost(a: np.ndarray, b: np.ndarray, scores=None) -> np.ndarray:
    """1 - IoU of fp32 boxes a [n, 4] against b [m, 4], fp32 [n, m]: bbox_ioa(iou=True) (metrics.py:34-49) under
    iou_distance (matching.py:101); with ``scores`` (fp32 [m]) fuse_score (matching.py:153-157) on top."""
    a = np.ascontiguousarray(a, dtype=F32).reshape(-1, 4)
    b = np.ascontiguousarray(b, dtype=F32).reshape(-1, 4)
    zero = F32(0)
    iw = np.maximum(np.minimum(a[:, 2][:, None], b[:, 2]) - np.maximum(a[:, 0][:, None], b[:, 0]), zero)
    ih = np.maximum(np.minimum(a[:, 3][:, None], b[:, 3]) - np.maximum(a[:, 1][:, None], b[:, 1]), zero)
    inter = (iw * ih).astype(F32)
    area2 = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F32)
    area1 = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).astype(F32)
    area = ((area2[None, :] + area1[:, None]).astype(F32) - inter).astype(F32)
    iou = (inter / (area + F32(1e-7)).astype(F32)).astype(F32)
    cost = (F32(1) - iou).astype(F32)
    if scores is not None:
        sim = (F32(1) - cost).astype(F32)
        cost = (F32(1) - (sim * np.asarray(scores, dtype=F32)[None, :]).astype(F32)).astype(F32)
    return cost


# ---- assignment ------------------------------------------------------------------------------------------------------
def extended_matrix(cost: np.ndarray, thresh: float) -> np.ndarray:
    n, m = cost.shape
    e = np.full((n + m, n + m), float(thresh) / 2.0, dtype=F64)
    e[n:, m:] = 0.0
    e[:n, :m] = cost.astype(F64)
    return e


def assign(cost: np.ndarray, thresh: float):
    """The matches [(i, j)] of lapjv(extend_cost=True, cost_limit=thresh) (see the module docstring), rows ascending."""
    n, m = cost.shape
    if n == 0 or m == 0:  # matching.py:39
        return []
    from scipy.optimize import linear_sum_assignment
    r, c = linear_sum_assignment(extended_matrix(cost, thresh))
    return [(int(i), int(j)) for i, j in zip(r, c) if i < n and j < m]


def objective(cost: np.ndarray, thresh: float, matches) -> float:
    return float(sum(float(cost[i, j]) - float(thresh) for i, j in matches))


# ---- Kalman filter, XYAH (kalman_filter.py:65-236), fp64 -------------------------------------------------------------
STD_POS = 1.0 / 20   # kalman_filter.py:62
STD_VEL = 1.0 / 160  # kalman_filter.py:63
_MOTION = np.eye(8, dtype=F64)
for _i in range(4):
    _MOTION[_i, 4 + _i] = 1.0


def kf_initiate(xyah32: np.ndarray):
    """kalman_filter.py:82-97: the fp32 measurement promoted; std from fp32 products with fp32(0.1) and fp32(0.0625)
    (2 * (1 / 20) and 10 * (1 / 160) times an np.float32 scalar stay fp32 under NumPy 2), squared in fp64."""
    z = np.asarray(xyah32, dtype=F32)
    mean = np.zeros(8, dtype=F64)
    mean[:4] = z.astype(F64)
    p = F64(F32(2 * STD_POS) * z[3])
    v = F64(F32(10 * STD_VEL) * z[3])
    std = np.array([p, p, 1e-2, p, v, v, 1e-5, v], dtype=F64)
    return mean, np.diag(np.square(std))


def kf_predict(mean: np.ndarray, cov: np.ndarray):
    """kalman_filter.py:117-134 (multi_predict 183-204 is the same per track)."""
    h = mean[3]
    std = np.array([STD_POS * h, STD_POS * h, 1e-2, STD_POS * h, STD_VEL * h, STD_VEL * h, 1e-5, STD_VEL * h], dtype=F64)
    return np.dot(mean, _MOTION.T), np.linalg.multi_dot((_MOTION, cov, _MOTION.T)) + np.diag(np.square(std))


def kf_update(mean: np.ndarray, cov: np.ndarray, xyah32: np.ndarray):
    """kalman_filter.py:153-163 (project) and 226-236 (update)."""
    import scipy.linalg
    h = mean[3]
    std = np.array([STD_POS * h, STD_POS * h, 1e-1, STD_POS * h], dtype=F64)
    pmean = mean[:4].copy()
    pcov = cov[:4, :4] + np.diag(np.square(std))
    chol, lower = scipy.linalg.cho_factor(pcov, lower=True, check_finite=False)
    gain = scipy.linalg.cho_solve((chol, lower), cov[:, :4].T, check_finite=False).T
    innovation = np.asarray(xyah32, dtype=F32).astype(F64) - pmean
    return mean + np.dot(innovation, gain.T), cov - np.linalg.multi_dot((gain, pcov, gain.T))


# ---- the tracker -----------------------------------------------------------------------------------------------------
class StreamTracker:
    """One stream's tracker over ``T`` slots. ``update(rows, count)`` takes the padded NMS rows fp32 [D, 6]
    (x1, y1, x2, y2, conf, cls) and their count; the row index is the reference's ``idx``. Returns fp32 [n, 8] rows
    (x1, y1, x2, y2, track_id, score, cls, idx), one per activated tracked track, ascending ``track_id``.

    ``observer(kind, **facts)``, if given, is told every decision: ("assign", which=1|2|3, cost, thresh, matches) and
    ("duplicates", dist) - the decision margins are computed from these (tests/bytetrack_ref.py)."""

    def __init__(self, capacity=256, observer=None, **kw):
        unknown = set(kw) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"StreamTracker: unknown arguments {sorted(unknown)}")
        p = dict(DEFAULTS, **kw)
        self.T = int(capacity)
        self.high = F32(p["track_high_thresh"])
        self.low = F32(p["track_low_thresh"])
        self.new = F32(p["new_track_thresh"])
        self.match_thresh = float(F32(p["match_thresh"]))
        self.fuse = bool(p["fuse_score"])
        self.max_time_lost = max_time_lost(p["frame_rate"], p["track_buffer"])
        self.observer = observer
        self.reset()

    def reset(self):
        T = self.T
        self.state = np.zeros(T, dtype=np.int32)
        self.activated = np.zeros(T, dtype=bool)
        self.wasrem = np.zeros(T, dtype=bool)
        self.tid = np.zeros(T, dtype=np.int32)
        self.start = np.zeros(T, dtype=np.int32)
        self.last = np.zeros(T, dtype=np.int32)
        self.score = np.zeros(T, dtype=F32)
        self.cls = np.zeros(T, dtype=F32)
        self.idx = np.zeros(T, dtype=np.int32)
        self.mean = np.zeros((T, 8), dtype=F64)
        self.cov = np.zeros((T, 8, 8), dtype=F64)
        self.frame = 0
        self.next_id = 1   # basetrack.py next_id(): the first id is 1; per stream here (Q3)
        self.overflow = 0

    # the pieces a mutation test overrides -----------------------------------------------------------------------------
    def _assign(self, cost, thresh):
        return assign(cost, thresh)

    def _fuse_second(self):
        return False  # byte_tracker.py:353: iou_distance alone, no fuse_score

    def _predicted(self, pool, unconfirmed):
        return pool  # byte_tracker.py:331: the pool only, unconfirmed tracks are not predicted

    def _zero_vh(self, slot):
        return self.state[slot] != TRACKED  # byte_tracker.py:96-97

    def _expired_drop_now(self):
        return False  # byte_tracker.py:399 subtracts the removed list from before this frame (Q4)

    # the pieces another motion model replaces (utils/botsort.py): the filter, the boxes, the step before association
    _kf_initiate = staticmethod(kf_initiate)
    _kf_predict = staticmethod(kf_predict)
    _kf_update = staticmethod(kf_update)
    _track_boxes = staticmethod(track_boxes)
    _ZEROED = (7,)  # the velocities zeroed before a track that is not Tracked is predicted (byte_tracker.py:96-97)

    def _measurements(self, rows, xyah):
        return xyah  # fp32 [n, 4], what the filter is initiated and updated with

    def _motion(self, pool, unconfirmed):
        for i in self._predicted(pool, unconfirmed):  # byte_tracker.py:331
            if self._zero_vh(i):
                self.mean[i, list(self._ZEROED)] = 0.0
            self.mean[i], self.cov[i] = self._kf_predict(self.mean[i], self.cov[i])

    # ------------------------------------------------------------------------------------------------------------------
    def _tell(self, kind, **facts):
        if self.observer is not None:
            self.observer(kind, **facts)

    def _associate(self, which, slots, dets, dxyxy, dscore, thresh, fused):
        """One association of track ``slots`` with detection rows ``dets``: returns (matches [(slot, row)], unmatched
        slots, unmatched rows), both unmatched lists ascending."""
        slots = list(slots)
        dets = list(dets)
        if not slots or not dets:
            return [], slots, dets
        cost = iou_cost(self._track_boxes(self.mean[slots]), dxyxy[dets], dscore[dets] if fused else None)
        m = self._assign(cost, thresh)
        self._tell("assign", which=which, cost=cost, thresh=thresh, matches=m, slots=slots, dets=dets)
        ms = {i for i, _ in m}
        md = {j for _, j in m}
        return ([(slots[i], dets[j]) for i, j in m], [s for k, s in enumerate(slots) if k not in ms],
                [d for k, d in enumerate(dets) if k not in md])

    def _matched(self, slot, row, xyah, rows, f):
        """STrack.update / re_activate(new_id=False) (byte_tracker.py:137-149, 165-178): the same in slot terms."""
        self.mean[slot], self.cov[slot] = self._kf_update(self.mean[slot], self.cov[slot], xyah[row])
        self.state[slot] = TRACKED
        self.activated[slot] = True
        self.last[slot] = f
        self.score[slot] = rows[row, 4]
        self.cls[slot] = rows[row, 5]
        self.idx[slot] = row

    def update(self, rows, count=None) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=F32).reshape(-1, 6)
        n = rows.shape[0] if count is None else max(0, min(int(count), rows.shape[0]))
        rows = rows[:n]
        self.frame += 1  # byte_tracker.py:295
        f = self.frame
        dxyxy, xyah, valid = det_boxes(rows)
        xyah = self._measurements(rows, xyah)
        s = rows[:, 4]
        with np.errstate(invalid="ignore"):
            high = valid & (s >= self.high)                     # byte_tracker.py:307
            second = valid & (s > self.low) & (s < self.high)   # byte_tracker.py:308-311
        d_high = [int(i) for i in np.flatnonzero(high)]
        d_second = [int(i) for i in np.flatnonzero(second)]

        # byte_tracker.py:321-329: unconfirmed apart; the pool is the activated tracked tracks plus the lost list
        st0 = self.state.copy()
        unconfirmed = [int(i) for i in np.flatnonzero((st0 == TRACKED) & ~self.activated)]
        pool = [int(i) for i in np.flatnonzero(((st0 == TRACKED) & self.activated) | (st0 == LOST) | (st0 == REMOVED))]
        old_lost = [i for i in pool if st0[i] != TRACKED]
        self._motion(pool, unconfirmed)

        # first association (byte_tracker.py:337-348)
        m1, u_track, u_det = self._associate(1, pool, d_high, dxyxy, s, self.match_thresh, self.fuse)
        for slot, row in m1:
            self._matched(slot, row, xyah, rows, f)
        # second association (byte_tracker.py:350-369): only tracks whose state is Tracked, not fused
        r_tracked = [i for i in u_track if st0[i] == TRACKED]
        m2, u_track2, _ = self._associate(2, r_tracked, d_second, dxyxy, s, SECOND_THRESH, self._fuse_second())
        for slot, row in m2:
            self._matched(slot, row, xyah, rows, f)
        new_lost = []
        for slot in u_track2:
            self.state[slot] = LOST  # mark_lost
            new_lost.append(slot)
        # unconfirmed tracks (byte_tracker.py:371-380)
        m3, u_unconfirmed, u_det = self._associate(3, unconfirmed, u_det, dxyxy, s, UNCONFIRMED_THRESH, self.fuse)
        for slot, row in m3:
            self._matched(slot, row, xyah, rows, f)
        for slot in u_unconfirmed:
            self.state[slot] = FREE  # mark_removed; byte_tracker.py:394 drops it from the tracked list
        # births (byte_tracker.py:382-387), ascending row index
        for row in u_det:
            if s[row] < self.new:
                continue
            free = np.flatnonzero(self.state == FREE)
            if free.size == 0:
                self.overflow += 1
                continue
            slot = int(free[0])
            self.mean[slot], self.cov[slot] = self._kf_initiate(xyah[row])
            self.state[slot] = TRACKED
            self.activated[slot] = f == 1  # byte_tracker.py:130-131
            self.wasrem[slot] = False
            self.tid[slot] = self.next_id
            self.next_id += 1
            self.start[slot] = self.last[slot] = f
            self.score[slot] = rows[row, 4]
            self.cls[slot] = rows[row, 5]
            self.idx[slot] = row
        # expiry (byte_tracker.py:389-399): marked now, subtracted against the removed list from before this frame
        pending = []
        for slot in old_lost:
            if self.state[slot] in (LOST, REMOVED) and f - self.last[slot] > self.max_time_lost:
                self.state[slot] = REMOVED
                pending.append(slot)
        for slot in [i for i in old_lost if self.state[i] in (LOST, REMOVED)] + new_lost:
            if self.wasrem[slot] or (self._expired_drop_now() and slot in pending):
                self.state[slot] = FREE
        for slot in pending:
            self.wasrem[slot] = True  # byte_tracker.py:401
        # duplicates (byte_tracker.py:400, 464-476)
        a = [int(i) for i in np.flatnonzero(self.state == TRACKED)]
        b = [int(i) for i in np.flatnonzero((self.state == LOST) | (self.state == REMOVED))]
        if a and b:
            dist = iou_cost(self._track_boxes(self.mean[a]), self._track_boxes(self.mean[b]))
            self._tell("duplicates", dist=dist, a=a, b=b)
            for p, q in zip(*np.where(dist < F32(DUPLICATE_DIST))):
                sa, sb = a[p], b[q]
                if self.last[sa] - self.start[sa] > self.last[sb] - self.start[sb]:
                    self.state[sb] = FREE
                else:
                    self.state[sa] = FREE
        return self.rows()

    def rows(self) -> np.ndarray:
        """byte_tracker.py:405 and STrack.result (228), ascending track_id."""
        live = [int(i) for i in np.flatnonzero((self.state == TRACKED) & self.activated)]
        live.sort(key=lambda i: int(self.tid[i]))
        out = np.zeros((len(live), 8), dtype=F32)
        if live:
            out[:, :4] = self._track_boxes(self.mean[live])
            out[:, 4] = self.tid[live].astype(F32)
            out[:, 5] = self.score[live]
            out[:, 6] = self.cls[live]
            out[:, 7] = self.idx[live].astype(F32)
        return out

    def snapshot(self) -> dict:
        """The per-slot state in the layout of the kernel's debug fetch (free slots hold whatever they held)."""
        flags = self.activated.astype(np.int32) | (self.wasrem.astype(np.int32) << 1)
        return dict(state=self.state.copy(), flags=flags, tid=self.tid.copy(), start=self.start.copy(),
                    last=self.last.copy(), score=self.score.copy(), cls=self.cls.copy(), idx=self.idx.copy(),
                    mean=self.mean.copy(), cov=self.cov.copy(), frame=self.frame, next_id=self.next_id,
                    overflow=self.overflow)
