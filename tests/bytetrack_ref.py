"""ByteTrack test helper: the restatement, its decision margins, the scenes.

The numpy restatement of the reference's ``BYTETracker.update`` is ``yolosod_amd.utils.bytetrack`` (written from
``byte_tracker.py:293-405``, ``basetrack.py``, ``kalman_filter.py:65-236``, ``matching.py:20-157``, ``metrics.py:20-49``
and ``ops.py``; its module docstring cites the lines and states the ``lapjv(extend_cost=True, cost_limit=thresh)`` ==
``linear_sum_assignment`` on the extended matrix equivalence). It is the steps' one implementation: the product's host
path runs it and the HIP kernel is held to it. This file re-exports it and adds what only tests need:

* decision margins, in the style of ``nms_margins.py``: for every assignment the objective gap to the best solution
  with each matched pair forbidden and with each unmatched pair of cost ``< thresh + 0.2`` forced (one re-solve each,
  inside the pair's connected component of the graph of pairs with cost ``< thresh + 0.2``: pairs at or above
  ``thresh`` are never in an optimum, so the optimum splits over these components); for every duplicate test
  ``|d - 0.15|``. Off by default: they dominate the run time.
* ``delta``: the change of a cost when the four fp32 coordinates of a track box each flip by one ulp,
  ``4 * ulp32(max |coord|) / min box side`` - the only way a track box can differ between two fp64 implementations.
  A scene is certified when every margin of every frame is at least ``32 * delta`` (32 covers matchings that differ in
  many rows).
* brute force over all partial matchings, for the assignment test.
* the directed scenes (one per trait Q0..Q6, capacity, invalid rows, empty frames) and the seeded random scenes.
"""
from __future__ import annotations

import numpy as np

from yolosod_amd.utils import bytetrack as bt
from yolosod_amd.utils.bytetrack import (FREE, LOST, REMOVED, TRACKED, StreamTracker, assign, extended_matrix,  # noqa: F401
                                         iou_cost, kf_initiate, kf_predict, kf_update, objective, track_boxes)

F32 = np.float32
MARGIN_BAND = 0.2
CERT_FACTOR = 32.0


# ---- brute force -----------------------------------------------------------------------------------------------------
def brute_force(cost: np.ndarray, thresh: float):
    """(best objective, its matches) of sum over matched (c_ij - thresh) over all partial matchings."""
    n, m = cost.shape
    best, arg = 0.0, []

    def rec(i, usedc, acc, cur):
        nonlocal best, arg
        if i == n:
            if acc < best:
                best, arg = acc, list(cur)
            return
        rec(i + 1, usedc, acc, cur)
        for j in range(m):
            if not usedc & (1 << j):
                cur.append((i, j))
                rec(i + 1, usedc | (1 << j), acc + float(cost[i, j]) - float(thresh), cur)
                cur.pop()

    rec(0, 0, 0.0, [])
    return best, arg


def greedy_assign(cost: np.ndarray, thresh: float):
    """A plausible wrong kernel: repeatedly take the cheapest remaining pair below thresh."""
    c = cost.astype(np.float64).copy()
    out = []
    while c.size and np.nanmin(c) < thresh:
        i, j = np.unravel_index(np.nanargmin(c), c.shape)
        out.append((int(i), int(j)))
        c[i, :] = np.inf
        c[:, j] = np.inf
    return sorted(out)


# ---- margins ---------------------------------------------------------------------------------------------------------
def assignment_margin(cost: np.ndarray, thresh: float, matches) -> float:
    """The smallest objective gap between the optimum and the best solution that differs in one forced decision."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n, m = cost.shape
    if n == 0 or m == 0:
        return np.inf
    near = cost < F32(thresh + MARGIN_BAND)
    ii, jj = np.nonzero(near)
    if ii.size == 0:
        return np.inf
    g = coo_matrix((np.ones(ii.size), (ii, jj + n)), shape=(n + m, n + m))
    _, lab = connected_components(g, directed=False)
    matched = set(matches)
    worst = np.inf
    for comp in np.unique(lab[ii]):
        rows = np.flatnonzero(lab[:n] == comp)
        cols = np.flatnonzero(lab[n:] == comp)
        sub = cost[np.ix_(rows, cols)]
        base = objective(sub, thresh, assign(sub, thresh))
        for a, r in enumerate(rows):
            for b, c in enumerate(cols):
                if not near[r, c]:
                    continue
                if (int(r), int(c)) in matched:  # forbidden
                    alt = sub.copy()
                    alt[a, b] = F32(thresh + 1.0)
                    gap = objective(alt, thresh, assign(alt, thresh)) - base
                else:  # forced
                    rest = np.delete(np.delete(sub, a, axis=0), b, axis=1)
                    gap = float(sub[a, b]) - float(thresh) + objective(rest, thresh, assign(rest, thresh)) - base
                worst = min(worst, gap)
    return worst


class Margins:
    """An observer for ``StreamTracker``: collects the smallest margin of every frame."""

    def __init__(self):
        self.frame_min = []
        self._cur = np.inf

    def __call__(self, kind, **f):
        if kind == "assign":
            self._cur = min(self._cur, assignment_margin(f["cost"], f["thresh"], f["matches"]))
        elif kind == "duplicates":
            self._cur = min(self._cur, float(np.abs(f["dist"].astype(np.float64) - bt.DUPLICATE_DIST).min()))

    def end_frame(self):
        self.frame_min.append(self._cur)
        self._cur = np.inf


def delta(frames) -> float:
    """4 * ulp32(max |coord|) / min box side over a scene's valid detections."""
    mx, side = 0.0, np.inf
    for rows, n in frames:
        r = rows[:n]
        ok = np.isfinite(r[:, :4]).all(axis=1) & (r[:, 2] > r[:, 0]) & (r[:, 3] > r[:, 1])
        r = r[ok]
        if len(r):
            mx = max(mx, float(np.abs(r[:, :4]).max()))
            side = min(side, float((r[:, 2] - r[:, 0]).min()), float((r[:, 3] - r[:, 1]).min()))
    return 4.0 * float(np.spacing(F32(mx))) / side if np.isfinite(side) else 0.0


# ---- running a scene -------------------------------------------------------------------------------------------------
def run_scene(frames, capacity=64, margins=False, cls=StreamTracker, **kw):
    """Every frame's (rows, snapshot) of a scene = [(padded rows fp32 [D, 6], count)], and the per-frame margins."""
    obs = Margins() if margins else None
    t = cls(capacity=capacity, observer=obs, **kw)
    res = []
    for rows, n in frames:
        out = t.update(rows, n)
        res.append((out, t.snapshot()))
        if obs:
            obs.end_frame()
    return res, (obs.frame_min if obs else None)


def summary(res):
    """Per frame (ids, idx, states of the slots that were ever used) - what the directed tests assert."""
    return [([int(v) for v in out[:, 4]], [int(v) for v in out[:, 7]], [int(s) for s in snap["state"]])
            for out, snap in res]


# ---- scenes ----------------------------------------------------------------------------------------------------------
def pad(dets, D=16):
    """[(x1, y1, x2, y2, conf, cls)] -> (fp32 [D, 6], count)."""
    rows = np.zeros((D, 6), dtype=F32)
    for i, d in enumerate(dets):
        rows[i] = np.asarray(d, dtype=F32)
    return rows, len(dets)


def box(x, y=100.0, s=0.9, c=0.0, w=40.0, h=60.0):
    return (x, y, x + w, y + h, s, c)


def random_scene(seed, objects, frames, width, height, min_side, max_side=None, D=300, p_miss=0.08, p_low=0.12,
                 p_false=0.02, crowd=False, stay=0.85):
    """A seeded scene: objects on straight paths with jitter, per frame and object a miss, a second-tier score or a
    high score, a few false alarms, rows in random order. ``crowd``: the objects start on a tight grid (overlapping
    neighbours: real augmenting paths). ``stay``: the share of objects present from the first / to the last frame."""
    rng = np.random.default_rng(seed)
    max_side = max_side or (1.5 if crowd else 3.0) * min_side
    w = rng.uniform(min_side, max_side, objects)
    h = rng.uniform(min_side, max_side, objects)
    if crowd:
        k = int(np.ceil(np.sqrt(objects)))
        gx, gy = np.meshgrid(np.arange(k), np.arange(k))
        pitch = 0.5 * min_side
        x = (width / 2 - k * pitch / 2 + gx.ravel()[:objects] * pitch).astype(np.float64)
        y = (height / 2 - k * pitch / 2 + gy.ravel()[:objects] * pitch).astype(np.float64)
    else:
        x = rng.uniform(0, width - max_side, objects)
        y = rng.uniform(0, height - max_side, objects)
    vmax = 0.5 if crowd else 3.0
    vx = rng.uniform(-vmax, vmax, objects)
    vy = rng.uniform(-vmax, vmax, objects)
    cls = rng.integers(0, 10, objects).astype(np.float64)
    born = np.where(rng.random(objects) < stay, 0, rng.integers(1, max(2, frames), objects))
    dies = np.where(rng.random(objects) < stay, frames, rng.integers(1, max(2, frames), objects))
    out = []
    for f in range(frames):
        dets = []
        for o in range(objects):
            if not born[o] <= f < dies[o]:
                continue
            u = rng.random()
            if u < p_miss:
                continue
            s = rng.uniform(0.11, 0.24) if u < p_miss + p_low else rng.uniform(0.3, 0.95)
            j = rng.normal(0, 0.02 * min_side, 4)
            x1 = float(np.clip(x[o] + j[0], 0, width - min_side))
            y1 = float(np.clip(y[o] + j[1], 0, height - min_side))
            dets.append((x1, y1, x1 + max(w[o] + j[2], min_side), y1 + max(h[o] + j[3], min_side), s, cls[o]))
        for _ in range(rng.poisson(p_false * objects)):
            fw, fh = rng.uniform(min_side, max_side, 2)
            x1, y1 = rng.uniform(0, width - max_side), rng.uniform(0, height - max_side)
            dets.append((x1, y1, x1 + fw, y1 + fh, rng.uniform(0.26, 0.6), float(rng.integers(0, 10))))
        order = rng.permutation(len(dets))[:D]
        out.append(pad([dets[i] for i in order], D))
        x += vx + rng.normal(0, 0.3, objects)
        y += vy + rng.normal(0, 0.3, objects)
    return out


# The certified random scenes the GPU test runs: name -> (scene arguments, tracker arguments). The seeds were chosen so
# that every frame certifies (test_bytetrack_cpu.py asserts it, no frame exempt).
RANDOM_SCENES = {
    "small64": (dict(seed=7, objects=64, frames=40, width=400, height=300, min_side=16, D=64, stay=0.6, p_false=0.05),
                dict(capacity=64)),
    "mid150": (dict(seed=3, objects=150, frames=25, width=1920, height=1080, min_side=16, D=300), dict(capacity=256)),
    "crowd80": (dict(seed=2, objects=80, frames=25, width=1920, height=1080, min_side=24, D=300, crowd=True),
                dict(capacity=256)),
    "big280": (dict(seed=5, objects=280, frames=6, width=2000, height=2000, min_side=24, D=300), dict(capacity=320)),
}


def directed_scenes():
    """name -> (frames, tracker arguments). One scene per trait; the expectations are in test_bytetrack_cpu.py."""
    A, B, C, P = 100.0, 300.0, 500.0, 700.0
    sc = {}
    # Q0: births at frame 1 are activated at once; a later birth is unconfirmed for one frame, not output, and removed
    # if it does not match in the third association (the one-frame false alarm at frame 3); D (from frame 5) is kept
    sc["q0_false_alarm"] = ([pad([box(A), box(B, s=0.8)]), pad([box(A), box(B, s=0.8)]),
                             pad([box(A), box(B, s=0.8), box(C, s=0.7)]), pad([box(A), box(B, s=0.8)]),
                             pad([box(A), box(B, s=0.8), box(P, s=0.7)]), pad([box(A), box(B, s=0.8), box(P, s=0.7)])], {})
    # Q1: A is missed at frames 4 and 5 and found again, with its id, at frame 6
    sc["q1_refind"] = ([pad([box(A), box(B)])] * 3 + [pad([box(B)])] * 2 + [pad([box(B), box(A)])], {})
    # Q2: A continues on a second-tier score at frame 3; B is missed at frame 3 (lost) and a second-tier detection at
    # frame 4 must not bring it back (lost tracks are not in the second association); a high one at frame 5 does
    sc["q2_low_score"] = ([pad([box(A), box(B)])] * 2 + [pad([box(A, s=0.15)]), pad([box(A), box(B, s=0.15)]),
                                                         pad([box(A), box(B)])], {})
    # Q3: ids in ascending row index; the 0.4 row is in the high tier but below new_track_thresh, the 0.2 row is not in
    # the high tier
    q3 = pad([box(C), box(A, s=0.4), box(B, s=0.7), box(P, s=0.2)])
    sc["q3_id_order"] = ([q3, q3], dict(new_track_thresh=0.6))
    # Q4 / Q5, track_buffer 2: A is last seen at frame 2, Lost at 3 and 4, marked Removed at 5 (5 - 2 > 2) but kept,
    # re-found with its id at frame 6; missed at 7 it disappears at once (its id is in the removed set); a new id at 8
    sc["q4_q5_resurrect"] = ([pad([box(A), box(B)])] * 2 + [pad([box(B)])] * 3 + [pad([box(B), box(A)]), pad([box(B)]),
                                                                                pad([box(B), box(A)]),
                                                                                pad([box(B), box(A)])],
                             dict(track_buffer=2))
    # Q4 without the return: the Removed track is dropped at frame 6
    sc["q4_expire"] = ([pad([box(A), box(B)])] * 2 + [pad([box(B)])] * 5, dict(track_buffer=2))
    # Q6, lost side older: with match_thresh 0.5 a 0.4 detection on top of the lost A (fused similarity 0.4) matches
    # nothing and is born as a duplicate; A has lived 2 frames, the newcomer 0: the tracked newcomer is dropped
    sc["q6_lost_survives"] = ([pad([box(A)])] * 3 + [pad([]), pad([box(A, s=0.4)]), pad([box(A)])],
                              dict(match_thresh=0.5))
    # Q6, tie: A lived 0 frames (born at 1, lost at 2), the newcomer 0: the tracked one is dropped
    sc["q6_tie"] = ([pad([box(A)]), pad([]), pad([box(A, s=0.4)]), pad([box(A)])], dict(match_thresh=0.5))
    # Q6, tracked side older: C is born at frame 1 and lost from frame 2 (lived 0 frames); A walks 8 px a frame towards
    # it and stops 2 px off (IoU 38 / 42 = 0.905 > 0.85); A keeps its detection (cheaper), C is the duplicate that goes
    xs = [A + 8.0 * min(f, 10) for f in range(13)]  # stops at A + 80
    sc["q6_tracked_survives"] = ([pad([box(xs[0]), box(A + 82.0)])] + [pad([box(x)]) for x in xs[1:]], {})
    # mean[7] = 0 for lost tracks (byte_tracker.py:96-97): A shrinks by 20 px a frame around a fixed centre (constant
    # aspect) for frames 1..5, is missed for frames 6..11 and comes back at frame 12 as it was at frame 5. With the
    # height velocity zeroed its predicted box keeps its size and it is found again; seven predictions at the learnt
    # velocity would shrink it to nothing
    def sized(hh, s=0.9):
        return (200.0 - hh / 4, 300.0 - hh / 2, 200.0 + hh / 4, 300.0 + hh / 2, s, 0.0)
    sc["q1_height_velocity"] = ([pad([sized(200.0 - 20.0 * f), box(P)]) for f in range(5)] + [pad([box(P)])] * 6
                                + [pad([sized(120.0), box(P)])], {})
    # exact assignment: tracks at 100 and 124, detections at 110 (row 0) and 84 (row 1). IoU (A, row 0) = 30 / 50 is
    # the largest, then (B, row 0) = 26 / 54 and (A, row 1) = 24 / 56; (B, row 1) do not overlap. Taking the best pair
    # first strands B; the optimum matches both: A -> row 1, B -> row 0
    sc["assign_swap"] = ([pad([box(A), box(A + 24.0)]), pad([box(A + 10.0), box(A - 16.0)])], {})
    # capacity: 70 objects on a grid for 64 slots: rows 64..69 overflow, every frame
    crowd = [box(20.0 + 60.0 * (i % 10), 20.0 + 80.0 * (i // 10)) for i in range(70)]
    sc["capacity_overflow"] = ([pad(crowd, 80)] * 3, {})
    # invalid rows are ignored and keep their index
    nan = float("nan")
    bad = [box(A), (nan, 100.0, 340.0, 160.0, 0.9, 0.0), box(B), box(C, s=nan), (500.0, 100.0, 540.0, 100.0, 0.9, 0.0),
           (740.0, 100.0, 700.0, 160.0, 0.9, 0.0), box(P, c=3.0)]
    sc["invalid_rows"] = ([pad(bad)] * 3, {})
    # an empty frame loses both tracks for a frame
    sc["empty_frame"] = ([pad([box(A), box(B)]), pad([]), pad([box(A), box(B)])], {})
    sc["empty_stream"] = ([pad([])] * 5, {})
    return sc
