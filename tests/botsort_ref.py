"""BoT-SORT test helper: the restatement with scripted warps, the scenes with camera motion.

The numpy restatement is ``yolosod_amd.utils.botsort`` (``BotSortStreamTracker``: ``bytetrack.StreamTracker`` with the
XYWH filter and the camera-motion warp; its module docstring cites the reference's lines). The margins, ``delta``, the
certification rule and ``run_scene`` are ``bytetrack_ref``'s, unchanged: a scene here is the same list of
(padded rows, count) plus one warp (fp64 [2, 3] or None) per frame, and :class:`Scripted` feeds the warps to
``update`` so that ``run_scene`` can drive it.

* the directed scenes, one per BoT-SORT trait (B1, the model, B3 on the pool / on unconfirmed tracks / zoom and
  rotation, identity warps, a NaN warp); the expectations are in test_botsort_cpu.py.
* the seeded random scenes with camera motion: ``bytetrack_ref.random_scene`` in world coordinates, seen through a
  camera whose frame-to-frame motion is a seeded random walk (translation up to +-12 px, rotation up to 0.5 degrees,
  scale 1 +- 0.01, about the frame centre); the detections are moved by the accumulated camera and the tracker is
  given the frame-to-frame warps.
"""
from __future__ import annotations

import numpy as np

from bytetrack_ref import Margins, box, delta, pad, random_scene, run_scene, summary  # noqa: F401
from yolosod_amd.utils import botsort as bs
from yolosod_amd.utils.botsort import (BotSortStreamTracker, gmc_apply, kf_initiate_xywh, kf_predict_xywh,  # noqa: F401
                                       kf_update_xywh, track_boxes_xywh)

F32 = np.float32
F64 = np.float64
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=F64)


class Scripted(BotSortStreamTracker):
    """BotSortStreamTracker that takes its warps as a per-frame list at construction (``warps[f]`` is the warp of the
    f-th update, None for none), so that ``bytetrack_ref.run_scene`` drives it."""

    def __init__(self, capacity=64, observer=None, warps=None, **kw):
        self.script = None if warps is None else list(warps)
        super().__init__(capacity=capacity, observer=observer, **kw)

    def update(self, rows, count=None, warp=None):
        if warp is None and self.script is not None:
            warp = self.script[self.frame]
        return super().update(rows, count, warp)


def run(frames, warps=None, capacity=64, margins=False, cls=Scripted, **kw):
    """``bytetrack_ref.run_scene`` with the scene's warps."""
    return run_scene(frames, capacity=capacity, margins=margins, cls=cls, warps=warps, **kw)


# ---- warps -------------------------------------------------------------------------------------------------------------
def similarity(tx=0.0, ty=0.0, angle_deg=0.0, scale=1.0, centre=(0.0, 0.0)) -> np.ndarray:
    """The 2x3 matrix of p -> scale * Rot(angle) (p - centre) + centre + (tx, ty), fp64."""
    a = np.deg2rad(angle_deg)
    R = scale * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], dtype=F64)
    c = np.asarray(centre, dtype=F64)
    return np.concatenate([R, (c - R @ c + np.array([tx, ty], dtype=F64))[:, None]], axis=1)


def compose(H2, H1) -> np.ndarray:
    """H2 after H1."""
    return np.concatenate([H2[:, :2] @ H1[:, :2], (H2[:, :2] @ H1[:, 2] + H2[:, 2])[:, None]], axis=1)


def move_rows(rows, n, A):
    """The padded rows seen through the camera ``A`` (world -> frame pixels): centres mapped by A, sides scaled by its
    scale (the boxes stay axis aligned, as a detector's are)."""
    out = rows.copy()
    r = rows[:n].astype(F64)
    s = np.sqrt(abs(np.linalg.det(A[:, :2])))
    c = np.stack([(r[:, 0] + r[:, 2]) / 2, (r[:, 1] + r[:, 3]) / 2], axis=1) @ A[:, :2].T + A[:, 2]
    w, h = (r[:, 2] - r[:, 0]) * s, (r[:, 3] - r[:, 1]) * s
    out[:n, :4] = np.stack([c[:, 0] - w / 2, c[:, 1] - h / 2, c[:, 0] + w / 2, c[:, 1] + h / 2], axis=1).astype(F32)
    return out


def camera_scene(seed, cam_seed=None, **kw):
    """(frames, warps): ``random_scene(seed, ...)`` seen through a camera on a seeded random walk. ``warps[0]`` is
    None (there is no previous frame); ``warps[f]`` maps frame f - 1's pixels to frame f's."""
    world = random_scene(seed=seed, **kw)
    rng = np.random.default_rng(1000 + seed if cam_seed is None else cam_seed)
    centre = (kw["width"] / 2.0, kw["height"] / 2.0)
    A = IDENTITY.copy()
    frames, warps = [], []
    for f, (rows, n) in enumerate(world):
        if f == 0:
            warps.append(None)
        else:
            H = similarity(rng.uniform(-12, 12), rng.uniform(-12, 12), rng.uniform(-0.5, 0.5), rng.uniform(0.99, 1.01),
                           centre)
            A = compose(H, A)
            warps.append(H)
        frames.append((move_rows(rows, n, A), n))
    return frames, warps


# The certified random scenes the GPU test runs: name -> (scene arguments, tracker arguments): bytetrack_ref's four
# sizes seen through a moving camera. The seeds were chosen so that every frame certifies (test_botsort_cpu.py asserts
# it, no frame exempt).
RANDOM_SCENES = {
    "small64": (dict(seed=7, objects=64, frames=40, width=400, height=300, min_side=16, D=64, stay=0.6, p_false=0.05),
                dict(capacity=64)),
    "mid150": (dict(seed=3, objects=150, frames=25, width=1920, height=1080, min_side=16, D=300), dict(capacity=256)),
    "crowd80": (dict(seed=6, objects=80, frames=25, width=1920, height=1080, min_side=24, D=300, crowd=True),
                dict(capacity=256)),
    "big280": (dict(seed=5, objects=280, frames=6, width=2000, height=2000, min_side=24, D=300), dict(capacity=320)),
}


# ---- directed scenes -----------------------------------------------------------------------------------------------------
def shifted(dets, dx, dy=0.0):
    return [(d[0] + dx, d[1] + dy, d[2] + dx, d[3] + dy, d[4], d[5]) for d in dets]


def directed_scenes():
    """name -> (frames, warps or None, tracker arguments). D 16, T 64."""
    A, B, C, P = 100.0, 300.0, 500.0, 700.0
    sc = {}

    # B1 (bot_sort.py:126-129): A shrinks by 10 px of width and 20 px of height a frame around a fixed centre for
    # frames 1..5, is missed for frames 6..11 and comes back at frame 12 as it was at frame 5. With both size
    # velocities zeroed its predicted box keeps its size and it is found again; with only mean[7] zeroed seven
    # predictions at the learnt width velocity shrink its width to nothing
    def sized(hh, s=0.9):
        return (200.0 - hh / 4, 300.0 - hh / 2, 200.0 + hh / 4, 300.0 + hh / 2, s, 0.0)
    sc["b1_size_velocity"] = ([pad([sized(200.0 - 20.0 * f), box(P)]) for f in range(5)] + [pad([box(P)])] * 6
                              + [pad([sized(120.0), box(P)])], None, {})

    # the model: A's width grows by 12 px a frame at a constant height (match_thresh 0.5). XYWH learns the width's
    # velocity and follows; XYAH's aspect ratio has a fixed, tiny noise (1e-2) and lags until the fused IoU drops under
    # the threshold: ByteTrack loses A and starts a new id, BoT-SORT keeps id 1
    def wide(f, s=0.9):
        w = 40.0 + 12.0 * f
        return (300.0 - w / 2, 100.0, 300.0 + w / 2, 160.0, s, 0.0)
    sc["model_width_growth"] = ([pad([wide(f)]) for f in range(10)], None, dict(match_thresh=0.5))

    # B3, the pool: the camera pans from frame 3 on, every detection moves 40 px a frame (a box is 40 px wide: no
    # overlap with where it was). With the warps the ids persist; without them both tracks are lost at frame 3 and
    # every later birth dies unconfirmed
    base = [box(A), box(B, s=0.8)]
    pan = [0, 0, 1, 2, 3, 4]
    sc["b3_pan"] = ([pad(shifted(base, 40.0 * k)) for k in pan],
                    [None, IDENTITY, similarity(40.0), similarity(40.0), similarity(40.0), similarity(40.0)], {})
    sc["b3_pan_no_warps"] = (sc["b3_pan"][0], None, {})

    # B3, unconfirmed: C is born at frame 2 (unconfirmed: not output), the pan is at frame 3. C is confirmed at frame 3
    # only if it was warped too (it is not in the pool and was not predicted)
    sc["b3_unconfirmed"] = ([pad([box(A)]), pad([box(A), box(C, s=0.7)]), pad(shifted([box(A), box(C, s=0.7)], 40.0)),
                             pad(shifted([box(A), box(C, s=0.7)], 40.0))],
                            [None, None, similarity(40.0), IDENTITY], {})

    # B3, zoom and a small rotation about the frame centre (400, 300) at frame 3: scale 1.25, 2 degrees. The boxes far
    # from the centre move by more than their size; R also scales (w, h)
    Z = similarity(0.0, 0.0, 2.0, 1.25, (400.0, 300.0))
    world = [box(A), box(P, 500.0, s=0.8), box(380.0, 270.0, s=0.7)]
    zoomed = move_rows(*pad(world), Z)
    sc["b3_zoom_rotation"] = ([pad(world)] * 2 + [(zoomed, 3)] * 3, [None, None, Z, IDENTITY, None], {})

    # warps=None against identity warps on a scene with a lost, a re-found and an unconfirmed track
    q = [pad([box(A), box(B)])] * 3 + [pad([box(B), box(C, s=0.7)])] * 2 + [pad([box(B), box(A), box(C, s=0.7)])]
    sc["identity_none"] = (q, None, {})
    sc["identity_warps"] = (q, [IDENTITY] * len(q), {})

    # rule of ours: the pan scene with a NaN in frame 3's warp. The warp is skipped and counted: frame 3 goes as
    # without a warp (both tracks lost, two unconfirmed births), and from frame 4 on the births are warped and live
    nanw = similarity(40.0)
    nanw[1, 2] = np.nan
    sc["bad_warp"] = (sc["b3_pan"][0], [None, IDENTITY, nanw, similarity(40.0), similarity(40.0), similarity(40.0)], {})
    return sc
