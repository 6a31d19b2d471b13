"""BoT-SORT, one stream at a time, in numpy: ``utils.bytetrack.StreamTracker`` with the reference's two differences
(``ultralytics/trackers/bot_sort.py``: ``BOTSORT(BYTETracker)``), on the same track slots. It is the one host
implementation: ``engine.tracker.BotSortTrackerHost`` runs it, ``tests/botsort_ref.py`` adds scenes with camera motion,
and the XYWH instantiation of the HIP kernel (csrc/track.hip) is held to it.

Written from reading ``bot_sort.py`` (BOTrack: predict / multi_predict 89-133, tlwh 110-117, tlwh_to_xywh 140-144;
BOTSORT: get_kalmanfilter 197-199, get_dists 211-224), ``byte_tracker.py:103-120`` (STrack.multi_gmc) and ``:293-405``
(update, where the warp is applied at 332-335) and ``utils/kalman_filter.py:289-491`` (KalmanFilterXYWH). In this
reference ReID is a stub (``bot_sort.py:192-194``: the encoder is always None), so ``get_dists`` is ``iou_distance``
plus ``fuse_score``: ByteTrack's costs. Every dtype is spelled out, as in ``utils/bytetrack.py``.

The differences from ByteTrack's Q-list:

B1  a pool track whose state is not Tracked has ``mean[6]`` and ``mean[7]`` zeroed before it is predicted.
B2  the state is (cx, cy, w, h) and its velocities; the track box is ``(cx - w/2, cy - h/2, w + left, h + top)`` in fp64
    (STrack.xyxy on BOTrack.tlwh), cast to fp32 once; the measurement is the fp32 ``(l + w/2, t + h/2, w, h)``.
B3  after the pool's prediction and before the first association a 2x3 camera-motion matrix, if one is given, is
    applied to every pool track and to every unconfirmed track (which were not predicted).
B4  costs as in ByteTrack (fused in the first and third association, plain IoU in the second).

The warp is an input here (the reference estimates it with OpenCV, ``utils/gmc.py``; ``update(results, img=None)``
skips it, and so does ``warp=None``). Rule of ours: a warp with a non-finite entry is treated as absent and counted in
``bad_warp``; a finite warp is applied as given, however degenerate.
"""
from __future__ import annotations

import numpy as np

from . import bytetrack as bt
from .bytetrack import F32, F64, STD_POS, STD_VEL, _MOTION


# ---- boxes -----------------------------------------------------------------------------------------------------------
def det_xywh(rows: np.ndarray) -> np.ndarray:
    """rows fp32 [n, 6] -> the fp32 measurement (l + w/2, t + h/2, w, h) of the same tlwh ``bytetrack.det_boxes`` uses
    (xyxy2xywh, xywh2ltwh, then BOTrack.tlwh_to_xywh, bot_sort.py:140-144), one rounding per operation."""
    r = np.ascontiguousarray(rows, dtype=F32).reshape(-1, 6)
    x1, y1, x2, y2 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    two = F32(2)
    with np.errstate(all="ignore"):
        cx = (x1 + x2) / two
        cy = (y1 + y2) / two
        w = x2 - x1
        h = y2 - y1
        left = cx - w / two
        top = cy - h / two
        return np.stack([left + w / two, top + h / two, w, h], axis=1).astype(F32)


def track_boxes_xywh(mean: np.ndarray) -> np.ndarray:
    """fp64 means [n, 8] -> xyxy fp32 [n, 4]: BOTrack.tlwh (bot_sort.py:110-117) and STrack.xyxy in fp64, one cast."""
    m = np.asarray(mean, dtype=F64).reshape(-1, 8)
    w = m[:, 2]
    h = m[:, 3]
    left = m[:, 0] - w / 2.0
    top = m[:, 1] - h / 2.0
    return np.stack([left, top, w + left, h + top], axis=1).astype(F32)


# ---- Kalman filter, XYWH (kalman_filter.py:289-491), fp64 --------------------------------------------------------------
def kf_initiate_xywh(xywh32: np.ndarray):
    """kalman_filter.py:347-362. All eight entries of the reference's ``std`` list are np.float32 (a Python float times
    an np.float32 scalar stays fp32 under NumPy 2), so ``np.square`` squares them in fp32 too: fp32 products with
    fp32(0.1) and fp32(0.0625), fp32 squares, then promoted. (XYAH's list mixes in Python floats and is squared in
    fp64.) The recorded fixture pins these points."""
    z = np.asarray(xywh32, dtype=F32)
    mean = np.zeros(8, dtype=F64)
    mean[:4] = z.astype(F64)
    pw, ph = F32(2 * STD_POS) * z[2], F32(2 * STD_POS) * z[3]
    vw, vh = F32(10 * STD_VEL) * z[2], F32(10 * STD_VEL) * z[3]
    std = np.array([pw, ph, pw, ph, vw, vh, vw, vh], dtype=F32)
    return mean, np.diag(np.square(std).astype(F64))


def kf_predict_xywh(mean: np.ndarray, cov: np.ndarray):
    """kalman_filter.py:382-399 (multi_predict 448-469 is the same per track): Q from mean[2], mean[3] before the step."""
    w, h = mean[2], mean[3]
    std = np.array([STD_POS * w, STD_POS * h, STD_POS * w, STD_POS * h, STD_VEL * w, STD_VEL * h, STD_VEL * w,
                    STD_VEL * h], dtype=F64)
    return np.dot(mean, _MOTION.T), np.linalg.multi_dot((_MOTION, cov, _MOTION.T)) + np.diag(np.square(std))


def kf_update_xywh(mean: np.ndarray, cov: np.ndarray, xywh32: np.ndarray):
    """kalman_filter.py:418-428 (project) and 226-236 (update, inherited): the same 4x4 Cholesky solve as XYAH."""
    import scipy.linalg
    w, h = mean[2], mean[3]
    std = np.array([STD_POS * w, STD_POS * h, STD_POS * w, STD_POS * h], dtype=F64)
    pmean = mean[:4].copy()
    pcov = cov[:4, :4] + np.diag(np.square(std))
    chol, lower = scipy.linalg.cho_factor(pcov, lower=True, check_finite=False)
    gain = scipy.linalg.cho_solve((chol, lower), cov[:, :4].T, check_finite=False).T
    innovation = np.asarray(xywh32, dtype=F32).astype(F64) - pmean
    return mean + np.dot(innovation, gain.T), cov - np.linalg.multi_dot((gain, pcov, gain.T))


# ---- camera motion (byte_tracker.py:103-120) ---------------------------------------------------------------------------
def gmc_apply(mean: np.ndarray, cov: np.ndarray, H: np.ndarray):
    """STrack.multi_gmc for one track, ``H`` fp64 [2, 3], ``R = H[:, :2]``: ``mean' = kron(I4, R) mean`` with
    ``H[:, 2]`` added to (cx, cy), ``cov' = kron(I4, R) cov kron(I4, R)'`` - in the block form the kernel uses: four
    2-vector products and the sixteen 2x2 blocks ``R C_ij R'``; the 8x8 is never formed. ``R`` mixes (w, h), (vx, vy)
    and (vw, vh) as it mixes (cx, cy): the reference's behaviour, kept."""
    H = np.asarray(H, dtype=F64).reshape(2, 3)
    R = H[:, :2]
    m = np.asarray(mean, dtype=F64).reshape(4, 2)
    out = np.empty((4, 2), dtype=F64)
    out[:, 0] = R[0, 0] * m[:, 0] + R[0, 1] * m[:, 1]
    out[:, 1] = R[1, 0] * m[:, 0] + R[1, 1] * m[:, 1]
    out[0] += H[:, 2]
    C = np.asarray(cov, dtype=F64).reshape(4, 2, 4, 2)
    c00, c01, c10, c11 = C[:, 0, :, 0], C[:, 0, :, 1], C[:, 1, :, 0], C[:, 1, :, 1]
    a, b, c, d = R[0, 0], R[0, 1], R[1, 0], R[1, 1]
    m00, m01 = a * c00 + b * c10, a * c01 + b * c11  # R C_ij
    m10, m11 = c * c00 + d * c10, c * c01 + d * c11
    P = np.empty((4, 2, 4, 2), dtype=F64)
    P[:, 0, :, 0] = m00 * a + m01 * b  # (R C_ij) R'
    P[:, 0, :, 1] = m00 * c + m01 * d
    P[:, 1, :, 0] = m10 * a + m11 * b
    P[:, 1, :, 1] = m10 * c + m11 * d
    return out.reshape(8), P.reshape(8, 8)


def warp_ok(warp) -> bool:
    """The rule of ours: a warp is applied when all six entries are finite."""
    return bool(np.isfinite(np.asarray(warp, dtype=F64)).all())


# ---- the tracker -------------------------------------------------------------------------------------------------------
BOTSORT_IGNORED = ("proximity_thresh", "appearance_thresh")  # they gate the ReID term only, which does not exist (B4)


class BotSortStreamTracker(bt.StreamTracker):
    """One stream's BoT-SORT over ``T`` slots: :class:`~.bytetrack.StreamTracker` with the XYWH filter, B1..B3.
    ``update(rows, count=None, warp=None)``: ``warp`` is the 2x3 camera motion from the previous frame to this one, in
    the pixels the rows are in, or None."""

    _kf_initiate = staticmethod(kf_initiate_xywh)
    _kf_predict = staticmethod(kf_predict_xywh)
    _kf_update = staticmethod(kf_update_xywh)
    _track_boxes = staticmethod(track_boxes_xywh)
    _ZEROED = (6, 7)  # B1, bot_sort.py:126-129

    def __init__(self, capacity=256, observer=None, with_reid=False, **kw):
        if with_reid:
            raise NotImplementedError("BoT-SORT with_reid: the reference's ReID is a stub (its encoder is always None); "
                                      "only with_reid: False is implemented")
        for k in BOTSORT_IGNORED:
            kw.pop(k, None)
        super().__init__(capacity=capacity, observer=observer, **kw)

    def reset(self):
        super().reset()
        self.bad_warp = 0
        self._warp = None

    # the pieces a mutation test overrides -----------------------------------------------------------------------------
    def _gmc(self, mean, cov, H):
        return gmc_apply(mean, cov, H)

    def _warped(self, pool, unconfirmed):
        return pool + unconfirmed  # byte_tracker.py:334-335

    def _measurements(self, rows, xyah):
        return det_xywh(rows)  # B2

    def _motion(self, pool, unconfirmed):
        super()._motion(pool, unconfirmed)  # multi_predict of the pool, byte_tracker.py:331
        self._warp_tracks(pool, unconfirmed)  # B3

    def _warp_tracks(self, pool, unconfirmed):
        if self._warp is not None:
            for i in self._warped(pool, unconfirmed):
                self.mean[i], self.cov[i] = self._gmc(self.mean[i], self.cov[i], self._warp)

    def update(self, rows, count=None, warp=None) -> np.ndarray:
        self._warp = None
        if warp is not None:
            H = np.asarray(warp, dtype=F64)
            if H.shape != (2, 3):
                raise ValueError(f"BotSortStreamTracker.update: warp of shape {H.shape}, [2, 3] expected")
            if warp_ok(H):
                self._warp = H
            else:
                self.bad_warp += 1
        return super().update(rows, count)

    def snapshot(self) -> dict:
        return dict(super().snapshot(), bad_warp=self.bad_warp)
