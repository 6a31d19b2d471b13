"""CPU: the BoT-SORT restatement (yolosod_amd.utils.botsort, tests/botsort_ref.py) - the definition the XYWH
instantiation of the HIP tracker kernel is held to (tests/test_gpu_botsort.py): its Kalman steps against the reference's
recorded ones, ``gmc_apply`` against the dense formula, one directed scene per trait with the expected ids / states /
idx reasoned from the reference's code and written here, the certification of the random scenes with camera motion that
the GPU test runs, mutations that show that plausible kernel bugs break these assertions, and the YAML routes."""
import functools

import numpy as np
import pytest

import botsort_ref as B
import bytetrack_ref as R
from bytetrack_ref import FREE, LOST, TRACKED
from conftest import golden

T_, L_, F_ = TRACKED, LOST, FREE


# ---- Kalman pin ------------------------------------------------------------------------------------------------------
KALMAN_TOL = 1e-12  # as for XYAH; measured when the fixture was made: 0 (the same operations in the same order)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_kalman_xywh_steps_match_the_reference_fixture():
    g = golden("kalman_xywh")
    assert float(g["max_rel_diff"]) < KALMAN_TOL / 100
    z = g["z"]
    for i in range(z.shape[1]):
        m, c = B.kf_initiate_xywh(z[0, i])
        assert m.dtype == np.float64 and c.dtype == np.float64
        assert _rel(m, g["init_mean"][i]) <= KALMAN_TOL and _rel(c, g["init_cov"][i]) <= KALMAN_TOL
        for step, k in (("pred1", None), ("upd1", 1), ("pred2", None), ("upd2", 2)):
            m, c = B.kf_predict_xywh(m, c) if k is None else B.kf_update_xywh(m, c, z[k, i])
            assert _rel(m, g[step + "_mean"][i]) <= KALMAN_TOL, (i, step)
            assert _rel(c, g[step + "_cov"][i]) <= KALMAN_TOL, (i, step)
            m, c = g[step + "_mean"][i].copy(), g[step + "_cov"][i].copy()
        m, c = B.kf_predict_xywh(g["upd2_mean"][i], g["upd2_cov"][i])  # multi_predict is predict per track
        assert _rel(m, g["multi_mean"][i]) <= KALMAN_TOL and _rel(c, g["multi_cov"][i]) <= KALMAN_TOL


def test_kalman_xywh_initiate_squares_in_fp32_as_the_reference_does():
    # the reference's std list is all np.float32, so np.square is fp32 (the fixture records float32 for both): an fp64
    # square of the fp32 product differs from the recorded value in the last bits of the fp32 mantissa
    g = golden("kalman_xywh")
    assert str(g["init_cov_dtype"]) == "float32" and str(g["init_mean_dtype"]) == "float32"
    z = g["z"][0, 0]
    _, c = B.kf_initiate_xywh(z)
    assert np.array_equal(c, g["init_cov"][0])
    in_fp64 = np.float64(np.float32(0.1) * z[2]) ** 2
    assert c[0, 0] == np.float64(np.float32(np.float32(0.1) * z[2]) ** 2) and c[0, 0] != in_fp64


def test_the_xyah_filter_is_untouched():
    g = golden("kalman_xyah")
    m, c = R.kf_initiate(g["z"][0, 0])
    assert _rel(m, g["init_mean"][0]) <= KALMAN_TOL and _rel(c, g["init_cov"][0]) <= KALMAN_TOL
    assert R.StreamTracker._ZEROED == (7,) and B.BotSortStreamTracker._ZEROED == (6, 7)


# ---- gmc_apply against the dense formula -------------------------------------------------------------------------------
def test_gmc_apply_is_the_dense_kron_formula():
    rng = np.random.default_rng(35)
    for i in range(20):
        mean = rng.normal(0, 1, 8) * np.array([900, 500, 80, 120, 6, 6, 2, 2.0])
        L = rng.normal(0, 1, (8, 8)) * np.array([4, 4, 3, 3, 1, 1, 0.5, 0.5])[:, None]
        cov = L @ L.T
        H = B.similarity(rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(-5, 5), rng.uniform(0.7, 1.4),
                         (rng.uniform(0, 1920), rng.uniform(0, 1080)))
        if i % 4 == 3:
            H = rng.normal(0, 1, (2, 3))  # any finite matrix, not only a similarity
        R8 = np.kron(np.eye(4, dtype=float), H[:, :2])  # byte_tracker.py:110-117
        em = R8.dot(mean)
        em[:2] += H[:, 2]
        ec = R8.dot(cov).dot(R8.transpose())
        m, c = B.gmc_apply(mean, cov, H)
        assert m.dtype == np.float64 and c.shape == (8, 8)
        assert _rel(m, em) <= 1e-12 and _rel(c, ec) <= 1e-12, i
    m, c = B.gmc_apply(mean, cov, B.IDENTITY)
    assert np.array_equal(m, mean) and np.array_equal(c, cov)


# ---- directed scenes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _directed(name, cls=B.Scripted):
    frames, warps, kw = B.directed_scenes()[name]
    res, _ = B.run(frames, warps, capacity=64, cls=cls, **kw)
    return res


def _check(name, expected):
    """expected: per frame (ids, idx, states of the first slots)."""
    got = B.summary(_directed(name))
    assert len(got) == len(expected)
    for f, ((ids, idx, st), (eids, eidx, est)) in enumerate(zip(got, expected), 1):
        assert ids == eids, (name, f, "ids", ids)
        assert idx == eidx, (name, f, "idx", idx)
        assert st[:len(est)] == est and not any(st[len(est):]), (name, f, "states", st[:len(est) + 1])


def test_b1_a_lost_track_is_predicted_without_both_size_velocities():
    _check("b1_size_velocity", [([1, 2], [0, 1], [T_, T_])] * 5 + [([2], [0], [L_, T_])] * 6
           + [([1, 2], [0, 1], [T_, T_])])
    snap = _directed("b1_size_velocity")[10][1]  # frame 11: lost for six frames, its size as after frame 5's update
    assert snap["mean"][0, 6] == 0.0 and snap["mean"][0, 7] == 0.0
    assert abs(snap["mean"][0, 2] - 60.0) < 8.0 and abs(snap["mean"][0, 3] - 120.0) < 16.0


def test_the_model_switches_bytetrack_and_botsort_end_with_different_ids():
    # width + 12 px a frame, match_thresh 0.5: XYWH follows (id 1 throughout); XYAH's aspect lags, A is lost at frame 4
    # and its successor (id 2, born unconfirmed at frame 4) at frame 10
    _check("model_width_growth", [([1], [0], [T_])] * 10)
    frames, _, kw = B.directed_scenes()["model_width_growth"]
    byte, _ = R.run_scene(frames, capacity=64, **kw)
    assert [s[0] for s in R.summary(byte)] == [[1]] * 3 + [[]] + [[2]] * 5 + [[]]
    assert R.summary(byte)[-1][2][:3] == [L_, L_, T_]


def test_b3_ids_persist_through_a_pan_with_warps_and_are_lost_without():
    _check("b3_pan", [([1, 2], [0, 1], [T_, T_])] * 6)
    assert _directed("b3_pan")[-1][1]["next_id"] == 3
    # without: both lost at frame 3; the births of every frame (slots 2, 3) never overlap their next detections, are
    # removed unconfirmed and their slots are taken by the next births: nothing is ever output again
    _check("b3_pan_no_warps", [([1, 2], [0, 1], [T_, T_])] * 2 + [([], [], [L_, L_, T_, T_])] * 4)
    assert [s["next_id"] for _, s in _directed("b3_pan_no_warps")] == [3, 3, 5, 7, 9, 11]
    # the warp moves the state, it does not teach the filter a velocity: the detection is where the warped mean is
    snap = _directed("b3_pan")[-1][1]
    assert abs(snap["mean"][0, 0] - (100.0 + 160.0 + 20.0)) < 1e-6 and abs(snap["mean"][0, 4]) < 1e-6


def test_b3_an_unconfirmed_track_is_warped_too():
    # C: born at frame 2 into slot 1 (id 2, not output), warped at frame 3 although it was not predicted, matched in
    # the third association and output from frame 3 on
    _check("b3_unconfirmed", [([1], [0], [T_]), ([1], [0], [T_, T_]), ([1, 2], [0, 1], [T_, T_]),
                              ([1, 2], [0, 1], [T_, T_])])
    res = _directed("b3_unconfirmed")
    assert [int(s["flags"][1]) & 1 for _, s in res] == [0, 0, 1, 1] and res[-1][1]["next_id"] == 3


def test_b3_zoom_and_rotation():
    _check("b3_zoom_rotation", [([1, 2, 3], [0, 1, 2], [T_, T_, T_])] * 5)
    res = _directed("b3_zoom_rotation")
    assert res[-1][1]["next_id"] == 4
    # track 2 (far from the centre) moved by more than its size at frame 3
    before, after = res[1][0][1, :4], res[2][0][1, :4]
    assert after[0] - before[0] > 60.0 and (after[2] - after[0]) > 1.15 * (before[2] - before[0])


def test_identity_warps_equal_no_warps_as_values():
    a, b = _directed("identity_none"), _directed("identity_warps")
    assert B.summary(a) == B.summary(b)
    for (ra, sa), (rb, sb) in zip(a, b):
        assert np.array_equal(ra, rb)
        live = sa["state"] != FREE
        # == on values: -0.0 + 0.0 flips a sign bit under the identity, the bytes may differ
        assert (sa["mean"][live] == sb["mean"][live]).all() and (sa["cov"][live] == sb["cov"][live]).all()
        assert sa["bad_warp"] == sb["bad_warp"] == 0
    _check("identity_warps", [([1, 2], [0, 1], [T_, T_])] * 3 + [([2], [0], [L_, T_, T_]), ([2, 3], [0, 1], [L_, T_, T_]),
                              ([1, 2, 3], [1, 0, 2], [T_, T_, T_])])


def test_a_nan_warp_is_skipped_and_counted():
    # frame 3 goes as b3_pan_no_warps' frame 3; its births (ids 3, 4) are warped at frame 4 and confirmed; the old
    # tracks are one frame's pan behind for good
    _check("bad_warp", [([1, 2], [0, 1], [T_, T_])] * 2 + [([], [], [L_, L_, T_, T_])]
           + [([3, 4], [0, 1], [L_, L_, T_, T_])] * 3)
    assert [s["bad_warp"] for _, s in _directed("bad_warp")] == [0, 0, 1, 1, 1, 1]
    assert B.summary(_directed("bad_warp"))[2] == B.summary(_directed("b3_pan_no_warps"))[2]
    t = B.BotSortStreamTracker(capacity=64)
    for bad in (np.inf, -np.inf, np.nan):
        w = B.IDENTITY.copy()
        w[0, 0] = bad
        t.update(*R.pad([R.box(100.0)]), warp=w)
    t.update(*R.pad([R.box(100.0)]), warp=np.zeros((2, 3)))  # finite, degenerate: applied as given, not counted
    assert t.bad_warp == 3
    with pytest.raises(ValueError, match="warp"):
        t.update(*R.pad([]), warp=np.eye(3))


# ---- certification of the random scenes ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random(name, cls=B.Scripted, margins=True):
    args, kw = B.RANDOM_SCENES[name]
    frames, warps = B.camera_scene(**args)
    res, m = B.run(frames, warps, margins=margins, cls=cls, **kw)
    return frames, warps, res, m


@pytest.mark.parametrize("name", sorted(B.RANDOM_SCENES))
def test_random_scenes_with_camera_motion_certify_on_every_frame(name):
    frames, warps, res, margins = _random(name)
    rule = R.CERT_FACTOR * R.delta(frames)
    print(f"{name}: rule {rule:.3e}, smallest margin {min(margins):.3e}")
    assert 0 < rule < 2e-3
    assert len(margins) == len(frames) == len(warps)
    assert all(m >= rule for m in margins), (rule, min(margins), int(np.argmin(margins)))
    assert warps[0] is None and all(w is not None and np.abs(w[:, 2]).max() > 0 for w in warps[1:])
    snap = res[-1][1]
    assert snap["next_id"] > len(res[0][0]) + 10 and (snap["state"] >= LOST).any()  # births and losses happen
    assert snap["bad_warp"] == 0
    if name == "small64":
        assert snap["overflow"] > 0  # capacity pressure
    if name == "big280":
        assert (snap["state"] != FREE).sum() > 256  # more tracks than lanes in a workgroup


def test_the_camera_motion_matters_in_the_random_scenes():
    """Without the warps the same detections give other ids: the scenes do exercise B3."""
    frames, warps, res, _ = _random("small64")
    plain, _ = B.run(frames, None, **B.RANDOM_SCENES["small64"][1])
    assert B.summary(plain) != B.summary(res)


# ---- mutations -----------------------------------------------------------------------------------------------------------
class NoGmcOnUnconfirmed(B.Scripted):
    def _warped(self, pool, unconfirmed):
        return pool


class ZeroVhOnly(B.Scripted):
    _ZEROED = (7,)


def _xyah_noise_predict(mean, cov):
    h = mean[3]
    std = np.array([B.bs.STD_POS * h, B.bs.STD_POS * h, 1e-2, B.bs.STD_POS * h, B.bs.STD_VEL * h, B.bs.STD_VEL * h,
                    1e-5, B.bs.STD_VEL * h])
    F = B.bs._MOTION
    return np.dot(mean, F.T), np.linalg.multi_dot((F, cov, F.T)) + np.diag(np.square(std))


class XyahNoise(B.Scripted):
    """XYAH's process noise (all from the height, 1e-2 / 1e-5 for the third component) in the XYWH filter's predict."""
    _kf_predict = staticmethod(_xyah_noise_predict)


class TranslationOnly(B.Scripted):
    def _gmc(self, mean, cov, H):
        m = mean.copy()
        m[:2] += H[:, 2]
        return m, cov


class WarpBeforePredict(B.Scripted):
    def _motion(self, pool, unconfirmed):
        self._warp_tracks(pool, unconfirmed)
        R.StreamTracker._motion(self, pool, unconfirmed)


DIRECTED = ("b1_size_velocity", "model_width_growth", "b3_pan", "b3_unconfirmed", "b3_zoom_rotation", "identity_warps",
            "bad_warp")


def _state_differs(a, b, tol=1e-6):
    """ids, idx or slot states differ in some frame - or, with those equal, a live fp64 mean by more than ``tol``
    relative (three orders above the 1e-9 the device is held to)."""
    if B.summary(a) != B.summary(b):
        return "ids"
    for (_, sa), (_, sb) in zip(a, b):
        live = sa["state"] != FREE
        if live.any():
            scale = np.abs(sb["mean"][live]).max(axis=1, keepdims=True)
            if float((np.abs(sa["mean"][live] - sb["mean"][live]) / scale).max()) > tol:
                return "means"
    return None


def _differs(cls):
    bad = {}
    for name in DIRECTED:
        d = _state_differs(_directed(name, cls), _directed(name))
        if d:
            bad[name] = d
    for name in ("small64",):
        d = _state_differs(_random(name, cls, False)[2], _random(name)[2])
        if d:
            bad[name] = d
    return bad


@pytest.mark.parametrize("cls", [NoGmcOnUnconfirmed, ZeroVhOnly, XyahNoise, TranslationOnly, WarpBeforePredict])
def test_mutations_change_ids_or_states(cls):
    bad = _differs(cls)
    print(cls.__name__, bad)
    assert bad, f"{cls.__name__}: no scene notices"
    if cls is NoGmcOnUnconfirmed:
        assert bad.get("b3_unconfirmed") == "ids"
    if cls is ZeroVhOnly:
        assert bad.get("b1_size_velocity") == "ids"
    if cls is XyahNoise:
        # the width's noise taken from the height: a 40 x 60 box still follows its width in the directed scenes (the
        # means move, the ids hold); among the small objects of the random scene the ids change
        assert bad.get("small64") == "ids" and bad.get("model_width_growth") == "means"
    if cls is TranslationOnly:
        assert bad.get("b3_zoom_rotation") == "ids"
    if cls is WarpBeforePredict:
        # the means of both orders are equal in exact arithmetic (R (x + v) + t either way); the covariances are not
        # (Q is added before the warp or after it, from other sizes), so the gains and the next means differ
        assert bad.get("b3_zoom_rotation") in ("ids", "means")


# ---- the product's classes -------------------------------------------------------------------------------------------------
BOTSORT_YAML = ("tracker_type: botsort\ntrack_high_thresh: 0.3\ntrack_low_thresh: 0.05\nnew_track_thresh: 0.4\n"
                "track_buffer: 12\nmatch_thresh: 0.7\nfuse_score: False\ngmc_method: sparseOptFlow\n"
                "proximity_thresh: 0.5\nappearance_thresh: 0.25\nwith_reid: False\n")


def test_host_tracker_runs_the_same_steps():
    import torch

    from yolosod_amd.engine.tracker import BotSortTrackerHost, ByteTrackerHost
    frames, warps, kw = B.directed_scenes()["b3_pan"]
    host = BotSortTrackerHost(streams=2, capacity=64, **kw)
    ref, plain = _directed("b3_pan"), _directed("b3_pan_no_warps")
    for f, ((rows, n), (out, _), (pout, _)) in enumerate(zip(frames, ref, plain)):
        w = None if warps[f] is None else np.stack([warps[f], B.IDENTITY]).astype(np.float32 if f % 2 else np.float64)
        tr = host.update(torch.from_numpy(np.stack([rows, rows])), torch.tensor([n, n], dtype=torch.int32), warps=w)
        assert tuple(tr.rows.shape) == (2, 64, 8) and tr.counts.tolist() == [len(out), len(pout)]
        assert np.array_equal(tr.rows[0, :len(out)].numpy(), out) and not tr.rows[0, len(out):].any()
        assert np.array_equal(tr.rows[1, :len(pout)].numpy(), pout)
    assert host.bad_warp.tolist() == [0, 0] and host.overflow.tolist() == [0, 0]
    nan = np.full((2, 2, 3), np.nan)
    nan[0] = B.IDENTITY
    host.update(np.zeros((2, 16, 6), np.float32), np.zeros(2, np.int64), warps=nan)
    assert host.bad_warp.tolist() == [0, 1]
    host.reset(streams=[1])
    assert host.bad_warp.tolist() == [0, 0] and host.trackers[0].frame == len(frames) + 1 and host.trackers[1].frame == 0
    for shape in ((2, 3), (1, 2, 3), (2, 3, 2)):
        with pytest.raises(ValueError, match="warps"):
            host.update(np.zeros((2, 16, 6), np.float32), np.zeros(2, np.int64), warps=np.zeros(shape))
    with pytest.raises(ValueError, match="fp32 or fp64"):
        host.update(np.zeros((2, 16, 6), np.float32), np.zeros(2, np.int64), warps=np.zeros((2, 2, 3), dtype=np.int32))
    with pytest.raises((TypeError, ValueError), match="warps"):
        ByteTrackerHost(streams=2, capacity=64).update(np.zeros((2, 16, 6), np.float32), np.zeros(2, np.int64),
                                                       warps=np.zeros((2, 2, 3)))


def test_from_yaml_routes(tmp_path):
    from yolosod_amd.engine.tracker import (BotSortTracker, BotSortTrackerHost, ByteTracker, ByteTrackerHost,
                                            tracker_from_yaml)
    bot, byte = tmp_path / "botsort.yaml", tmp_path / "bytetrack.yaml"
    bot.write_text(BOTSORT_YAML)
    byte.write_text("tracker_type: bytetrack\nmatch_thresh: 0.7\n")
    h = BotSortTrackerHost.from_yaml(bot, streams=1)
    assert h.params.tolist() == [np.float32(v) for v in (0.3, 0.05, 0.4, 0.7, 0.5, 0.7, 12, 0)]
    assert h.gmc_method == "sparseOptFlow" and h.with_reid is False
    assert (h.proximity_thresh, h.appearance_thresh) == (0.5, 0.25)
    assert isinstance(h.trackers[0], B.BotSortStreamTracker) and h.trackers[0].max_time_lost == 12
    assert BotSortTrackerHost(streams=1).gmc_method == "none"
    with pytest.raises(ValueError, match="bytetrack"):
        BotSortTrackerHost.from_yaml(byte, streams=1)
    with pytest.raises(ValueError, match="bytetrack"):
        BotSortTracker.from_yaml(byte, streams=1)
    for cls in (ByteTrackerHost, ByteTracker):  # still refused, and said to be ByteTrack's refusal
        with pytest.raises(NotImplementedError, match="ByteTrack"):
            cls.from_yaml(bot, streams=1)
    a, b = tracker_from_yaml(bot, streams=2, device="cpu"), tracker_from_yaml(byte, streams=2, device="cpu")
    assert type(a) is BotSortTrackerHost and type(b) is ByteTrackerHost and a.streams == b.streams == 2
    assert a.params[3] == b.params[3] == np.float32(0.7) and a.gmc_method == "sparseOptFlow"
    with pytest.raises(RuntimeError, match="GPU"):
        BotSortTracker(streams=1, device="cpu")
    other = tmp_path / "other.yaml"
    other.write_text("tracker_type: deepsort\n")
    for make in (lambda: tracker_from_yaml(other, streams=1, device="cpu"), lambda: BotSortTrackerHost.from_yaml(other, 1),
                 lambda: ByteTrackerHost.from_yaml(other, 1)):
        with pytest.raises(ValueError, match="deepsort"):
            make()
    reid = tmp_path / "reid.yaml"
    reid.write_text(BOTSORT_YAML.replace("with_reid: False", "with_reid: True"))
    with pytest.raises(NotImplementedError, match="with_reid"):
        tracker_from_yaml(reid, streams=1, device="cpu")
    with pytest.raises(NotImplementedError, match="with_reid"):
        B.BotSortStreamTracker(with_reid=True)
    t = B.BotSortStreamTracker(capacity=64, proximity_thresh=0.1, appearance_thresh=0.9, with_reid=False)  # ignored
    assert t.T == 64


def test_predictors_refuse_warps_for_a_bytetrack_tracker():
    from yolosod_amd.engine import predictor as P
    from yolosod_amd.engine.tracker import BotSortTrackerHost, ByteTrackerHost
    frames = [np.zeros((48, 64, 3), dtype=np.uint8)] * 2
    for cls in (P.DetectionPredictor, P.SlicedPredictor):
        p = cls.__new__(cls)  # no model: the refusal comes before predict_padded
        p.tracker = ByteTrackerHost(streams=2, capacity=64)
        with pytest.raises(ValueError, match="ByteTrack"):
            p.track_padded(frames, warps=np.zeros((2, 2, 3)))
        with pytest.raises(ValueError, match="ByteTrack"):
            p.track(frames, warps=np.zeros((2, 2, 3)))
        p.tracker = BotSortTrackerHost(streams=2, capacity=64)
        import torch
        p.predict_padded = lambda batch: (torch.zeros(2, 16, 6), torch.zeros(2, dtype=torch.int32),
                                          torch.zeros(2, 16, dtype=torch.int32))
        rows, n, *_ = p.track_padded(frames, warps=np.stack([B.IDENTITY] * 2))
        assert tuple(rows.shape) == (2, 64, 8) and n.tolist() == [0, 0]
        assert len(p.track(frames, warps=None)) == 2
