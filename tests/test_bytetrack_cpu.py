"""CPU: the ByteTrack restatement (yolosod_amd.utils.bytetrack, tests/bytetrack_ref.py) - the definition the HIP tracker
kernel is held to (tests/test_gpu_track.py): its Kalman steps against the reference's recorded ones, its assignment
against brute force, one directed scene per trait with the expected ids / states / idx reasoned from the reference's
code and written here, the certification of the random scenes the GPU test runs, and mutations that show that
plausible kernel bugs break these assertions."""
import functools

import numpy as np
import pytest

import bytetrack_ref as R
from bytetrack_ref import FREE, LOST, REMOVED, TRACKED
from conftest import golden


# ---- Kalman pin ------------------------------------------------------------------------------------------------------
KALMAN_TOL = 1e-12  # both sides fp64, only the summation order differs; measured when the fixture was made: 1.35e-16


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_kalman_steps_match_the_reference_fixture():
    g = golden("kalman_xyah")
    assert float(g["max_rel_diff"]) < KALMAN_TOL / 100
    z = g["z"]
    for i in range(z.shape[1]):
        m, c = R.kf_initiate(z[0, i])
        assert m.dtype == np.float64 and c.dtype == np.float64
        assert _rel(m, g["init_mean"][i]) <= KALMAN_TOL and _rel(c, g["init_cov"][i]) <= KALMAN_TOL
        for step, k in (("pred1", None), ("upd1", 1), ("pred2", None), ("upd2", 2)):
            m, c = R.kf_predict(m, c) if k is None else R.kf_update(m, c, z[k, i])
            assert _rel(m, g[step + "_mean"][i]) <= KALMAN_TOL, (i, step)
            assert _rel(c, g[step + "_cov"][i]) <= KALMAN_TOL, (i, step)
            m, c = g[step + "_mean"][i].copy(), g[step + "_cov"][i].copy()
        m, c = R.kf_predict(g["upd2_mean"][i], g["upd2_cov"][i])  # multi_predict is predict per track
        assert _rel(m, g["multi_mean"][i]) <= KALMAN_TOL and _rel(c, g["multi_cov"][i]) <= KALMAN_TOL


# ---- assignment ------------------------------------------------------------------------------------------------------
def test_assignment_is_the_brute_force_optimum():
    rng = np.random.default_rng(5)
    for t in range(200):
        n, m = rng.integers(1, 8, 2)
        cost = rng.random((n, m)).astype(np.float32)
        if t % 2:
            cost = np.where(rng.random((n, m)) < 0.5, np.float32(1.0), cost)  # sparse, as IoU graphs are
        thresh = (0.8, 0.5, 0.7)[t % 3]
        best, _ = R.brute_force(cost, thresh)
        got = R.assign(cost, thresh)
        assert len({i for i, _ in got}) == len(got) == len({j for _, j in got})
        assert abs(R.objective(cost, thresh, got) - best) <= 1e-12, (t, got)


def test_greedy_is_not_the_optimum_somewhere():
    cost = np.array([[0.10, 0.20], [0.15, 0.90]], dtype=np.float32)  # greedy takes (0, 0) and strands row 1
    assert R.greedy_assign(cost, 0.8) == [(0, 0)]
    assert sorted(R.assign(cost, 0.8)) == [(0, 1), (1, 0)]


# ---- directed scenes -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _directed(name, cls=R.StreamTracker):
    frames, kw = R.directed_scenes()[name]
    res, _ = R.run_scene(frames, capacity=64, cls=cls, **kw)
    return res


def _check(name, expected):
    """expected: per frame (ids, idx, states of the first slots)."""
    got = R.summary(_directed(name))
    assert len(got) == len(expected)
    for f, ((ids, idx, st), (eids, eidx, est)) in enumerate(zip(got, expected), 1):
        assert ids == eids, (name, f, "ids", ids)
        assert idx == eidx, (name, f, "idx", idx)
        assert st[:len(est)] == est and not any(st[len(est):]), (name, f, "states", st[:len(est) + 1])


T_, L_, X_, F_ = TRACKED, LOST, REMOVED, FREE


def test_q0_birth_is_unconfirmed_for_a_frame_and_a_false_alarm_goes():
    # frame 1 births are activated at once (byte_tracker.py:130); the frame-3 alarm takes slot 2 and id 3, is not
    # output, finds nothing at frame 4 and is removed (:377-380); the frame-5 birth (id 4) is output from frame 6
    _check("q0_false_alarm", [([1, 2], [0, 1], [T_, T_]), ([1, 2], [0, 1], [T_, T_]), ([1, 2], [0, 1], [T_, T_, T_]),
                              ([1, 2], [0, 1], [T_, T_, F_]), ([1, 2], [0, 1], [T_, T_, T_]),
                              ([1, 2, 4], [0, 1, 2], [T_, T_, T_])])
    res = _directed("q0_false_alarm")
    assert [int(s["flags"][2]) & 1 for _, s in res] == [0, 0, 0, 0, 0, 1]
    assert [s["next_id"] for _, s in res] == [3, 3, 4, 4, 5, 5]


def test_q1_a_lost_track_is_found_again_with_its_id():
    _check("q1_refind", [([1, 2], [0, 1], [T_, T_])] * 3 + [([2], [0], [L_, T_])] * 2 + [([1, 2], [1, 0], [T_, T_])])


def test_q1_a_lost_track_is_predicted_without_its_height_velocity():
    _check("q1_height_velocity", [([1, 2], [0, 1], [T_, T_])] * 5 + [([2], [0], [L_, T_])] * 6
           + [([1, 2], [0, 1], [T_, T_])])


def test_q2_second_tier_continues_tracked_tracks_only():
    # frame 3: A (0.15) continues through the second association, B is lost; frame 4: the 0.15 detection on B is in the
    # second tier, where lost tracks do not take part (:351), and it starts nothing (not in the high tier)
    _check("q2_low_score", [([1, 2], [0, 1], [T_, T_])] * 2 + [([1], [0], [T_, L_]), ([1], [0], [T_, L_]),
                                                                ([1, 2], [0, 1], [T_, T_])])
    res = _directed("q2_low_score")
    assert res[2][0][0, 5] == np.float32(0.15) and res[3][1]["next_id"] == 3


def test_q3_ids_follow_the_row_index_and_new_track_thresh():
    _check("q3_id_order", [([1, 2], [0, 2], [T_, T_])] * 2)
    assert _directed("q3_id_order")[1][1]["next_id"] == 3


def test_q4_q5_expiry_is_a_frame_late_and_a_resurrected_track_dies_at_once():
    _check("q4_q5_resurrect", [([1, 2], [0, 1], [T_, T_])] * 2 + [([2], [0], [L_, T_])] * 2 + [([2], [0], [X_, T_]),
                               ([1, 2], [1, 0], [T_, T_]), ([2], [0], [F_, T_]), ([2], [0], [T_, T_]),
                               ([2, 3], [0, 1], [T_, T_])])
    res = _directed("q4_q5_resurrect")
    assert [int(s["flags"][0]) >> 1 for _, s in res[3:7]] == [0, 1, 1, 1]  # in the removed set from frame 5 on
    _check("q4_expire", [([1, 2], [0, 1], [T_, T_])] * 2 + [([2], [0], [L_, T_])] * 2 + [([2], [0], [X_, T_])]
           + [([2], [0], [F_, T_])] * 2)


def test_q6_duplicates_the_longer_lived_side_survives_and_ties_drop_the_tracked_one():
    # the newcomer (id 2, slot 1) is born and dropped within frame 5; A is found again at frame 6
    _check("q6_lost_survives", [([1], [0], [T_])] * 3 + [([], [], [L_]), ([], [], [L_, F_]), ([1], [0], [T_])])
    assert [s["next_id"] for _, s in _directed("q6_lost_survives")] == [2, 2, 2, 2, 3, 3]
    _check("q6_tie", [([1], [0], [T_]), ([], [], [L_]), ([], [], [L_, F_]), ([1], [0], [T_])])
    assert [s["next_id"] for _, s in _directed("q6_tie")] == [2, 2, 3, 3]
    # C (id 2, slot 1) is lost from frame 2; A's detection stops 2 px off C at frame 11 (IoU 0.905): C goes then
    _check("q6_tracked_survives", [([1, 2], [0, 1], [T_, T_])] + [([1], [0], [T_, L_])] * 9 + [([1], [0], [T_, F_])] * 3)


def test_assignment_is_optimal_not_greedy():
    _check("assign_swap", [([1, 2], [0, 1], [T_, T_]), ([1, 2], [1, 0], [T_, T_])])
    assert _directed("assign_swap")[1][1]["next_id"] == 3


def test_capacity_overflow_skips_births_and_counts_them():
    res = _directed("capacity_overflow")
    for f, (out, snap) in enumerate(res, 1):
        assert [int(v) for v in out[:, 4]] == list(range(1, 65)) and [int(v) for v in out[:, 7]] == list(range(64))
        assert snap["overflow"] == 6 * f and snap["next_id"] == 65 and (snap["state"] == TRACKED).all()


def test_invalid_rows_are_ignored_and_keep_their_index():
    _check("invalid_rows", [([1, 2, 3], [0, 2, 6], [T_, T_, T_])] * 3)
    assert _directed("invalid_rows")[0][0][2, 6] == 3.0


def test_empty_frame_and_empty_stream():
    _check("empty_frame", [([1, 2], [0, 1], [T_, T_]), ([], [], [L_, L_]), ([1, 2], [0, 1], [T_, T_])])
    _check("empty_stream", [([], [], [])] * 5)
    snap = _directed("empty_stream")[-1][1]
    assert snap["frame"] == 5 and snap["next_id"] == 1


# ---- certification of the random scenes --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random(name, cls=R.StreamTracker, margins=True):
    args, kw = R.RANDOM_SCENES[name]
    frames = R.random_scene(**args)
    res, m = R.run_scene(frames, margins=margins, cls=cls, **kw)
    return frames, res, m


@pytest.mark.parametrize("name", sorted(R.RANDOM_SCENES))
def test_random_scenes_certify_on_every_frame(name):
    frames, res, margins = _random(name)
    rule = R.CERT_FACTOR * R.delta(frames)
    print(f"{name}: rule {rule:.3e}, smallest margin {min(margins):.3e}")
    assert 0 < rule < 2e-3
    assert all(m >= rule for m in margins), (rule, min(margins), int(np.argmin(margins)))
    snap = res[-1][1]
    assert snap["next_id"] > len(res[0][0]) + 10 and (snap["state"] >= LOST).any()  # births and losses happen
    if name == "small64":
        assert snap["overflow"] > 0  # capacity pressure
    if name == "big280":
        assert (snap["state"] != FREE).sum() > 256  # more tracks than lanes in a workgroup


# ---- mutations ---------------------------------------------------------------------------------------------------------
class Greedy(R.StreamTracker):
    def _assign(self, cost, thresh):
        return R.greedy_assign(cost, thresh)


class FuseSecond(R.StreamTracker):
    def _fuse_second(self):
        return True


class PredictUnconfirmed(R.StreamTracker):
    def _predicted(self, pool, unconfirmed):
        return pool + unconfirmed


class KeepVh(R.StreamTracker):
    def _zero_vh(self, slot):
        return False


class ExpireNow(R.StreamTracker):
    def _expired_drop_now(self):
        return True


def _differs(cls):
    """The scenes in which the mutated tracker's ids or states differ from the restatement's."""
    bad = []
    for name in R.directed_scenes():
        if R.summary(_directed(name, cls)) != R.summary(_directed(name)):
            bad.append(name)
    for name in ("small64", "crowd80"):
        if R.summary(_random(name, cls, False)[1]) != R.summary(_random(name)[1]):
            bad.append(name)
    return bad


@pytest.mark.parametrize("cls", [Greedy, FuseSecond, PredictUnconfirmed, KeepVh, ExpireNow])
def test_mutations_change_ids_or_states(cls):
    bad = _differs(cls)
    print(cls.__name__, bad)
    assert bad, f"{cls.__name__}: no scene notices"
    if cls is ExpireNow:
        assert "q4_q5_resurrect" in bad
    if cls is KeepVh:
        assert "q1_height_velocity" in bad
    if cls is Greedy:
        assert "assign_swap" in bad and "crowd80" in bad


# ---- the product's host class ------------------------------------------------------------------------------------------
def test_host_tracker_runs_the_same_steps(tmp_path):
    import torch

    from yolosod_amd.engine.tracker import ByteTracker, ByteTrackerHost
    frames, kw = R.directed_scenes()["q4_q5_resurrect"]
    host = ByteTrackerHost(streams=2, capacity=64, **kw)
    ref = _directed("q4_q5_resurrect")
    for (rows, n), (out, _) in zip(frames, ref):
        tr = host.update(torch.from_numpy(np.stack([rows, rows])), torch.tensor([n, 0], dtype=torch.int32))
        assert tuple(tr.rows.shape) == (2, 64, 8) and tr.counts.tolist() == [len(out), 0]
        assert np.array_equal(tr.rows[0, :len(out)].numpy(), out) and not tr.rows[0, len(out):].any()
    host.reset(streams=[0])
    assert host.trackers[0].frame == 0 and host.trackers[1].frame == len(frames) and host.overflow.tolist() == [0, 0]
    y = tmp_path / "bytetrack.yaml"
    y.write_text("tracker_type: bytetrack\ntrack_high_thresh: 0.3\ntrack_low_thresh: 0.05\nnew_track_thresh: 0.4\n"
                 "track_buffer: 12\nmatch_thresh: 0.7\nfuse_score: False\n")
    h = ByteTrackerHost.from_yaml(y, streams=1)
    assert h.params.tolist() == [np.float32(v) for v in (0.3, 0.05, 0.4, 0.7, 0.5, 0.7, 12, 0)]
    y.write_text("tracker_type: botsort\ngmc_method: sparseOptFlow\n")
    with pytest.raises(NotImplementedError, match="ByteTrack"):
        ByteTrackerHost.from_yaml(y, streams=1)
    with pytest.raises(RuntimeError, match="GPU"):
        ByteTracker(streams=1, device="cpu")
