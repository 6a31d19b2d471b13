"""GPU: the HIP ByteTrack kernel (csrc/track.hip, engine.tracker.ByteTracker) against the restatement
(yolosod_amd.utils.bytetrack), frame by frame: n_tracks, ids, idx, cls and scores equal; the per-slot state and the
frame / id / overflow counters equal; boxes within one fp32 ulp of the restatement's fp32 rows (both sides are fp64
underneath, so only a rounding flip can remain); the fp64 means within 1e-9 relative. The random scenes are the ones
tests/test_bytetrack_cpu.py certifies (every decision margin >= 32 delta), so exact equality is owed."""
import functools

import numpy as np
import pytest
import torch

import bytetrack_ref as R
from yolosod_amd import _hip
from yolosod_amd.engine.tracker import ByteTracker, ByteTrackerHost, Tracked
from yolosod_amd.utils import bytetrack as bt

pytestmark = pytest.mark.gpu

MEAN_TOL = 1e-9
_worst = {"mean": 0.0}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(frames, tracker arguments, capacity, reference results) of a directed or random scene; computed once."""
    if name in R.RANDOM_SCENES:
        args, kw = R.RANDOM_SCENES[name]
        frames = R.random_scene(**args)
        kw = dict(kw)
        T = kw.pop("capacity")
    else:
        frames, kw = R.directed_scenes()[name]
        T = 64
    res, _ = R.run_scene(frames, capacity=T, **kw)
    return frames, kw, T, res


def _upload(frames_at_f, dev):
    out = torch.from_numpy(np.stack([r for r, _ in frames_at_f])).to(dev)
    counts = torch.tensor([n for _, n in frames_at_f], dtype=torch.int32, device=dev)
    return out, counts


def _compare(what, rows, n, st, ref_out, ref):
    assert n == len(ref_out), (what, "n_tracks", n, len(ref_out))
    got = rows[:n]
    for col, name in ((4, "ids"), (5, "scores"), (6, "cls"), (7, "idx")):
        assert np.array_equal(got[:, col], ref_out[:, col]), (what, name, got[:, col], ref_out[:, col])
    ulp = np.spacing(np.maximum(np.abs(got[:, :4]), np.abs(ref_out[:, :4])).astype(np.float32))
    assert (np.abs(got[:, :4].astype(np.float64) - ref_out[:, :4]) <= ulp).all(), (what, "boxes")
    assert not rows[n:].any(), (what, "padding rows")
    assert (st["frame"], st["next_id"], st["overflow"]) == (ref["frame"], ref["next_id"], ref["overflow"]), (what, "counters")
    assert np.array_equal(st["state"], ref["state"]), (what, "states", st["state"], ref["state"])
    live = ref["state"] != R.FREE
    for k in ("flags", "tid", "start", "last", "idx", "score", "cls"):
        assert np.array_equal(st[k][live], ref[k][live]), (what, k)
    if live.any():
        scale = np.abs(ref["mean"][live]).max(axis=1, keepdims=True)
        err = float((np.abs(st["mean"][live] - ref["mean"][live]) / scale).max())
        _worst["mean"] = max(_worst["mean"], err)
        assert err <= MEAN_TOL, (what, "means", err)


def _run_and_compare(name, cuda):
    frames, kw, T, res = _scene(name)
    trk = ByteTracker(streams=1, capacity=T, device=cuda, **kw)
    for f, (fr, (ref_out, ref)) in enumerate(zip(frames, res), 1):
        out, counts = _upload([fr], cuda)
        tr = trk.update(out, counts)
        _compare(f"{name} frame {f}", tr.rows[0].cpu().numpy(), int(tr.counts[0]), trk.fetch_state()[0], ref_out, ref)
    last = _hip.track_last_launch()
    assert (last["T"], last["D"], last["B"], last["layout"], last["lanes"]) == (T, frames[0][0].shape[0], 1, 1, 256)
    print(f"{name}: largest relative difference of the fp64 means so far {_worst['mean']:.3e}")


@pytest.mark.parametrize("name", sorted(R.directed_scenes()))
def test_directed_scenes(cuda, name):
    _run_and_compare(name, cuda)


@pytest.mark.parametrize("name", ["small64", "mid150", "crowd80", "big280"])
def test_certified_random_scenes(cuda, name):
    """small64: capacity pressure, one wavefront of tracks; mid150 / crowd80 (T 256, D 300): tracks and detections cross
    the 64-lane boundary, the crowd gives real augmenting paths; big280 (T 320): more tracks than lanes."""
    _run_and_compare(name, cuda)


def _padded(name, n):
    frames = list(_scene(name)[0])[:n]
    return frames + [R.pad([])] * (n - len(frames))


def test_batch_streams_are_independent_and_reset_is_per_stream(cuda):
    names, n = ("q1_refind", "empty_stream", "q4_q5_resurrect"), 9
    kw = dict(track_buffer=2)
    scenes = [_padded(k, n) for k in names]
    alone = []
    for s in scenes:
        t = ByteTracker(streams=1, capacity=64, device=cuda, **kw)
        per = []
        for fr in s:
            tr = t.update(*_upload([fr], cuda))
            per.append((tr.rows[0].cpu().numpy().copy(), int(tr.counts[0]), t.fetch_state()[0]["raw"].copy()))
        alone.append(per)
    t = ByteTracker(streams=3, capacity=64, device=cuda, **kw)
    fresh = t.fetch_state()[1]["raw"].copy()
    for f in range(n):
        tr = t.update(*_upload([s[f] for s in scenes], cuda))
        rows, cnt, st = tr.rows.cpu().numpy(), tr.counts.cpu().numpy(), t.fetch_state()
        for b in range(3):
            assert cnt[b] == alone[b][f][1]
            assert rows[b].tobytes() == alone[b][f][0].tobytes(), (names[b], f, "rows")
            assert st[b]["raw"].tobytes() == alone[b][f][2].tobytes(), (names[b], f, "state bytes")
    assert max(a[1] for a in alone[0]) == 2 and max(a[1] for a in alone[1]) == 0 and int(cnt[2]) == 2
    assert st[1]["frame"] == n and st[1]["next_id"] == 1
    before = [s["raw"].copy() for s in st]
    t.reset(streams=[1])
    after = t.fetch_state()
    assert after[1]["raw"].tobytes() == fresh.tobytes() and after[1]["frame"] == 0 and after[1]["next_id"] == 1
    assert after[0]["raw"].tobytes() == before[0].tobytes() and after[2]["raw"].tobytes() == before[2].tobytes()
    t.reset()
    assert all(s["raw"].tobytes() == fresh.tobytes() for s in t.fetch_state())


def test_invalid_detections_leave_the_other_tracks_bit_identical(cuda):
    frames = _scene("invalid_rows")[0]
    clean = [R.pad([tuple(r) for r in rows[:n][[0, 2, 6]]]) for rows, n in frames]
    runs = []
    for fr in (frames, clean):
        t = ByteTracker(streams=1, capacity=64, device=cuda)
        per = []
        for x in fr:
            tr = t.update(*_upload([x], cuda))
            per.append((tr.rows[0].cpu().numpy().copy(), int(tr.counts[0]), t.fetch_state()[0]))
        runs.append(per)
    for (ra, na, sa), (rb, nb, sb) in zip(*runs):
        assert na == nb == 3
        assert ra[:, :7].tobytes() == rb[:, :7].tobytes()
        assert ra[:3, 7].tolist() == [0, 2, 6] and rb[:3, 7].tolist() == [0, 1, 2]
        for k in ("mean", "cov", "state", "flags", "tid", "score", "cls", "start", "last"):
            assert sa[k].tobytes() == sb[k].tobytes(), k


def test_refusals_before_launch_and_report_hook(cuda):
    lib = _hip.load_library()
    T, D = 64, 16
    t = ByteTracker(streams=1, capacity=T, device=cuda)
    out, counts = _upload([R.pad([R.box(100.0)])], cuda)
    t.update(out, counts)
    assert _hip.track_last_launch() == dict(T=T, D=D, B=1, layout=1, lanes=256,
                                            workspace_per_stream=(T * D * 4 + T * 16 + D * 16 + 255) // 256 * 256)
    assert lib.yolosod_track_workspace(1, T, D) == _hip.track_last_launch()["workspace_per_stream"]
    frame = t.fetch_state()[0]["frame"]
    prm = np.ascontiguousarray(t.params)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=cuda)
    rows, n = torch.empty(1, 128, 8, device=cuda), torch.empty(1, dtype=torch.int32, device=cuda)
    state100 = torch.zeros(1, int(lib.yolosod_track_state_bytes(128)), dtype=torch.uint8, device=cuda)
    rc = lib.yolosod_track_update(state100.data_ptr(), 1, 100, out.data_ptr(), counts.data_ptr(), D, prm.ctypes.data,
                                  rows.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"T=100" in lib.yolosod_last_error()
    rc = lib.yolosod_track_update(t.state.data_ptr(), 1, T, out.data_ptr(), counts.data_ptr(), 2000, prm.ctypes.data,
                                  rows.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"D=2000" in lib.yolosod_last_error()
    rc = lib.yolosod_track_update(t.state.data_ptr(), 0, T, out.data_ptr(), counts.data_ptr(), D, prm.ctypes.data,
                                  rows.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"B=0" in lib.yolosod_last_error()
    with pytest.raises(RuntimeError, match="T 100"):
        _hip.track_update(t.state, 100, out, counts, t.params)
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.track_update(t.state, T, torch.zeros(1, 2000, 6, device=cuda), counts, t.params)
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.track_update(t.state, T, out.cpu(), counts, t.params)
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.track_update(t.state.cpu(), T, out, counts, t.params)
    with pytest.raises(RuntimeError, match="expected torch.int32"):
        _hip.track_update(t.state, T, out, counts.long(), t.params)
    with pytest.raises(ValueError, match="capacity"):
        ByteTracker(streams=1, capacity=100, device=cuda)
    with pytest.raises(ValueError, match="streams"):
        t.update(torch.zeros(2, D, 6, device=cuda), torch.zeros(2, dtype=torch.int32, device=cuda))
    torch.cuda.synchronize()
    assert t.fetch_state()[0]["frame"] == frame  # nothing was launched by the refused calls
    assert _hip.track_last_launch()["D"] == D


def test_update_does_not_sync_the_host(cuda):
    frames = _scene("q4_q5_resurrect")[0] + _scene("q1_refind")[0][:1]
    assert len(frames) == 10
    ups = [_upload([fr], cuda) for fr in frames]
    t = ByteTracker(streams=1, capacity=64, device=cuda, track_buffer=2)
    t.update(*ups[0])  # the first call allocates the workspace
    t.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for out, counts in ups:
            tr = t.update(out, counts)
        ov = t.overflow
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(tr.counts[0]) >= 1 and int(ov[0]) == 0 and t.fetch_state()[0]["frame"] == 10


def test_host_tracker_has_the_same_interface_and_results(cuda):
    frames = _scene("q2_low_score")[0]
    dev, host = ByteTracker(streams=2, capacity=64, device=cuda), ByteTrackerHost(streams=2, capacity=64)
    for fr in frames:
        out, counts = _upload([fr, fr], cuda)
        a, b = dev.update(out, counts), host.update(out, counts)
        assert a.counts.cpu().tolist() == b.counts.tolist()
        ra, rb = a.rows.cpu().numpy(), b.rows.numpy()
        assert np.array_equal(ra[..., 4:], rb[..., 4:]) and np.abs(ra[..., :4] - rb[..., :4]).max() <= 1e-4
    assert dev.overflow.cpu().tolist() == host.overflow.tolist() == [0, 0]


class _Canned:
    """A predictor's predict_padded with canned rows: track_padded / track are plumbing over it."""

    def __init__(self, frames, dev):
        self.frames, self.dev, self.f = frames, dev, 0

    def __call__(self, batch):
        out, counts = _upload([self.frames[self.f]] * len(batch), self.dev)
        self.f += 1
        index = torch.arange(out.shape[1], dtype=torch.int32, device=self.dev).repeat(len(batch), 1) + 1000
        return out, counts, index


@pytest.mark.parametrize("kind", ["detection", "sliced"])
def test_predictors_track(cuda, kind):
    from yolosod_amd.engine import predictor as P
    cls = P.DetectionPredictor if kind == "detection" else P.SlicedPredictor
    p = cls.__new__(cls)  # no model: predict_padded is canned
    p.tracker = ByteTracker(streams=2, capacity=64, device=cuda)
    p.predict_padded = _Canned(_scene("q1_refind")[0], cuda)
    batch = [np.zeros((480, 640, 3), dtype=np.uint8)] * 2
    rows, n_tracks, out, counts, index = p.track_padded(batch)
    assert tuple(rows.shape) == (2, 64, 8) and n_tracks.cpu().tolist() == [2, 2]
    res = p.track(batch)
    assert len(res) == 2 and all(isinstance(r, Tracked) for r in res)
    for r in res:
        assert tuple(r.boxes.shape) == (2, 7) and r.boxes[:, 4].cpu().tolist() == [1.0, 2.0]
        assert r.index.cpu().tolist() == [1000, 1001] and r.orig_shape == (480, 640)
    with pytest.raises(ValueError, match="streams"):
        p.track_padded(batch[:1])
    p.tracker = None
    with pytest.raises(RuntimeError, match="tracker"):
        p.track_padded(batch)
