"""GPU: the XYWH instantiation of the HIP tracker kernel with its camera-motion phase (csrc/track.hip,
engine.tracker.BotSortTracker) against the restatement (yolosod_amd.utils.botsort), frame by frame: n_tracks, ids, idx,
cls and scores equal; the per-slot state and the frame / id / overflow / bad_warp counters equal; boxes within one fp32
ulp of the restatement's fp32 rows; the fp64 means within 1e-9 relative (DESIGN section 34's bound). The random scenes
are the ones tests/test_botsort_cpu.py certifies (every decision margin >= 32 delta), so exact equality is owed."""
import functools

import numpy as np
import pytest
import torch

import botsort_ref as B
import bytetrack_ref as R
from yolosod_amd import _hip
from yolosod_amd.engine.tracker import (BotSortTracker, BotSortTrackerHost, ByteTracker, Tracked, tracker_from_yaml)

pytestmark = pytest.mark.gpu

MEAN_TOL = 1e-9
_worst = {"mean": 0.0}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(frames, warps, tracker arguments, capacity, reference results) of a directed or random scene; computed once."""
    if name in B.RANDOM_SCENES:
        args, kw = B.RANDOM_SCENES[name]
        frames, warps = B.camera_scene(**args)
        kw = dict(kw)
        T = kw.pop("capacity")
    else:
        frames, warps, kw = B.directed_scenes()[name]
        T = 64
    warps = [None] * len(frames) if warps is None else list(warps)
    res, _ = B.run(frames, warps, capacity=T, **kw)
    return frames, warps, kw, T, res


def _upload(frames_at_f, dev):
    out = torch.from_numpy(np.stack([r for r, _ in frames_at_f])).to(dev)
    counts = torch.tensor([n for _, n in frames_at_f], dtype=torch.int32, device=dev)
    return out, counts


def _warps(ws, dev):
    """Per-stream warps of one frame -> a device tensor [B, 2, 3] fp64, or None when no stream has one (a stream
    without one among streams that have one gets the identity)."""
    if all(w is None for w in ws):
        return None
    return torch.from_numpy(np.stack([B.IDENTITY if w is None else w for w in ws])).to(dev)


def _compare(what, rows, n, st, ref_out, ref):
    assert n == len(ref_out), (what, "n_tracks", n, len(ref_out))
    got = rows[:n]
    for col, name in ((4, "ids"), (5, "scores"), (6, "cls"), (7, "idx")):
        assert np.array_equal(got[:, col], ref_out[:, col]), (what, name, got[:, col], ref_out[:, col])
    ulp = np.spacing(np.maximum(np.abs(got[:, :4]), np.abs(ref_out[:, :4])).astype(np.float32))
    assert (np.abs(got[:, :4].astype(np.float64) - ref_out[:, :4]) <= ulp).all(), (what, "boxes")
    assert not rows[n:].any(), (what, "padding rows")
    assert (st["frame"], st["next_id"], st["overflow"], st["bad_warp"]) == (ref["frame"], ref["next_id"], ref["overflow"],
                                                                           ref["bad_warp"]), (what, "counters")
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
    frames, warps, kw, T, res = _scene(name)
    trk = BotSortTracker(streams=1, capacity=T, device=cuda, **kw)
    for f, (fr, w, (ref_out, ref)) in enumerate(zip(frames, warps, res), 1):
        out, counts = _upload([fr], cuda)
        tr = trk.update(out, counts, warps=_warps([w], cuda))
        _compare(f"{name} frame {f}", tr.rows[0].cpu().numpy(), int(tr.counts[0]), trk.fetch_state()[0], ref_out, ref)
    last = _hip.track_last_launch()
    assert (last["T"], last["D"], last["B"], last["layout"], last["lanes"]) == (T, frames[0][0].shape[0], 1, 1, 256)
    assert _hip.track_last_model() == dict(model=1, warps=int(warps[-1] is not None))
    print(f"{name}: largest relative difference of the fp64 means so far {_worst['mean']:.3e}")


@pytest.mark.parametrize("name", sorted(B.directed_scenes()))
def test_directed_scenes(cuda, name):
    _run_and_compare(name, cuda)


@pytest.mark.parametrize("name", ["small64", "mid150", "crowd80", "big280"])
def test_certified_random_scenes(cuda, name):
    """small64: capacity pressure, one wavefront of tracks; mid150 / crowd80 (T 256, D 300): tracks and detections cross
    the 64-lane boundary; big280 (T 320): more tracks than lanes, so a lane warps two slots."""
    _run_and_compare(name, cuda)


def _padded(name, n):
    frames, warps = _scene(name)[:2]
    frames, warps = list(frames)[:n], list(warps)[:n]
    return frames + [R.pad([])] * (n - len(frames)), warps + [None] * (n - len(warps))


def _alone(frames, warps, cuda, **kw):
    """Per frame (rows, count, state bytes) of one stream run alone. In a batch a stream without a warp among streams
    that have one is given the identity, so the run alone gets the same."""
    t = BotSortTracker(streams=1, capacity=64, device=cuda, **kw)
    per = []
    for fr, w in zip(frames, warps):
        wt = torch.from_numpy((B.IDENTITY if w is None else w)[None]).to(cuda)
        tr = t.update(*_upload([fr], cuda), warps=wt)
        per.append((tr.rows[0].cpu().numpy().copy(), int(tr.counts[0]), t.fetch_state()[0]["raw"].copy()))
    return per


def test_batch_streams_are_independent_and_reset_is_per_stream(cuda):
    """B = 3: a different warp per stream - the pan, the identity throughout, an empty stream under the zoom."""
    n = 6
    f0, w0 = _padded("b3_pan", n)
    f1, _ = _padded("identity_warps", n)
    w1 = [B.IDENTITY] * n
    f2, w2 = [R.pad([])] * n, _padded("b3_zoom_rotation", n)[1]
    scenes, warps = [f0, f1, f2], [w0, w1, w2]
    alone = [_alone(s, w, cuda) for s, w in zip(scenes, warps)]
    t = BotSortTracker(streams=3, capacity=64, device=cuda)
    fresh = t.fetch_state()[1]["raw"].copy()
    for f in range(n):
        tr = t.update(*_upload([s[f] for s in scenes], cuda), warps=_warps([w[f] for w in warps], cuda))
        rows, cnt, st = tr.rows.cpu().numpy(), tr.counts.cpu().numpy(), t.fetch_state()
        for b in range(3):
            assert cnt[b] == alone[b][f][1]
            assert rows[b].tobytes() == alone[b][f][0].tobytes(), (b, f, "rows")
            assert st[b]["raw"].tobytes() == alone[b][f][2].tobytes(), (b, f, "state bytes")
    assert cnt.tolist() == [2, 3, 0] and st[2]["frame"] == n and st[2]["next_id"] == 1
    assert t.bad_warp.cpu().tolist() == [0, 0, 0]
    before = [s["raw"].copy() for s in st]
    t.reset(streams=[1])
    after = t.fetch_state()
    assert after[1]["raw"].tobytes() == fresh.tobytes() and after[1]["frame"] == 0 and after[1]["next_id"] == 1
    assert after[0]["raw"].tobytes() == before[0].tobytes() and after[2]["raw"].tobytes() == before[2].tobytes()
    t.reset()
    assert all(s["raw"].tobytes() == fresh.tobytes() for s in t.fetch_state())


def test_a_bytetracker_beside_a_botsort_tracker_is_bit_identical(cuda):
    frames = R.directed_scenes()["q4_q5_resurrect"][0]
    bframes, bwarps = _padded("b3_pan", len(frames))

    def run(with_other):
        t = ByteTracker(streams=1, capacity=64, device=cuda, track_buffer=2)
        other = BotSortTracker(streams=1, capacity=64, device=cuda) if with_other else None
        per = []
        for f, fr in enumerate(frames):
            tr = t.update(*_upload([fr], cuda))
            per.append((tr.rows[0].cpu().numpy().copy(), int(tr.counts[0]), t.fetch_state()[0]["raw"].copy()))
            if other is not None:
                other.update(*_upload([bframes[f]], cuda), warps=_warps([bwarps[f]], cuda))
                assert _hip.track_last_model()["model"] == 1
        return per, other
    (a, _), (b, other) = run(False), run(True)
    for f, ((ra, na, sa), (rb, nb, sb)) in enumerate(zip(a, b)):
        assert na == nb and ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes(), f
    assert sa[:64].view(np.int32)[3] == 0  # ByteTrack never touches the fourth header word
    assert int(other.fetch_state()[0]["frame"]) == len(frames)


def test_a_nan_warp_is_skipped_for_its_stream_only(cuda):
    n = 6
    f0, w0 = _padded("b3_pan", n)
    scenes, warps = [f0, f0, f0], [list(w0), list(w0), list(w0)]
    ref = _alone(f0, w0, cuda)
    bad = B.similarity(40.0)
    bad[0, 1] = np.nan
    warps[1][3] = bad  # frame 4 of stream 1
    t = BotSortTracker(streams=3, capacity=64, device=cuda)
    for f in range(n):
        tr = t.update(*_upload([s[f] for s in scenes], cuda), warps=_warps([w[f] for w in warps], cuda))
        rows, st = tr.rows.cpu().numpy(), t.fetch_state()
        for b in (0, 2):
            assert rows[b].tobytes() == ref[f][0].tobytes() and st[b]["raw"].tobytes() == ref[f][2].tobytes(), (b, f)
        assert t.bad_warp.cpu().tolist() == [0, int(f >= 3), 0]
        assert st[1]["bad_warp"] == int(f >= 3)
    # stream 1: both tracks lost at frame 4, that frame's births confirmed at frame 5
    assert int(tr.counts[1]) == 2 and rows[1, :2, 4].tolist() == [3.0, 4.0]
    host = BotSortTrackerHost(streams=1, capacity=64)
    for f in range(n):
        w = warps[1][f]
        hr = host.update(scenes[1][f][0][None], np.array([scenes[1][f][1]]), warps=None if w is None else w[None])
    assert hr.counts.tolist() == [2] and np.array_equal(hr.rows[0, :2, 4:].numpy(), rows[1, :2, 4:])


def test_refusals_before_launch_and_report_hook(cuda):
    lib = _hip.load_library()
    T, D = 64, 16
    t = BotSortTracker(streams=1, capacity=T, device=cuda)
    out, counts = _upload([R.pad([R.box(100.0)])], cuda)
    ident = torch.from_numpy(B.IDENTITY[None].copy()).to(cuda)
    # the report hook after each kind of launch
    t.update(out, counts)
    assert _hip.track_last_model() == dict(model=1, warps=0)
    t.update(out, counts, warps=ident)
    assert _hip.track_last_model() == dict(model=1, warps=1)
    assert _hip.track_last_launch() == dict(T=T, D=D, B=1, layout=1, lanes=256,
                                            workspace_per_stream=(T * D * 4 + T * 16 + D * 16 + 255) // 256 * 256)
    byte = ByteTracker(streams=1, capacity=T, device=cuda)
    byte.update(out, counts)
    assert _hip.track_last_model() == dict(model=0, warps=0)
    assert [lib.yolosod_debug_track_last(i) for i in (6, 7, 8, -1)] == [0, 0, -1, -1]
    prm = np.ascontiguousarray(t.params)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=cuda)
    rows, n = torch.empty(1, 128, 8, device=cuda), torch.empty(1, dtype=torch.int32, device=cuda)
    ex = lib.yolosod_track_update_ex
    frame = t.fetch_state()[0]["frame"]

    def refused(needle, state=None, T_=T, B_=1, D_=D, model=1, warps=ident.data_ptr(), params=prm, ws_bytes=None):
        rc = ex((t.state if state is None else state).data_ptr(), B_, T_, out.data_ptr(), counts.data_ptr(), D_,
                params.ctypes.data, model, warps, rows.data_ptr(), n.data_ptr(), ws.data_ptr(),
                ws.numel() if ws_bytes is None else ws_bytes, None)
        err = lib.yolosod_last_error()
        assert rc != 0 and needle in err, (needle, rc, err)
    refused(b"model=2", model=2)
    refused(b"model=-1", model=-1)
    refused(b"warps with model 0", model=0)
    refused(b"misaligned warps", warps=ident.data_ptr() + 4)
    # everything yolosod_track_update refuses
    state128 = torch.zeros(1, int(lib.yolosod_track_state_bytes(128)), dtype=torch.uint8, device=cuda)
    refused(b"T=100", state=state128, T_=100)
    refused(b"D=2000", D_=2000)
    refused(b"B=0", B_=0)
    refused(b"workspace", ws_bytes=16)
    bad_prm = prm.copy()
    bad_prm[3] = np.nan
    refused(b"params[3]", params=bad_prm)
    rc = ex(None, 1, T, out.data_ptr(), counts.data_ptr(), D, prm.ctypes.data, 1, None, rows.data_ptr(), n.data_ptr(),
            ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"null pointer" in lib.yolosod_last_error()
    rc = ex(t.state.data_ptr() + 4, 1, T, out.data_ptr(), counts.data_ptr(), D, prm.ctypes.data, 1, None, rows.data_ptr(),
            n.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"misaligned pointer" in lib.yolosod_last_error()
    # the wrapper and the classes
    with pytest.raises(RuntimeError, match="model"):
        _hip.track_update(t.state, T, out, counts, t.params, model="xyzw")
    with pytest.raises(RuntimeError, match="warps with model"):
        _hip.track_update(t.state, T, out, counts, t.params, warps=ident)
    with pytest.raises(RuntimeError, match="expected torch.float64"):
        _hip.track_update(t.state, T, out, counts, t.params, model="xywh", warps=ident.float())
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.track_update(t.state, T, out, counts, t.params, model="xywh", warps=ident.cpu())
    with pytest.raises(RuntimeError, match=r"\[1, 2, 3\]"):
        _hip.track_update(t.state, T, out, counts, t.params, model="xywh", warps=ident[:, :, :2].contiguous())
    with pytest.raises(ValueError, match="warps"):
        t.update(out, counts, warps=torch.zeros(2, 2, 3, device=cuda))
    with pytest.raises(ValueError, match="warps"):
        t.update(out, counts, warps=torch.zeros(1, 3, 3, device=cuda))
    with pytest.raises((TypeError, ValueError), match="warps"):
        byte.update(out, counts, warps=ident)
    with pytest.raises(NotImplementedError, match="with_reid"):
        BotSortTracker(streams=1, capacity=T, device=cuda, with_reid=True)
    torch.cuda.synchronize()
    assert t.fetch_state()[0]["frame"] == frame  # nothing was launched by the refused calls
    assert _hip.track_last_model() == dict(model=0, warps=0)  # still the ByteTracker's launch above, the last one made


def test_update_with_device_warps_does_not_sync_the_host(cuda):
    frames, warps = _padded("b3_pan", 10)
    ups = [_upload([fr], cuda) for fr in frames]
    w32 = [torch.from_numpy((B.IDENTITY if w is None else w)[None].astype(np.float32 if f % 2 else np.float64)).to(cuda)
           for f, w in enumerate(warps)]  # fp32 and fp64, both moved to fp64 on the device
    t = BotSortTracker(streams=1, capacity=64, device=cuda)
    t.update(*ups[0], warps=w32[0])  # the first call allocates the workspace
    t.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for (out, counts), w in zip(ups, w32):
            tr = t.update(out, counts, warps=w)
        ov, bw = t.overflow, t.bad_warp
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(tr.counts[0]) == 0 and int(ov[0]) == 0 and int(bw[0]) == 0 and t.fetch_state()[0]["frame"] == 10
    assert t.fetch_state()[0]["next_id"] == 3  # ids 1 and 2 through the pan (the padding frames lose them)


def test_host_tracker_has_the_same_interface_and_results(cuda, tmp_path):
    frames, warps = _scene("b3_zoom_rotation")[:2]
    y = tmp_path / "botsort.yaml"
    y.write_text("tracker_type: botsort\ngmc_method: sparseOptFlow\nwith_reid: False\n")
    dev = tracker_from_yaml(y, streams=2, device=cuda, capacity=64)
    host = tracker_from_yaml(y, streams=2, device="cpu", capacity=64)
    assert type(dev) is BotSortTracker and type(host) is BotSortTrackerHost and dev.gmc_method == "sparseOptFlow"
    for fr, w in zip(frames, warps):
        out, counts = _upload([fr, fr], cuda)
        ws = None if w is None else torch.from_numpy(np.stack([w, B.IDENTITY])).to(cuda)
        a, b = dev.update(out, counts, warps=ws), host.update(out, counts, warps=None if ws is None else ws.cpu())
        assert a.counts.cpu().tolist() == b.counts.tolist()
        ra, rb = a.rows.cpu().numpy(), b.rows.numpy()
        assert np.array_equal(ra[..., 4:], rb[..., 4:]) and np.abs(ra[..., :4] - rb[..., :4]).max() <= 1e-4
    # without the zoom's warp only the box at the centre keeps its id; the other two are born again
    assert a.counts.cpu().tolist() == [3, 3]
    assert ra[0, :3, 4].tolist() == [1.0, 2.0, 3.0] and ra[1, :3, 4].tolist() == [3.0, 4.0, 5.0]
    assert dev.overflow.cpu().tolist() == host.overflow.tolist() == [0, 0]
    assert dev.bad_warp.cpu().tolist() == host.bad_warp.tolist() == [0, 0]


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
def test_predictors_track_with_warps(cuda, kind):
    from yolosod_amd.engine import predictor as P
    cls = P.DetectionPredictor if kind == "detection" else P.SlicedPredictor
    frames, warps = _scene("b3_pan")[:2]
    p = cls.__new__(cls)  # no model: predict_padded is canned
    p.tracker = BotSortTracker(streams=2, capacity=64, device=cuda)
    p.predict_padded = _Canned(frames, cuda)
    batch = [np.zeros((48, 64, 3), dtype=np.uint8)] * 2
    for f, w in enumerate(warps[:4]):  # stream 0 gets the warps, stream 1 the identity: it loses its tracks at frame 3
        ws = None if w is None else np.stack([w, B.IDENTITY]).astype(np.float32)
        if f % 2:
            rows, n_tracks, out, counts, index = p.track_padded(batch, warps=ws)
        else:
            rows, n_tracks, *_ = p.track_padded(batch) if ws is None else p.track_padded(batch, ws)
        assert tuple(rows.shape) == (2, 64, 8)
    assert n_tracks.cpu().tolist() == [2, 0]
    res = p.track(batch, warps=torch.from_numpy(np.stack([warps[4], B.IDENTITY])).to(cuda))
    assert len(res) == 2 and all(isinstance(r, Tracked) for r in res)
    assert tuple(res[0].boxes.shape) == (2, 7) and res[0].boxes[:, 4].cpu().tolist() == [1.0, 2.0]
    assert res[0].index.cpu().tolist() == [1000, 1001] and res[0].orig_shape == (48, 64)
    p.tracker = ByteTracker(streams=2, capacity=64, device=cuda)
    with pytest.raises(ValueError, match="ByteTrack"):
        p.track_padded(batch, warps=np.stack([B.IDENTITY] * 2))
    with pytest.raises(ValueError, match="ByteTrack"):
        p.track(batch, warps=np.stack([B.IDENTITY] * 2))
