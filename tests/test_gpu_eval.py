"""GPU: device-side validation - csrc/eval_match.hip against the reference's own tp matrix
(tests/golden/metrics_eval.npz) and against its numpy restatement (tests/eval_match_ref.py) bit for bit, and the
evaluator's padded path (update_padded / get_stats / validate) against the host path (update) on the same tensors.
Every comparison of a tp matrix is torch.equal."""
import warnings

import numpy as np
import pytest
import torch

from conftest import golden
from eval_match_ref import crowd, match_batch_ref
from yolosod_amd import _hip
from yolosod_amd.engine import validator as V
from yolosod_amd.utils.metrics import IOU_THRESHOLDS

pytestmark = pytest.mark.gpu

F32 = np.float32
CHUNK = _hip.EVAL_MATCH_LABEL_CHUNK
IOUV = IOU_THRESHOLDS.numpy()
THRESHOLDS = {1: np.array([0.5], F32), 10: IOUV, 16: np.linspace(0.2, 0.95, 16).astype(F32)}
LABEL_LOADS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]


def _launch_into(tp, out, counts, labels, label_off, iouv):
    """The C-ABI entry point on a tp tensor of the test's own (the wrapper allocates its own)."""
    lib = _hip.load_library()
    thr = np.ascontiguousarray(iouv, dtype=F32)
    B, D, T = tp.shape
    rc = _hip._launch(("match_predictions", (B, D, T), None), out.device, lib.yolosod_match_predictions,
                      out.data_ptr(), counts.data_ptr(), B, D, labels.data_ptr() if labels.shape[0] else None,
                      label_off.data_ptr(), thr.ctypes.data, T, tp.data_ptr(), _hip._stream(out.device))
    assert rc == 0, lib.yolosod_last_error()
    return tp


def _match(out, counts, targets, iouv, cuda):
    """(wrapper's tp, tp written into a tensor pre-filled with 0xFF), both on the host."""
    o = torch.from_numpy(out).to(cuda)
    c = torch.tensor(list(counts), dtype=torch.int32, device=cuda)
    labels, off = V.pack_labels(targets, cuda)
    got = _hip.match_predictions(o, c, labels, off, iouv)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (*out.shape[:2], len(iouv))
    pre = torch.full(tuple(got.shape), 0xFF, dtype=torch.uint8, device=cuda)
    _launch_into(pre, o, c, labels, off, iouv)
    return got.cpu(), pre.cpu()


def test_fixture_in_one_launch_is_the_reference_tp(cuda):
    z = golden("metrics_eval")
    gi, pi = np.cumsum(np.r_[0, z["gt_n"]]), np.cumsum(np.r_[0, z["pred_n"]])
    B, D = len(z["gt_n"]), 32
    assert B == 24 and int(z["pred_n"].max()) <= D
    targets = [(z["gt_cls"][gi[i]:gi[i + 1]], z["gt_boxes"][gi[i]:gi[i + 1]]) for i in range(B)]
    out = np.random.default_rng(3).uniform(-50, 700, (B, D, 6)).astype(F32)  # garbage in the padding rows
    out[..., 5] = np.random.default_rng(4).integers(0, 6, (B, D))
    for i in range(B):
        out[i, :z["pred_n"][i]] = z["pred"][pi[i]:pi[i + 1]]
    got, pre = _match(out, z["pred_n"], targets, IOUV, cuda)
    kept = torch.cat([got[i, :int(n)] for i, n in enumerate(z["pred_n"])])
    assert int(kept.sum()) == 619
    assert torch.equal(kept, torch.from_numpy(z["tp"].astype(np.uint8))), "differs from the reference's tp"
    assert all(not got[i, int(n):].any() for i, n in enumerate(z["pred_n"])), "a padding row is not 0"
    assert torch.equal(pre, got)


@pytest.fixture(scope="module")
def crowds():
    """33 crowds of 1024 detections; image b has LABEL_LOADS[b % 6] labels. Smaller D take the first D rows."""
    return [crowd(1000 + b, n_labels=LABEL_LOADS[b % len(LABEL_LOADS)], n_det=1024) for b in range(33)]


@pytest.mark.parametrize("D", [1, 63, 64, 65, 300, 1024])
@pytest.mark.parametrize("B", [1, 33])
def test_crowds_match_the_restatement(B, D, crowds, cuda):
    # B = 1: the image with the most labels, full; B = 33: counts of D, 0 and in between, every label load
    picks = [5] if B == 1 else list(range(33))
    between = [D, 0, (D + 1) // 2, D - 1, D, 1, D // 3]
    counts = [D] if B == 1 else [min(max(between[b % len(between)], 0), D) for b in range(B)]
    out = np.full((B, D, 6), np.nan, dtype=F32)  # padding rows: NaN
    targets = []
    for i, b in enumerate(picks):
        cls, boxes, det = crowds[b]
        out[i, :counts[i]] = det[:counts[i]]
        targets.append((cls, boxes))
    for T, iouv in THRESHOLDS.items():
        ref = torch.from_numpy(match_batch_ref(out, counts, targets, iouv))
        got, pre = _match(out, counts, targets, iouv, cuda)
        assert torch.equal(got, ref), f"T={T}: {int((got != ref).sum())} bytes differ from the restatement"
        assert torch.equal(pre, ref), f"T={T}: a byte of tp was not written (or written wrong)"
        if B == 33 and D >= 63 and T == 10:
            assert int(ref.sum()) > 100, "nothing matches: the comparison is empty"


def test_iou_exactly_at_the_threshold(cuda):
    """label (0, 0, 2, 1), detection (0, 0, 1, 1): inter 1, union 2 + 1e-7 rounds to 2 in fp32, so IoU is exactly 0.5
    and the row is a true positive at 0.5 (double arithmetic, or a > compare, says otherwise); one fp32 step shorter and
    it is not."""
    short = np.nextafter(F32(1), F32(0))
    out = np.zeros((2, 1, 6), F32)
    out[0, 0] = (0, 0, 1, 1, 0.9, 0)
    out[1, 0] = (0, 0, short, 1, 0.9, 0)
    targets = [(np.zeros(1, F32), np.array([[0, 0, 2, 1]], F32))] * 2
    for iouv in (np.array([0.5], F32), IOUV):
        got, pre = _match(out, [1, 1], targets, iouv, cuda)
        assert torch.equal(got, torch.from_numpy(match_batch_ref(out, [1, 1], targets, iouv)))
        assert got[0, 0].tolist() == [1] + [0] * (len(iouv) - 1)
        assert got[1, 0].tolist() == [0] * len(iouv)
        assert torch.equal(pre, got)


@pytest.mark.parametrize("p,q", [(1, CHUNK + 5), (1, 7), (CHUNK + 5, 1), (2 * CHUNK - 1, 2 * CHUNK)])
def test_tie_takes_the_highest_label_index(p, q, cuda):
    """Labels P = (0, 0, 10, 10) at index p and Q = (2, 0, 12, 10) at index q; row 0 = (0, 0, 10, 10.5) belongs to P
    alone, row 1 = (1, 0, 11, 10) overlaps P and Q by exactly 90 / 110. With the tie going to the higher index, row 1
    takes Q when q > p (unclaimed: a true positive up to 0.8) and P when p > q (claimed by row 0 at 0.952: nothing).
    Checked against the restatement only: numpy's order for ties is unspecified."""
    L = 2 * CHUNK + 9
    rng = np.random.default_rng(5)
    xy = rng.uniform(200, 600, (L, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(4, 40, (L, 2))], 1).astype(F32)
    boxes[p], boxes[q] = (0, 0, 10, 10), (2, 0, 12, 10)
    targets = [(np.zeros(L, F32), boxes)]
    out = np.array([[[0, 0, 10, 10.5, 0.9, 0], [1, 0, 11, 10, 0.8, 0], [0, 0, 10, 10, 0.7, 1]]], F32)
    ref = torch.from_numpy(match_batch_ref(out, [3], targets, IOUV))
    got, pre = _match(out, [3], targets, IOUV, cuda)
    assert torch.equal(got, ref) and torch.equal(pre, ref)
    assert got[0, 0].tolist() == [1] * 10                                     # 100 / 105 = 0.952
    assert got[0, 1].tolist() == ([1] * 7 + [0] * 3 if q > p else [0] * 10)   # 90 / 110 = 0.818
    assert not got[0, 2].any()                                                # another class


def test_duplicated_labels_are_claimed_once(cuda):
    """The same label three times (indices 3, CHUNK - 1 and CHUNK + 2) and twice more elsewhere: every row on it ties
    all its copies and takes the last one, so the first row claims it and the later ones find it claimed - as long as
    all rows break the tie the same way. Against the restatement only."""
    L = CHUNK + 40
    rng = np.random.default_rng(6)
    xy = rng.uniform(200, 600, (L, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(4, 40, (L, 2))], 1).astype(F32)
    boxes[[3, CHUNK - 1, CHUNK + 2]] = (10, 10, 30, 30)
    boxes[[0, CHUNK + 39]] = (100, 100, 120, 140)
    targets = [(np.zeros(L, F32), boxes)]
    out = np.array([[[10, 10, 30, 29.5, 0.9, 0], [10, 10, 30, 30, 0.8, 0], [100, 101, 120, 140, 0.7, 0],
                     [11, 10, 30, 30, 0.6, 0], [100, 100, 120, 140, 0.5, 0]]], F32)
    ref = torch.from_numpy(match_batch_ref(out, [5], targets, IOUV))
    got, pre = _match(out, [5], targets, IOUV, cuda)
    assert torch.equal(got, ref) and torch.equal(pre, ref)
    assert got[0, 0].tolist() == [1] * 10 and got[0, 2].tolist() == [1] * 10   # both 0.975: the first row claims
    assert got[0, 1].tolist() == [0] * 10 and got[0, 3].tolist() == [0] * 10   # IoU 1 and 0.95, claimed at 0.975 / 1
    assert got[0, 4].tolist() == [0] * 10                                      # IoU 1, claimed at 0.975


def test_chain_on_one_label(cuda):
    """Rows whose best label is the same one, IoU rising with the row index (0.57, 0.72, 0.92, then 0.6): the first
    counts at the thresholds it reaches, a later one exactly at the thresholds above the earlier maximum."""
    targets = [(np.zeros(1, F32), np.array([[0, 0, 20, 1]], F32))]
    out = np.array([[[0, 0, w, 1, 0.9 - 0.1 * i, 0] for i, w in enumerate((11.4, 14.4, 18.4, 12.0))]], F32)
    got, pre = _match(out, [4], targets, IOUV, cuda)
    assert torch.equal(got, torch.from_numpy(match_batch_ref(out, [4], targets, IOUV))) and torch.equal(pre, got)
    assert got[0, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert got[0, 1].tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert got[0, 2].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0]
    assert not got[0, 3].any()


def test_wrapper_refusals_launch_nothing(cuda):
    out, counts = torch.zeros(2, 8, 6, device=cuda), torch.zeros(2, dtype=torch.int32, device=cuda)
    labels, off = torch.zeros(3, 5, device=cuda), torch.zeros(3, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="float32"):
        _hip.match_predictions(out.half(), counts, labels, off)
    with pytest.raises(RuntimeError, match="int32"):
        _hip.match_predictions(out, counts.long(), labels, off)
    with pytest.raises(RuntimeError, match="contiguous"):
        _hip.match_predictions(torch.zeros(2, 6, 8, device=cuda).transpose(1, 2), counts, labels, off)
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.match_predictions(torch.zeros(2, 1025, 6, device=cuda), counts, labels, off)
    with pytest.raises(RuntimeError, match="images"):
        _hip.match_predictions(out, counts, labels, off[:2])
    with pytest.raises(RuntimeError, match="cls, x1"):
        _hip.match_predictions(out, counts, torch.zeros(3, 4, device=cuda), off)
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.match_predictions(out, counts, labels.cpu(), off)
    with pytest.raises(RuntimeError, match="thresholds"):
        _hip.match_predictions(out, counts, labels, off, [0.5, 0.0])
    with pytest.raises(RuntimeError, match="thresholds"):
        _hip.match_predictions(out, counts, labels, off, np.linspace(0.1, 0.9, 17))
    with pytest.raises(RuntimeError, match="host"):
        _hip.match_predictions(out, counts, labels, off, IOU_THRESHOLDS.to(cuda))


# ---- evaluator -----------------------------------------------------------------------------------------------------
STRIDES = [4.0, 8.0, 16.0, 32.0]


def _same_metrics(a, b):
    assert a.get_stats() == b.get_stats()
    for k in ("all_ap", "p", "r", "ap_class_index"):
        u, v = getattr(a.metrics, k), getattr(b.metrics, k)
        assert u.shape == v.shape and (u == v).all(), k
    assert a.seen == b.seen


@pytest.fixture(scope="module")
def val_batch(cuda):
    """Val-mode NMS output of synthetic Detect maps (as tests/test_gpu_map.py makes them) and labels made of jittered
    predict-mode detections plus random boxes; image 1 has no labels."""
    from yolosod_amd.utils.ops import non_max_suppression, non_max_suppression_padded
    B, img, nc = 4, 256, 10
    g = torch.Generator().manual_seed(0)
    maps = []
    for s in STRIDES:
        h = w = int(img // s)
        maps.append(torch.cat([torch.randn(B, 64, h, w, generator=g) * 2.0,
                               torch.randn(B, nc, h, w, generator=g) * 2.5 - 3.0], 1).to(cuda))
    y = _hip.detect_decode(maps, STRIDES, nc)
    predict_mode = non_max_suppression(y.clone(), conf_thres=0.25, iou_thres=0.7)  # NMS rewrites its input's boxes
    out, counts, _ = non_max_suppression_padded(y, **V.VAL_NMS)
    rng = np.random.default_rng(0)
    targets = []
    for b, d in enumerate(predict_mode):
        d = d.cpu().numpy()
        keep = d[rng.uniform(size=len(d)) < 0.6]
        m = int(rng.integers(0, 8))
        xy = rng.uniform(0, img - 30, (m, 2))
        rnd = np.concatenate([xy, xy + rng.uniform(6, 60, (m, 2))], 1)
        cls = np.concatenate([keep[:, 5], rng.integers(0, nc, m)]).astype(F32)
        boxes = np.concatenate([keep[:, :4] + rng.normal(0, 2.0, (len(keep), 4)), rnd]).astype(F32)
        targets.append((cls[:0], boxes[:0]) if b == 1 else (cls, boxes))
    return out, counts, targets, nc


def test_update_padded_scores_as_update_on_the_same_tensors(val_batch):
    out, counts, targets, nc = val_batch
    n = counts.cpu().tolist()
    assert max(n) == 300 and tuple(out.shape) == (4, 300, 6)
    slices = [out[i, :n[i]] for i in range(len(n))]
    dev, host = V.DetectionEvaluator(nc), V.DetectionEvaluator(nc)
    dev.update_padded(out, counts, targets)
    host.update(slices, targets)
    _same_metrics(dev, host)
    res = dev.get_stats()
    assert res["metrics/mAP50-95(B)"] > 0.05, res  # a non-trivial workload
    for k in host.stats:
        assert len(dev.stats[k]) == len(host.stats[k])
        assert all(u.dtype == v.dtype and np.array_equal(u, v) for u, v in zip(dev.stats[k], host.stats[k])), k


def test_an_evaluator_fed_both_ways_keeps_call_order(val_batch):
    out, counts, targets, nc = val_batch
    n = counts.cpu().tolist()
    slices = [out[i, :n[i]] for i in range(len(n))]
    mixed, host = V.DetectionEvaluator(nc), V.DetectionEvaluator(nc)
    empty = (torch.zeros(0, 6), (np.zeros(0, F32), np.zeros((0, 4), F32)))  # neither rows nor labels: leaves no entry
    mixed.update(slices[:1] + [empty[0]], targets[:1] + [empty[1]])
    mixed.update_padded(out[1:3].contiguous(), counts[1:3].contiguous(), targets[1:3])
    mixed.update(slices[3:], targets[3:])
    mixed.update_padded(out[:2].contiguous(), torch.zeros_like(counts[:2]), targets[:2])  # no rows at all
    host.update(slices[:1] + [empty[0]] + slices[1:], targets[:1] + [empty[1]] + targets[1:])
    host.update([s[:0] for s in slices[:2]], targets[:2])
    _same_metrics(mixed, host)
    for k in host.stats:
        assert all(np.array_equal(u, v) for u, v in zip(mixed.stats[k], host.stats[k])), k


class _Canned:
    """A stub predictor: predict_padded hands out tensors made beforehand."""

    def __init__(self, results):
        self.results, self.calls = list(results), 0

    def predict_padded(self, batch):
        self.calls += 1
        return self.results[batch]


class _no_sync:
    def __enter__(self):
        self.mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "prototype feature" notice
            torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.mode)
        return False


def test_update_padded_and_the_validate_loop_make_no_synchronising_call(val_batch, cuda, monkeypatch):
    out, counts, targets, nc = val_batch
    index = torch.zeros(out.shape[:2], dtype=torch.int32, device=cuda)
    results = [(out[:2].contiguous(), counts[:2].contiguous(), index[:2]),
               (out[2:].contiguous(), counts[2:].contiguous(), index[2:])]
    warm = V.DetectionEvaluator(nc)
    warm.update_padded(*results[0][:2], targets[:2])  # first use: pinned blocks and the code object are set up
    torch.cuda.synchronize()
    ev = V.DetectionEvaluator(nc)
    with _no_sync():
        ev.update_padded(*results[0][:2], targets[:2])
        ev.update_padded(*results[1][:2], targets[2:])
    # validate: the loop under the error mode, the one fetch at the end outside it
    fetched = []
    real = V.DetectionEvaluator.get_stats

    def get_stats(self):
        torch.cuda.set_sync_debug_mode(mode)
        fetched.append(self)
        return real(self)

    monkeypatch.setattr(V.DetectionEvaluator, "get_stats", get_stats)
    stub = _Canned(results)
    mode = torch.cuda.get_sync_debug_mode()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.cuda.set_sync_debug_mode("error")
        res = V.validate(stub, [(0, targets[:2]), (1, targets[2:])], nc)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    monkeypatch.undo()
    assert stub.calls == 2 and len(fetched) == 1
    host = V.DetectionEvaluator(nc)
    n = counts.cpu().tolist()
    host.update([out[i, :n[i]] for i in range(len(n))], targets)
    assert res == host.get_stats() == ev.get_stats()
    _same_metrics(ev, host)
    _same_metrics(fetched[0], host)


# ---- validate end to end ---------------------------------------------------------------------------------------------
PLANT_SHAPES = [(200, 300), (90, 150)]
PLANTED = [(60.0, 50.0, 24.0, 18.0), (140.0, 120.0, 30.0, 22.0), (250.0, 70.0, 16.0, 24.0), (100.0, 100.0, 20.0, 20.0)]


def _planted_frame(h, w, seed):
    """uint8 BGR frame: noise with one flat rectangle per planted object that fits; (frame, cls, boxes xyxy)."""
    rng = np.random.default_rng(seed)
    f = np.full((h, w, 3), 96.0) + rng.normal(0, 10, (h, w, 3))
    cls, boxes = [], []
    for j, (cx, cy, bw, bh) in enumerate(PLANTED):
        x1, y1, x2, y2 = cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2
        if x2 >= w or y2 >= h:
            continue
        f[int(y1):int(y2), int(x1):int(x2)] = rng.integers(0, 256, 3)
        cls.append(j % 3)
        boxes.append((x1, y1, x2, y2))
    return np.clip(f, 0, 255).astype(np.uint8), np.array(cls, F32), np.array(boxes, F32).reshape(-1, 4)


class _Recording:
    def __init__(self, predictor):
        self.predictor, self.seen = predictor, []

    def predict_padded(self, frames):
        res = self.predictor.predict_padded(frames)
        self.seen.append(tuple(t.clone() for t in res))
        return res


def test_validate_with_the_sliced_predictor_end_to_end(tmp_path, cuda):
    """validate() over SlicedPredictor on two small frames, labels in frame pixels; the predictor's own output is
    recorded during that run (never a second forward: MIOpen's split-K solvers are not run-to-run deterministic) and fed
    to a second evaluator through update()."""
    import re
    from yolosod_amd.engine.predictor import SlicedPredictor
    from yolosod_amd.nn.checkpoint import attempt_load_one_weight, save_checkpoint
    from yolosod_amd.nn.tasks import DetectionModel
    torch.manual_seed(0)
    m = DetectionModel("yolov12-sod-fusion-v5-simple.yaml")
    nc = m.yaml["nc"]
    shift = torch.linspace(6.0, 12.0, nc)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if re.fullmatch(r"model\.39\.cv3\.\d\.2\.bias", k):
                v.add_(shift)
    model = attempt_load_one_weight(save_checkpoint(m, tmp_path / "trained_like.pt"), device=cuda)[0]
    sp = SlicedPredictor(model, slice=128, overlap=0.25, full_frame=True, cut_margin=2.0, imgsz=128,
                         conf=V.VAL_NMS["conf_thres"], iou=V.VAL_NMS["iou_thres"], multi_label=True, max_det=300)
    planted = [_planted_frame(h, w, 70 + i) for i, (h, w) in enumerate(PLANT_SHAPES)]
    assert [len(c) for _, c, _ in planted] == [4, 1]
    batches = [([f for f, _, _ in planted], [(cls, boxes) for _, cls, boxes in planted])]  # one batch: one model shape
    rec = _Recording(sp)
    res = V.validate(rec, batches, nc)
    assert len(rec.seen) == 1 and (sp.conf, sp.iou, sp.max_det) == (0.001, 0.7, 300), "validate changed the predictor"
    host = V.DetectionEvaluator(nc)
    total = 0
    for (out, counts, _), (_, targets) in zip(rec.seen, batches):
        n = counts.cpu().tolist()
        total += sum(n)
        host.update([out[i, :n[i]] for i in range(len(n))], targets)
    assert total > 0, "nothing detected: the comparison is empty"
    assert res == host.get_stats()
    assert set(res) == set(V.DetMetrics.keys) | {"fitness"}
