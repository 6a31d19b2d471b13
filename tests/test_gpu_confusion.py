"""GPU: the device-side confusion matrix - csrc/eval_confusion.hip against the reference's own matrices
(tests/golden/confusion_eval.npz) and against its numpy restatement (tests/confusion_ref.py) cell for cell, and the
evaluator's padded path (update_padded / get_stats / validate with confusion=True) against the host path (update, the
reference's steps) on the same tensors. Every comparison of a matrix is torch.equal / ==. Every launch also writes into
a sentinel-filled buffer of the test's own whose guard words must survive, and every matrix must conserve its inputs:
column sums the labels per class, row sums the kept rows per class."""
import warnings

import numpy as np
import pytest
import torch

from confusion_ref import confusion_batch_ref, conserved, crowd, fixture_sets, iou_all, lab5
from yolosod_amd import _hip
from yolosod_amd.engine import validator as V
from yolosod_amd.utils.metrics import ConfusionMatrix

pytestmark = pytest.mark.gpu

F32 = np.float32
CHUNK = _hip.EVAL_CONFUSION_LABEL_CHUNK
MAX_NC = _hip.EVAL_CONFUSION_MAX_NC
LABEL_LOADS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
CONF, IOU = 0.25, 0.45
GUARD, SENTINEL = 64, 0x5A5A5A5A


def _launch_guarded(o, c, labels, off, nc, conf, iou):
    """The C-ABI entry point on a cm inside a larger sentinel-filled buffer: (cm, the guard words are intact)."""
    lib = _hip.load_library()
    B, D = o.shape[:2]
    cells = B * (nc + 1) * (nc + 1)
    buf = torch.full((GUARD + cells + GUARD,), SENTINEL, dtype=torch.int32, device=o.device)
    cm = buf[GUARD:GUARD + cells]
    rc = _hip._launch(("confusion_matrix", (B, D, nc), None), o.device, lib.yolosod_confusion_matrix, o.data_ptr(),
                      c.data_ptr(), B, D, labels.data_ptr() if labels.shape[0] else None, off.data_ptr(), nc,
                      float(conf), float(iou), cm.data_ptr(), _hip._stream(o.device))
    assert rc == 0, lib.yolosod_last_error()
    buf = buf.cpu()
    intact = bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + cells:] == SENTINEL).all())
    return buf[GUARD:GUARD + cells].view(B, nc + 1, nc + 1), intact


def _cm(out, counts, targets, nc, cuda, conf=CONF, iou=IOU):
    """The wrapper's cm on the host (int32 [B, nc+1, nc+1]), after the checks every case gets."""
    o = torch.from_numpy(out).to(cuda)
    c = torch.tensor(list(counts), dtype=torch.int32, device=cuda)
    labels, off = V.pack_labels(targets, cuda)
    got = _hip.confusion_matrix(o, c, labels, off, nc, conf, iou)
    assert got.dtype == torch.int32 and tuple(got.shape) == (out.shape[0], nc + 1, nc + 1)
    got = got.cpu()
    pre, intact = _launch_guarded(o, c, labels, off, nc, conf, iou)
    assert intact, "a word outside cm was written"
    assert torch.equal(pre, got), "a cell of cm was not written (or the two launches differ)"
    return got


def _check(out, counts, targets, nc, cuda, conf=CONF, iou=IOU, conserve=True):
    """cm equals the restatement; returns (cm as int64 numpy, the restatement's tie count)."""
    ref, ties = confusion_batch_ref(out, counts, targets, nc, conf, iou)
    got = _cm(out, counts, targets, nc, cuda, conf, iou)
    assert torch.equal(got, torch.from_numpy(ref).int()), \
        f"{int((got != torch.from_numpy(ref).int()).sum())} cells differ from the restatement"
    if conserve:
        for b, (cls, boxes) in enumerate(targets):
            assert conserved(ref[b], lab5(cls, boxes), out[b, :int(counts[b])], nc, conf), b
    return got.numpy().astype(np.int64), ties


def _garbage(B, D, nc, seed):
    """Padding rows: random boxes and classes, confidences above the threshold, NaN sprinkled over every column."""
    rng = np.random.default_rng(seed)
    out = rng.uniform(-50, 700, (B, D, 6)).astype(F32)
    out[..., 4] = rng.uniform(0.3, 1.0, (B, D))
    out[..., 5] = rng.integers(0, nc, (B, D))
    out[rng.uniform(size=(B, D, 6)) < 0.1] = np.nan
    return out


@pytest.mark.parametrize("which,D", [("a", 32), ("b", 320)])
def test_fixture_in_one_launch_is_the_reference_matrices(which, D, cuda):
    nc, images, ref = fixture_sets()[which]
    B = len(images)
    counts = [len(d) for _, _, d in images]
    assert B == 24 and max(counts) <= D
    out = _garbage(B, D, nc, 3)
    for i, (_, _, d) in enumerate(images):
        out[i, :len(d)] = d
    assert np.isnan(out).any()
    targets = [(c, b) for c, b, _ in images]
    got, ties = _check(out, counts, targets, nc, cuda)
    assert ties == 0
    assert np.array_equal(got, ref), "differs from the reference's matrices"
    assert np.array_equal(got.sum(0), ref.sum(0)) and np.trace(got.sum(0)) > 0


@pytest.fixture(scope="module")
def crowds():
    """Per nc, 33 crowds of 1024 rows; image b has LABEL_LOADS[b % 6] labels. Smaller D take the first D rows."""
    return {nc: [crowd(1000 + b, n_labels=LABEL_LOADS[b % len(LABEL_LOADS)], n_det=1024, nc=nc) for b in range(33)]
            for nc in (1, 10, MAX_NC)}


@pytest.mark.parametrize("nc", [1, 10, MAX_NC])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 300, 1024])
@pytest.mark.parametrize("B", [1, 33])
def test_crowds_match_the_restatement(B, D, nc, crowds, cuda):
    # B = 1: the image with the most labels, full; B = 33: counts of D, 0 and in between, every label load
    picks = [5] if B == 1 else list(range(33))
    between = [D, 0, (D + 1) // 2, D - 1, D, 1, D // 3]
    counts = [D] if B == 1 else [min(max(between[b % len(between)], 0), D) for b in range(B)]
    out = _garbage(B, D, nc, 11)
    targets = []
    for i, b in enumerate(picks):
        cls, boxes, det = crowds[nc][b]
        # the kept rows are not the first rows: confidences descend, so a short count would keep them all
        out[i, :counts[i]] = det[np.linspace(0, 1023, counts[i]).astype(int)] if counts[i] else det[:0]
        targets.append((cls, boxes))
    got, _ = _check(out, counts, targets, nc, cuda)
    if B == 33 and D >= 63:
        tot = got.sum(0)
        assert np.trace(tot[:nc, :nc]) > 20 and tot[nc, :nc].sum() > 0 and tot[:nc, nc].sum() > 0, "an empty comparison"
        if nc > 1:
            assert tot[:nc, :nc].sum() > np.trace(tot[:nc, :nc]), "no off-diagonal cell"


def test_conf_threshold_is_strict_in_fp32(cuda):
    up = np.nextafter(F32(0.25), F32(1))
    targets = [(np.zeros(1, F32), np.array([[0, 0, 10, 10]], F32))] * 2
    out = np.zeros((2, 1, 6), F32)
    out[0, 0] = (0, 0, 10, 10, 0.25, 1)
    out[1, 0] = (0, 0, 10, 10, up, 1)
    got, _ = _check(out, [1, 1], targets, 3, cuda)
    assert got[0, 3, 0] == 1 and got[0].sum() == 1, "a row at conf 0.25 was kept"
    assert got[1, 1, 0] == 1 and got[1].sum() == 1, "a row one step above 0.25 was not kept"
    # 0.25 as the host class holds it (a Python float) and as fp32 are the same threshold
    assert F32(0.25) == 0.25


def test_iou_threshold_is_strict_in_fp32(cuda):
    lab = np.array([[2, 0, 0, 20, 10]], F32)
    out = np.array([[[0, 0, 13.7, 10, 0.9, 1]]], F32)
    iou = iou_all(lab, out[0])[0, 0]
    assert iou.dtype == F32 and 0.6 < iou < 0.7
    targets = [(lab[:, 0], lab[:, 1:])]
    at, _ = _check(out, [1], targets, 3, cuda, iou=float(iou))
    assert at[0, 1, 3] == 1 and at[0, 3, 2] == 1 and at[0].sum() == 2, "IoU == threshold matched"
    below, _ = _check(out, [1], targets, 3, cuda, iou=float(np.nextafter(iou, F32(0))))
    assert below[0, 1, 2] == 1 and below[0].sum() == 1, "IoU one step above the threshold did not match"
    zero, _ = _check(out, [1], targets, 3, cuda, iou=0.0)
    assert zero[0, 1, 2] == 1 and zero[0].sum() == 1


def test_nan_conf_and_nan_boxes(cuda):
    nan = np.nan
    lab = np.array([[0, 0, 0, 10, 10], [1, 50, 50, 60, 60], [2, nan, 100, 110, 110]], F32)
    out = np.array([[[0, 0, 10, 10, nan, 0],        # NaN conf: not kept, label 0 goes to the next row
                     [0, 0, 10, 9, 0.9, 1],
                     [50, nan, 60, 60, 0.9, 1],     # NaN box: kept, matches nothing
                     [nan, nan, nan, nan, 0.9, 2],
                     [100, 100, 110, 110, 0.9, 2]]], F32)  # on the NaN label: matches nothing
    got, _ = _check(out, [5], [(lab[:, 0], lab[:, 1:])], 3, cuda)
    want = np.zeros((4, 4), np.int64)
    want[1, 0] = 1
    want[1, 3] = 1
    want[2, 3] = 2
    want[3, 1] = 1
    want[3, 2] = 1
    assert np.array_equal(got[0], want)


def test_classes_out_of_range_are_counted_nowhere(cuda):
    nan = np.nan
    lab = np.array([[2.9, 0, 0, 10, 10], [-1, 50, 50, 60, 60], [nan, 100, 100, 110, 110], [4, 150, 150, 160, 160],
                    [-0.5, 200, 200, 210, 210], [1, 250, 250, 260, 260]], F32)
    out = np.array([[[0, 0, 10, 10, 0.9, 2.9], [50, 50, 60, 60, 0.9, 1], [300, 300, 310, 310, 0.9, nan],
                     [150, 150, 160, 160, 0.9, -1], [400, 400, 410, 410, 0.9, 4], [200, 200, 210, 210, 0.9, 3],
                     [250, 250, 260, 260, 0.9, 1e9], [500, 500, 510, 510, 0.9, -1e9]]], F32)
    got, _ = _check(out, [8], [(lab[:, 0], lab[:, 1:])], 4, cuda, conserve=False)
    want = np.zeros((5, 5), np.int64)
    want[2, 2] = 1  # 2.9 truncates to 2 on both sides
    want[3, 0] = 1  # -0.5 truncates to 0
    # the labels of class -1 and 4 (= nc) are won (by class 1 and by class -1) and the label of class 1 is won by
    # class 1e9: counted nowhere and not missed; the rows of class NaN, 4 and -1e9 on nothing and the NaN label: nowhere
    assert np.array_equal(got[0], want)


def test_chain_on_one_label_goes_to_the_best_iou(cuda):
    """Rows on one label with IoU 0.57, 0.72, 0.92, 0.6 and falling confidence: the third takes it, the others stand on
    background (match_predictions would give it to the first)."""
    targets = [(np.ones(1, F32), np.array([[0, 0, 20, 1]], F32))]
    out = np.array([[[0, 0, w, 1, 0.9 - 0.1 * i, c] for i, (w, c) in
                     enumerate(((11.4, 0), (14.4, 2), (18.4, 3), (12.0, 0)))]], F32)
    got, ties = _check(out, [4], targets, 4, cuda)
    want = np.zeros((5, 5), np.int64)
    want[3, 1], want[0, 4], want[2, 4] = 1, 2, 1
    assert ties == 0 and np.array_equal(got[0], want)


@pytest.mark.parametrize("p,q", [(1, CHUNK + 5), (1, 7), (CHUNK + 5, 1), (2 * CHUNK - 1, 2 * CHUNK)])
def test_label_tie_takes_the_highest_label_index(p, q, cuda):
    """Labels P = (0, 0, 10, 10) of class 1 at index p and Q = (2, 0, 12, 10) of class 2 at index q; the row
    (1, 0, 11, 10) overlaps both by exactly 90 / 110 and takes the one with the higher index. Against the restatement
    only: numpy's order for ties is unspecified."""
    L = 2 * CHUNK + 9
    rng = np.random.default_rng(5)
    xy = rng.uniform(200, 600, (L, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(4, 40, (L, 2))], 1).astype(F32)
    boxes[p], boxes[q] = (0, 0, 10, 10), (2, 0, 12, 10)
    cls = np.zeros(L, F32)
    cls[p], cls[q] = 1, 2
    out = np.array([[[1, 0, 11, 10, 0.8, 3]]], F32)
    got, ties = _check(out, [1], [(cls, boxes)], 4, cuda)
    assert ties == 1
    hi, lo = (2, 1) if q > p else (1, 2)
    assert got[0, 3, hi] == 1 and got[0, 4, lo] == 1 and got[0, 4, 0] == L - 2 and got[0].sum() == L


def test_row_tie_takes_the_highest_row_and_duplicated_labels_are_claimed_once(cuda):
    """The same label three times (indices 3, CHUNK - 1 and CHUNK + 2, classes 1, 2, 3): every row on it ties all its
    copies and takes the last one, so one row wins that copy and the other copies are missed. Rows 1 and 3 are the same
    box (IoU 1 both): the higher row wins. Against the restatement only."""
    L = CHUNK + 40
    rng = np.random.default_rng(6)
    xy = rng.uniform(200, 600, (L, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(4, 40, (L, 2))], 1).astype(F32)
    boxes[[3, CHUNK - 1, CHUNK + 2]] = (10, 10, 30, 30)
    cls = np.zeros(L, F32)
    cls[[3, CHUNK - 1, CHUNK + 2]] = (1, 2, 3)
    out = np.array([[[10, 10, 30, 29.5, 0.9, 1], [10, 10, 30, 30, 0.8, 2], [11, 10, 30, 30, 0.7, 3],
                     [10, 10, 30, 30, 0.6, 4]]], F32)
    got, ties = _check(out, [4], [(cls, boxes)], 5, cuda)
    assert ties == 5  # four rows tie three labels, one label ties two rows
    want = np.zeros((6, 6), np.int64)
    want[4, 3] = 1                       # row 3 (class 4) wins the last copy (class 3)
    want[1, 5] = want[2, 5] = want[3, 5] = 1
    want[5, 1] = want[5, 2] = 1          # the other copies
    want[5, 0] = L - 3
    assert np.array_equal(got[0], want)


def test_wrapper_refusals_launch_nothing(cuda):
    out, counts = torch.zeros(2, 8, 6, device=cuda), torch.zeros(2, dtype=torch.int32, device=cuda)
    labels, off = torch.zeros(3, 5, device=cuda), torch.zeros(3, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="float32"):
        _hip.confusion_matrix(out.half(), counts, labels, off, 3)
    with pytest.raises(RuntimeError, match="int32"):
        _hip.confusion_matrix(out, counts.long(), labels, off, 3)
    with pytest.raises(RuntimeError, match="contiguous"):
        _hip.confusion_matrix(torch.zeros(2, 6, 8, device=cuda).transpose(1, 2), counts, labels, off, 3)
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.confusion_matrix(torch.zeros(2, 1025, 6, device=cuda), counts, labels, off, 3)
    with pytest.raises(RuntimeError, match="images"):
        _hip.confusion_matrix(out, counts, labels, off[:2], 3)
    with pytest.raises(RuntimeError, match="cls, x1"):
        _hip.confusion_matrix(out, counts, torch.zeros(3, 4, device=cuda), off, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.confusion_matrix(out, counts, labels.cpu(), off, 3)
    for nc in (0, MAX_NC + 1, 3.0, True):
        with pytest.raises(RuntimeError, match="nc"):
            _hip.confusion_matrix(out, counts, labels, off, nc)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="conf"):
            _hip.confusion_matrix(out, counts, labels, off, 3, conf=bad)
        with pytest.raises(RuntimeError, match="iou_thres"):
            _hip.confusion_matrix(out, counts, labels, off, 3, iou_thres=bad)


def test_op_timer_key(cuda):
    out, counts = torch.zeros(2, 8, 6, device=cuda), torch.zeros(2, dtype=torch.int32, device=cuda)
    labels, off = torch.zeros(3, 5, device=cuda), torch.tensor([0, 1, 3], dtype=torch.int32, device=cuda)
    with _hip.op_timer() as t:
        _hip.confusion_matrix(out, counts, labels, off, 7)
    keys = [k for k, _ in t.durations_ms()]
    assert keys == [("confusion_matrix", (2, 8, 7), 3)]


# ---- evaluator -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory, cuda):
    """The paper model with a trained-like head through a checkpoint file, as tests/test_gpu_eval.py and
    tests/test_gpu_ingest.py build it, run at 128 px. (tests/golden/ckpt_tiny.pt, the reduced-width checkpoint, cannot
    stand here: its widths are no multiples of 32 and the HIP Swin kernel refuses them.)"""
    import re
    from yolosod_amd.nn.checkpoint import attempt_load_one_weight, save_checkpoint
    from yolosod_amd.nn.tasks import DetectionModel
    torch.manual_seed(0)
    m = DetectionModel("yolov12-sod-fusion-v5-simple.yaml")
    shift = torch.linspace(6.0, 12.0, m.yaml["nc"])
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if re.fullmatch(r"model\.39\.cv3\.\d\.2\.bias", k):
                v.add_(shift)
    path = save_checkpoint(m, tmp_path_factory.mktemp("confusion") / "trained_like.pt")
    return attempt_load_one_weight(path, device=cuda)[0]


@pytest.fixture(scope="module")
def val_batch(model, cuda):
    """Val-mode NMS output of the checkpoint model on a seeded batch, and labels made of jittered predict-mode
    detections (a third with another class) plus random boxes; image 1 has no labels. Returns (out, counts, targets,
    nc)."""
    from yolosod_amd.engine.predictor import DetectionPredictor
    nc, B, img = model.yaml["nc"], 4, 128
    x = torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(3)).to(cuda)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        out, counts = DetectionPredictor(model, conf=V.VAL_NMS["conf_thres"], iou=V.VAL_NMS["iou_thres"],
                                         multi_label=True, max_det=300).predict_padded(x)[:2]
    finally:
        torch.backends.cudnn.deterministic = det
    # multi_label rows repeat a box once per class, so a label's best IoU is held by several rows: an exact tie, where
    # the reference's steps (numpy's sort) are unspecified. A seeded sub-pixel jitter per row takes the ties out.
    out = out.clone()
    out[..., :4] += (torch.randn(out[..., :4].shape, generator=torch.Generator().manual_seed(4)) * 0.05).to(cuda)
    rng = np.random.default_rng(0)
    host, n = out.cpu().numpy(), counts.cpu().tolist()
    targets = []
    for b in range(B):
        d = host[b, :n[b]]
        d = d[d[:, 4] > 0.25]
        keep = d[rng.uniform(size=len(d)) < 0.6][:40]
        m = int(rng.integers(1, 8))
        xy = rng.uniform(0, img - 30, (m, 2))
        rnd = np.concatenate([xy, xy + rng.uniform(6, 60, (m, 2))], 1)
        kcls = keep[:, 5].copy()
        wrong = rng.uniform(size=len(kcls)) < 0.33
        kcls[wrong] = rng.integers(0, nc, int(wrong.sum()))
        cls = np.concatenate([kcls, rng.integers(0, nc, m)]).astype(F32)
        boxes = np.concatenate([keep[:, :4] + rng.normal(0, 1.0, (len(keep), 4)), rnd]).astype(F32)
        targets.append((cls[:0], boxes[:0]) if b == 1 else (cls, boxes))
    return out, counts, targets, nc


def _slices(out, counts):
    n = counts.cpu().tolist()
    return [out[i, :n[i]] for i in range(len(n))]


def _restated(out, counts, targets, nc, conf=CONF, iou=IOU):
    """The restatement's summed matrix of a batch on the device, asserted to hold no tie: only then do the reference's
    steps (the host class) define a result to compare with."""
    ref, ties = confusion_batch_ref(out.cpu().numpy(), counts.cpu().tolist(), targets, nc, conf, iou)
    assert ties == 0, f"{ties} exact IoU ties: the host path is not defined on this batch"
    return ref.sum(0)


def test_update_padded_counts_as_update_on_the_same_tensors(val_batch):
    out, counts, targets, nc = val_batch
    assert tuple(out.shape) == (4, 300, 6)
    dev, host = V.DetectionEvaluator(nc, confusion=True), V.DetectionEvaluator(nc, confusion=True)
    dev.update_padded(out, counts, targets)
    assert not dev.confusion_matrix.matrix.any(), "the matrix was fetched before get_stats"
    host.update(_slices(out, counts), targets)
    assert dev.get_stats() == host.get_stats()
    a, b = dev.confusion_matrix.matrix, host.confusion_matrix.matrix
    assert a.dtype == np.float64 and a.shape == (nc + 1, nc + 1)
    assert (a == _restated(out, counts, targets, nc)).all() and (a == b).all()
    assert np.trace(a[:nc, :nc]) > 0 and a[:nc, :nc].sum() > np.trace(a[:nc, :nc]), "a trivial workload"
    assert a[nc, :nc].sum() > 0 and a[:nc, nc].sum() > 0
    assert (dev.nt_per_class == host.nt_per_class).all() and (dev.nt_per_image == host.nt_per_image).all()
    assert dev.nt_per_class.sum() == sum(len(c) for c, _ in targets) == a[:, :nc].sum()
    assert dev.get_stats() == host.get_stats() and (dev.confusion_matrix.matrix == b).all(), "a second get_stats added"
    # thresholds of the caller's
    own_d, own_h = ConfusionMatrix(nc, conf=0.5, iou_thres=0.6), ConfusionMatrix(nc, conf=0.5, iou_thres=0.6)
    dev2, host2 = V.DetectionEvaluator(nc, confusion=own_d), V.DetectionEvaluator(nc, confusion=own_h)
    dev2.update_padded(out, counts, targets)
    host2.update(_slices(out, counts), targets)
    dev2.get_stats(), host2.get_stats()
    assert (own_d.matrix == _restated(out, counts, targets, nc, 0.5, 0.6)).all()
    assert (own_d.matrix == own_h.matrix).all() and not (own_d.matrix == b).all()


def test_an_evaluator_fed_both_ways_holds_the_sum(val_batch):
    out, counts, targets, nc = val_batch
    slices = _slices(out, counts)
    mixed, host = V.DetectionEvaluator(nc, confusion=True), V.DetectionEvaluator(nc, confusion=True)
    mixed.update(slices[:1], targets[:1])
    mixed.update_padded(out[1:3].contiguous(), counts[1:3].contiguous(), targets[1:3])
    mixed.update(slices[3:], targets[3:])
    mixed.update_padded(out[:2].contiguous(), torch.zeros_like(counts[:2]), targets[:2])  # no rows at all
    host.update(slices, targets)
    host.update([s[:0] for s in slices[:2]], targets[:2])
    assert mixed.get_stats() == host.get_stats()
    assert (mixed.confusion_matrix.matrix == host.confusion_matrix.matrix).all()
    # more after a fetch: the accumulator starts again and the matrix keeps growing
    mixed.update_padded(out, counts, targets)
    host.update(slices, targets)
    mixed.get_stats(), host.get_stats()
    assert (mixed.confusion_matrix.matrix == host.confusion_matrix.matrix).all()
    off = V.DetectionEvaluator(nc)
    off.update_padded(out, counts, targets)
    assert off.confusion_matrix is None and off._cm_dev is None


class _no_sync:
    def __enter__(self):
        self.mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "prototype feature" notice
            torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.mode)
        return False


def test_update_padded_with_confusion_makes_no_synchronising_call(val_batch):
    out, counts, targets, nc = val_batch
    halves = [(out[:2].contiguous(), counts[:2].contiguous(), targets[:2]),
              (out[2:].contiguous(), counts[2:].contiguous(), targets[2:])]
    warm = V.DetectionEvaluator(nc, confusion=True)
    warm.update_padded(*halves[0])  # first use: pinned blocks and the code object are set up
    torch.cuda.synchronize()
    ev = V.DetectionEvaluator(nc, confusion=True)
    with _no_sync():
        for h in halves:
            ev.update_padded(*h)
        with pytest.raises(RuntimeError, match="synchroniz"):
            ev.get_stats()  # the one fetch is the sync
    host = V.DetectionEvaluator(nc, confusion=True)
    host.update(_slices(out, counts), targets)
    assert ev.get_stats() == host.get_stats()
    assert (ev.confusion_matrix.matrix == host.confusion_matrix.matrix).all()


PLANT_SHAPES = [(200, 300), (90, 150)]
PLANTED = [(60.0, 50.0, 24.0, 18.0), (140.0, 120.0, 30.0, 22.0), (250.0, 70.0, 16.0, 24.0), (100.0, 100.0, 20.0, 20.0)]


def _planted_frame(h, w, seed):
    """uint8 BGR frame: noise with one flat rectangle per planted object that fits; (frame, cls, boxes xyxy). The
    frames of tests/test_gpu_eval.py."""
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


def test_validate_with_an_evaluator_over_the_sliced_predictor(model, cuda):
    """validate(..., evaluator=DetectionEvaluator(nc, confusion=True)) over SlicedPredictor on two small frames, labels
    in frame pixels; the predictor's own output is recorded during that run (never a second forward) and fed to a host
    evaluator through update(). One row per anchor (multi_label=False): rows that repeat a box once per class tie on
    every label, and the recorded output cannot be nudged apart as val_batch's is."""
    from yolosod_amd.engine.predictor import SlicedPredictor
    nc = model.yaml["nc"]
    sp = SlicedPredictor(model, slice=128, overlap=0.25, full_frame=True, cut_margin=2.0, imgsz=128,
                         conf=V.VAL_NMS["conf_thres"], iou=V.VAL_NMS["iou_thres"], multi_label=False, max_det=300)
    planted = [_planted_frame(h, w, 70 + i) for i, (h, w) in enumerate(PLANT_SHAPES)]
    batches = [([f for f, _, _ in planted], [(cls, boxes) for _, cls, boxes in planted])]
    rec = _Recording(sp)
    ev = V.DetectionEvaluator(nc, confusion=ConfusionMatrix(nc, conf=0.05, iou_thres=0.1))
    res = V.validate(rec, batches, nc, evaluator=ev)
    assert len(rec.seen) == 1 and res == ev.metrics.results_dict
    host = V.DetectionEvaluator(nc, confusion=ConfusionMatrix(nc, conf=0.05, iou_thres=0.1))
    restated = 0
    for (out, counts, _), (_, targets) in zip(rec.seen, batches):
        host.update(_slices(out, counts), targets)
        restated = restated + _restated(out, counts, targets, nc, 0.05, 0.1)
    assert res == host.get_stats()
    a, b = ev.confusion_matrix.matrix, host.confusion_matrix.matrix
    assert (a == restated).all() and (a == b).all() and a[:, :nc].sum() == 5 and a[:nc].sum() > 0, "nothing kept: the comparison is empty"
    assert (ev.nt_per_class == host.nt_per_class).all() and ev.nt_per_class.sum() == 5
    with pytest.raises(ValueError, match="another nc"):
        V.validate(rec, [], nc + 1, evaluator=ev)
    assert V.validate(rec, [], nc) == V.DetMetrics().results_dict  # evaluator=None: a fresh one, as before
