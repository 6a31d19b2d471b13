"""CPU: device-side validation, everything that needs no GPU - the restatement of the matching rule
(tests/eval_match_ref.py) against the host path (utils.metrics.match_predictions over box_iou) and against the
reference's own tp matrix (tests/golden/metrics_eval.npz), the C-ABI entry point's refusals, the wrappers' refusal of
CPU tensors, and pack_labels."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from eval_match_ref import crowd, match_batch_ref, match_ref
from yolosod_amd import _hip
from yolosod_amd.engine import validator as V
from yolosod_amd.utils.metrics import IOU_THRESHOLDS, box_iou, match_predictions

IOUV = IOU_THRESHOLDS.numpy()


def _fixture():
    z = golden("metrics_eval")
    gi, pi = np.cumsum(np.r_[0, z["gt_n"]]), np.cumsum(np.r_[0, z["pred_n"]])
    gt = [(z["gt_cls"][gi[i]:gi[i + 1]], z["gt_boxes"][gi[i]:gi[i + 1]]) for i in range(len(z["gt_n"]))]
    preds = [z["pred"][pi[i]:pi[i + 1]] for i in range(len(z["pred_n"]))]
    return z, gt, preds


def _host_path(cls, boxes, det):
    """What DetectionEvaluator.update computes for one image."""
    if len(det) == 0 or len(cls) == 0:
        return np.zeros((len(det), len(IOUV)), bool)
    p = torch.from_numpy(det)
    return match_predictions(p[:, 5], torch.from_numpy(cls), box_iou(torch.from_numpy(boxes), p[:, :4]))


def _lab(cls, boxes):
    return np.concatenate([np.asarray(cls, np.float32).reshape(-1, 1), np.asarray(boxes, np.float32).reshape(-1, 4)], 1)


def test_restatement_is_the_reference_tp_on_the_fixture():
    z, gt, preds = _fixture()
    mine, host = [], []
    for (cls, boxes), det in zip(gt, preds):
        if len(det):
            mine.append(match_ref(_lab(cls, boxes), det, IOUV))
            host.append(_host_path(cls, boxes, det))
    mine = np.concatenate(mine)
    assert mine.dtype == np.uint8 and int(z["tp"].sum()) == 619
    assert np.array_equal(mine.astype(bool), z["tp"]), "the restatement differs from the reference's tp"
    assert np.array_equal(mine.astype(bool), np.concatenate(host)), "the restatement differs from match_predictions"


@pytest.mark.parametrize("lo", [0, 50, 100, 150])
def test_restatement_is_match_predictions_on_the_crowds(lo):
    hits = 0
    for seed in range(lo, lo + 50):
        cls, boxes, det = crowd(seed)
        mine = match_ref(_lab(cls, boxes), det, IOUV)
        assert np.array_equal(mine.astype(bool), _host_path(cls, boxes, det)), seed
        hits += int(mine.sum())
    assert hits > 1000, "the crowds match nothing: the comparison is empty"


def test_restatement_chain_and_tie_rules():
    # three detections on one label with rising IoU 0.57, 0.72, 0.92 (widths 11.4, 14.4, 18.4 inside a label of
    # width 20, height 1)
    lab = np.array([[0, 0, 0, 20, 1]], np.float32)
    det = np.array([[0, 0, w, 1, 0.9 - 0.1 * i, 0] for i, w in enumerate((11.4, 14.4, 18.4))], np.float32)
    tp = match_ref(lab, det, IOUV).astype(bool)
    assert tp[0].tolist() == [True, True] + [False] * 8            # 0.5, 0.55
    assert tp[1].tolist() == [False, False, True, True, True] + [False] * 5   # 0.6 .. 0.7: above the earlier 0.57
    assert tp[2].tolist() == [False] * 5 + [True, True, True, True, False]    # 0.75 .. 0.9: above the earlier 0.72
    assert np.array_equal(tp, _host_path(lab[:, 0], lab[:, 1:], det))
    # a duplicated label: the higher index takes the detection, so a second detection finds the label claimed
    lab2 = np.array([[0, 0, 0, 10, 10], [0, 0, 0, 10, 10], [0, 50, 50, 60, 60]], np.float32)
    det2 = np.array([[0, 0, 10, 10, 0.9, 0], [0, 0, 10, 9.5, 0.8, 0]], np.float32)
    tp2 = match_ref(lab2, det2, IOUV).astype(bool)
    assert tp2[0].all() and not tp2[1].any()


def test_symbol_is_exported_with_a_signature_and_the_chunk_constant_agrees():
    lib = _hip.load_library()
    assert hasattr(lib, "yolosod_match_predictions") and "yolosod_match_predictions" in _hip.SIGNATURES
    assert "yolosod_match_predictions" in (ROOT / "include" / "yolosod_hip.h").read_text()
    assert lib.yolosod_abi_version() == 1
    src = (ROOT / "yolo-sod_amd" / "csrc" / "eval_match.hip").read_text()
    assert int(re.search(r"constexpr int CHUNK = (\d+);", src).group(1)) == _hip.EVAL_MATCH_LABEL_CHUNK
    assert int(re.search(r"constexpr int MAX_D = (\d+);", src).group(1)) == _hip.EVAL_MATCH_MAX_D == 1024
    assert int(re.search(r"constexpr int MAX_T = (\d+);", src).group(1)) == _hip.EVAL_MATCH_MAX_T == 16


def test_entry_point_refusals_without_gpu():
    """Every refusal happens before anything is launched: the pointers below name no memory."""
    lib = _hip.load_library()
    p = ctypes.c_void_p(64)
    good = (ctypes.c_float * 10)(*IOUV.tolist())
    iouv = ctypes.cast(good, ctypes.c_void_p)

    def call(det=p, counts=p, B=2, D=300, labels=p, off=p, thr=iouv, T=10, tp=p):
        rc = lib.yolosod_match_predictions(det, counts, B, D, labels, off, thr, T, tp, None)
        return rc, lib.yolosod_last_error()

    for name in ("det", "counts", "off", "thr", "tp"):
        rc, msg = call(**{name: None})
        assert rc != 0 and b"null" in msg, (name, msg)
    for B in (0, -1):
        rc, msg = call(B=B)
        assert rc != 0 and b"B=" in msg, msg
    for D in (0, -5, 1025):
        rc, msg = call(D=D)
        assert rc != 0 and b"D=" in msg, msg
    for T in (0, 17):
        rc, msg = call(T=T)
        assert rc != 0 and b"T=" in msg, msg
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        vals = IOUV.tolist()
        vals[3] = bad
        arr = (ctypes.c_float * 10)(*vals)
        rc, msg = call(thr=ctypes.cast(arr, ctypes.c_void_p))
        assert rc != 0 and b"threshold 3" in msg, (bad, msg)


def test_wrappers_refuse_cpu_tensors():
    out, counts = torch.zeros(2, 8, 6), torch.zeros(2, dtype=torch.int32)
    labels, off = torch.zeros(0, 5), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.match_predictions(out, counts, labels, off)
    ev = V.DetectionEvaluator(nc=3)
    with pytest.raises(RuntimeError, match="GPU"):
        ev.update_padded(out, counts, [(np.zeros(0), np.zeros((0, 4)))] * 2)
    assert ev.seen == 0 and not ev.stats["tp"], "a refused batch left something behind"


def test_pack_labels_offsets():
    targets = [(np.array([1, 2]), np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.float64)),
               (np.zeros(0), np.zeros((0, 4))),
               (torch.tensor([5.0]), torch.tensor([[8.0, 9.0, 10.0, 11.0]])),
               (np.zeros(0, np.float32), np.zeros((0, 4), np.float32))]
    labels, off = V.pack_labels(targets, "cpu")
    assert labels.dtype == torch.float32 and off.dtype == torch.int32
    assert off.tolist() == [0, 2, 2, 3, 3]
    assert labels.tolist() == [[1, 0, 1, 2, 3], [2, 4, 5, 6, 7], [5, 8, 9, 10, 11]]
    assert labels.is_contiguous() and off.is_contiguous()
    labels, off = V.pack_labels([(np.zeros(0), np.zeros((0, 4)))] * 3, "cpu")
    assert tuple(labels.shape) == (0, 5) and off.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="classes"):
        V.pack_labels([(np.zeros(2), np.zeros((1, 4)))], "cpu")


def test_batch_restatement_pads_with_zeros():
    z, gt, preds = _fixture()
    D = 32
    assert max(len(p) for p in preds) <= D
    out = np.full((len(preds), D, 6), np.nan, np.float32)
    for i, p in enumerate(preds):
        out[i, :len(p)] = p
    counts = [len(p) for p in preds]
    tp = match_batch_ref(out, counts, gt, IOUV)
    assert np.array_equal(np.concatenate([tp[i, :n] for i, n in enumerate(counts)]).astype(bool), z["tp"])
    assert all(not tp[i, n:].any() for i, n in enumerate(counts))
