"""CPU: merge-NMS, everything that needs no GPU - the restatement (tests/nms_merge_ref.py) on the cases where the merged
box is known exactly, on planted objects (what merging is for: the cluster's mean is closer to the object than its
best-scoring candidate), the keyword's surface and refusals, and the exported entry point."""
import ctypes

import numpy as np
import pytest
import torch

import recipes
from conftest import ROOT
from nms_merge_ref import nms_merge_ref, ulp_diff
from yolosod_amd import _hip
from yolosod_amd.utils import ops


@pytest.mark.parametrize("name", ["nms_predict", "nms_val", "nms_degenerate"])
def test_restatement_iou_one_is_plain_nms(name):
    """No IoU exceeds 1: every cluster is the row's own candidate and (s * c) / s is exact."""
    pred, kw = recipes.nms_case(name)
    kw["iou_thres"] = 1.0
    rows, _, merged, _, nmer = nms_merge_ref(pred, **kw)
    assert sum(len(r) for r in rows) > 0
    for b in range(len(rows)):
        assert (nmer[b] == 1).all()
        assert np.array_equal(merged[b], rows[b])


@pytest.mark.parametrize("name", ["nms_predict", "nms_val", "nms_agnostic", "nms_cuts", "nms_degenerate"])
def test_restatement_clusters_of_one_keep_their_box(name):
    pred, kw = recipes.nms_case(name)
    rows, _, merged, _, nmer = nms_merge_ref(pred, **kw)
    for b in range(len(rows)):
        assert (nmer[b] >= 1).all()
        assert np.array_equal(merged[b][:, 4:], rows[b][:, 4:])
        one = nmer[b] == 1
        assert np.array_equal(merged[b][one], rows[b][one])


def test_restatement_zero_area_kept_boxes_stay_finite_and_unchanged():
    """A zero-area box has IoU 0 / 0 = NaN with itself and with its exact duplicates, and 0 with everything else: its
    cluster is its own candidate alone, which the definition always counts."""
    pred, kw = recipes.nms_case("nms_degenerate")
    rows, _, merged, _, nmer = nms_merge_ref(pred, **kw)
    seen = 0
    for b in range(len(rows)):
        z = ((rows[b][:, 2] - rows[b][:, 0]) * (rows[b][:, 3] - rows[b][:, 1])) == 0
        seen += int(z.sum())
        assert np.isfinite(merged[b]).all()
        assert (nmer[b][z] == 1).all()
        assert np.array_equal(merged[b][z], rows[b][z])
    assert seen > 0


def _planted(seed):
    """24 objects on a 6 x 4 grid 90 px apart, sides U(16, 40); 12 candidates each, every coordinate jittered by
    N(0, 0.06 side), scores U(0.3, 0.95). Returns (prediction [1, 5, 288] xywh, the objects' xyxy [24, 4])."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(6), np.arange(4))
    cx, cy = 60.0 + 90.0 * gx.ravel(), 60.0 + 90.0 * gy.ravel()
    w, h = rng.uniform(16, 40, 24), rng.uniform(16, 40, 24)
    gt = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    side = np.stack([w, h, w, h], 1)
    cand = gt[:, None, :] + rng.normal(0, 1, (24, 12, 4)) * 0.06 * side[:, None, :]
    cand = cand.reshape(-1, 4)
    pred = np.zeros((1, 5, cand.shape[0]), np.float32)
    pred[0, 0] = (cand[:, 0] + cand[:, 2]) / 2
    pred[0, 1] = (cand[:, 1] + cand[:, 3]) / 2
    pred[0, 2] = cand[:, 2] - cand[:, 0]
    pred[0, 3] = cand[:, 3] - cand[:, 1]
    pred[0, 4] = rng.uniform(0.3, 0.95, cand.shape[0])
    return pred, gt


def planted_errors(boxes, gt):
    """Mean |coordinate error| of each box against the object it lies on (the nearest centre)."""
    c = (boxes[:, None, :2] + boxes[:, None, 2:4]) / 2 - (gt[None, :, :2] + gt[None, :, 2:]) / 2
    near = (c ** 2).sum(-1).argmin(1)
    return float(np.abs(boxes[:, :4] - gt[near]).mean())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_objects_merged_boxes_are_closer(seed):
    pred, gt = _planted(seed)
    rows, _, merged, _, nmer = nms_merge_ref(pred, conf_thres=0.25, iou_thres=0.5)
    assert len(rows[0]) >= 24
    e_kept, e_merged = planted_errors(rows[0][:, :4], gt), planted_errors(merged[0][:, :4], gt)
    print(f"seed {seed}: kept {len(rows[0])}, mean |err| kept {e_kept:.4f} merged {e_merged:.4f} "
          f"ratio {e_merged / e_kept:.3f}, mean cluster {nmer[0].mean():.2f}")
    assert e_merged < 0.5 * e_kept


def test_ulp_diff():
    a = np.array([1.0, -1.0, 0.0, 3.5], np.float32)
    assert ulp_diff(a, a).tolist() == [0, 0, 0, 0]
    assert ulp_diff(a, np.nextafter(a, np.float32(10))).tolist() == [1, 1, 1, 1]
    assert ulp_diff(np.float32([0.0]), np.float32([-0.0])).tolist() == [0]


def test_merge_keyword_on_cpu_tensors_raises_no_cpu_fallback():
    pred = torch.from_numpy(recipes.synthetic_predictions(1, 1, 85, 3))
    for fn in (ops.non_max_suppression_padded, ops.non_max_suppression):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(pred, 0.25, 0.5, merge=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _hip.ops().nms_merged_batched(pred, 0.25, 0.5, None, False, False, 300, 30000, 7680.0, True, None)


def test_merge_false_returns_three_values(monkeypatch):
    """The default takes the plain NMS wrapper with the arguments it always had."""
    seen = {}

    def fake(*a):
        seen["args"] = a
        return 1, 2, 3

    monkeypatch.setattr(_hip, "nms", fake)
    monkeypatch.setattr(_hip, "nms_merged", lambda *a, **k: pytest.fail("merge=False reached the merged wrapper"))
    pred = torch.zeros(1, 7, 85)
    assert ops.non_max_suppression_padded(pred, 0.25, 0.5) == (1, 2, 3)
    assert ops.non_max_suppression_padded(pred, 0.25, 0.5, merge=False) == (1, 2, 3)
    assert seen["args"][1:] == (0.25, 0.5, None, False, False, 300, 30000, 7680, True)


def test_merge_true_reaches_the_merged_wrapper_and_returns_four(monkeypatch):
    monkeypatch.setattr(_hip, "nms_merged", lambda *a: (1, 2, 3, 4))
    assert ops.non_max_suppression_padded(torch.zeros(1, 7, 85), 0.25, 0.5, merge=True) == (1, 2, 3, 4)


def test_max_det_above_1024_is_refused_with_merge_only():
    lib = _hip.load_library()
    p = ctypes.c_void_p(64)  # every refusal happens before anything is launched: the pointers name no memory
    args = [p, 1, 3, 85, 0.25, 0.5, None, 0, 0, 0]
    tail = [30000, 7680.0, 0, p, p, p, p, p, 1 << 20, None]
    assert lib.yolosod_nms_merged(*args, 1025, *tail) != 0
    assert b"max_det=1025" in lib.yolosod_last_error()
    assert lib.yolosod_nms_merged(*args, 0, *tail) != 0
    tail[6] = None  # n_merged
    assert lib.yolosod_nms_merged(*args, 300, *tail) != 0
    assert _hip.NMS_MERGE_MAX_DET == 1024


def test_symbol_is_exported_and_declared():
    lib = _hip.load_library()
    assert hasattr(lib, "yolosod_nms_merged") and "yolosod_nms_merged" in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["yolosod_nms_merged"][1]) == len(_hip.SIGNATURES["yolosod_nms"][1]) + 1
    assert "yolosod_nms_merged" in (ROOT / "include" / "yolosod_hip.h").read_text()
    assert lib.yolosod_abi_version() == 1
    assert hasattr(_hip.ops(), "nms_merged_batched")


def test_predictors_take_merge_nms_and_default_off():
    import inspect
    from yolosod_amd.engine.predictor import DetectionPredictor, SlicedPredictor
    for cls in (DetectionPredictor, SlicedPredictor):
        assert inspect.signature(cls.__init__).parameters["merge_nms"].default is False
