"""CPU: the confusion matrix of validation, everything that needs no GPU - the restatement of the kernel's rule
(tests/confusion_ref.py) and the host class (utils.metrics.ConfusionMatrix, the reference's steps) against the
reference's own matrices (tests/golden/confusion_eval.npz) and against each other on seeded tie-free crowds, the
evaluator's host path, the C-ABI entry point's refusals and the wrappers' refusal of CPU tensors."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from confusion_ref import confusion_ref, conserved, crowd, fixture_sets, lab5
from yolosod_amd import _hip
from yolosod_amd.engine import validator as V
from yolosod_amd.utils.metrics import ConfusionMatrix

CONF, IOU = 0.25, 0.45


def _host_image(cm, cls, boxes, det):
    """One image through the host class, called as DetectionEvaluator.update (and val.py:140-159) calls it."""
    if len(det) == 0:
        if len(cls):
            cm.process_batch(None, torch.from_numpy(boxes), torch.from_numpy(cls))
    else:
        cm.process_batch(torch.from_numpy(det), torch.from_numpy(boxes), torch.from_numpy(cls))


def _host_matrix(nc, cls, boxes, det, conf=CONF, iou=IOU):
    cm = ConfusionMatrix(nc, conf=conf, iou_thres=iou)
    _host_image(cm, cls, boxes, det)
    assert cm.matrix.dtype == np.float64 and cm.matrix.shape == (nc + 1, nc + 1)
    return cm.matrix


def test_fixture_is_the_recipe_and_fills_every_region():
    z = golden("confusion_eval")
    m = fixture_sets()
    a_gold = golden("metrics_eval")
    assert np.array_equal(np.concatenate([d for _, _, d in m["a"][1]]), a_gold["pred"]), "set (a) is not the recipe"
    assert m["a"][2].shape == (24, 7, 7) and m["b"][2].shape == (24, 11, 11)
    tot, nc = m["b"][2].sum(0), 10
    assert np.trace(tot[:nc, :nc]) > 0 and tot[:nc, :nc].sum() > np.trace(tot[:nc, :nc])  # off-diagonal cells
    assert tot[nc, :nc].sum() > 0 and tot[:nc, nc].sum() > 0 and tot[nc, nc] == 0
    assert set(z.files) == {"conf", "iou_thres", "a_nc", "a_cm", "b_nc", "b_cm", "b_gt_cls", "b_gt_boxes", "b_gt_n",
                            "b_pred", "b_pred_n"}


@pytest.mark.parametrize("which", ["a", "b"])
def test_restatement_is_the_reference_on_the_fixture(which):
    nc, images, ref = fixture_sets()[which]
    mine = []
    for cls, boxes, det in images:
        M, ties = confusion_ref(lab5(cls, boxes), det, nc, CONF, IOU)
        assert ties == 0, "the fixture holds a tie"
        assert conserved(M, lab5(cls, boxes), det, nc, CONF)
        mine.append(M)
    mine = np.stack(mine)
    assert np.array_equal(mine, ref), "the restatement differs from the reference per image"
    assert np.array_equal(mine.sum(0), ref.sum(0))


@pytest.mark.parametrize("which", ["a", "b"])
def test_host_class_is_the_reference_on_the_fixture(which):
    nc, images, ref = fixture_sets()[which]
    total = ConfusionMatrix(nc)
    for (cls, boxes, det), r in zip(images, ref):
        assert np.array_equal(_host_matrix(nc, cls, boxes, det), r)
        _host_image(total, cls, boxes, det)
    assert np.array_equal(total.matrix, ref.sum(0))


@pytest.mark.parametrize("lo", [0, 50, 100, 150])
def test_restatement_is_the_host_class_on_the_crowds(lo):
    nc, counted, sizes = 10, 0, []
    for seed in range(lo, lo + 50):
        fixed = {0: (0, 0), 1: (0, None), 2: (None, 0), 3: (399, 299)}.get(seed - lo, (None, None))
        cls, boxes, det = crowd(7000 + seed, n_labels=fixed[0], n_det=fixed[1], nc=nc)
        thr = (CONF, IOU) if seed % 3 else (0.6, 0.3)
        M, ties = confusion_ref(lab5(cls, boxes), det, nc, *thr)
        assert ties == 0, seed
        assert np.array_equal(M, _host_matrix(nc, cls, boxes, det, *thr)), seed
        assert conserved(M, lab5(cls, boxes), det, nc, thr[0]), seed
        counted += int(np.trace(M[:nc, :nc]))
        sizes.append((len(cls), len(det)))
    assert counted > 1000, "the crowds match nothing: the comparison is empty"
    assert min(s[0] for s in sizes) == 0 and min(s[1] for s in sizes) == 0 and max(s[0] for s in sizes) == 399


def test_restatement_chain_ties_and_odd_classes():
    # three rows on one label with IoU 0.57, 0.72, 0.92 and falling confidence: the best IoU takes it
    lab = np.array([[1, 0, 0, 20, 1]], np.float32)
    det = np.array([[0, 0, w, 1, 0.9 - 0.1 * i, c] for i, (w, c) in enumerate(((11.4, 0), (14.4, 2), (18.4, 3)))],
                   np.float32)
    M, ties = confusion_ref(lab, det, 4)
    assert ties == 0 and M[3, 1] == 1 and M[0, 4] == 1 and M[2, 4] == 1 and M.sum() == 3
    assert np.array_equal(M, _host_matrix(4, lab[:, 0], lab[:, 1:], det))
    # a duplicated label: both rows take the higher index, the higher row wins it, the lower copy is missed
    lab2 = np.array([[0, 0, 0, 10, 10], [1, 0, 0, 10, 10]], np.float32)
    det2 = np.array([[0, 0, 10, 10, 0.9, 2], [0, 0, 10, 10, 0.8, 3]], np.float32)
    M2, ties2 = confusion_ref(lab2, det2, 4)
    assert ties2 == 3 and M2[3, 1] == 1 and M2[2, 4] == 1 and M2[4, 0] == 1 and M2.sum() == 3
    # classes -1, nc and NaN are counted nowhere, 2.9 is class 2, -0.5 truncates to 0
    lab3 = np.array([[2.9, 0, 0, 10, 10], [-1, 50, 50, 60, 60], [np.nan, 100, 100, 110, 110], [4, 150, 150, 160, 160],
                     [-0.5, 200, 200, 210, 210]], np.float32)
    det3 = np.array([[0, 0, 10, 10, 0.9, 2.9], [50, 50, 60, 60, 0.9, 1], [300, 300, 310, 310, 0.9, np.nan],
                     [150, 150, 160, 160, 0.9, -1], [400, 400, 410, 410, 0.9, 4], [200, 200, 210, 210, 0.9, 3]],
                    np.float32)
    M3, _ = confusion_ref(lab3, det3, 4)
    want = np.zeros((5, 5), np.int64)
    want[2, 2] = 1  # 2.9 on 2.9
    want[3, 0] = 1  # class 3 on the label of class -0.5
    # row 1 won the label of class -1 and the row of class -1 won the label of class 4 (= nc): counted nowhere, and
    # those labels are not missed; the rows of class NaN and 4 on nothing: counted nowhere; the NaN label: nowhere
    assert np.array_equal(M3, want)


def test_conf_rule_and_thresholds_are_strict():
    assert ConfusionMatrix(3, conf=None).conf == 0.25 and ConfusionMatrix(3, conf=0.001).conf == 0.25
    assert ConfusionMatrix(3).conf == 0.25 and ConfusionMatrix(3).iou_thres == 0.45
    assert ConfusionMatrix(3, conf=0.5, iou_thres=0.6).conf == 0.5 and ConfusionMatrix(3, conf=0.002).conf == 0.002
    up = np.nextafter(np.float32(0.25), np.float32(1))
    lab = np.array([[0, 0, 0, 10, 10]], np.float32)
    det = np.array([[0, 0, 10, 10, 0.25, 1], [0, 0, 10, 10, up, 2]], np.float32)
    M, _ = confusion_ref(lab, det, 3)
    assert M[2, 0] == 1 and M.sum() == 1, "conf 0.25 is not above 0.25"
    assert np.array_equal(M, _host_matrix(3, lab[:, 0], lab[:, 1:], det))


def test_tp_fp_and_add():
    nc, images, ref = fixture_sets()["b"]
    cm = ConfusionMatrix(nc)
    cm.add(ref)  # a stack of integer matrices
    cm.add(ref[0].astype(np.int32))
    tot = ref.sum(0) + ref[0]
    assert cm.matrix.dtype == np.float64 and np.array_equal(cm.matrix, tot)
    tp, fp = cm.tp_fp()
    assert tp.shape == fp.shape == (nc,)
    assert np.array_equal(tp, np.diag(tot)[:nc]) and np.array_equal(fp, (tot.sum(1) - np.diag(tot))[:nc])
    assert tp.sum() > 0 and fp.sum() > 0
    with pytest.raises(ValueError, match="integer"):
        cm.add(np.zeros((nc + 1, nc + 1)))
    with pytest.raises(ValueError, match="integer"):
        cm.add(np.zeros((nc, nc), np.int64))


def _evaluators(nc, images, **kw):
    ev = V.DetectionEvaluator(nc, **kw)
    ev.update([torch.from_numpy(d) for _, _, d in images], [(c, b) for c, b, _ in images])
    return ev


@pytest.mark.parametrize("which", ["a", "b"])
def test_evaluator_host_path_holds_the_reference_matrix_and_label_counts(which):
    nc, images, ref = fixture_sets()[which]
    ev = _evaluators(nc, images, confusion=True)
    assert isinstance(ev.confusion_matrix, ConfusionMatrix) and ev.confusion_matrix.conf == 0.25
    ev.get_stats()
    assert np.array_equal(ev.confusion_matrix.matrix, ref.sum(0))
    cls = np.concatenate([c for c, _, _ in images]).astype(int)
    img = np.concatenate([np.unique(c) for c, _, _ in images]).astype(int)
    assert np.array_equal(ev.nt_per_class, np.bincount(cls, minlength=nc)) and ev.nt_per_class.sum() == len(cls)
    assert np.array_equal(ev.nt_per_image, np.bincount(img, minlength=nc))
    own = ConfusionMatrix(nc, conf=0.6, iou_thres=0.3)
    ev2 = _evaluators(nc, images, confusion=own)
    assert ev2.confusion_matrix is own and own.matrix.sum() > 0 and not np.array_equal(own.matrix, ref.sum(0))
    with pytest.raises(ValueError, match="classes"):
        V.DetectionEvaluator(nc, confusion=ConfusionMatrix(nc + 1))


def test_evaluator_without_confusion_is_unchanged():
    nc, images, _ = fixture_sets()["a"]
    z = golden("metrics_eval")
    plain, default, with_cm = _evaluators(nc, images), _evaluators(nc, images, confusion=False), \
        _evaluators(nc, images, confusion=True)
    assert plain.confusion_matrix is None and default.confusion_matrix is None
    assert list(plain.stats) == ["tp", "conf", "pred_cls", "target_cls", "target_img"]
    res = plain.get_stats()
    assert res == default.get_stats() == with_cm.get_stats()
    assert np.array_equal(np.concatenate(plain.stats["tp"]), z["tp"])
    for k in ("all_ap", "p", "r"):
        np.testing.assert_allclose(getattr(plain.metrics, k), z[k], rtol=0, atol=1e-12)  # tests/test_metrics.py's bound
        assert np.array_equal(getattr(with_cm.metrics, k), getattr(plain.metrics, k)), k
    empty = V.DetectionEvaluator(3, confusion=True)
    assert empty.get_stats() == V.DetMetrics().results_dict and not empty.confusion_matrix.matrix.any()
    assert empty.nt_per_class.tolist() == [0, 0, 0] and empty.nt_per_image.tolist() == [0, 0, 0]


def test_label_counts_are_two_arrays_and_leave_odd_classes_to_the_ap_arithmetic():
    """nt_per_class / nt_per_image are always [nc] and never one object; a label class that is negative, NaN or >= nc
    is left out of them, and get_stats scores such a set exactly as it did before the counts existed."""
    nc, images, _ = fixture_sets()["a"]
    fresh = V.DetectionEvaluator(nc)
    assert fresh.nt_per_class is not fresh.nt_per_image
    fresh.nt_per_class[0] = 7
    assert fresh.nt_per_image[0] == 0
    odd = [(np.array([-1, np.nan, nc + 3, 2, 2], np.float32), np.tile(np.array([[1, 1, 9, 9]], np.float32), (5, 1)))]
    ev = V.DetectionEvaluator(nc)
    ev.update([torch.from_numpy(d) for _, _, d in images] + [torch.tensor([[1, 1, 9, 9, 0.9, 2]])],
              [(c, b) for c, b, _ in images] + odd)
    res = ev.get_stats()
    assert ev.nt_per_class is not ev.nt_per_image and ev.nt_per_class.shape == ev.nt_per_image.shape == (nc,)
    base = _evaluators(nc, images)
    base.get_stats()
    assert (ev.nt_per_class - base.nt_per_class).tolist() == [0, 0, 2, 0, 0, 0]
    assert (ev.nt_per_image - base.nt_per_image).tolist() == [0, 0, 1, 0, 0, 0]
    # the metrics are what the AP arithmetic makes of the same arrays, odd classes included
    from yolosod_amd.utils.metrics import DetMetrics
    st = {k: np.concatenate(v, 0) for k, v in ev.stats.items()}
    want = DetMetrics()
    want.process(st["tp"], st["conf"], st["pred_cls"], st["target_cls"])
    assert res == want.results_dict


def test_symbol_is_exported_with_a_signature_and_the_constants_agree():
    lib = _hip.load_library()
    assert hasattr(lib, "yolosod_confusion_matrix") and "yolosod_confusion_matrix" in _hip.SIGNATURES
    assert "yolosod_confusion_matrix" in (ROOT / "include" / "yolosod_hip.h").read_text()
    assert lib.yolosod_abi_version() == 1
    src = (ROOT / "yolo-sod_amd" / "csrc" / "eval_confusion.hip").read_text()
    assert int(re.search(r"constexpr int CHUNK = (\d+);", src).group(1)) == _hip.EVAL_CONFUSION_LABEL_CHUNK
    assert int(re.search(r"constexpr int MAX_D = (\d+);", src).group(1)) == _hip.EVAL_CONFUSION_MAX_D == 1024
    assert int(re.search(r"constexpr int MAX_NC = (\d+);", src).group(1)) == _hip.EVAL_CONFUSION_MAX_NC >= 80
    build = (ROOT / "yolo-sod_amd" / "build.py").read_text()
    assert re.search(r'"eval_confusion\.hip": \["-ffp-contract=off"\]', build)


def test_entry_point_refusals_without_gpu():
    """Every refusal happens before anything is launched: the pointers below name no memory."""
    lib = _hip.load_library()
    p = ctypes.c_void_p(64)

    def call(det=p, counts=p, B=2, D=300, labels=p, off=p, nc=10, conf=0.25, iou=0.45, cm=p):
        rc = lib.yolosod_confusion_matrix(det, counts, B, D, labels, off, nc, conf, iou, cm, None)
        return rc, lib.yolosod_last_error()

    for name in ("det", "counts", "off", "cm"):
        rc, msg = call(**{name: None})
        assert rc != 0 and b"null" in msg, (name, msg)
    for B in (0, -1):
        rc, msg = call(B=B)
        assert rc != 0 and b"B=" in msg, msg
    for D in (0, -5, 1025):
        rc, msg = call(D=D)
        assert rc != 0 and b"D=" in msg, msg
    for nc in (0, -3, _hip.EVAL_CONFUSION_MAX_NC + 1):
        rc, msg = call(nc=nc)
        assert rc != 0 and b"nc=" in msg, msg
    for bad in (-0.5, float("inf"), float("-inf"), float("nan")):
        rc, msg = call(conf=bad)
        assert rc != 0 and b"conf_thr" in msg, (bad, msg)
        rc, msg = call(iou=bad)
        assert rc != 0 and b"iou_thr" in msg, (bad, msg)
    for name in ("det", "counts", "labels", "off", "cm"):
        rc, msg = call(**{name: ctypes.c_void_p(66)})
        assert rc != 0 and b"misaligned" in msg, (name, msg)


def test_wrappers_refuse_cpu_tensors():
    out, counts = torch.zeros(2, 8, 6), torch.zeros(2, dtype=torch.int32)
    labels, off = torch.zeros(0, 5), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU.*no CPU fallback"):
        _hip.confusion_matrix(out, counts, labels, off, 3)
    with pytest.raises(TypeError, match="tensor"):
        _hip.confusion_matrix(out.numpy(), counts, labels, off, 3)
    ev = V.DetectionEvaluator(nc=3, confusion=True)
    with pytest.raises(RuntimeError, match="GPU"):
        ev.update_padded(out, counts, [(np.zeros(0), np.zeros((0, 4)))] * 2)
    assert ev.seen == 0 and not ev.stats["tp"] and not ev.confusion_matrix.matrix.any() and ev._cm_dev is None
