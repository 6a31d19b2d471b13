"""GPU merge-NMS (nms_merge_kernel, csrc/nms.hip) against the restatement (tests/nms_merge_ref.py): conf, cls, index,
counts and the order are plain NMS's bit for bit, n_merged is exact, and every merged coordinate lies within one fp32 ulp
of the restatement's fp64 value rounded to fp32 (the two fp64 sums run in different orders: about n * 2^-53 relative,
which can move the final rounding by one ulp at most)."""
import warnings

import numpy as np
import pytest
import torch

import recipes
from nms_merge_ref import candidates_ref, nms_merge_ref, ulp_diff
from test_gpu_sliced import PLANT_SHAPE, SHAPES, _deterministic, _scene_bgr, model, planted  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _both(pred_np, cuda, in_place=True, **kw):
    from yolosod_amd.utils.ops import non_max_suppression_padded
    p0 = torch.from_numpy(pred_np.copy()).to(cuda)
    p1 = torch.from_numpy(pred_np.copy()).to(cuda)
    plain = non_max_suppression_padded(p0, in_place=in_place, **kw)
    merged = non_max_suppression_padded(p1, in_place=in_place, merge=True, **kw)
    assert len(plain) == 3 and len(merged) == 4
    return p0, p1, plain, merged


def _check(pred_np, cuda, **kw):
    """The GPU's merge=True call against its merge=False call and the restatement; returns n_merged per image."""
    p0, p1, (out0, counts0, index0), (out, counts, index, nm) = _both(pred_np, cuda, **kw)
    assert torch.equal(p0, p1), "the in-place rewrite differs with merge"
    assert torch.equal(counts, counts0) and torch.equal(index, index0)
    assert torch.equal(out[..., 4:], out0[..., 4:])
    B, D = out.shape[:2]
    assert tuple(nm.shape) == (B, D) and nm.dtype == torch.int32
    rows, idx, mref, _, nref = nms_merge_ref(pred_np, **kw)
    out, out0, nm, counts = out.cpu().numpy(), out0.cpu().numpy(), nm.cpu().numpy(), counts.cpu().numpy()
    assert counts.tolist() == [len(r) for r in rows]
    worst = 0
    for b in range(B):
        n = counts[b]
        assert np.array_equal(out0[b, :n], rows[b]), b
        assert np.array_equal(nm[b, :n], nref[b]), (b, np.nonzero(nm[b, :n] != nref[b])[0][:8])
        assert (nm[b, n:] == 0).all() and (out[b, n:] == 0).all()
        assert np.isfinite(out[b, :n]).all()
        if n:
            d = ulp_diff(out[b, :n, :4], mref[b][:, :4])
            worst = max(worst, int(d.max()))
            assert d.max() <= 1, (b, int(d.max()), np.argwhere(d > 1)[:8].tolist())
            one = nref[b] == 1
            assert np.array_equal(out[b, :n][one], rows[b][one]), "a cluster of one must keep its box bit for bit"
    print(f"counts {counts.tolist()}, mean cluster {[round(float(c.mean()), 2) if len(c) else 0 for c in nref]}, "
          f"worst coordinate {worst} ulp")
    return nref


@pytest.mark.parametrize("name", list(recipes.NMS_CASES))
def test_fixture_cases(name, cuda):
    pred, kw = recipes.nms_case(name)
    nref = _check(pred, cuda, **kw)
    if name != "nms_empty":
        assert max(int(c.max()) for c in nref if len(c)) > 1, "nothing was merged"


@pytest.mark.parametrize("nc", [1, 10])
def test_odd_small_shape(nc, cuda):
    """A = 85: odd, less than one 256-anchor block."""
    pred = recipes.synthetic_predictions(85 + nc, 2, 85, nc, n_clusters=6)
    _check(pred, cuda, conf_thres=0.25, iou_thres=0.5)
    _check(pred, cuda, conf_thres=0.05, iou_thres=0.5, multi_label=True, max_det=7)


def test_images_without_detections(cuda):
    pred = recipes.synthetic_predictions(5, 1, 85, 3)
    pred[:, 4:] = 0.0
    _check(pred, cuda, conf_thres=0.25, iou_thres=0.5)
    pred = recipes.synthetic_predictions(6, 2, 700, 3, n_clusters=5)
    pred[0, 4:] = 0.0  # B = 2, the first image empty
    nref = _check(pred, cuda, conf_thres=0.25, iou_thres=0.5)
    assert len(nref[0]) == 0 and len(nref[1]) > 0


def test_remainder_path(cuda):
    """More than 2048 candidates per image in three clusters: nms_resolve runs out of its sorted prefix before max_det and
    goes through the remainder (which reorders the candidate compaction in the workspace); 40 % of the boxes lie across
    x = max_wh, in the next class's band of the offset space, where they overlap that class's boxes."""
    B, A = 2, 34000
    pred = recipes.synthetic_predictions(3131, B, A, 10, n_clusters=3)
    rng = np.random.default_rng(9)
    for b in range(B):
        u = rng.uniform(0, 1, A)
        pred[b, 0, u < 0.4] += 7680.0 - 320.0
        pred[b, 0, (u >= 0.4) & (u < 0.5)] -= 640.0
    # the remainder ran: the sorted prefix holds at most the 2048 best candidates, and rows were kept from below them
    from oracle.nms import non_max_suppression_ref
    kept = non_max_suppression_ref(pred.copy(), 0.25, 0.45)[0]
    for b in range(B):
        scores = np.sort(candidates_ref(pred[b], 0.25)[1])[::-1]
        assert len(scores) > 3 * 2048 and len(kept[b]) < 300 and kept[b][:, 4].min() < scores[2047], b
    _check(pred, cuda, conf_thres=0.25, iou_thres=0.45)


def test_sliced_range(cuda):
    """A = 34000, B = 2, about 10 000 candidates per image, positions up to 3840 px, max_wh 7680."""
    pred = recipes.synthetic_predictions(777, 2, 34000, 10, n_clusters=400, img=3840.0)
    n = [(pred[b, 4:].max(0) > np.float32(0.92)).sum() for b in range(2)]
    assert all(8000 <= v <= 12000 for v in n), n
    assert pred[:, :2].max() > 3800
    _check(pred, cuda, conf_thres=0.92, iou_thres=0.6, max_wh=7680)


def test_iou_one_is_plain_nms_and_runs_repeat(cuda):
    pred, kw = recipes.nms_case("nms_degenerate")
    kw1 = dict(kw, iou_thres=1.0)
    _, _, (out0, counts0, index0), (out, counts, index, nm) = _both(pred, cuda, **kw1)
    assert int(counts.sum()) > 0
    assert torch.equal(out, out0) and torch.equal(counts, counts0) and torch.equal(index, index0)
    assert torch.equal(nm, (out0[..., 4] > 0).to(torch.int32))
    pred, kw = recipes.nms_case("nms_val")
    a = _both(pred, cuda, **kw)[3]
    b = _both(pred, cuda, **kw)[3]
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_in_place(cuda):
    pred, kw = recipes.nms_case("nms_predict")
    p0, p1, plain, merged = _both(pred, cuda, in_place=False, **kw)
    assert torch.equal(p1.cpu(), torch.from_numpy(pred)), "in_place=False must leave the prediction untouched"
    q0, q1, plain_ip, merged_ip = _both(pred, cuda, in_place=True, **kw)
    assert torch.equal(q0, q1) and not torch.equal(q1, p1)
    for u, v in zip(merged, merged_ip):
        assert torch.equal(u, v)


def test_list_form_returns_the_merged_rows(cuda):
    from yolosod_amd.utils.ops import non_max_suppression, non_max_suppression_padded
    pred, kw = recipes.nms_case("nms_predict")
    res = non_max_suppression(torch.from_numpy(pred.copy()).to(cuda), merge=True, **kw)
    out, counts, _, _ = non_max_suppression_padded(torch.from_numpy(pred.copy()).to(cuda), merge=True, **kw)
    assert [len(r) for r in res] == counts.tolist()
    for b, r in enumerate(res):
        assert torch.equal(r, out[b, :len(r)])


def test_refusals(cuda):
    from yolosod_amd import _hip
    from yolosod_amd.utils.ops import non_max_suppression_padded
    pred = torch.from_numpy(recipes.synthetic_predictions(1, 2, 85, 3)).to(cuda)
    with pytest.raises((ValueError, RuntimeError), match="max_det"):
        non_max_suppression_padded(pred, 0.25, 0.5, max_det=1025, merge=True)
    assert len(non_max_suppression_padded(pred.clone(), 0.25, 0.5, max_det=1025)) == 3  # plain NMS keeps its range
    op = _hip.ops().nms_merged_batched
    args = (pred, 0.25, 0.5, None, False, False, 300, 30000, 7680.0, False)
    with pytest.raises(RuntimeError, match="max_det"):
        op(pred, 0.25, 0.5, None, False, False, 1025, 30000, 7680.0, False, None)
    for bad in (torch.zeros(2, 299, dtype=torch.int32, device=cuda), torch.zeros(2, 300, dtype=torch.int32),
                torch.zeros(2, 300, dtype=torch.int64, device=cuda), torch.zeros(600, dtype=torch.int32, device=cuda)):
        with pytest.raises(RuntimeError, match="n_merged"):
            op(*args, bad)
    mine = torch.full((2, 300), -7, dtype=torch.int32, device=cuda)
    res = op(*args, mine)
    assert res[3].data_ptr() == mine.data_ptr() and int(mine.min()) == 0
    assert torch.equal(mine, op(*args, None)[3])


def test_planted_tiles_merge_across_slots(planted, cuda):  # noqa: F811
    """The planted objects of tests/test_gpu_sliced.py: every object is seen whole by up to four tiles and the whole
    frame; one merge-NMS over the merged tensor averages those copies."""
    from tile_merge_ref import tile_merge_ref
    plan, y, _ = planted
    A = y.shape[2]
    rows = plan.merge_rows(0, len(plan))
    ref = tile_merge_ref(y, rows, np.zeros((1, y.shape[1], plan.S * A), dtype=np.float32), A, 2.0)
    nref = _check(ref, cuda, conf_thres=0.25, iou_thres=0.5, max_wh=max(7680, max(PLANT_SHAPE)))
    assert len(nref[0]) == 7 and nref[0].min() >= 2


def _sync_free(fn):
    ref = fn()  # first use: pinned blocks and code objects are set up
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "prototype feature" notice
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    return got


def test_detection_predictor_merge_nms_is_the_composition(model, cuda):  # noqa: F811
    from yolosod_amd import _hip
    from yolosod_amd.engine.predictor import DetectionPredictor
    from yolosod_amd.utils import ops
    frames = [torch.from_numpy(_scene_bgr(h, w, 50 + i)).to(cuda) for i, (h, w) in enumerate(SHAPES)]
    dp = DetectionPredictor(model, conf=0.001, iou=0.7, imgsz=128, rect=False, merge_nms=True)
    plain = DetectionPredictor(model, conf=0.001, iou=0.7, imgsz=128, rect=False)
    assert dp.n_merged is None
    with _deterministic():
        got = _sync_free(lambda: dp.predict_padded(frames))
        nm = dp.n_merged
        with torch.inference_mode():
            ing = dp.ingest(frames)
            y = dp._forward(ing.x)
            y0 = y.clone()
            out, counts, index, nmer = ops.non_max_suppression_padded(y, 0.001, 0.7, max_det=300, in_place=False,
                                                                      merge=True)
            assert torch.equal(y, y0)
            _hip.scale_boxes_padded(out, counts, ing.geom)
        base = plain.predict_padded(frames)
    assert len(got) == 3 and plain.n_merged is None
    for a, b in zip(got, (out, counts, index)):
        assert torch.equal(a, b)
    assert torch.equal(nm, nmer) and int(counts.sum()) > 0 and int(nmer.max()) > 1
    assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]) and torch.equal(got[0][..., 4:], base[0][..., 4:])
    assert not torch.equal(got[0], base[0])
    dets = dp(frames)
    assert all(torch.equal(d.boxes, got[0][i, :int(counts[i])]) for i, d in enumerate(dets))


def test_sliced_predictor_merge_nms_augment_is_the_composition(model, cuda):  # noqa: F811
    from yolosod_amd import _hip
    from yolosod_amd.engine.predictor import SlicedPredictor
    from yolosod_amd.utils import ops
    frames = [torch.from_numpy(_scene_bgr(h, w, 50 + i)).to(cuda) for i, (h, w) in enumerate(SHAPES)]
    sp = SlicedPredictor(model, slice=128, overlap=0.25, full_frame=True, cut_margin=2.0, conf=0.001, iou=0.7, imgsz=128,
                         augment=True, merge_nms=True)
    plan = sp.plan(SHAPES)
    with _deterministic():
        got = _sync_free(lambda: sp.predict_padded(frames))
        nm = sp.n_merged
        merged = sp.merge(sp.forward_tiles(frames, plan), plan)
        out, counts, index, nmer = ops.non_max_suppression_padded(merged, 0.001, 0.7, max_det=300, max_wh=7680,
                                                                  in_place=False, merge=True)
        geom = torch.tensor([[1.0, 0.0, 0.0, w, h] for h, w in SHAPES], dtype=torch.float32, device=cuda)
        _hip.scale_boxes_padded(out, counts, geom)
    for a, b in zip(got, (out, counts, index)):
        assert torch.equal(a, b)
    assert torch.equal(nm, nmer) and int(counts.sum()) > 0 and int(nmer.max()) > 1
    for i, (h, w) in enumerate(SHAPES):
        n = int(counts[i])
        if n:
            assert float(out[i, :n][:, [0, 2]].max()) <= w and float(out[i, :n][:, [1, 3]].max()) <= h
