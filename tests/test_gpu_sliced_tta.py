"""GPU: sliced inference with test-time augmentation - csrc/tile_merge_tta.hip against its numpy restatement
(tests/tile_merge_tta_ref.py) bit for bit after every launch, against the two launches it replaces on the device, the
wrapper's refusals, and SlicedPredictor(augment=True) stage by stage on lists of uint8 BGR frames.

Shapes: canvas 128, so the three views have 1360 / 1360 / 765 anchors and A_tot = 1344 + 1360 + 189 = 2893 (odd, as
62281 is at canvas 640: no slot of merged starts 16-byte aligned in general), and a small odd branch set, A_tot 147."""
import warnings

import numpy as np
import pytest
import torch

from sliced_tta_cases import (CANVAS, FRAMES, NONE, SLOTS, assert_each_outcome_occurs, edge_outcomes, launches,
                              merge_tta_case)
from tile_merge_tta_ref import tile_merge_tta_ref

pytestmark = pytest.mark.gpu

F32 = np.float32


def _bits_equal(t, ref):
    return torch.equal(t.cpu().view(torch.int32), torch.from_numpy(ref).view(torch.int32))


# ---- merge kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut_margin", [None, 0.0, 2.0])
@pytest.mark.parametrize("nc", [1, 10])
@pytest.mark.parametrize("name", ["a", "b"])
def test_merge_matches_the_restatement_after_every_launch(name, nc, cut_margin, cuda):
    from yolosod_amd import _hip
    ys, rows, branches, A_tot = merge_tta_case(name, nc)
    no = 4 + nc
    N = FRAMES * no * SLOTS * A_tot
    lead, tail = 1, 64                                   # merged sits one float into its allocation
    ref = np.full(lead + N + tail, np.nan, dtype=F32)
    ref_m = ref[lead:lead + N].reshape(FRAMES, no, SLOTS * A_tot)
    buf = torch.full((lead + N + tail,), float("nan"), device=cuda)
    merged = buf[lead:lead + N].view(FRAMES, no, SLOTS * A_tot)
    assert merged.data_ptr() % 16 == 4 and merged.is_contiguous()
    dev_y = {}
    for c, k, y, r, b in launches(ys, rows, branches):
        tile_merge_tta_ref(y, r, ref_m, A_tot, b, CANVAS, cut_margin)
        dev_y[c, k] = torch.from_numpy(y).to(cuda)
        out = _hip.tile_merge_tta(dev_y[c, k], r, merged, A_tot, b, CANVAS, cut_margin)
        assert out is merged
        # the whole buffer's bit patterns: NaN marks what no launch has named yet, and the slack, and must match too
        assert _bits_equal(buf, ref), (name, nc, cut_margin, c, k)
    assert not np.isnan(ref_m).any() and not torch.isnan(merged).any(), "every element is defined after all launches"
    assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + N:]).all(), "nothing outside merged is touched"
    assert (merged[0, :, A_tot:2 * A_tot] == 0).all() and (ref_m[0, :, A_tot:2 * A_tot] == 0).all(), "the empty slot"
    if name == "a":  # the boundary boxes do what they were built for (on the restatement), in every branch
        for cut in edge_outcomes(ref_m, ys, branches, A_tot):
            assert_each_outcome_occurs(cut, cut_margin)


@pytest.mark.parametrize("name", ["a", "b"])
def test_merge_is_the_two_launches_it_replaces_on_the_device(name, cuda):
    """tta_merge into a concatenated tensor, then tile_merge of it with A = A_tot: the same bits."""
    from yolosod_amd import _hip
    nc, cut_margin = 10, 2.0
    ys, rows, branches, A_tot = merge_tta_case(name, nc)
    no = 4 + nc
    fused = torch.full((FRAMES, no, SLOTS * A_tot), float("nan"), device=cuda)
    chain = torch.full((FRAMES, no, SLOTS * A_tot), float("nan"), device=cuda)
    for c, call in enumerate(ys):
        cat = torch.full((call[0].shape[0], no, A_tot), float("nan"), device=cuda)
        for y, b in zip(call, branches):
            yd = torch.from_numpy(y).to(cuda)
            _hip.tile_merge_tta(yd, rows[c], fused, A_tot, b, CANVAS, cut_margin)
            _hip.tta_merge(yd, cat, b[0], b[1], b[2], b[3], b[4], CANVAS)
        _hip.tile_merge(cat, rows[c], chain, A_tot, cut_margin)
    assert not torch.isnan(chain).any()
    assert torch.equal(fused, chain)
    assert torch.equal(fused.view(torch.int32), chain.view(torch.int32))


def test_wrapper_refusals_launch_nothing(cuda):
    from yolosod_amd import _hip
    from yolosod_amd.data.tta import TTAPlan
    A, A_tot = 85, 147
    y = torch.zeros(2, 14, A, device=cuda)
    merged = torch.full((1, 14, 3 * A_tot), float("nan"), device=cuda)
    row = (0, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE)
    br = (0, 84, 0, 1.0, None)

    def refused(match, y=y, rows=(row,), merged=merged, A_tot=A_tot, branch=br, canvas=CANVAS, cut=None,
                exc=RuntimeError):
        with pytest.raises(exc, match=match):
            _hip.tile_merge_tta(y, list(rows), merged, A_tot, branch, canvas, cut)

    refused("float32", y=y.half())
    refused("float32", merged=merged.double())
    refused("expected a tensor", y=y.cpu().numpy(), exc=TypeError)
    refused("GPU", y=y.cpu())
    refused("GPU", merged=merged.cpu())
    refused("contiguous", y=torch.zeros(2, A, 14, device=cuda).transpose(1, 2))
    refused("contiguous", merged=torch.zeros(1, 3 * A_tot, 14, device=cuda).transpose(1, 2))
    refused("3 dimensions", y=y[0])
    refused("3 dimensions", merged=merged[0])
    refused("unsupported", y=torch.zeros(2, 4, A, device=cuda))            # no class row
    refused("unsupported", y=torch.zeros(2, 4 + 65, A, device=cuda))
    refused("is not", merged=torch.zeros(1, 9, 3 * A_tot, device=cuda))    # another 4 + nc
    refused(r"S \* 146", A_tot=146)                                        # 441 is no multiple of 146
    refused(r"S \* 0", A_tot=0)
    refused("slot 3", rows=(row, (1, 0, 3, 1.0, 0, 0, 0, 0, 128, 128, NONE)))
    refused("slot -1", rows=((0, 0, -1, 1.0, 0, 0, 0, 0, 128, 128, NONE),))
    refused("frame 1", rows=((0, 1, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE),))
    refused("src 2", rows=((2, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE),))
    refused("src -2", rows=((-2, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE),))
    refused("named twice", rows=(row, (1, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE)))
    refused("gain", rows=((0, 0, 0, 0.0, 0, 0, 0, 0, 128, 128, NONE),))
    refused("rows", rows=())
    refused("expected", rows=((0, 0, 0, 1.0),))
    refused("source anchors", branch=(2, 84, 0, 1.0, None))
    refused("source anchors", branch=(-1, 84, 0, 1.0, None))
    refused("source anchors", branch=(0, 0, 0, 1.0, None))
    refused("destination anchors", branch=(0, 84, 64, 1.0, None))
    refused("destination anchors", branch=(0, 84, -1, 1.0, None))
    refused("scale", branch=(0, 84, 0, 0.0, None))
    refused("scale", branch=(0, 84, 0, float("inf"), None))
    refused("scale", branch=(0, 84, 0, float("nan"), None))
    refused("flip", branch=(0, 84, 0, 1.0, 1))
    refused("branch", branch=(0, 84, 0, 1.0))
    refused("the branch 1360", branch=TTAPlan((128, 128), stride=(4, 8, 16, 32), nl=4).branches[0])  # another A_k
    refused("NaN", cut=float("nan"))
    torch.cuda.synchronize()
    assert torch.isnan(merged).all(), "a refused call wrote to merged"
    # and the same arguments unrefused do write
    _hip.tile_merge_tta(y, [row], merged, A_tot, br, CANVAS)
    assert not torch.isnan(merged[0, :, :84]).any() and torch.isnan(merged[0, :, 84:]).all()


# ---- predictor -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory, cuda):
    """The paper model with a trained-like head, as tests/test_gpu_sliced.py builds it."""
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
    path = save_checkpoint(m, tmp_path_factory.mktemp("sliced_tta") / "trained_like.pt")
    return attempt_load_one_weight(path, device=cuda)[0]


def _scene_bgr(h, w, seed):
    """uint8 BGR frame with flat rectangles under noise (something for the network to respond to)."""
    rng = np.random.default_rng(seed)
    f = np.empty((h, w, 3), dtype=np.float64)
    f[:] = rng.integers(0, 256, 3)
    for _ in range(8):
        y0, x0 = rng.integers(0, h - 2), rng.integers(0, w - 2)
        f[y0:y0 + rng.integers(3, max(4, h // 2)), x0:x0 + rng.integers(3, max(4, w // 2))] = rng.integers(0, 256, 3)
    return np.clip(f + rng.normal(0, 12, f.shape), 0, 255).astype(np.uint8)


class _deterministic:
    """MIOpen split-K atomics otherwise vary run to run."""

    def __enter__(self):
        self.prev = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.prev
        return False


SHAPES = [(200, 300), (90, 150), (128, 128)]
A_KS, A_TOT = (1360, 1360, 765), 2893
KW = dict(slice=128, overlap=0.25, full_frame=True, cut_margin=2.0, conf=0.001, iou=0.7, imgsz=128)


@pytest.fixture(scope="module")
def staged(model, cuda):
    """The three frames through every stage of one SlicedPredictor(augment=True), once, for the tests below."""
    from yolosod_amd.engine.predictor import SlicedPredictor
    frames = [_scene_bgr(h, w, 50 + i) for i, (h, w) in enumerate(SHAPES)]
    inputs = [frames[0], torch.from_numpy(frames[1]), torch.from_numpy(frames[2]).to(cuda)]  # numpy, CPU, GPU
    sp = SlicedPredictor(model, augment=True, **KW)
    plan = sp.plan(SHAPES)
    with _deterministic():
        x = sp.ingest_tiles(inputs, plan)
        ys = sp.forward_tiles(inputs, plan)
        merged = sp.merge(ys, plan)
        post = sp.postprocess(merged, plan)
        padded = sp.predict_padded(inputs)
        guarded = sp.predict_padded_guarded(inputs)
        dets = sp(inputs)
    return dict(sp=sp, plan=plan, tp=sp.tta_plan(plan), frames=frames, inputs=inputs, x=x, ys=ys, merged=merged,
                post=post, padded=padded, guarded=guarded, dets=dets)


def test_predictor_forward_is_the_model_on_the_views_of_the_ingested_tiles(staged, cuda):
    plan, tp, sp = staged["plan"], staged["tp"], staged["sp"]
    assert plan.S == 7 and len(plan) == 12 and plan.canvas == (128, 128)
    assert tp.A_tot == A_TOT and tuple(b.A for b in tp.branches) == A_KS
    assert tuple(staged["x"].shape) == (12, 3, 128, 128)
    ys = staged["ys"]
    assert len(ys) == 1 and isinstance(ys[0], tuple) and len(ys[0]) == 3
    assert [tuple(y.shape) for y in ys[0]] == [(12, 14, a) for a in A_KS]
    assert all(y.dtype == torch.float32 and y.is_contiguous() for y in ys[0])
    views = tp.make_views(staged["x"])
    assert views[0] is staged["x"] and tuple(views[1].shape[-2:]) == tp.branches[1].padded
    with _deterministic(), torch.inference_mode():
        for k, v in enumerate(views):
            assert torch.equal(sp.model(v)[0], ys[0][k]), k


def test_predictor_merge_is_the_restatement_and_the_two_pass_composition(staged, cuda):
    from yolosod_amd import _hip
    plan, tp, sp = staged["plan"], staged["tp"], staged["sp"]
    rows = plan.merge_rows(0, len(plan))
    ref = np.full((3, 14, plan.S * A_TOT), np.nan, dtype=F32)
    for k, b in enumerate(tp.branches):
        tile_merge_tta_ref(staged["ys"][0][k].cpu().numpy(), rows, ref, A_TOT, b, plan.canvas, sp.cut_margin)
    assert not np.isnan(ref).any()
    assert tuple(staged["merged"].shape) == (3, 14, 7 * A_TOT)
    assert torch.equal(staged["merged"].cpu(), torch.from_numpy(ref))
    assert (ref[1, :, 3 * A_TOT:] == 0).all() and (ref[2, :, 2 * A_TOT:] == 0).all(), "empty slots hold zeros"
    cut = ref[0, 4:].max(0) == 0
    for b in tp.branches:  # in a tile slot of frame 0, per branch
        assert int(cut[A_TOT + b.dst:A_TOT + b.dst + b.n].sum()) > 0, "nothing was cut: the margin is not exercised"
    # the model's own concatenation of the same tiles, merged by the one-scale kernel
    with _deterministic(), torch.inference_mode():
        cat = sp.model(staged["x"], augment=True)[0]
    assert tuple(cat.shape) == (12, 14, A_TOT)
    two_pass = _hip.tile_merge(cat, rows, torch.full_like(staged["merged"], float("nan")), A_TOT, sp.cut_margin)
    assert torch.equal(staged["merged"], two_pass)


def test_predictor_merge_does_not_depend_on_the_batch(staged, model):
    """batch = 4: the same rows regrouped into three model calls, and into uneven ones, give the same merged tensor."""
    from yolosod_amd.engine.predictor import SlicedPredictor
    sp4 = SlicedPredictor(model, batch=4, augment=True, **KW)
    plan = sp4.plan(SHAPES)
    assert plan.chunks(4) == [(0, 4), (4, 8), (8, 12)]
    ys = staged["ys"][0]
    chunks = [tuple(y[lo:hi] for y in ys) for lo, hi in plan.chunks(4)]
    assert all(y.is_contiguous() for c in chunks for y in c)
    assert torch.equal(sp4.merge(chunks, plan), staged["merged"])
    uneven = [tuple(y[lo:hi] for y in ys) for lo, hi in ((0, 5), (5, 6), (6, 12))]
    assert torch.equal(sp4.merge(uneven, plan), staged["merged"])
    with pytest.raises(ValueError, match="tiles"):
        sp4.merge(chunks[:2], plan)
    with pytest.raises(ValueError, match="branch outputs"):
        sp4.merge([c[:2] for c in chunks], plan)
    with pytest.raises(ValueError, match="branch outputs"):
        sp4.merge([ys[0]], plan)


def test_predictor_with_batch_4_runs_three_calls(staged, model):
    from yolosod_amd.engine.predictor import SlicedPredictor
    sp4 = SlicedPredictor(model, batch=4, augment=True, **KW)
    plan = sp4.plan(SHAPES)
    with _deterministic():
        ys = sp4.forward_tiles(staged["inputs"], plan)
        padded = sp4.predict_padded(staged["inputs"])
    assert [[tuple(y.shape) for y in c] for c in ys] == [[(4, 14, a) for a in A_KS]] * 3
    # the model's arithmetic may depend on the batch it runs in; the merge of these calls may not
    ref = np.full((3, 14, plan.S * A_TOT), np.nan, dtype=F32)
    for (lo, hi), c in zip(plan.chunks(4), ys):
        for k, b in enumerate(sp4.tta_plan(plan).branches):
            tile_merge_tta_ref(c[k].cpu().numpy(), plan.merge_rows(lo, hi), ref, A_TOT, b, plan.canvas, 2.0)
    merged = sp4.merge(ys, plan)
    assert torch.equal(merged.cpu(), torch.from_numpy(ref))
    for a, b in zip(padded, sp4.postprocess(merged, plan)):
        assert torch.equal(a, b)


def test_predictor_postprocess_is_the_oracle_nms_clipped_to_the_frame(staged):
    from oracle.nms import clip_boxes_ref, non_max_suppression_ref
    sp, tp = staged["sp"], staged["tp"]
    out, counts, index = (t.cpu() for t in staged["post"])
    want, widx = non_max_suppression_ref(staged["merged"].cpu().numpy().copy(), sp.conf, sp.iou, max_det=sp.max_det,
                                         max_wh=7680)
    assert tuple(out.shape) == (3, 300, 6) and tuple(index.shape) == (3, 300)
    total = 0
    for i, shape in enumerate(SHAPES):
        n = int(counts[i])
        total += n
        assert n == len(want[i]), (i, n, len(want[i]))
        rows = want[i].copy()
        clip_boxes_ref(rows[:, :4], shape)
        assert np.array_equal(out[i, :n].numpy(), rows), i
        assert np.array_equal(index[i, :n].numpy(), widx[i]), i
        if n:
            slots = widx[i] // A_TOT
            assert int(slots.max()) < len(staged["plan"].slots[i]), "a detection from an empty slot"
            assert float(rows[:, [0, 2]].max()) <= shape[1] and float(rows[:, [1, 3]].max()) <= shape[0]
    assert total > 0, "nothing kept: the comparison is empty"
    kept = [sp.locate(j, staged["plan"]) for j in widx[0]]
    assert len({s for s, _, _ in kept}) >= 2, "frame 0's detections come from one slot only"
    assert len({k for _, k, _ in kept}) >= 2, "frame 0's detections come from one branch only"


def test_predictor_locate_names_a_real_slot_branch_and_anchor(staged):
    sp, plan, tp = staged["sp"], staged["plan"], staged["tp"]
    out, counts, index = (t.cpu() for t in staged["post"])
    n = int(counts[0])
    assert n > 0
    for j in index[0, :n].tolist():
        slot, k, a = sp.locate(j, plan)
        b = tp.branches[k]
        assert 0 <= slot < len(plan.slots[0]) and b.src_lo <= a < b.src_lo + b.n
        assert sp.index(slot, k, a, plan) == j
        # the detection's score is that anchor's best score in that branch's output of that tile (scores are copied)
        src = plan.order.index((0, slot))
        assert float(staged["ys"][0][k][src, 4:, a].max()) == float(staged["merged"][0, 4:, j].max())


def test_predictor_public_calls(staged):
    out, counts, index = staged["padded"]
    assert tuple(out.shape) == (3, 300, 6) and tuple(counts.shape) == (3,) and tuple(index.shape) == (3, 300)
    for a, b in zip(staged["padded"], staged["post"]):
        assert torch.equal(a, b)
    for a, b in zip(staged["guarded"], staged["padded"]):
        assert torch.equal(a, b)
    dets = staged["dets"]
    assert len(dets) == 3
    for i, d in enumerate(dets):
        n = int(counts[i])
        assert d.orig_shape == SHAPES[i] and tuple(d.boxes.shape) == (n, 6)
        assert torch.equal(d.boxes, out[i, :n]) and torch.equal(d.index, index[i, :n])


def test_one_tile_without_the_full_frame_is_the_augmented_plain_predictor(model, cuda):
    """One 128 x 128 frame, full_frame=False: one tile, gain 1, pad 0, offset 0 - the second step is the identity and
    merged is the model's own concatenation."""
    from yolosod_amd.engine.predictor import DetectionPredictor, SlicedPredictor
    frame = _scene_bgr(128, 128, 60)
    sp = SlicedPredictor(model, slice=128, overlap=0.25, full_frame=False, conf=0.001, imgsz=128, augment=True)
    dp = DetectionPredictor(model, conf=0.001, imgsz=128, rect=False, augment=True)
    plan = sp.plan([(128, 128)])
    assert plan.S == 1 and plan.slot(0, 0).gain == 1.0 and plan.slot(0, 0).interior == NONE
    with _deterministic():
        a = sp([frame])[0]
        b = dp([frame])[0]
        pa, pb = sp.predict_padded([frame]), dp.predict_padded([frame])
    assert a.boxes.shape[0] > 0
    assert torch.equal(a.boxes, b.boxes) and torch.equal(a.index, b.index) and a.orig_shape == b.orig_shape
    for u, v in zip(pa, pb):
        assert torch.equal(u, v)


def test_augment_false_is_unchanged(model, staged):
    from yolosod_amd.engine.predictor import SlicedPredictor
    old, new = SlicedPredictor(model, **KW), SlicedPredictor(model, augment=False, scales=None, flips=None, **KW)
    plan = old.plan(SHAPES)
    with _deterministic():
        ys_old, ys_new = old.forward_tiles(staged["inputs"], plan), new.forward_tiles(staged["inputs"], plan)
        m_old, m_new = old.merge(ys_old, plan), new.merge(ys_new, plan)
        p_old, p_new = old.predict_padded(staged["inputs"]), new.predict_padded(staged["inputs"])
    assert len(ys_old) == 1 and isinstance(ys_old[0], torch.Tensor) and tuple(ys_old[0].shape) == (12, 14, 1360)
    assert torch.equal(ys_old[0], ys_new[0])
    assert tuple(m_old.shape) == (3, 14, 7 * 1360) and torch.equal(m_old, m_new)
    for a, b in zip(p_old, p_new):
        assert torch.equal(a, b)
    for a, b in zip(p_old, old.postprocess(m_old, plan)):
        assert torch.equal(a, b)
    assert int(p_old[1].sum()) > 0
    # the augmented predictor's first branch is the one-scale predictor's output
    assert torch.equal(staged["ys"][0][0], ys_old[0])


def test_predict_padded_makes_no_synchronising_call(staged, cuda):
    sp = staged["sp"]
    frames = [torch.from_numpy(f).to(cuda) for f in staged["frames"]]
    with _deterministic():
        ref = sp.predict_padded(frames)  # first use: pinned blocks and code objects are set up
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "prototype feature" notice
            torch.cuda.set_sync_debug_mode("error")
        try:
            got = sp.predict_padded(frames)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    for a, b in zip(got, staged["padded"]):
        assert torch.equal(a, b)


def test_validate_takes_the_augmented_sliced_predictor(model, staged):
    """validate() needs nothing but predict_padded: the same dictionary as the host evaluator fed sp(frames)."""
    from yolosod_amd.engine import validator as V
    from yolosod_amd.engine.predictor import SlicedPredictor
    nc = 10
    sp = SlicedPredictor(model, slice=128, overlap=0.25, full_frame=True, cut_margin=2.0, imgsz=128, augment=True,
                         conf=V.VAL_NMS["conf_thres"], iou=V.VAL_NMS["iou_thres"], multi_label=True, max_det=300)
    frames = staged["frames"]
    targets = [(np.array([0, 3], F32), np.array([[20, 30, 60, 70], [150, 100, 190, 150]], F32)),
               (np.array([9], F32), np.array([[10, 10, 50, 40]], F32)),
               (np.zeros(0, F32), np.zeros((0, 4), F32))]
    with _deterministic():
        res = V.validate(sp, [(frames, targets)], nc)
        dets = sp(frames)
    assert sum(d.boxes.shape[0] for d in dets) > 0, "nothing detected: the comparison is empty"
    host = V.DetectionEvaluator(nc)
    host.update([d.boxes for d in dets], targets)
    assert res == host.get_stats()
    assert set(res) == set(V.DetMetrics.keys) | {"fitness"}
