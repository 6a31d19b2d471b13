"""GPU: test-time augmentation - csrc/tta.hip's two kernels against their numpy restatement (tests/tta_ref.py) bit for
bit, ``model(x, augment=True)`` stage by stage (views, branches, merge) and against the CPU oracle model, and
``DetectionPredictor(augment=True)`` on tensors and on lists of uint8 BGR frames.

Shapes: inputs of 64x96 / 40x50 / 64x64 (two views per launch, an upscale, no padding at all), branches of 85 / 52 /
40 anchors; the model at 256x256 (the reference's recorded case) and 192x256."""
import re
import warnings

import numpy as np
import pytest
import torch

from oplib import BOX_ATOL, pred_close
from tta_ref import bf16_round, predict_augment_ref, tta_merge_ref, tta_view_ref

pytestmark = pytest.mark.gpu

F32 = np.float32


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class _deterministic:
    """MIOpen split-K atomics otherwise vary run to run."""

    def __enter__(self):
        self.prev = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.prev
        return False


# ---- views kernel --------------------------------------------------------------------------------------------------
# (H, W, [(flip, sh, sw, ph, pw), ...]): the views of one launch
VIEW_CASES = [
    (64, 96, [(3, 53, 79, 64, 96), (None, 42, 64, 64, 96)]),   # ratios 0.83 / 0.67: both in one launch
    (40, 50, [(2, 33, 41, 64, 64)]),                            # ratio 0.83, up-down
    (40, 50, [(3, 60, 75, 64, 96)]),                            # ratio 1.5: an upscale, both index clamps
    (64, 64, [(None, 32, 32, 32, 32)]),                         # ratio 0.5: no padding at all
]
SLACK = 64  # elements between the views of a launch (a multiple of 8: bf16 views stay 16-byte aligned)


def _canaried_outs(views, B, C, dtype, dev):
    """One NaN-filled allocation with the views of a launch inside it, SLACK elements before, between and after."""
    sizes = [B * C * v[3] * v[4] for v in views]
    buf = torch.full((SLACK + sum(n + SLACK for n in sizes),), float("nan"), dtype=dtype, device=dev)
    outs, o = [], SLACK
    for v, n in zip(views, sizes):
        outs.append(buf[o:o + n].view(B, C, v[3], v[4]))
        o += n + SLACK
    return buf, outs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", range(len(VIEW_CASES)))
def test_views_kernel_is_the_restatement(case, dtype, cuda):
    from yolosod_amd import _hip
    from yolosod_amd.data.tta import TTAPlan
    H, W, views = VIEW_CASES[case]
    ratios = {0: (0.83, 0.67), 1: (0.83,), 2: (1.5,), 3: (0.5,)}[case]
    plan = TTAPlan((H, W), ratios, tuple(v[0] for v in views), stride=32, nl=4)
    assert plan.views == views, "the table's sizes are TTAPlan's"
    B, C = 2, 3
    x = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(200 + case))
    bf = dtype == torch.bfloat16
    xn = bf16_round(x.numpy()) if bf else x.numpy()
    xg = torch.from_numpy(xn).to(cuda).to(dtype)
    buf, outs = _canaried_outs(views, B, C, dtype, cuda)
    before = _bits(buf).clone()
    got = _hip.tta_views(xg, views, outs=outs)
    assert len(got) == len(views) and all(a.data_ptr() == b.data_ptr() for a, b in zip(got, outs))
    touched = torch.zeros(buf.numel(), dtype=torch.bool, device=cuda)
    o = SLACK
    for v, t in zip(views, outs):
        ref = tta_view_ref(xn, v, bf16=bf)
        assert tuple(t.shape) == ref.shape and t.dtype == dtype
        assert np.array_equal(t.float().cpu().numpy().view(np.int32), ref.view(np.int32)), v
        touched[o:o + t.numel()] = True
        o += t.numel() + SLACK
    assert torch.equal(_bits(buf)[~touched], before[~touched]), "something outside the views was written"
    # the allocating form gives the same views, and twice the same (deterministic)
    for _ in range(2):
        again = _hip.tta_views(xg, views)
        for a, b in zip(again, outs):
            assert a.is_contiguous() and a.data_ptr() % 16 == 0 and torch.equal(_bits(a), _bits(b))


def test_views_wrapper_refusals_launch_nothing(cuda):
    from yolosod_amd import _hip
    v = [(3, 53, 79, 64, 96)]
    x = torch.rand(2, 3, 64, 96, device=cuda)
    buf, outs = _canaried_outs(v, 2, 3, torch.float32, cuda)
    with _hip.op_timer() as t:
        with pytest.raises(RuntimeError, match="float32 or bfloat16"):
            _hip.tta_views(x.half(), v, outs=outs)
        with pytest.raises(RuntimeError, match="contiguous"):
            _hip.tta_views(torch.rand(2, 3, 96, 64, device=cuda).transpose(2, 3), v, outs=outs)
        with pytest.raises(RuntimeError, match="GPU"):
            _hip.tta_views(x.cpu(), v, outs=outs)
        with pytest.raises(RuntimeError, match="multiple of 4"):
            _hip.tta_views(x, [(3, 53, 79, 64, 94)])
        with pytest.raises(RuntimeError, match="unsupported"):
            _hip.tta_views(x, [(3, 65, 79, 64, 96)], outs=outs)        # resized taller than padded
        with pytest.raises(RuntimeError, match="expected"):
            _hip.tta_views(x, [(1, 53, 79, 64, 96)], outs=outs)        # no such flip
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            _hip.tta_views(x, v, outs=[buf[1:1 + outs[0].numel()].view(2, 3, 64, 96)])
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            _hip.tta_views(x, v, outs=[outs[0].to(torch.bfloat16)])
        with pytest.raises(RuntimeError, match="outputs for"):
            _hip.tta_views(x, v, outs=[])
        with pytest.raises(RuntimeError, match="views"):
            _hip.tta_views(x, [])
    assert t.records == [], "a refused call launched something"
    assert bool(torch.isnan(buf).all())


# ---- merge kernel --------------------------------------------------------------------------------------------------
# (A_k, src_lo, n, scale, flip): the kept ranges [0, 84), [0, 52), [9, 40)
BRANCHES = [(85, 0, 84, 1, None), (52, 0, 52, 0.83, 3), (40, 9, 31, 0.67, 2)]
IMG = (64, 96)


@pytest.mark.parametrize("nc", [1, 10])
def test_merge_kernel_is_the_restatement(nc, cuda):
    from yolosod_amd import _hip
    rng = np.random.default_rng(300 + nc)
    B, no = 2, 4 + nc
    A_tot = sum(b[2] for b in BRANCHES)
    assert A_tot == 167
    N = B * no * A_tot
    buf = torch.full((1 + N + 63,), float("nan"), device=cuda)
    cat = buf[1:1 + N].view(B, no, A_tot)   # one float into its allocation: no row is 16-byte aligned
    assert cat.data_ptr() % 16 == 4 and cat.is_contiguous()
    ref = np.full((B, no, A_tot), np.nan, dtype=F32)
    dst = 0
    for A, lo, n, scale, flip in BRANCHES:
        y = np.empty((B, no, A), dtype=F32)
        y[:, :2] = rng.uniform(-4, 100, (B, 2, A))
        y[:, 2:4] = rng.uniform(0.5, 40, (B, 2, A))
        y[:, 4:] = rng.uniform(0, 1, (B, nc, A))
        tta_merge_ref(y, ref, lo, n, dst, scale, flip, IMG)
        assert _hip.tta_merge(torch.from_numpy(y).to(cuda), cat, lo, n, dst, scale, flip, IMG) is cat
        # after each launch: this branch's range is written, later ranges and the canaries still hold NaN
        assert np.array_equal(cat.cpu().numpy().view(np.int32), ref.view(np.int32)), (A, scale, flip)
        dst += n
    assert not np.isnan(ref).any()
    assert bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + N:]).all())


def test_merge_wrapper_refusals_launch_nothing(cuda):
    from yolosod_amd import _hip
    y = torch.rand(2, 14, 85, device=cuda)
    cat = torch.full((2, 14, 167), float("nan"), device=cuda)
    with _hip.op_timer() as t:
        with pytest.raises(RuntimeError, match="float32"):
            _hip.tta_merge(y.half(), cat, 0, 84, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="float32"):
            _hip.tta_merge(y, cat.double(), 0, 84, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="contiguous"):
            _hip.tta_merge(torch.rand(2, 85, 14, device=cuda).transpose(1, 2), cat, 0, 84, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="source"):
            _hip.tta_merge(y, cat, 2, 84, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="source"):
            _hip.tta_merge(y, cat, -1, 84, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="source"):
            _hip.tta_merge(y, cat, 0, 0, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="destination"):
            _hip.tta_merge(y, cat, 0, 84, 84, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="is not"):
            _hip.tta_merge(y, torch.zeros(2, 9, 167, device=cuda), 0, 84, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="GPU"):
            _hip.tta_merge(y.cpu(), cat, 0, 84, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="GPU"):
            _hip.tta_merge(y, cat.cpu(), 0, 84, 0, 1.0, None, IMG)
        with pytest.raises(RuntimeError, match="scale"):
            _hip.tta_merge(y, cat, 0, 84, 0, 0.0, None, IMG)
        with pytest.raises(RuntimeError, match="scale"):
            _hip.tta_merge(y, cat, 0, 84, 0, float("nan"), None, IMG)
        with pytest.raises(RuntimeError, match="flip"):
            _hip.tta_merge(y, cat, 0, 84, 0, 1.0, 1, IMG)
        with pytest.raises(RuntimeError, match="classes"):
            _hip.tta_merge(torch.rand(2, 4, 85, device=cuda), torch.zeros(2, 4, 167, device=cuda), 0, 84, 0, 1.0, None,
                           IMG)
    assert t.records == [], "a refused call launched something"
    assert bool(torch.isnan(cat).all())


# ---- model ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_model(cuda):
    from yolosod_amd.nn.tasks import build_model
    return build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda)


@pytest.fixture(scope="module")
def cpu_model(gpu_model):
    from oracle.model_ref import build_cpu_model
    cpu = build_cpu_model()
    cpu.load_state_dict({k: v.cpu() for k, v in gpu_model.state_dict().items()})
    return cpu


MODEL_SHAPES = {"256x256": (1, 256, 256, 10297), "192x256": (2, 192, 256, 7637)}


@pytest.fixture(scope="module")
def flows(gpu_model, cpu_model, cuda):
    """``model(x, augment=True)`` once per shape, with what went into and came out of its launches recorded, the same
    views through the model directly, and the flow restated on the CPU oracle."""
    from yolosod_amd import _hip
    res = {}
    for name, (B, H, W, A_tot) in MODEL_SHAPES.items():
        x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
        xg = x.to(cuda)
        seen = {"views": [], "ys": []}
        views0, merge0 = _hip.tta_views, _hip.tta_merge

        def views(*a, **k):
            out = views0(*a, **k)
            seen["views"] += [t.clone() for t in out]
            return out

        def merge(y, *a, **k):
            seen["ys"].append(y.clone())
            return merge0(y, *a, **k)

        _hip.tta_views, _hip.tta_merge = views, merge
        try:
            with _deterministic(), torch.inference_mode():
                out = gpu_model(xg, augment=True)
        finally:
            _hip.tta_views, _hip.tta_merge = views0, merge0
        plan = gpu_model.tta_plan((H, W))
        with _deterministic(), torch.inference_mode():
            direct = [gpu_model(xg if b.view is None else v)[0]
                      for b, v in zip(plan.branches, [None] + seen["views"])]
        ref_cat, ref_views, _ = predict_augment_ref(cpu_model, x, plan)
        res[name] = dict(x=x, out=out, plan=plan, seen=seen, direct=direct, ref_cat=ref_cat, ref_views=ref_views)
    return res


@pytest.mark.parametrize("name", list(MODEL_SHAPES))
def test_model_augment_returns_the_concatenation(flows, name):
    """Without the feature the flag is ignored and the first shape is 5440 (4080)."""
    B, H, W, A_tot = MODEL_SHAPES[name]
    out = flows[name]["out"]
    assert isinstance(out, tuple) and len(out) == 2 and out[1] is None
    y = out[0]
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, 14, A_tot) and y.shape[-1] == A_tot
    assert flows[name]["plan"].A_tot == A_tot
    assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("name", list(MODEL_SHAPES))
def test_model_augment_stages(flows, name):
    f = flows[name]
    plan, seen = f["plan"], f["seen"]
    assert len(seen["views"]) == 2 and len(seen["ys"]) == 3
    # the views are the restatement
    for got, ref in zip(seen["views"], f["ref_views"][1:]):
        assert tuple(got.shape) == tuple(ref.shape)
        assert torch.equal(_bits(got.cpu()), _bits(ref))
    # each branch is the model on that view
    for k, (got, want) in enumerate(zip(seen["ys"], f["direct"])):
        assert tuple(got.shape)[-1] == plan.branches[k].A
        assert torch.equal(got, want), k
    # cat is the restated merge of those
    y = f["out"][0]
    ref = np.full(tuple(y.shape), np.nan, dtype=F32)
    for b, yk in zip(plan.branches, seen["ys"]):
        tta_merge_ref(yk.cpu().numpy(), ref, b.src_lo, b.n, b.dst, b.scale, b.flip, plan.shape)
    assert not np.isnan(ref).any()
    assert np.array_equal(y.cpu().numpy().view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize("name", list(MODEL_SHAPES))
def test_model_augment_matches_the_cpu_oracle(flows, name):
    f = flows[name]
    y = f["out"][0].cpu()
    for b in f["plan"].branches:
        sl = slice(b.dst, b.dst + b.n)
        ok, msg = pred_close(y[:, :, sl], torch.from_numpy(f["ref_cat"][:, :, sl]), box_atol=BOX_ATOL / b.scale)
        print(f"{name} branch scale {b.scale} flip {b.flip}: {msg}")
        assert ok, (b.scale, msg)


def test_model_augment_matches_the_reference_recording(flows):
    """The reference's own predict(augment=True) on the same seeded input (tests/golden/make_tta_golden.py)."""
    from conftest import golden
    f = flows["256x256"]
    want = torch.from_numpy(golden("tta_model_256")["y"])
    y = f["out"][0].cpu()
    assert tuple(y.shape) == tuple(want.shape)
    for b in f["plan"].branches:
        sl = slice(b.dst, b.dst + b.n)
        ok, msg = pred_close(y[:, :, sl], want[:, :, sl], box_atol=BOX_ATOL / b.scale)
        assert ok, (b.scale, msg)


def test_model_augment_with_other_scales_and_flips(gpu_model, cuda):
    """An up-down flipped scale of 1 (a view of the same size), a flipped upscale and the batch itself."""
    scales, flips = (1, 1.5, 1), (2, 3, None)
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(5))
    xg = x.to(cuda)
    plan = gpu_model.tta_plan((128, 128), scales, flips)
    assert plan.views == [(2, 128, 128, 128, 128), (3, 192, 192, 192, 192)] and plan.branches[2].view is None
    assert [(b.A, b.src_lo, b.n, b.dst) for b in plan.branches] == [(1360, 0, 1344, 0), (3060, 0, 3060, 1344),
                                                                   (1360, 1024, 336, 4404)]
    with _deterministic(), torch.inference_mode():
        y, none = gpu_model._predict_augment(xg, scales, flips)
        ref = np.full((2, 14, plan.A_tot), np.nan, dtype=F32)
        for b in plan.branches:
            xi = xg if b.view is None else torch.from_numpy(tta_view_ref(x.numpy(), b.view)).to(cuda)
            tta_merge_ref(gpu_model(xi)[0].cpu().numpy(), ref, b.src_lo, b.n, b.dst, b.scale, b.flip, plan.shape)
    assert none is None and tuple(y.shape) == (2, 14, 4740)
    assert np.array_equal(y.cpu().numpy().view(np.int32), ref.view(np.int32))


def test_model_augment_refuses_cpu_input(gpu_model):
    with pytest.raises(RuntimeError, match="HIP kernel requires GPU tensors"):
        gpu_model(torch.zeros(1, 3, 64, 64), augment=True)


# ---- predictor -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory, cuda):
    """The paper model with a trained-like head, as tests/test_gpu_sliced.py builds it."""
    from yolosod_amd.nn.checkpoint import attempt_load_one_weight, save_checkpoint
    from yolosod_amd.nn.tasks import DetectionModel
    torch.manual_seed(0)
    m = DetectionModel("yolov12-sod-fusion-v5-simple.yaml")
    shift = torch.linspace(6.0, 12.0, m.yaml["nc"])
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if re.fullmatch(r"model\.39\.cv3\.\d\.2\.bias", k):
                v.add_(shift)
    path = save_checkpoint(m, tmp_path_factory.mktemp("tta") / "trained_like.pt")
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


CANVAS = (128, 160)
FRAME_SHAPES = [(100, 150), (128, 160)]


@pytest.fixture(scope="module")
def predicted(model, cuda):
    """One batch through the predictor with and without augment, once, for the tests below."""
    from yolosod_amd.engine.predictor import DetectionPredictor
    frames = [_scene_bgr(h, w, 70 + i) for i, (h, w) in enumerate(FRAME_SHAPES)]
    inputs = [frames[0], torch.from_numpy(frames[1]).to(cuda)]
    kw = dict(conf=0.001, iou=0.7, imgsz=CANVAS, rect=False)
    aug, plain = DetectionPredictor(model, augment=True, **kw), DetectionPredictor(model, **kw)
    with _deterministic(), torch.inference_mode():
        ing = plain.ingest(inputs)
        x = ing.x
        cat = model(x, augment=True)[0]
        y1 = model(x)[0]
        res = dict(aug_t=aug.predict_padded(x), plain_t=plain.predict_padded(x), aug_l=aug.predict_padded(inputs),
                   plain_l=plain.predict_padded(inputs), off_t=DetectionPredictor(model, augment=False,
                                                                                  **kw).predict_padded(x))
    return dict(aug=aug, plain=plain, frames=frames, inputs=inputs, ing=ing, x=x, cat=cat, y1=y1, **res)


def test_predictor_augment_is_the_oracle_nms_of_cat_clipped(predicted, model):
    from oracle.nms import clip_boxes_ref, non_max_suppression_ref
    p = predicted
    assert tuple(p["x"].shape) == (2, 3, *CANVAS)
    plan = model.tta_plan(CANVAS)
    assert tuple(p["cat"].shape) == (2, 14, plan.A_tot) and plan.A_tot == 3632
    out, counts, index = (t.cpu() for t in p["aug_t"])
    want, widx = non_max_suppression_ref(p["cat"].cpu().numpy().copy(), 0.001, 0.7, max_det=300)
    assert tuple(out.shape) == (2, 300, 6) and tuple(index.shape) == (2, 300)
    for i in range(2):
        n = int(counts[i])
        assert n == len(want[i]) and n > 0
        rows = want[i].copy()
        clip_boxes_ref(rows[:, :4], CANVAS)
        assert np.array_equal(out[i, :n].numpy(), rows), i
        assert np.array_equal(index[i, :n].numpy(), widx[i]), i
        branches = np.bincount([plan.locate(j)[0] for j in index[i, :n].tolist()], minlength=3)
        print(f"image {i}: kept rows per branch {branches.tolist()}")
        assert (branches >= 1).all(), "a branch contributes nothing: the concatenation is not exercised"


def test_predictor_augment_on_frames_maps_boxes_back_as_without(predicted):
    """List input: NMS of cat, then the same ``scale_boxes`` launch with the same geometry as without augment."""
    from yolosod_amd import _hip
    from yolosod_amd.utils import ops
    p = predicted
    out, counts, index = ops.non_max_suppression_padded(p["cat"], 0.001, 0.7, max_det=300, in_place=False)
    _hip.scale_boxes_padded(out, counts, p["ing"].geom)
    for a, b in zip(p["aug_l"], (out, counts, index)):
        assert torch.equal(a, b)
    n = p["aug_l"][1].tolist()
    assert min(n) > 0
    for i, (h, w) in enumerate(FRAME_SHAPES):
        rows = p["aug_l"][0][i, :n[i]]
        assert float(rows[:, [0, 2]].max()) <= w and float(rows[:, [1, 3]].max()) <= h and float(rows[:, :4].min()) >= 0
    assert not torch.equal(p["aug_l"][0], p["plain_l"][0])


def test_predictor_without_augment_is_unchanged(predicted):
    from yolosod_amd.utils import ops
    p = predicted
    out, counts, index = ops.non_max_suppression_padded(p["y1"], 0.001, 0.7, max_det=300, in_place=False)
    ops.clip_boxes(out[..., :4], CANVAS)
    for a, b, c in zip(p["plain_t"], p["off_t"], (out, counts, index)):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert p["plain"].augment is False


def test_predictor_augment_makes_no_synchronising_call(predicted, cuda):
    p = predicted
    frames = [torch.from_numpy(f).to(cuda) for f in p["frames"]]
    with _deterministic():
        ref_l = p["aug"].predict_padded(frames)   # first use of this list: pinned blocks are set up
        ref_t = p["aug"].predict_padded(p["x"])
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "prototype feature" notice
            torch.cuda.set_sync_debug_mode("error")
        try:
            got_t = p["aug"].predict_padded(p["x"])
            got_l = p["aug"].predict_padded(frames)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    for a, b in zip(got_t + got_l, ref_t + ref_l):
        assert torch.equal(a, b)
    for a, b in zip(ref_t + ref_l, p["aug_t"] + p["aug_l"]):
        assert torch.equal(a, b)
