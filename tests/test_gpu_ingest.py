"""GPU: the raw-frame front door - csrc/ingest.hip against its numpy restatement (tests/ingest_ref.py) bit for bit,
boxes back to frame pixels against utils.ops.scale_boxes on the CPU bit for bit, and DetectionPredictor on lists of
uint8 BGR frames against the same model fed the restated tensor.

Kernel cases (canvas 64 x 96, one 16 x 64 tile grid of 4 x 2 with a partial second tile column): every way a source
row can be misaligned (3 w % 4 = 3, 1; a cropped view whose base address is 3 mod 4 and whose pitch is not 3 w),
clamped taps (1 x 1, 2 x 3), the identity, borders on either axis and of unequal size, and the three staging forms:
the contiguous source-row range (up-scales, mild down-scales), the two-rows-per-output-row form (3x down-scale) and
the tile whose source window exceeds the LDS block (9x down-scale: taps straight from global memory)."""
import warnings

import numpy as np
import pytest
import torch

from ingest_ref import ingest_ref

pytestmark = pytest.mark.gpu

CANVAS = (64, 96)


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _lb_geom(shape, canvas=CANVAS, **kw):
    from yolosod_amd.data.augment import LetterBox
    return LetterBox(canvas, **kw).geometry(shape)


def _cases():
    """name -> (frame as a numpy array (possibly a view), geometry)"""
    c = {}
    c["down_37x53"] = (_frame(37, 53, 1), (23, 33, 20, 31, *CANVAS))       # 3 w % 4 = 3
    c["up_9x7"] = (_frame(9, 7, 2), (20, 16, 22, 40, *CANVAS))             # 3 w % 4 = 1
    c["one_pixel"] = (_frame(1, 1, 3), (4, 4, 30, 46, *CANVAS))            # every tap clamped
    c["two_by_three"] = (_frame(2, 3, 4), (7, 5, 28, 45, *CANVAS))
    c["identity"] = (_frame(64, 96, 5), _lb_geom((64, 96)))                # no border
    c["portrait"] = (_frame(100, 60, 6), _lb_geom((100, 60)))              # left / right border
    c["odd_dh"] = (_frame(47, 96, 7), _lb_geom((47, 96)))                  # top 8, bottom 9
    c["down3_200x300"] = (_frame(200, 300, 8), _lb_geom((200, 300)))       # two staged rows per output row
    c["down9_120x900"] = (_frame(120, 900, 9), _lb_geom((120, 900)))       # source window larger than the LDS block
    return c


def _to_gpu(frame, cuda, offset=0):
    """The frame on the GPU at ``offset`` bytes into its own allocation."""
    buf = torch.empty(frame.size + offset, dtype=torch.uint8, device=cuda)
    t = buf[offset:].view(frame.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(frame)))
    return t


@pytest.fixture(scope="module")
def crop_case(cuda):
    """A (20, 30) crop at (3, 5) of a (40, 50) frame that starts 2 bytes into its allocation: pitch 150 != 90 and a
    base address that is 3 mod 4."""
    full = _frame(40, 50, 10)
    g = _to_gpu(full, cuda, offset=2)[3:23, 5:35]
    assert g.data_ptr() % 4 == 3 and g.stride(0) == 150
    return full[3:23, 5:35], g, _lb_geom((20, 30))


def test_assumptions_of_the_cases():
    assert _lb_geom((47, 96))[2:4] == (8, 0) and _lb_geom((47, 96))[4] - 47 - 8 == 9
    assert _lb_geom((100, 60))[3] > 0 and _lb_geom((100, 60))[2] == 0
    assert _lb_geom((120, 900))[:2] == (13, 96)


@pytest.mark.parametrize("name", list(_cases()))
def test_ingest_matches_the_restatement(name, cuda):
    from yolosod_amd import _hip
    frame, geom = _cases()[name]
    ref = ingest_ref([frame], [geom])
    got = _hip.letterbox_ingest([_to_gpu(frame, cuda)], CANVAS, [geom])
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, *CANVAS)
    assert torch.equal(got.cpu(), ref), (name, float((got.cpu() - ref).abs().max()))


def test_ingest_cropped_view(crop_case, cuda):
    from yolosod_amd import _hip
    frame, g, geom = crop_case
    got = _hip.letterbox_ingest([g], CANVAS, [geom])
    assert torch.equal(got.cpu(), ingest_ref([frame], [geom]))


@pytest.fixture(scope="module")
def mixed_batch(crop_case, cuda):
    """Four frames of different sizes in one launch, written through a batch stride larger than one image into a
    NaN-filled buffer: (frames, geoms, reference, the buffer, the [4, 3, 64, 96] view the kernel wrote)."""
    from yolosod_amd import _hip
    cs = _cases()
    names = ["down_37x53", "portrait", "down9_120x900"]
    frames = [cs[n][0] for n in names] + [crop_case[0]]
    geoms = [cs[n][1] for n in names] + [crop_case[2]]
    dev = [_to_gpu(f, cuda, offset=i) for i, f in enumerate(frames[:3])] + [crop_case[1]]
    n = 3 * CANVAS[0] * CANVAS[1]
    buf = torch.full((4, n + 64), float("nan"), device=cuda)
    view = buf[:, :n].view(4, 3, *CANVAS)
    _hip.letterbox_ingest(dev, CANVAS, geoms, out=view)
    return dev, geoms, ingest_ref(frames, geoms), buf.cpu(), view


def test_mixed_batch_in_one_launch_writes_every_element_and_nothing_else(mixed_batch):
    _, _, ref, buf, view = mixed_batch
    n = ref[0].numel()
    assert not torch.isnan(buf[:, :n]).any()
    assert torch.isnan(buf[:, n:]).all()
    assert torch.equal(view.cpu(), ref)


def test_bf16_output_is_the_fp32_result_rounded_once(mixed_batch, cuda):
    from yolosod_amd import _hip
    dev, geoms, ref, _, _ = mixed_batch
    got = _hip.letterbox_ingest(dev, CANVAS, geoms, dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.cpu().view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))


def test_wrapper_refusals_launch_nothing(cuda):
    from yolosod_amd import _hip
    g = [(64, 64, 0, 16, *CANVAS)]
    with pytest.raises(RuntimeError, match="uint8"):
        _hip.letterbox_ingest([torch.zeros(8, 8, 3, device=cuda)], CANVAS, g)
    with pytest.raises(RuntimeError, match=r"\[h, w, 3\]"):
        _hip.letterbox_ingest([torch.zeros(8, 8, 4, dtype=torch.uint8, device=cuda)], CANVAS, g)
    rgba = torch.zeros(8, 8, 4, dtype=torch.uint8, device=cuda)
    with pytest.raises(RuntimeError, match="pixel stride"):
        _hip.letterbox_ingest([rgba[:, :, :3]], CANVAS, g)
    with pytest.raises(RuntimeError, match="channel stride"):
        _hip.letterbox_ingest([torch.zeros(3, 8, 8, dtype=torch.uint8, device=cuda).permute(1, 2, 0)], CANVAS, g)
    with pytest.raises(RuntimeError, match="canvas"):
        _hip.letterbox_ingest([torch.zeros(8, 8, 3, dtype=torch.uint8, device=cuda)], CANVAS, [(64, 96, 8, 0, *CANVAS)])
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.letterbox_ingest([torch.zeros(8, 8, 3, dtype=torch.uint8, device=cuda)], (64, 30), [(30, 30, 17, 0, 64, 30)])


def test_scale_boxes_padded_matches_cpu_scale_boxes(cuda):
    """B = 3, D = 8, counts (8, 3, 0); landscape, portrait and up-scaled frames on a 128 x 128 canvas; boxes spill
    past the canvas on every side."""
    from yolosod_amd import _hip
    from yolosod_amd.utils.ops import scale_boxes
    canvas = (128, 128)
    shapes = [(1080, 1920), (100, 60), (33, 47)]
    g = torch.Generator().manual_seed(11)
    det = torch.rand(3, 8, 6, generator=g)
    det[..., :4] = det[..., :4] * 168 - 20  # [-20, 148): beyond every edge of the canvas
    det[0, 0, :4] = torch.tensor([-5.0, -7.0, 140.0, 133.0])
    counts = torch.tensor([8, 3, 0], dtype=torch.int32)
    rows = []
    for h0, w0 in shapes:
        gain = min(canvas[0] / h0, canvas[1] / w0)
        rows.append([gain, round((canvas[1] - w0 * gain) / 2 - 0.1), round((canvas[0] - h0 * gain) / 2 - 0.1), w0, h0])
    geom = torch.tensor(rows, dtype=torch.float64).float()
    got = _hip.scale_boxes_padded(det.to(cuda), counts.to(cuda), geom.to(cuda)).cpu()
    spilled = 0
    for b, (shape, n) in enumerate(zip(shapes, counts.tolist())):
        want = scale_boxes(canvas, det[b, :n, :4].clone(), shape)
        assert torch.equal(got[b, :n, :4], want), (b, got[b, :n, :4], want)
        assert torch.equal(got[b, n:], det[b, n:]) and torch.equal(got[b, :, 4:], det[b, :, 4:])
        spilled += int(((want == 0).any(1) | (want[:, [0, 2]] == shape[1]).any(1)
                        | (want[:, [1, 3]] == shape[0]).any(1)).sum())
    assert spilled > 0, "no box was clamped"


# ---- predictor -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory, cuda):
    """The paper model with a trained-like head, as tests/test_gpu_checkpoint.py builds it."""
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
    path = save_checkpoint(m, tmp_path_factory.mktemp("ingest") / "trained_like.pt")
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


def _check_predictor(pred, frames, inputs, canvas, cuda):
    """pred(inputs) (raw frames) against the same predictor's model and NMS fed the restated tensor, followed by the
    CPU scale_boxes per image (predict.py:23-41). Returns the number of kept boxes."""
    from yolosod_amd.data.augment import LetterBox
    from yolosod_amd.utils import ops
    shapes = [f.shape[:2] for f in frames]
    auto = all(s == shapes[0] for s in shapes) if pred.rect is None else pred.rect
    geoms = [LetterBox(pred.imgsz, auto=auto, stride=32).geometry(s) for s in shapes]
    assert all(g[4:] == canvas for g in geoms)
    x = ingest_ref(frames, geoms).to(cuda)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True  # MIOpen split-K atomics otherwise vary run to run
    try:
        got = pred(inputs)
        with torch.inference_mode():
            assert torch.equal(pred.preprocess(inputs), x)
            y = pred.model(x)[0]
            out, counts, index = ops.non_max_suppression_padded(y, pred.conf, pred.iou, max_det=pred.max_det,
                                                                in_place=False)
            tout, tcounts, tindex = pred.predict_padded(x)  # the tensor path: same rows, boxes clipped to the canvas
    finally:
        torch.backends.cudnn.deterministic = det
    assert torch.equal(tcounts, counts) and torch.equal(tindex, index) and torch.equal(tout[..., 4:], out[..., 4:])
    out, index = out.cpu(), index.cpu()
    total = 0
    for i, (d, shape) in enumerate(zip(got, shapes)):
        n = int(counts[i])
        total += n
        assert d.orig_shape == tuple(shape) and d.boxes.shape == (n, 6)
        want = out[i, :n].clone()
        want[:, :4] = ops.scale_boxes(canvas, want[:, :4].clone(), shape)
        assert torch.equal(d.boxes.cpu(), want), (i, float((d.boxes.cpu() - want).abs().max()))
        assert torch.equal(d.index.cpu(), index[i, :n])
        if n:
            assert float(want[:, [0, 2]].max()) <= shape[1] and float(want[:, [1, 3]].max()) <= shape[0]
    return total, got


def test_predictor_on_raw_frames_square_canvas(model, cuda):
    from yolosod_amd.engine.predictor import DetectionPredictor
    pred = DetectionPredictor(model, conf=0.001, iou=0.7, imgsz=128)
    frames = [_scene_bgr(h, w, 20 + i) for i, (h, w) in enumerate([(60, 100), (100, 60), (128, 128), (33, 47)])]
    # numpy arrays, a CPU tensor and a GPU tensor in one list
    inputs = [frames[0], torch.from_numpy(frames[1]), frames[2], torch.from_numpy(frames[3]).to(cuda)]
    total, got = _check_predictor(pred, frames, inputs, (128, 128), cuda)
    assert total > 0, "nothing kept: the comparison is empty"
    # the same frame as a numpy array and as a GPU tensor
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        a = pred([frames[0]])[0]
        b = pred([torch.from_numpy(frames[0]).to(cuda)])[0]
    finally:
        torch.backends.cudnn.deterministic = det
    assert torch.equal(a.boxes, b.boxes) and torch.equal(a.index, b.index) and a.orig_shape == b.orig_shape == (60, 100)


def test_predictor_on_raw_frames_rect_canvas(model, cuda):
    """Four same-shape (60, 100) frames: rect=None takes the minimal rectangle, 96 x 128."""
    from yolosod_amd.engine.predictor import DetectionPredictor
    pred = DetectionPredictor(model, conf=0.001, iou=0.7, imgsz=128)
    frames = [_scene_bgr(60, 100, 30 + i) for i in range(4)]
    total, _ = _check_predictor(pred, frames, frames, (96, 128), cuda)
    assert total > 0
    out, counts, index = pred.predict_padded(frames)
    assert tuple(out.shape) == (4, 300, 6) and int(counts.sum()) == total
    # rect=False forces the square canvas
    sq = DetectionPredictor(model, conf=0.001, iou=0.7, imgsz=128, rect=False)
    assert tuple(sq.preprocess(frames).shape) == (4, 3, 128, 128)


def test_ingest_and_boxes_back_make_no_synchronising_call(model, cuda):
    """predict_padded stays free of host syncs: what the list branch adds to it (ingest of CPU and GPU frames, the
    geometry upload, the boxes-back launch) runs under torch's sync debug mode set to raise."""
    from yolosod_amd import _hip
    from yolosod_amd.engine.predictor import DetectionPredictor
    pred = DetectionPredictor(model, imgsz=128)
    frames = [_scene_bgr(60, 100, 40), torch.from_numpy(_scene_bgr(33, 47, 41)).to(cuda)]
    out = torch.rand(2, 300, 6, device=cuda) * 128
    counts = torch.tensor([300, 7], dtype=torch.int32, device=cuda)
    ref = pred.ingest(frames)  # first use: pinned blocks and code objects are set up
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "prototype feature" notice
        torch.cuda.set_sync_debug_mode("error")
    try:
        ing = pred.ingest(frames)
        _hip.scale_boxes_padded(out, counts, ing.geom)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(ing.x, ref.x) and ing.shapes == [(60, 100), (33, 47)]


def test_model_at_a_rect_shape_matches_oracle(model, cuda):
    """The whole model at 96 x 128 (no other whole-model test is non-square) against the CPU oracle, with the
    tolerances tests/test_gpu_model.py uses at 128 x 128 (oplib.pred_close)."""
    from oplib import pred_close
    from oracle.model_ref import build_cpu_model
    from yolosod_amd.nn.tasks import build_model
    gm = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda)
    cpu = build_cpu_model()
    cpu.load_state_dict({k: v.cpu() for k, v in gm.state_dict().items()})
    x = torch.rand(2, 3, 96, 128, generator=torch.Generator().manual_seed(12))
    with torch.inference_mode():
        y = gm(x.to(cuda))[0].cpu()
        ref = cpu(x)[0]
    assert y.shape == ref.shape == (2, 14, 24 * 32 + 12 * 16 + 6 * 8 + 3 * 4)
    ok, msg = pred_close(y, ref)
    assert ok, msg
