"""GPU: sliced inference - csrc/tile_merge.hip against its numpy restatement (tests/tile_merge_ref.py) bit for bit,
merge + NMS on planted objects against the oracle NMS on the restated tensor, and SlicedPredictor stage by stage on
lists of uint8 BGR frames.

Shapes: canvas 128, so A = 32^2 + 16^2 + 8^2 + 4^2 = 1360 (a multiple of 4: the 16-byte form), and a raw A = 85 (the
element-wise form: no row of y and no slot of merged is 16-byte aligned in general)."""
import warnings

import numpy as np
import pytest
import torch

from ingest_ref import ingest_ref
from tile_merge_ref import tile_merge_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = (True, True, True, True)
NONE = (False, False, False, False)


# ---- merge kernel ----------------------------------------------------------------------------------------------
def _merge_case(A, nc, seed):
    """5 source rows into F = 2, S = 3 in two calls (3 + 3 descriptor rows, the last one an empty slot). Rows with gain
    1 / pad 0 carry, in their first anchors, boxes built to sit exactly on the cut comparison's boundary for margins 0
    and 2 and one fp32 step to either side of it; the other rows have a non-trivial gain and pad."""
    rng = np.random.default_rng(seed)
    no = 4 + nc
    ys = []
    for n in (3, 2):
        y = np.empty((n, no, A), dtype=F32)
        y[:, 0:2] = rng.uniform(-4, 132, (n, 2, A))
        y[:, 2:4] = rng.uniform(0.5, 40, (n, 2, A))
        y[:, 4:] = rng.uniform(0, 1, (n, nc, A))
        ys.append(y)
    up, dn = (lambda v: np.nextafter(F32(v), F32(1e9))), (lambda v: np.nextafter(F32(v), F32(-1e9)))
    edge = []  # (x, y, w, h) on a 128 x 128 tile, gain 1, pad 0
    for m in (0.0, 2.0):
        for c in (5 + m, dn(5 + m), up(5 + m)):            # x1 / y1 = m, just below, just above
            edge += [(c, 64, 10, 10), (64, c, 10, 10)]
        for c in (123 - m, dn(123 - m), up(123 - m)):      # x2 / y2 = 128 - m, just below, just above
            edge += [(c, 64, 10, 10), (64, c, 10, 10)]
    edge = np.array(edge, dtype=F32).T                     # [4, 24]
    for y, k in ((ys[0], 0), (ys[0], 2), (ys[1], 0)):
        y[k, :4, :edge.shape[1]] = edge
    g = 128 / 300
    calls = [
        [(0, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, ALL),
         (1, 0, 2, g, 0, 21, 0, 0, 300, 200, NONE),                       # whole-frame slot of a (200, 300) frame
         (2, 1, 1, 1.0, 0, 0, 96, 72, 128, 128, (True, False, False, True))],
        [(0, 1, 0, 1.0, 0, 0, 172, 0, 128, 128, (False, True, True, False)),
         (-1, 0, 1, 1.0, 0, 0, 0, 0, 0, 0, NONE),
         (1, 1, 2, 128 / 150, 0, 25, 22, 3, 150, 90, ALL)],
    ]
    return ys, calls, edge.shape[1]


@pytest.mark.parametrize("cut_margin", [None, 0.0, 2.0])
@pytest.mark.parametrize("A,nc", [(85, 1), (85, 10), (1360, 1), (1360, 10)])
def test_merge_matches_the_restatement(A, nc, cut_margin, cuda):
    from yolosod_amd import _hip
    ys, calls, n_edge = _merge_case(A, nc, 100 * nc + A)
    no, Fr, S = 4 + nc, 2, 3
    N = Fr * no * S * A
    ref = np.full((Fr, no, S * A), np.nan, dtype=F32)
    buf = torch.full((N + 64,), float("nan"), device=cuda)
    merged = buf[:N].view(Fr, no, S * A)
    for k, (y, rows) in enumerate(zip(ys, calls)):
        tile_merge_ref(y, rows, ref, A, cut_margin)
        out = _hip.tile_merge(torch.from_numpy(y).to(cuda), rows, merged, A, cut_margin)
        assert out is merged
        # the bit patterns: NaN marks what no call has named yet, and must match too
        assert torch.equal(merged.cpu().view(torch.int32), torch.from_numpy(ref).view(torch.int32)), (k, A, nc)
    assert not np.isnan(ref).any() and not torch.isnan(merged).any(), "every element is defined after both calls"
    assert torch.isnan(buf[N:]).all(), "nothing outside merged is touched"
    assert (ref[0, :, A:2 * A] == 0).all(), "the empty slot holds zeros"
    # the boundary boxes do what they were built for (on the restatement): slot (0, 0), every edge interior
    s = ref[0, 4, :n_edge].reshape(2, 2, 3, 2)  # [margin 0 / 2][low / high side][on, inside-step, outside-step][x / y]
    y0 = ys[0][0, 4, :n_edge].reshape(2, 2, 3, 2)
    if cut_margin is None:
        assert (s == y0).all()
    else:
        mi = 0 if cut_margin == 0.0 else 1
        assert (s[mi, 0, 0] == 0).all() and (s[mi, 0, 1] == 0).all() and (s[mi, 0, 2] == y0[mi, 0, 2]).all()
        assert (s[mi, 1, 0] == 0).all() and (s[mi, 1, 1] == y0[mi, 1, 1]).all() and (s[mi, 1, 2] == 0).all()


def test_merge_into_a_tensor_that_is_not_16_byte_aligned(cuda):
    """A = 1360 with merged one float into its allocation: the entry point takes the element-wise form."""
    from yolosod_amd import _hip
    A, nc = 1360, 3
    ys, calls, _ = _merge_case(A, nc, 7)
    N = 2 * (4 + nc) * 3 * A
    buf = torch.full((N + 8,), float("nan"), device=cuda)
    merged = buf[1:N + 1].view(2, 4 + nc, 3 * A)
    assert merged.data_ptr() % 16 == 4 and merged.is_contiguous()
    ref = np.full((2, 4 + nc, 3 * A), np.nan, dtype=F32)
    for y, rows in zip(ys, calls):
        tile_merge_ref(y, rows, ref, A, 2.0)
        _hip.tile_merge(torch.from_numpy(y).to(cuda), rows, merged, A, 2.0)
    assert torch.equal(merged.cpu(), torch.from_numpy(ref))
    assert torch.isnan(buf[:1]).all() and torch.isnan(buf[N + 1:]).all()


def test_wrapper_refusals_launch_nothing(cuda):
    from yolosod_amd import _hip
    A = 85
    y = torch.zeros(2, 14, A, device=cuda)
    merged = torch.full((1, 14, 3 * A), float("nan"), device=cuda)
    row = (0, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE)
    with pytest.raises(RuntimeError, match="float32"):
        _hip.tile_merge(y.half(), [row], merged, A)
    with pytest.raises(RuntimeError, match="float32"):
        _hip.tile_merge(y, [row], merged.double(), A)
    with pytest.raises(RuntimeError, match="contiguous"):
        _hip.tile_merge(torch.zeros(2, A, 14, device=cuda).transpose(1, 2), [row], merged, A)
    with pytest.raises(RuntimeError, match="slot 3"):
        _hip.tile_merge(y, [row, (1, 0, 3, 1.0, 0, 0, 0, 0, 128, 128, NONE)], merged, A)
    with pytest.raises(RuntimeError, match="frame 1"):
        _hip.tile_merge(y, [(0, 1, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE)], merged, A)
    with pytest.raises(RuntimeError, match="src 2"):
        _hip.tile_merge(y, [(2, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE)], merged, A)
    with pytest.raises(RuntimeError, match="named twice"):
        _hip.tile_merge(y, [row, (1, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, NONE)], merged, A)
    with pytest.raises(RuntimeError, match="anchors"):
        _hip.tile_merge(y, [row], merged, 84)
    with pytest.raises(RuntimeError, match=r"S \* 80"):
        _hip.tile_merge(torch.zeros(2, 14, 80, device=cuda), [row], merged, 80)   # 255 is no multiple of 80
    with pytest.raises(RuntimeError, match="is not"):
        _hip.tile_merge(y, [row], torch.zeros(1, 9, 3 * A, device=cuda), A)
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.tile_merge(y.cpu(), [row], merged, A)
    with pytest.raises(RuntimeError, match="gain"):
        _hip.tile_merge(y, [(0, 0, 0, 0.0, 0, 0, 0, 0, 128, 128, NONE)], merged, A)
    with pytest.raises(RuntimeError, match="rows"):
        _hip.tile_merge(y, [], merged, A)
    torch.cuda.synchronize()
    assert torch.isnan(merged).all(), "a refused call wrote to merged"


# ---- planted objects ---------------------------------------------------------------------------------------------
PLANT_SHAPE = (200, 300)
# ground truth (cx, cy, w, h) in frame pixels, all smaller than the 32-pixel overlap: inside one tile only; in the
# overlap of two columns; cut by a column border; in the overlap of both rows and two columns; cut by a row border;
# in a corner; whole in one tile but within 2 px of its interior edge (the neighbour holds it with room to spare)
PLANTED = [(40.0, 30.0, 20.0, 16.0), (110.0, 40.0, 18.0, 22.0), (132.0, 100.0, 24.0, 14.0), (190.0, 100.0, 14.0, 20.0),
           (250.0, 70.0, 16.0, 24.0), (285.0, 185.0, 22.0, 20.0), (215.0, 30.0, 16.0, 12.0)]


@pytest.fixture(scope="module")
def planted():
    """(plan, y [7, 4+nc, 85] float32 in canvas pixels, scores) for the (200, 300) frame, slice 128, overlap 0.25:
    every slot gets, per object, the whole box if it holds it whole, the box clipped to the tile if it cuts it, nothing
    if it misses it; the whole-frame slot gets every object. Copies of object j score s_j - 0.001 * slot in the tiles
    and s_j - 0.009 in the whole-frame slot, so the best copy NMS can keep is a tile's."""
    from yolosod_amd.data.slicing import SlicePlan
    plan = SlicePlan([PLANT_SHAPE], 128, 0.25, True, 128)
    A, nc = 85, 3
    y = np.zeros((len(plan), 4 + nc, A), dtype=F32)
    y[:, 0:2] = 64
    y[:, 2:4] = 4  # background anchors: a small box in the middle, score 0
    scores = [0.9 - 0.07 * j for j in range(len(PLANTED))]
    whole = clipped = 0
    for k, slot in enumerate(plan.slots[0]):
        ty0, tx0, ty1, tx1 = slot.rect
        for j, (cx, cy, w, h) in enumerate(PLANTED):
            x1, y1, x2, y2 = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
            ix1, iy1, ix2, iy2 = max(x1, tx0), max(y1, ty0), min(x2, tx1), min(y2, ty1)
            if ix2 <= ix1 or iy2 <= iy1:
                continue
            whole += (ix1, iy1, ix2, iy2) == (x1, y1, x2, y2)
            clipped += (ix1, iy1, ix2, iy2) != (x1, y1, x2, y2)
            a = 5 + 11 * j
            y[k, 0, a] = ((ix1 + ix2) / 2 - tx0) * slot.gain + slot.pad_x
            y[k, 1, a] = ((iy1 + iy2) / 2 - ty0) * slot.gain + slot.pad_y
            y[k, 2, a] = (ix2 - ix1) * slot.gain
            y[k, 3, a] = (iy2 - iy1) * slot.gain
            y[k, 4 + j % nc, a] = scores[j] - 0.001 * (k or 9)
    assert whole > len(PLANTED) and clipped == 3, (whole, clipped)
    return plan, y, scores


def _iou(a, b):
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    return iw * ih / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - iw * ih)


@pytest.mark.parametrize("cut_margin", [None, 2.0])
def test_planted_objects_merge_and_nms_match_the_oracle(planted, cut_margin, cuda):
    from oracle.nms import non_max_suppression_ref
    from yolosod_amd import _hip
    from yolosod_amd.utils import ops
    plan, y, scores = planted
    A = y.shape[2]
    rows = plan.merge_rows(0, len(plan))
    ref = tile_merge_ref(y, rows, np.full((1, y.shape[1], plan.S * A), np.nan, dtype=F32), A, cut_margin)
    merged = torch.full((1, y.shape[1], plan.S * A), float("nan"), device=cuda)
    _hip.tile_merge(torch.from_numpy(y).to(cuda), rows, merged, A, cut_margin)
    assert torch.equal(merged.cpu(), torch.from_numpy(ref))
    max_wh = max(7680, max(PLANT_SHAPE))
    out, counts, index = ops.non_max_suppression_padded(merged, 0.25, 0.5, max_det=300, max_wh=max_wh, in_place=False)
    want, widx = non_max_suppression_ref(ref.copy(), 0.25, 0.5, max_det=300, max_wh=max_wh)
    n = int(counts[0])
    assert n == len(want[0])
    assert np.array_equal(out[0, :n].cpu().numpy(), want[0]), "rows differ from the oracle"
    assert np.array_equal(index[0, :n].cpu().numpy(), widx[0]), "indices differ from the oracle"
    # what the oracle kept, against the ground truth
    gt = [(cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2) for cx, cy, w, h in PLANTED]
    hits = [[i for i, r in enumerate(want[0]) if _iou(r[:4], g) > 0.9 and int(r[5]) == j % 3]
            for j, g in enumerate(gt)]
    print(f"cut_margin {cut_margin}: oracle kept {len(want[0])} rows for {len(gt)} objects")
    assert all(len(h) >= 1 for h in hits), "an object was lost"
    if cut_margin is None:
        assert len(want[0]) > len(gt), "no truncated copy survived NMS: the cut has nothing to remove here"
    else:
        assert len(want[0]) == len(gt) and all(len(h) == 1 for h in hits), "every object exactly once"
        # the kept copy of object j is a tile's whole copy (never a clipped one, nor the lower-scoring whole-frame one)
        for j, h in enumerate(hits):
            slot = int(widx[0][h[0]]) // A
            assert slot >= 1 and abs(float(want[0][h[0], 4]) - (scores[j] - 0.001 * slot)) < 1e-6


# ---- predictor -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory, cuda):
    """The paper model with a trained-like head, as tests/test_gpu_ingest.py builds it."""
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
    path = save_checkpoint(m, tmp_path_factory.mktemp("sliced") / "trained_like.pt")
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


@pytest.fixture(scope="module")
def staged(model, cuda):
    """The three frames through every stage of one SlicedPredictor, once, for the tests below."""
    from yolosod_amd.engine.predictor import SlicedPredictor
    frames = [_scene_bgr(h, w, 50 + i) for i, (h, w) in enumerate(SHAPES)]
    inputs = [frames[0], torch.from_numpy(frames[1]), torch.from_numpy(frames[2]).to(cuda)]  # numpy, CPU, GPU
    sp = SlicedPredictor(model, slice=128, overlap=0.25, full_frame=True, cut_margin=2.0, conf=0.001, iou=0.7,
                         imgsz=128)
    plan = sp.plan(SHAPES)
    with _deterministic():
        x = sp.ingest_tiles(inputs, plan)
        ys = sp.forward_tiles(inputs, plan)
        merged = sp.merge(ys, plan)
        post = sp.postprocess(merged, plan)
        padded = sp.predict_padded(inputs)
        dets = sp(inputs)
    return dict(sp=sp, plan=plan, frames=frames, inputs=inputs, x=x, ys=ys, merged=merged, post=post, padded=padded,
                dets=dets)


def test_predictor_tiles_are_ingested_from_the_frames_memory(staged, cuda):
    plan, frames = staged["plan"], staged["frames"]
    assert plan.S == 7 and len(plan) == 12
    crops, geoms = [], []
    for f, k in plan.order:
        y0, x0, y1, x1 = plan.slot(f, k).rect
        crops.append(frames[f][y0:y1, x0:x1])
        geoms.append(plan.slot(f, k).geometry)
    ref = ingest_ref(crops, geoms)
    assert tuple(staged["x"].shape) == (12, 3, 128, 128)
    assert torch.equal(staged["x"].cpu(), ref)
    # forward_tiles ran the model on exactly that tensor
    assert len(staged["ys"]) == 1 and tuple(staged["ys"][0].shape) == (12, 14, 1360)
    assert staged["ys"][0].dtype == torch.float32
    with _deterministic(), torch.inference_mode():
        y = staged["sp"].model(ref.to(cuda))[0]
    assert torch.equal(y, staged["ys"][0])


def test_predictor_merge_is_the_restatement(staged):
    plan, sp = staged["plan"], staged["sp"]
    A = 1360
    y = staged["ys"][0].cpu().numpy()
    ref = tile_merge_ref(y, plan.merge_rows(0, len(plan)), np.full((3, 14, plan.S * A), np.nan, dtype=F32), A,
                         sp.cut_margin)
    assert not np.isnan(ref).any()
    assert tuple(staged["merged"].shape) == (3, 14, 7 * A)
    assert torch.equal(staged["merged"].cpu(), torch.from_numpy(ref))
    assert (ref[1, :, 3 * A:] == 0).all() and (ref[2, :, 2 * A:] == 0).all(), "empty slots hold zeros"
    assert int((ref[0, 4:].max(0) == 0).sum()) > 0, "nothing was cut: the margin is not exercised"


def test_predictor_merge_does_not_depend_on_the_batch(staged, model):
    """batch = 4: the same y rows regrouped into three model calls give the same merged tensor."""
    from yolosod_amd.engine.predictor import SlicedPredictor
    sp4 = SlicedPredictor(model, slice=128, overlap=0.25, cut_margin=2.0, batch=4, conf=0.001, imgsz=128)
    plan = sp4.plan(SHAPES)
    assert plan.chunks(4) == [(0, 4), (4, 8), (8, 12)]
    chunks = list(torch.split(staged["ys"][0], 4))
    assert [c.shape[0] for c in chunks] == [4, 4, 4] and all(c.is_contiguous() for c in chunks)
    assert torch.equal(sp4.merge(chunks, plan), staged["merged"])
    uneven = [staged["ys"][0][:5], staged["ys"][0][5:6], staged["ys"][0][6:]]
    assert torch.equal(sp4.merge(uneven, plan), staged["merged"])
    with pytest.raises(ValueError, match="tiles"):
        sp4.merge(chunks[:2], plan)


def test_predictor_postprocess_is_the_oracle_nms_clipped_to_the_frame(staged):
    from oracle.nms import clip_boxes_ref, non_max_suppression_ref
    sp = staged["sp"]
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
            slots = widx[i] // 1360
            assert int(slots.max()) < len(staged["plan"].slots[i]), "a detection from an empty slot"
            assert float(rows[:, [0, 2]].max()) <= shape[1] and float(rows[:, [1, 3]].max()) <= shape[0]
    assert total > 0, "nothing kept: the comparison is empty"


def test_predictor_public_calls(staged):
    out, counts, index = staged["padded"]
    assert tuple(out.shape) == (3, 300, 6) and tuple(counts.shape) == (3,) and tuple(index.shape) == (3, 300)
    for a, b in zip(staged["padded"], staged["post"]):
        assert torch.equal(a, b)
    dets = staged["dets"]
    assert len(dets) == 3
    for i, d in enumerate(dets):
        n = int(counts[i])
        assert d.orig_shape == SHAPES[i] and tuple(d.boxes.shape) == (n, 6)
        assert torch.equal(d.boxes, out[i, :n]) and torch.equal(d.index, index[i, :n])
    with _deterministic():
        g = staged["sp"].predict_padded_guarded(staged["inputs"])
    for a, b in zip(g, staged["padded"]):
        assert torch.equal(a, b)


def test_one_tile_without_the_full_frame_is_the_plain_predictor(model, cuda):
    """One 128 x 128 frame, full_frame=False: one tile, gain 1, pad 0, offset 0 - the merge is the identity."""
    from yolosod_amd.engine.predictor import DetectionPredictor, SlicedPredictor
    frame = _scene_bgr(128, 128, 60)
    sp = SlicedPredictor(model, slice=128, overlap=0.25, full_frame=False, conf=0.001, imgsz=128)
    dp = DetectionPredictor(model, conf=0.001, imgsz=128, rect=False)
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
