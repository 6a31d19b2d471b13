"""GPU: the NV12 front door - csrc/ingest_nv12.hip against its numpy restatement (tests/nv12_ref.py: the integer colour
conversion, then tests/ingest_ref.py) bit for bit, against the BGR kernel on the converted frames, and both predictors
on lists of NV12Frame against themselves on the converted BGR frames.

Kernel cases (canvas 64 x 96, a 4 x 2 grid of 16 x 64 tiles with a partial second tile column) are the NV12
counterparts of tests/test_gpu_ingest.py's, with even sizes: clamped taps (2 x 2, thin frames), the identity, borders
on either axis and of unequal size, and the three staging forms - the contiguous source-row range, the
two-rows-per-output-row form (3x down-scale) and the tile whose window exceeds the LDS block (taps converted from
global memory). LetterBox centres a 46 x 96 frame on this canvas with 9 rows above and below, so that case takes the
geometry by hand: 8 above, 10 below. Then every way the two planes can be misaligned and pitched, crops at all four
origin parities with odd extents, the arithmetic of each matrix on every (U, V) pair, and one mixed launch."""
import warnings

import numpy as np
import pytest
import torch

from ingest_ref import ingest_ref
from nv12_ref import frame_to_bgr_u8, ingest_nv12_ref, make_nv12, nv12_to_bgr_u8

pytestmark = pytest.mark.gpu

CANVAS = (64, 96)
MATRICES = ("bt601", "bt709", "bt601_full", "bt709_full")


def _lb_geom(shape, canvas=CANVAS, **kw):
    from yolosod_amd.data.augment import LetterBox
    return LetterBox(canvas, **kw).geometry(shape)


def _plane_to_gpu(a, cuda, offset=0, pitch=None, fill=0):
    """The [rows, n] or [rows, n/2, 2] uint8 plane on the GPU, ``offset`` bytes into its own allocation, rows ``pitch``
    bytes apart (None: packed); the bytes between the rows hold ``fill``."""
    rows, n = a.shape[0], a[0].size
    pitch = n if pitch is None else pitch
    buf = torch.full((offset + rows * pitch,), fill, dtype=torch.uint8, device=cuda)
    t = buf[offset:].as_strided((rows, n), (pitch, 1), offset)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(rows, n)))
    return t if a.ndim == 2 else buf.as_strided((rows, n // 2, 2), (pitch, 2, 1), offset)


def _surface(y, uv, cuda, matrix="bt601", yoff=0, uvoff=0, pitch=None, fill=0):
    from yolosod_amd.data import NV12Frame
    return NV12Frame(_plane_to_gpu(y, cuda, yoff, pitch, fill), _plane_to_gpu(uv, cuda, uvoff, pitch, fill), matrix)


def _cases():
    """name -> ((h, w), geometry)"""
    c = {}
    c["smallest_2x2"] = ((2, 2), (4, 4, 30, 46, *CANVAS))                  # every tap clamped
    c["up_10x8"] = ((10, 8), (20, 16, 22, 40, *CANVAS))
    c["thin_2x6"] = ((2, 6), _lb_geom((2, 6)))
    c["thin_6x2"] = ((6, 2), _lb_geom((6, 2)))
    c["identity"] = ((64, 96), _lb_geom((64, 96)))                         # no border
    c["portrait"] = ((100, 60), _lb_geom((100, 60)))                       # left / right border
    c["odd_dh"] = ((46, 96), (46, 96, 8, 0, *CANVAS))                      # top 8, bottom 10
    c["down3_200x300"] = ((200, 300), _lb_geom((200, 300)))                # two staged rows per output row
    c["down9_120x900"] = ((120, 900), _lb_geom((120, 900)))                # source window larger than the LDS block
    c["down_38x54"] = ((38, 54), (23, 33, 20, 31, *CANVAS))                # contiguous staging
    return c


def test_assumptions_of_the_cases():
    assert _lb_geom((100, 60))[3] > 0 and _lb_geom((100, 60))[2] == 0
    assert _lb_geom((120, 900))[:2] == (13, 96)
    assert _lb_geom((64, 96)) == (64, 96, 0, 0, 64, 96)
    assert _lb_geom((200, 300))[:2] == (64, 96)
    g = _cases()["odd_dh"][1]
    assert g[2] == 8 and g[4] - g[0] - g[2] == 10


@pytest.mark.parametrize("name", list(_cases()))
def test_ingest_matches_the_restatement(name, cuda):
    from yolosod_amd import _hip
    (h, w), geom = _cases()[name]
    k = list(_cases()).index(name)
    matrix = MATRICES[k % 4]
    y, uv = make_nv12(h, w, 100 + k)
    ref = ingest_nv12_ref([(y, uv, matrix)], [geom])
    got = _hip.letterbox_ingest_nv12([_surface(y, uv, cuda, matrix)], CANVAS, [geom])
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, *CANVAS)
    assert torch.equal(got.cpu(), ref), (name, float((got.cpu() - ref).abs().max()))
    if name == "identity":  # the converted frame / 255 itself
        bgr = nv12_to_bgr_u8(y, uv, matrix)
        want = torch.from_numpy(np.ascontiguousarray(bgr[:, :, ::-1].transpose(2, 0, 1))).float() / 255
        assert torch.equal(got[0].cpu(), want)


# ---- addresses and pitches -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("yoff,uvoff", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (3, 1), (1, 2)])
def test_planes_at_any_byte_address(yoff, uvoff, cuda):
    from yolosod_amd import _hip
    geoms = [_cases()["down_38x54"][1], _cases()["up_10x8"][1], _lb_geom((200, 300))]
    planes = [make_nv12(38, 54, 120), make_nv12(10, 8, 121), make_nv12(200, 300, 122)]
    fs = [_surface(y, uv, cuda, "bt601", yoff, uvoff) for y, uv in planes]
    assert all(f.y.data_ptr() % 4 == yoff and f.uv.data_ptr() % 4 == uvoff for f in fs)
    got = _hip.letterbox_ingest_nv12(fs, CANVAS, geoms)
    assert torch.equal(got.cpu(), ingest_nv12_ref([(y, uv, "bt601") for y, uv in planes], geoms))


def test_pitched_planes_do_not_leak_their_padding(cuda):
    """w = 100 with pitch 128 on both planes; the padding holds 255, the picture never does."""
    from yolosod_amd import _hip
    y, uv = (np.minimum(p, 254) for p in make_nv12(40, 100, 130))
    for yoff, uvoff in [(0, 0), (1, 2)]:
        f = _surface(y, uv, cuda, "bt709", yoff, uvoff, pitch=128, fill=255)
        assert f.y.stride() == (128, 1) and f.uv.stride() == (128, 2, 1)
        for geom in (_lb_geom((40, 100)), (40, 96, 12, 0, *CANVAS)):
            got = _hip.letterbox_ingest_nv12([f], CANVAS, [geom])
            assert torch.equal(got.cpu(), ingest_nv12_ref([(y, uv, "bt709")], [geom]))


def test_separate_allocations_and_one_packed_buffer(cuda):
    from yolosod_amd import _hip
    from yolosod_amd.data import NV12Frame
    y, uv = make_nv12(38, 54, 131)
    geom = _cases()["down_38x54"][1]
    ref = ingest_nv12_ref([(y, uv, "bt601_full")], [geom])
    packed = torch.from_numpy(np.concatenate([y, uv.reshape(19, 54)])).to(cuda)
    a = NV12Frame.from_packed(packed, "bt601_full")
    assert a.uv.data_ptr() == a.y.data_ptr() + 38 * 54
    b = _surface(y, uv, cuda, "bt601_full")
    assert abs(b.uv.data_ptr() - b.y.data_ptr()) != 38 * 54
    for f in (a, b):
        assert torch.equal(_hip.letterbox_ingest_nv12([f], CANVAS, [geom]).cpu(), ref)


# ---- crops -------------------------------------------------------------------------------------------------------------
CROPS = [(2, 4, 22, 34), (3, 4, 22, 33), (2, 5, 21, 34), (3, 5, 40, 50), (1, 1, 2, 2), (39, 49, 40, 50), (5, 3, 40, 4),
         (7, 0, 8, 50), (1, 7, 38, 50), (0, 0, 40, 50), (4, 6, 10, 17)]


def test_crops_at_every_origin_parity_with_even_and_odd_extents(cuda):
    """Views of a 40 x 50 surface that starts 1 byte into its allocations, pitch 56: all four origin parities, even and
    odd extents, single rows / columns / pixels, and crops that end on the surface's last (odd) row and column."""
    from yolosod_amd import _hip
    y, uv = make_nv12(40, 50, 140)
    surf = _surface(y, uv, cuda, "bt709_full", 1, 1, pitch=56, fill=255)
    full = nv12_to_bgr_u8(y, uv, "bt709_full")
    views = [surf.crop(*r) for r in CROPS]
    assert {v.parity for v in views} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(v.shape[0] & 1, v.shape[1] & 1) for v in views} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(r[2] == 40 and r[3] == 50 and r[0] & 1 and r[1] & 1 for r in CROPS)
    geoms = [_lb_geom(v.shape) for v in views]
    got = _hip.letterbox_ingest_nv12(views, CANVAS, geoms)
    ref = ingest_ref([full[y0:y1, x0:x1] for y0, x0, y1, x1 in CROPS], geoms)
    for i, r in enumerate(CROPS):
        assert torch.equal(got[i].cpu(), ref[i]), (r, float((got[i].cpu() - ref[i]).abs().max()))
    # a crop of a crop is the crop
    v = surf.crop(1, 1, 40, 50).crop(2, 4, 39, 48)
    g = _lb_geom(v.shape)
    assert torch.equal(_hip.letterbox_ingest_nv12([v], CANVAS, [g]).cpu(), ingest_ref([full[3:40, 5:49]], [g]))


# ---- arithmetic --------------------------------------------------------------------------------------------------------
YVALS = (0, 1, 15, 16, 17, 64, 128, 200, 234, 235, 236, 240, 254, 255)


@pytest.fixture(scope="module")
def every_pair():
    """A 1024 x 1024 surface: the 512 x 512 chroma plane holds each of the 65536 (U, V) pairs four times (pair id =
    (i * 512 + j) mod 65536, repetition i // 128), and the 16 luma pixels under the four copies of a pair hold
    YVALS (the first two twice)."""
    i, j = np.meshgrid(np.arange(512), np.arange(512), indexing="ij")
    pid = (i * 512 + j) % 65536
    uv = np.stack([pid >> 8, pid & 255], -1).astype(np.uint8)
    r, c = np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij")
    slot = (r >> 8) * 4 + (r & 1) * 2 + (c & 1)  # (r >> 1) // 128 = r >> 8
    y = np.asarray(YVALS, dtype=np.uint8)[slot % len(YVALS)]
    combos = (y.astype(np.int64) << 16) | (uv[r >> 1, c >> 1, 0].astype(np.int64) << 8) | uv[r >> 1, c >> 1, 1]
    assert len(np.unique(combos)) == len(YVALS) * 65536, "the image does not hold every (Y, U, V) combination"
    return y, uv


@pytest.mark.parametrize("matrix", MATRICES)
def test_every_chroma_pair_under_the_luma_edge_values(matrix, every_pair, cuda):
    from yolosod_amd import _hip
    y, uv = every_pair
    geom = (1024, 1024, 0, 0, 1024, 1024)
    bgr = nv12_to_bgr_u8(y, uv, matrix)
    assert bgr.min() == 0 and bgr.max() == 255, "neither saturation is reached"
    want = torch.from_numpy(np.ascontiguousarray(bgr[:, :, ::-1].transpose(2, 0, 1))).float() / 255
    got = _hip.letterbox_ingest_nv12([_surface(y, uv, cuda, matrix)], (1024, 1024), [geom])[0].cpu()
    assert torch.equal(got, want), float((got - want).abs().max())
    if matrix == "bt601":  # the identity of the restated resize, once
        assert torch.equal(ingest_ref([bgr], [geom])[0], want)


# ---- one launch, mixed -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_batch(cuda):
    """Four frames of different sizes, matrices and alignments in one launch, written through a batch stride larger
    than one image into a NaN-filled buffer: (frames, geoms, BGR frames, reference, the buffer, the view written)."""
    from yolosod_amd import _hip
    specs = [((38, 54), "bt601", 1, 2, None, _cases()["down_38x54"][1]),
             ((100, 60), "bt709", 2, 1, 64, _lb_geom((100, 60))),
             ((120, 900), "bt601_full", 3, 0, None, _lb_geom((120, 900))),
             ((40, 50), "bt709_full", 0, 1, 56, None)]
    frames, bgr = [], []
    for k, ((h, w), matrix, yoff, uvoff, pitch, _) in enumerate(specs):
        y, uv = make_nv12(h, w, 150 + k)
        f = _surface(y, uv, cuda, matrix, yoff, uvoff, pitch, fill=255)
        full = nv12_to_bgr_u8(y, uv, matrix)
        if k == 3:  # an odd-sized view at an odd origin
            f, full = f.crop(3, 5, 24, 36), full[3:24, 5:36]
        frames.append(f)
        bgr.append(full)
    geoms = [s[5] for s in specs[:3]] + [_lb_geom((21, 31))]
    n = 3 * CANVAS[0] * CANVAS[1]
    buf = torch.full((4, n + 64), float("nan"), device=cuda)
    view = buf[:, :n].view(4, 3, *CANVAS)
    assert _hip.letterbox_ingest_nv12(frames, CANVAS, geoms, out=view) is view
    return frames, geoms, bgr, ingest_ref(bgr, geoms), buf.cpu(), view


def test_mixed_batch_in_one_launch_writes_every_element_and_nothing_else(mixed_batch):
    _, _, _, ref, buf, view = mixed_batch
    n = ref[0].numel()
    assert not torch.isnan(buf[:, :n]).any()
    assert torch.isnan(buf[:, n:]).all()
    assert torch.equal(view.cpu(), ref)


def test_mixed_batch_equals_the_bgr_kernel_on_the_converted_frames(mixed_batch, cuda):
    from yolosod_amd import _hip
    frames, geoms, bgr, ref, _, view = mixed_batch
    for f, b in zip(frames, bgr):
        assert np.array_equal(frame_to_bgr_u8(f), b)
    dev = [torch.from_numpy(np.ascontiguousarray(b)).to(cuda) for b in bgr]
    assert torch.equal(_hip.letterbox_ingest(dev, CANVAS, geoms), view)
    got = _hip.letterbox_ingest_nv12(frames, CANVAS, geoms, dtype=torch.bfloat16)
    assert torch.equal(_hip.letterbox_ingest(dev, CANVAS, geoms, dtype=torch.bfloat16), got)


def test_bf16_output_is_the_fp32_result_rounded_once(mixed_batch):
    from yolosod_amd import _hip
    frames, geoms, _, ref, _, _ = mixed_batch
    got = _hip.letterbox_ingest_nv12(frames, CANVAS, geoms, dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.cpu().view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))


def test_other_pad_value_and_op_timer_key(mixed_batch):
    from yolosod_amd import _hip
    frames, geoms, bgr, _, _, _ = mixed_batch
    with _hip.op_timer() as t:
        got = _hip.letterbox_ingest_nv12(frames, CANVAS, geoms, pad_value=0)
        _hip.letterbox_ingest_nv12(frames, CANVAS, geoms, dtype=torch.bfloat16)
    assert torch.equal(got.cpu(), ingest_ref(bgr, geoms, pad=0))
    assert [k for k, _ in t.durations_ms()] == [("ingest_nv12", (4, 3, *CANVAS), None),
                                                ("ingest_nv12", (4, 3, *CANVAS), 2)]


def test_wrapper_refusals_launch_nothing(cuda):
    from yolosod_amd import _hip
    from yolosod_amd.data import NV12Frame
    y, uv = make_nv12(8, 8, 160)
    ok = _surface(y, uv, cuda)
    g = [(64, 64, 0, 16, *CANVAS)]
    out = torch.full((1, 3, *CANVAS), float("nan"), device=cuda)
    run = lambda frames, geoms=g, canvas=CANVAS, **kw: _hip.letterbox_ingest_nv12(frames, canvas, geoms, out=out, **kw)
    with pytest.raises(TypeError, match="NV12Frame"):
        run([torch.zeros(8, 8, 3, dtype=torch.uint8, device=cuda)])
    with pytest.raises(RuntimeError, match="GPU"):
        run([NV12Frame(y, uv)])
    with pytest.raises(RuntimeError, match="GPU"):
        run([NV12Frame(ok.y, uv)])                                          # uv left on the CPU
    with pytest.raises(RuntimeError, match="element stride"):
        run([NV12Frame(torch.zeros(8, 16, dtype=torch.uint8, device=cuda)[:, ::2], ok.uv)])
    with pytest.raises(RuntimeError, match="pixel stride"):
        run([NV12Frame(ok.y, torch.zeros(4, 8, 2, dtype=torch.uint8, device=cuda)[:, ::2])])
    with pytest.raises(RuntimeError, match="channel stride"):
        run([NV12Frame(ok.y, torch.zeros(4, 2, 4, dtype=torch.uint8, device=cuda).permute(0, 2, 1)[:, :, :2])])
    big = NV12Frame(torch.zeros(2, 16386, dtype=torch.uint8, device=cuda),
                    torch.zeros(1, 8193, 2, dtype=torch.uint8, device=cuda))
    with pytest.raises(RuntimeError, match="outside"):
        run([big])
    with pytest.raises(RuntimeError, match="canvas"):
        run([ok], [(64, 96, 8, 0, *CANVAS)])
    with pytest.raises(RuntimeError, match="unsupported"):
        _hip.letterbox_ingest_nv12([ok], (64, 30), [(30, 30, 17, 0, 64, 30)])
    with pytest.raises(RuntimeError, match="out must be"):
        _hip.letterbox_ingest_nv12([ok], CANVAS, g, out=out.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="out must be"):
        _hip.letterbox_ingest_nv12([ok], CANVAS, g, out=torch.zeros(3 * 64 * 96 + 4, device=cuda)[1:-3].view(1, 3, *CANVAS))
    with pytest.raises(RuntimeError, match="dtype"):
        run([ok], dtype=torch.float16)
    with pytest.raises(RuntimeError, match="geometries"):
        run([ok, ok])
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to out"
    run([ok])
    assert not torch.isnan(out).any()


# ---- predictors --------------------------------------------------------------------------------------------------------
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
    path = save_checkpoint(m, tmp_path_factory.mktemp("ingest_nv12") / "trained_like.pt")
    return attempt_load_one_weight(path, device=cuda)[0]


def _scene_nv12(h, w, seed):
    """(y, uv) with flat rectangles under noise in the luma and two colours per rectangle in the chroma."""
    rng = np.random.default_rng(seed)
    y = np.empty((h, w), dtype=np.float64)
    uv = np.empty((h // 2, w // 2, 2), dtype=np.float64)
    y[:], uv[:] = rng.integers(16, 236), rng.integers(16, 241, 2)
    for _ in range(8):
        y0, x0 = rng.integers(0, h - 2), rng.integers(0, w - 2)
        y1, x1 = y0 + rng.integers(3, max(4, h // 2)), x0 + rng.integers(3, max(4, w // 2))
        y[y0:y1, x0:x1] = rng.integers(0, 256)
        uv[y0 // 2:y1 // 2, x0 // 2:x1 // 2] = rng.integers(0, 256, 2)
    return (np.clip(y + rng.normal(0, 12, y.shape), 0, 255).astype(np.uint8),
            np.clip(uv + rng.normal(0, 4, uv.shape), 0, 255).astype(np.uint8))


class _deterministic:
    """MIOpen split-K atomics otherwise vary run to run."""

    def __enter__(self):
        self.prev = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.prev
        return False


def _same_detections(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.orig_shape == v.orig_shape
        assert torch.equal(u.boxes, v.boxes) and torch.equal(u.index, v.index)


@pytest.mark.parametrize("canvas,shapes", [((128, 128), [(60, 100), (100, 60), (128, 128), (34, 46)]),
                                           ((96, 128), [(60, 100)] * 4)])
def test_predictor_on_nv12_frames(canvas, shapes, model, cuda):
    """Square canvas (mixed sizes, CPU and GPU frames, numpy and torch planes, two matrices) and the minimal rectangle of
    same-shape frames: ingest and detections against the same predictor on the converted BGR frames, and the detections
    as tests/test_gpu_ingest.py's _check_predictor compares them (model and NMS on the restated tensor, CPU scale_boxes)."""
    from test_gpu_ingest import _check_predictor
    from yolosod_amd.data import NV12Frame
    from yolosod_amd.engine.predictor import DetectionPredictor
    pred = DetectionPredictor(model, conf=0.001, iou=0.7, imgsz=128)
    planes = [_scene_nv12(h, w, 170 + i) for i, (h, w) in enumerate(shapes)]
    mats = ["bt601", "bt709", "bt601", "bt709"]
    bgr = [nv12_to_bgr_u8(y, uv, m) for (y, uv), m in zip(planes, mats)]
    nv = [NV12Frame(planes[0][0], planes[0][1], mats[0]),
          NV12Frame(torch.from_numpy(planes[1][0]), torch.from_numpy(planes[1][1]), mats[1]),
          NV12Frame.from_packed(np.concatenate([planes[2][0], planes[2][1].reshape(shapes[2][0] // 2, -1)]), mats[2]),
          NV12Frame(planes[3][0], planes[3][1], mats[3]).to(cuda)]
    a, b = pred.ingest(nv), pred.ingest(bgr)
    assert tuple(a.x.shape) == (4, 3, *canvas)
    assert torch.equal(a.x, b.x) and a.shapes == b.shapes == [tuple(s) for s in shapes] and torch.equal(a.geom, b.geom)
    total, got = _check_predictor(pred, bgr, nv, canvas, cuda)
    assert total > 0, "nothing kept: the comparison is empty"
    with _deterministic():
        _same_detections(got, pred(bgr))
        # CPU-resident and GPU-resident frames give the same result
        _same_detections(got, pred([f.to(cuda) for f in nv]))
        for u, v in zip(pred.predict_padded(nv), pred.predict_padded(bgr)):
            assert torch.equal(u, v)
        for u, v in zip(pred.predict_padded_guarded(nv), pred.predict_padded(bgr)):
            assert torch.equal(u, v)


def test_predictor_refuses_a_mixed_list(model, cuda):
    from yolosod_amd.data import NV12Frame
    from yolosod_amd.engine.predictor import DetectionPredictor
    y, uv = _scene_nv12(60, 100, 180)
    with pytest.raises(TypeError, match="mixes BGR arrays and NV12Frame"):
        DetectionPredictor(model, imgsz=128)([NV12Frame(y, uv), nv12_to_bgr_u8(y, uv)])


def test_predict_padded_on_nv12_frames_makes_no_synchronising_call(model, cuda):
    from yolosod_amd.data import NV12Frame
    from yolosod_amd.engine.predictor import DetectionPredictor
    pred = DetectionPredictor(model, imgsz=128)
    frames = [NV12Frame(*_scene_nv12(60, 100, 190)), NV12Frame(*_scene_nv12(34, 46, 191), matrix="bt709").to(cuda)]
    with _deterministic():
        ref = pred.predict_padded(frames)  # first use: pinned blocks and code objects are set up
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "prototype feature" notice
            torch.cuda.set_sync_debug_mode("error")
        try:
            got = pred.predict_padded(frames)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("full_frame", [True, False])
def test_sliced_predictor_on_an_nv12_frame(full_frame, model, cuda):
    """A 100 x 128 surface in 37 x 37 tiles: odd-sized tiles whose origins have all four parities."""
    from yolosod_amd.data import NV12Frame
    from yolosod_amd.engine.predictor import SlicedPredictor
    y, uv = _scene_nv12(100, 128, 200)
    bgr = nv12_to_bgr_u8(y, uv, "bt709")
    sp = SlicedPredictor(model, slice=37, overlap=0.2, full_frame=full_frame, conf=0.001, iou=0.7, imgsz=128)
    plan = sp.plan([(100, 128)])
    tiles = [s.rect for s in plan.slots[0] if not s.full]
    assert sorted({r[0] for r in tiles}) == [0, 30, 60, 63] and sorted({r[1] for r in tiles}) == [0, 30, 60, 90, 91]
    assert all((r[2] - r[0], r[3] - r[1]) == (37, 37) for r in tiles) and len(tiles) == 20
    assert {(r[0] & 1, r[1] & 1) for r in tiles} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert len(plan) == 20 + int(full_frame)
    for nv in (NV12Frame(y, uv, "bt709"), NV12Frame(y, uv, "bt709").to(cuda)):
        x = sp.ingest_tiles([nv], plan)
        assert tuple(x.shape) == (len(plan), 3, 128, 128)
        assert torch.equal(x, sp.ingest_tiles([bgr], plan))
    crops = [bgr[r[0]:r[2], r[1]:r[3]] for r in (plan.slot(f, k).rect for f, k in plan.order)]
    assert torch.equal(x.cpu(), ingest_ref(crops, [plan.slot(f, k).geometry for f, k in plan.order]))
    with _deterministic():
        a, b = sp.predict_padded([nv]), sp.predict_padded([bgr])
        assert int(a[1].sum()) > 0, "nothing kept: the comparison is empty"
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        for u, v in zip(sp.forward_tiles([nv], plan), sp.forward_tiles([bgr], plan)):
            assert torch.equal(u, v)
        _same_detections(sp([nv]), sp([bgr]))
