"""CPU: sliced inference without a GPU - the tile planner (yolo-sod_amd/data/slicing.py) on its stated properties and
a worked example, the plan's way-back terms against DetectionPredictor.ingest's own arithmetic, the numpy restatement
of the merge (tests/tile_merge_ref.py) on a round trip, and the C-ABI entry point's host-side argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tile_merge_ref import tile_merge_ref
from yolosod_amd import _hip
from yolosod_amd.data.augment import LetterBox
from yolosod_amd.data.slicing import SlicePlan, axis_starts, slice_grid

# (n, s, r): n < s, n == s, n == s + 1, a flush start equal to the last regular start (n = 224: 0, 96 and 224 - 128 =
# 96), r = 0 (also with n a multiple of s and not), a large ratio, and sizes around them
AXIS_CASES = [(90, 128, 0.25), (128, 128, 0.25), (129, 128, 0.25), (224, 128, 0.25), (225, 128, 0.25), (223, 128, 0.25),
              (300, 128, 0.25), (200, 128, 0.25), (256, 128, 0.0), (300, 128, 0.0), (1, 128, 0.0), (1, 1, 0.5),
              (3840, 640, 0.2), (2160, 640, 0.2), (1000, 100, 0.9), (641, 640, 0.5), (7, 3, 0.34)]


@pytest.mark.parametrize("n,s,r", AXIS_CASES)
def test_axis_rule_properties(n, s, r):
    t, starts = axis_starts(n, s, r)
    ov = math.floor(r * t)
    assert t == min(s, n) and all(isinstance(v, int) for v in starts)
    assert starts[0] == 0 and starts[-1] == n - t, "first tile at 0, last tile flush with the far border"
    assert all(b > a for a, b in zip(starts, starts[1:])), "strictly increasing: no duplicate of the flush start"
    assert all(0 <= a and a + t <= n for a in starts), "every tile inside, exactly t long"
    covered = np.zeros(n, dtype=bool)
    for a in starts:
        covered[a:a + t] = True
    assert covered.all(), "union covers the axis"
    assert all(a + t - b >= ov for a, b in zip(starts, starts[1:])), "neighbours overlap by at least floor(r t)"
    # regular starts are multiples of the step; only the last may be pulled in
    step = t - ov
    assert [a for a in starts[:-1]] == [k * step for k in range(len(starts) - 1)]
    if n <= s:
        assert starts == [0]


def test_the_sweep_holds_the_cases_it_claims():
    assert axis_starts(224, 128, 0.25)[1] == [0, 96]          # flush start == last regular start: listed once
    assert axis_starts(225, 128, 0.25)[1] == [0, 96, 97]
    assert axis_starts(129, 128, 0.25)[1] == [0, 1]
    assert axis_starts(256, 128, 0.0)[1] == [0, 128]
    assert axis_starts(300, 128, 0.0)[1] == [0, 128, 172]
    assert axis_starts(90, 128, 0.25) == (90, [0])


def test_refusals():
    assert axis_starts(10, 1, 0.5)[1] == list(range(10))           # floor(0.5) = 0: step 1
    assert axis_starts(100, 100, 0.999) == (100, [0])
    assert axis_starts(103, 100, 0.999)[1] == [0, 1, 2, 3]         # step = 100 - 99 = 1, the smallest allowed
    with pytest.raises(ValueError, match="overlap"):
        axis_starts(10, 4, 1.0)
    with pytest.raises(ValueError, match="overlap"):
        axis_starts(10, 4, -0.1)
    with pytest.raises(ValueError):
        slice_grid((0, 10), 4, 0.0)


def test_worked_example():
    """(200, 300), slice 128, overlap 0.25: x starts 0, 96, 172, y starts 0, 72; 6 tiles row-major, 7 slots with the
    whole frame."""
    assert axis_starts(300, 128, 0.25) == (128, [0, 96, 172])
    assert axis_starts(200, 128, 0.25) == (128, [0, 72])
    tiles = slice_grid((200, 300), slice=128, overlap=0.25)
    assert tiles == [(0, 0, 128, 128), (0, 96, 128, 224), (0, 172, 128, 300),
                     (72, 0, 200, 128), (72, 96, 200, 224), (72, 172, 200, 300)]
    assert tiles == sorted(tiles), "row-major: y outer, x inner"
    assert slice_grid((200, 300), slice=(128, 128), overlap=(0.25, 0.25)) == tiles
    plan = SlicePlan([(200, 300)], 128, 0.25, True, 128)
    assert plan.S == 7 and len(plan) == 7
    assert plan.slots[0][0].rect == (0, 0, 200, 300) and plan.slots[0][0].full
    assert plan.slots[0][0].interior == (False, False, False, False)
    assert [s.rect for s in plan.slots[0][1:]] == tiles
    assert plan.slots[0][1].interior == (False, True, False, True)   # top-left tile: right and bottom edges interior
    assert plan.slots[0][5].interior == (True, True, True, False)    # bottom-middle
    assert SlicePlan([(200, 300)], 128, 0.25, False, 128).S == 6


def test_plan_of_a_mixed_batch():
    plan = SlicePlan([(200, 300), (90, 150), (128, 128)], 128, 0.25, True, 128)
    assert [len(r) for r in plan.slots] == [7, 3, 2] and plan.S == 7 and len(plan) == 12
    assert plan.order[:2] == [(0, 0), (0, 1)] and plan.order[7] == (1, 0) and plan.order[-1] == (2, 1)
    assert [s.rect for s in plan.slots[1]] == [(0, 0, 90, 150), (0, 0, 90, 128), (0, 22, 90, 150)]
    assert all(s.geometry[4:] == (128, 128) for r in plan.slots for s in r), "one canvas for every slot"
    # any chunking names every (frame, slot) of the merged tensor exactly once
    for batch in (1, 4, 5, 12, 32):
        named = []
        for lo, hi in plan.chunks(batch):
            assert 0 < hi - lo <= batch
            rows = plan.merge_rows(lo, hi)
            assert sorted(r[0] for r in rows if r[0] >= 0) == list(range(hi - lo))
            named += [(r[1], r[2]) for r in rows]
        assert sorted(named) == [(f, k) for f in range(3) for k in range(7)], batch
    empty = [r for r in plan.merge_rows(0, 12) if r[0] < 0]
    assert sorted((r[1], r[2]) for r in empty) == [(1, k) for k in range(3, 7)] + [(2, k) for k in range(2, 7)]


@pytest.mark.parametrize("shape", [(200, 300), (90, 150), (128, 128), (2160, 3840), (77, 1000)])
def test_plan_way_back_terms_are_ingests_own(shape):
    """gain / pad of every slot equal what DetectionPredictor.ingest puts in ``geom`` for a frame of the tile's shape
    (scale_boxes' rule), and the letterbox geometry is LetterBox(auto=False)'s on the fixed canvas."""
    imgsz = 128 if max(shape) < 1000 else 640
    canvas = (imgsz, imgsz)
    plan = SlicePlan([shape], imgsz if imgsz == 640 else 128, 0.25, True, imgsz)
    lb = LetterBox(canvas, auto=False, stride=32)
    for s in plan.slots[0]:
        h0, w0 = s.shape
        gain = min(canvas[0] / h0, canvas[1] / w0)
        want = (gain, round((canvas[1] - w0 * gain) / 2 - 0.1), round((canvas[0] - h0 * gain) / 2 - 0.1))
        assert (s.gain, s.pad_x, s.pad_y) == want
        assert s.geometry == lb.geometry((h0, w0))
        assert abs(s.geometry[3] - s.pad_x) <= 1 and abs(s.geometry[2] - s.pad_y) <= 1


@pytest.mark.parametrize("shape,sl,imgsz", [((200, 300), 128, 128), ((2160, 3840), 640, 640), ((90, 150), 128, 128)])
def test_round_trip_through_the_restatement(shape, sl, imgsz):
    """A box in frame coordinates, mapped (in float64) into each slot's canvas and back through the fp32 restatement,
    returns within 1e-3 px: the fp32 roundings are the canvas coordinate (half an ulp below 1024: 3e-5, times 1 / gain
    <= 6 for the whole-frame slot), the subtraction, the division and the addition of the offset (half an ulp below
    4096 each: 1.2e-4) - under 6e-4 in all."""
    plan = SlicePlan([shape], sl, 0.25, True, imgsz)
    rng = np.random.default_rng(5)
    A = 16
    worst = 0.0
    for lo in range(len(plan)):
        slot = plan.slots[0][lo]
        y0, x0, y1, x1 = slot.rect
        cx, cy = rng.uniform(x0, x1, A), rng.uniform(y0, y1, A)
        w, h = rng.uniform(2, 40, A), rng.uniform(2, 40, A)
        y = np.zeros((1, 5, A), dtype=np.float32)
        y[0, 0] = (cx - x0) * slot.gain + slot.pad_x
        y[0, 1] = (cy - y0) * slot.gain + slot.pad_y
        y[0, 2], y[0, 3], y[0, 4] = w * slot.gain, h * slot.gain, 0.5
        rows = [r for r in plan.merge_rows(lo, lo + 1) if r[0] >= 0]
        merged = np.full((1, 5, plan.S * A), np.nan, dtype=np.float32)
        tile_merge_ref(y, rows, merged, A)
        got = merged[0, :4, lo * A:(lo + 1) * A].astype(np.float64)
        worst = max(worst, float(np.abs(got - np.stack([cx, cy, w, h])).max()))
        assert np.isnan(np.delete(merged[0], np.s_[lo * A:(lo + 1) * A], axis=1)).all(), "only the named slot"
        assert (merged[0, 4, lo * A:(lo + 1) * A] == 0.5).all()
    print(f"{shape}: max round-trip error {worst:.2e} px")
    assert worst <= 1e-3, worst


def test_restatement_cut_and_empty_slots():
    """Hand-checked: a 100 x 100 tile at (50, 20) whose left and bottom edges are interior, gain 1, margin 2."""
    y = np.zeros((1, 6, 5), dtype=np.float32)
    #            inside        touches left   left side at 2   bottom at 98     right edge (not interior)
    y[0, :4] = np.array([[50, 50, 10, 10], [4, 50, 8, 10], [7, 50, 10, 10], [50, 94, 10, 8], [97, 50, 6, 10]],
                        dtype=np.float32).T
    y[0, 4], y[0, 5] = 0.9, 0.1
    rows = [(0, 0, 1, 1.0, 0, 0, 20, 50, 100, 100, (True, False, False, True)),
            (-1, 0, 0, 1.0, 0, 0, 0, 0, 0, 0, (False,) * 4)]
    m = tile_merge_ref(y, rows, np.full((1, 6, 10), np.nan, dtype=np.float32), 5, cut_margin=2)
    assert (m[0, :, :5] == 0).all()
    assert m[0, :4, 5:].T.tolist() == [[70, 100, 10, 10], [24, 100, 8, 10], [27, 100, 10, 10], [70, 144, 10, 8],
                                       [117, 100, 6, 10]]
    assert m[0, 4, 5:].tolist() == [np.float32(0.9), 0, 0, 0, np.float32(0.9)]   # x1 = 0 <= 2; x1 = 2 <= 2; y2 = 98 >= 98
    assert m[0, 5, 5:].tolist() == [np.float32(0.1), 0, 0, 0, np.float32(0.1)]
    off = tile_merge_ref(y, rows, np.full((1, 6, 10), np.nan, dtype=np.float32), 5, cut_margin=None)
    assert (off[0, 4, 5:] == np.float32(0.9)).all()


def test_abi_exports_and_validates_the_merge_entry_point():
    from conftest import ROOT
    assert "yolosod_tile_merge" in (ROOT / "include" / "yolosod_hip.h").read_text()
    lib = _hip.load_library()
    assert hasattr(lib, "yolosod_tile_merge") and "yolosod_tile_merge" in _hip.SIGNATURES
    assert lib.yolosod_abi_version() == 1
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its host checks first
    rc = lib.yolosod_tile_merge(None, 1, 10, 85, p, 1, p, 1, 1, -1.0, None)
    assert rc != 0 and b"null" in lib.yolosod_last_error()
    rc = lib.yolosod_tile_merge(p, 1, 10, 85, None, 1, p, 1, 1, -1.0, None)
    assert rc != 0 and b"null" in lib.yolosod_last_error()
    rc = lib.yolosod_tile_merge(p, 1, 10, 85, p, 1, None, 1, 1, -1.0, None)
    assert rc != 0 and b"null" in lib.yolosod_last_error()
    rc = lib.yolosod_tile_merge(p, 1, 0, 85, p, 1, p, 1, 1, -1.0, None)
    assert rc != 0 and b"nc=0" in lib.yolosod_last_error()
    rc = lib.yolosod_tile_merge(p, 1, 65, 85, p, 1, p, 1, 1, -1.0, None)
    assert rc != 0 and b"nc=65" in lib.yolosod_last_error()
    rc = lib.yolosod_tile_merge(p, 0, 10, 85, p, 1, p, 1, 1, -1.0, None)
    assert rc != 0 and b"n=0" in lib.yolosod_last_error()
    rc = lib.yolosod_tile_merge(p, 1, 10, 0, p, 1, p, 1, 1, -1.0, None)
    assert rc != 0 and b"A=0" in lib.yolosod_last_error()
    rc = lib.yolosod_tile_merge(p, 1, 10, 85, p, 1, p, 1, 0, -1.0, None)
    assert rc != 0 and b"S=0" in lib.yolosod_last_error()
    rc = lib.yolosod_tile_merge(p, 1, 64, 1 << 20, p, 1, p, 1, 64, -1.0, None)   # S*A*nc = 2^32
    assert rc != 0 and b"2^32" in lib.yolosod_last_error()


def test_no_cpu_fallback():
    from yolosod_amd.engine.predictor import SlicedPredictor
    y = torch.zeros(1, 14, 85)
    rows = [(0, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, (False,) * 4)]
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.tile_merge(y, rows, torch.zeros(1, 14, 85), 85)
    sp = SlicedPredictor(torch.nn.Linear(1, 1), slice=128, full_frame=False, imgsz=128)
    plan = sp.plan([(128, 128)])
    assert plan.S == 1 and len(plan) == 1
    with pytest.raises(RuntimeError, match="GPU"):
        sp.merge([y], plan)
