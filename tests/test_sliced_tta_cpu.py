"""CPU: sliced inference with test-time augmentation without a GPU - the numpy restatement of the fused branch merge
(tests/tile_merge_tta_ref.py) against the two restated launches it replaces (tta_merge_ref into a concatenated tensor,
then tile_merge_ref of it), bit for bit on the cases the GPU kernel is tested on; the plan arithmetic the predictor
relies on; the C-ABI entry point's host-side argument checks; and no CPU fallback."""
import ctypes

import numpy as np
import pytest
import torch

from sliced_tta_cases import (BRANCH_SETS, CANVAS, FRAMES, N_EDGE, SLOTS, assert_each_outcome_occurs, edge_outcomes,
                              launches, merge_tta_case)
from tile_merge_ref import tile_merge_ref
from tile_merge_tta_ref import tile_merge_tta_ref
from tta_ref import tta_merge_ref
from yolosod_amd import _hip
from yolosod_amd.data.tta import TTAPlan

F32 = np.float32
STRIDES = (4, 8, 16, 32)  # the paper model's Detect levels
SHAPES = [(200, 300), (90, 150), (128, 128)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the restatement against the chain ---------------------------------------------------------------------------
@pytest.mark.parametrize("cut_margin", [None, 0.0, 2.0])
@pytest.mark.parametrize("nc", [1, 10])
@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_is_the_chain_of_the_two_restated_launches(name, nc, cut_margin):
    ys, rows, branches, A_tot = merge_tta_case(name, nc)
    no = 4 + nc
    fused = np.full((FRAMES, no, SLOTS * A_tot), np.nan, dtype=F32)
    chain = np.full((FRAMES, no, SLOTS * A_tot), np.nan, dtype=F32)
    for c, call in enumerate(ys):
        cat = np.full((call[0].shape[0], no, A_tot), np.nan, dtype=F32)
        for k, (y, b) in enumerate(zip(call, branches)):
            tile_merge_tta_ref(y, rows[c], fused, A_tot, b, CANVAS, cut_margin)
            tta_merge_ref(y, cat, b[0], b[1], b[2], b[3], b[4], CANVAS)
        assert not np.isnan(cat).any(), "the branches' kept ranges tile [0, A_tot)"
        tile_merge_ref(cat, rows[c], chain, A_tot, cut_margin)
    assert not np.isnan(chain).any() and not np.isnan(fused).any()
    assert np.array_equal(_bits(fused), _bits(chain))
    assert (fused[0, :, A_tot:2 * A_tot] == 0).all(), "the empty slot holds zeros"
    if name == "a":
        for cut in edge_outcomes(fused, ys, branches, A_tot):
            assert_each_outcome_occurs(cut, cut_margin)


def test_restatement_writes_one_branch_range_per_launch():
    """After every launch exactly the launches' ranges of the named slots are defined, everything else still NaN."""
    ys, rows, branches, A_tot = merge_tta_case("b", 3)
    m = np.full((FRAMES, 7, SLOTS * A_tot), np.nan, dtype=F32)
    want = np.zeros(m.shape, dtype=bool)
    for c, k, y, r, b in launches(ys, rows, branches):
        tile_merge_tta_ref(y, r, m, A_tot, b, CANVAS, 2.0)
        for row in r:
            lo = row[2] * A_tot + b[2]
            assert not want[row[1], :, lo:lo + b[1]].any(), "a range written twice"
            want[row[1], :, lo:lo + b[1]] = True
        assert np.array_equal(~np.isnan(m), want), (c, k)
    assert want.all()


# ---- plan arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canvas,A_tot,terms", [
    (128, 2893, [(1360, 0, 1344, 0), (1360, 0, 1360, 1344), (765, 576, 189, 2704)]),
    (640, 62281, [(34000, 0, 33600, 0), (24565, 0, 24565, 33600), (16660, 12544, 4116, 58165)]),
])
def test_tile_canvas_plans(canvas, A_tot, terms):
    tp = TTAPlan((canvas, canvas), stride=STRIDES, nl=4)
    assert tp.A_tot == A_tot and A_tot % 2 == 1
    assert [(b.A, b.src_lo, b.n, b.dst) for b in tp.branches] == terms
    if canvas == 128:  # branch set "a" of the kernel tests is this plan
        assert [(b.A, (b.src_lo, b.n, b.dst, b.scale, b.flip)) for b in tp.branches] == BRANCH_SETS["a"][0]
        assert BRANCH_SETS["a"][1] == A_tot and all(b.n >= N_EDGE for b in tp.branches)


class _PlanOnly(torch.nn.Module):
    """What SlicedPredictor asks of a model before any tensor runs: a parameter, the strides, tta_plan."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.stride = torch.tensor([float(s) for s in STRIDES])

    def tta_plan(self, shape, scales=None, flips=None):
        from yolosod_amd.data.tta import DEFAULT_FLIPS, DEFAULT_SCALES
        return TTAPlan(shape, scales or DEFAULT_SCALES, flips or DEFAULT_FLIPS, stride=STRIDES, nl=4)


def test_predictor_plan_and_locate_round_trip():
    from yolosod_amd.engine.predictor import SlicedPredictor
    sp = SlicedPredictor(_PlanOnly(), slice=128, overlap=0.25, full_frame=True, imgsz=128, augment=True)
    plan = sp.plan(SHAPES)
    tp = sp.tta_plan(plan)
    assert plan.S == 7 and len(plan) == 12 and plan.canvas == (128, 128) and tp.A_tot == 2893 and len(tp) == 3
    # merged is [3, 14, 7 * 2893]
    for slot in (0, 3, 6):
        for k, b in enumerate(tp.branches):
            for j in (b.dst, b.dst + 1, b.dst + b.n - 1):  # first, second, last index of the branch
                s, kk, a = sp.locate(slot * tp.A_tot + j, plan)
                assert (s, kk) == (slot, k) and a == b.src_lo + j - b.dst
                assert sp.index(s, kk, a, plan) == slot * tp.A_tot + j
            if b.src_lo + b.n < b.A:  # the clipped tail of the first branch
                assert sp.index(slot, k, b.src_lo + b.n, plan) is None
            if b.src_lo > 0:          # the clipped head of the last
                assert sp.index(slot, k, b.src_lo - 1, plan) is None
    assert sp.locate(7 * 2893 - 1, plan) == (6, 2, 764)
    for bad in (-1, 7 * 2893):
        with pytest.raises(IndexError):
            sp.locate(bad, plan)
    # without augment: one branch, slot * A + anchor
    sp0 = SlicedPredictor(_PlanOnly(), slice=128, overlap=0.25, full_frame=True, imgsz=128)
    assert sp0.locate(3 * 1360 + 7, plan) == (3, 0, 7) and sp0.index(3, 0, 7, plan) == 3 * 1360 + 7
    with pytest.raises(ValueError, match="augment"):
        SlicedPredictor(_PlanOnly(), scales=(1, 0.5), flips=(None, 3))


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_abi_exports_and_validates_the_entry_point():
    from conftest import ROOT
    assert "yolosod_tile_merge_tta" in (ROOT / "include" / "yolosod_hip.h").read_text()
    lib = _hip.load_library()
    assert hasattr(lib, "yolosod_tile_merge_tta") and "yolosod_tile_merge_tta" in _hip.SIGNATURES
    assert lib.yolosod_abi_version() == 1
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)  # never dereferenced: every call fails its host checks first
    inf, nan = float("inf"), float("nan")

    def call(y=p, n=1, nc=10, A=85, src_lo=0, n_k=84, desc=p, rows=1, merged=p, F=1, S=1, A_tot=147, dst=0, scale=1.0,
             flip=0, img_w=128.0, img_h=128.0, cut=-1.0):
        rc = lib.yolosod_tile_merge_tta(y, n, nc, A, src_lo, n_k, desc, rows, merged, F, S, A_tot, dst, scale, flip,
                                        img_w, img_h, cut, None)
        return rc, lib.yolosod_last_error()

    for kw, word in [(dict(y=None), b"null"), (dict(desc=None), b"null"), (dict(merged=None), b"null"),
                     (dict(n=0), b"n=0"), (dict(A=0), b"A=0"), (dict(F=0), b"F=0"), (dict(S=0), b"S=0"),
                     (dict(A_tot=0), b"A_tot=0"), (dict(nc=0), b"nc=0"), (dict(nc=65), b"nc=65"),
                     (dict(rows=0), b"rows=0"), (dict(rows=65536), b"rows=65536"),
                     (dict(src_lo=2), b"source"), (dict(src_lo=-1), b"source"), (dict(n_k=0), b"source"),
                     (dict(dst=64), b"destination"), (dict(dst=-1), b"destination"),
                     (dict(nc=64, S=64, A_tot=1 << 20), b"2^32"),
                     (dict(scale=0.0), b"scale"), (dict(scale=-1.0), b"scale"), (dict(scale=inf), b"scale"),
                     (dict(scale=nan), b"scale"), (dict(flip=1), b"flip=1"), (dict(flip=4), b"flip=4"),
                     (dict(cut=nan), b"NaN"), (dict(img_w=nan), b"NaN"),
                     (dict(y=odd), b"misaligned"), (dict(desc=odd), b"misaligned"), (dict(merged=odd), b"misaligned")]:
        rc, err = call(**kw)
        assert rc != 0 and word in err, (kw, rc, err)


# ---- no CPU fallback -------------------------------------------------------------------------------------------------
def test_no_cpu_fallback():
    from yolosod_amd.engine.predictor import SlicedPredictor
    rows = [(0, 0, 0, 1.0, 0, 0, 0, 0, 128, 128, (False,) * 4)]
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.tile_merge_tta(torch.zeros(1, 14, 85), rows, torch.zeros(1, 14, 147), 147, (0, 84, 0, 1.0, None), CANVAS)
    sp = SlicedPredictor(_PlanOnly(), slice=128, full_frame=False, imgsz=128, augment=True)
    plan = sp.plan([(128, 128)])
    assert plan.S == 1 and len(plan) == 1
    ys = tuple(torch.zeros(1, 14, b.A) for b in sp.tta_plan(plan).branches)
    with pytest.raises(RuntimeError, match="GPU"):
        sp.merge([ys], plan)
