"""CPU: test-time augmentation without a GPU - the numpy restatement of csrc/tta.hip (tests/tta_ref.py) against the
reference's recorded ``scale_img`` / ``_descale_pred`` outputs, ``TTAPlan``'s integers against the reference's shapes,
the whole flow on the CPU oracle model against the reference's recorded ``predict(augment=True)``, the C-ABI entry
points' host-side argument checks, and no CPU fallback."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
from make_tta_golden import DESCALE_CASES, DESCALE_IMG, SCALE_IMG_CASES, case_input, descale_input
from oplib import BOX_ATOL, pred_close
from tta_ref import bf16_round, predict_augment_ref, tta_merge_ref, tta_view_ref
from yolosod_amd import _hip
from yolosod_amd.data.tta import TTAPlan

F32 = np.float32
STRIDES = [4, 8, 16, 32]  # the paper model's (P2..P5)


def _view_of(h, w, r, f):
    b = TTAPlan((h, w), (1, r), (None, f), stride=32, nl=4).branches[1]
    return b.view


def test_plan_restates_scale_img_sizes():
    z = golden("tta_scale_img")
    want = [(53, 79, 64, 96), (42, 64, 64, 96), (33, 41, 64, 64), (60, 75, 64, 96), (32, 32, 32, 32)]
    for i, (h, w, r, f) in enumerate(SCALE_IMG_CASES):
        view = _view_of(h, w, r, f)
        assert view == (f, *want[i])
        assert z[f"y{i}"].shape == (2, 3, *want[i][2:])


@pytest.mark.parametrize("i", range(len(SCALE_IMG_CASES)))
def test_views_restatement_against_recorded_scale_img(i):
    """Bound: one ulp of the source coordinate per axis (torch may contract scale * (d + 0.5) - 0.5 into an FMA), a
    coordinate below max(H, W) = 2^-23 * max(H, W) each on values in [0, 1], plus the blend's roundings."""
    h, w, r, f = SCALE_IMG_CASES[i]
    x = case_input(i, h, w).numpy()
    view = _view_of(h, w, r, f)
    got = tta_view_ref(x, view)
    want = golden("tta_scale_img")[f"y{i}"]
    assert got.dtype == F32 and got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max())
    bound = 2.0 ** -23 * (2 * max(h, w) + 8)
    print(f"case {i} {h}x{w} ratio {r} flip {f}: max|err| {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    sh, sw = view[1:3]
    assert (got[:, :, sh:] == F32(0.447)).all() and (got[:, :, :, sw:] == F32(0.447)).all()
    assert np.array_equal(got[:, :, sh:], want[:, :, sh:]) and np.array_equal(got[:, :, :, sw:], want[:, :, :, sw:])
    # bf16: against the recorded fp32 result rounded to bf16, within one bf16 step of the value
    xb = bf16_round(x)
    gb = tta_view_ref(xb, view, bf16=True)
    assert np.array_equal(gb, bf16_round(gb))
    wb = bf16_round(want)
    # (the input's own rounding, 2^-9 relative on each tap of a convex blend, moves the value by half a step at most)
    big = np.maximum(np.maximum(np.abs(gb), np.abs(wb)), F32(2.0 ** -100))
    step = np.exp2(np.floor(np.log2(big.astype(np.float64))) - 7)  # the spacing of bf16 at the value
    worst = float((np.abs(gb.astype(np.float64) - wb) / step).max())
    print(f"case {i} bf16: max |err| / step {worst:.3g}, {float((gb != wb).mean()):.3f} of the elements differ")
    assert worst <= 1.0
    exact = bf16_round(tta_view_ref(xb, view))
    assert np.array_equal(gb, exact)


def test_merge_restatement_is_bit_equal_to_recorded_descale_pred():
    z = golden("tta_descale")
    p = descale_input().numpy()
    for i, (f, s) in enumerate(DESCALE_CASES):
        cat = np.full((2, 14, 85), np.nan, dtype=F32)
        tta_merge_ref(p, cat, 0, 85, 0, s, f, DESCALE_IMG)
        assert np.array_equal(cat.view(np.int32), z[f"y{i}"].view(np.int32)), (f, s)
    # a range: only [dst, dst + n) is written, from [src_lo, src_lo + n)
    cat = np.full((2, 14, 90), np.nan, dtype=F32)
    tta_merge_ref(p, cat, 9, 31, 50, 0.67, 2, DESCALE_IMG)
    assert np.array_equal(cat[:, :, 50:81], z["y2"][:, :, 9:40])
    assert np.isnan(cat[:, :, :50]).all() and np.isnan(cat[:, :, 81:]).all()


def test_plan_counts_and_offsets():
    p = TTAPlan((256, 256), stride=32, nl=4)
    assert [b.padded for b in p.branches] == [(256, 256), (224, 224), (192, 192)]
    assert [b.resized for b in p.branches] == [(256, 256), (212, 212), (171, 171)]
    assert [b.A for b in p.branches] == [5440, 4165, 3060]
    assert [(b.src_lo, b.n, b.dst) for b in p.branches] == [(0, 5376, 0), (0, 4165, 5376), (2304, 756, 9541)]
    assert p.A_tot == 10297 == golden("tta_model_256")["y"].shape[-1]
    assert p.branches[0].view is None and p.views == [(3, 212, 212, 224, 224), (None, 171, 171, 192, 192)]
    p = TTAPlan((192, 256), stride=STRIDES, nl=4)
    assert [b.padded for b in p.branches] == [(192, 256), (160, 224), (160, 192)]
    assert [b.resized for b in p.branches] == [(192, 256), (159, 212), (128, 171)]
    assert [b.A for b in p.branches] == [4080, 2975, 2550]
    assert [b.n for b in p.branches] == [4032, 2975, 630] and p.A_tot == 7637
    p = TTAPlan((640, 640), stride=32, nl=4)
    assert [b.A for b in p.branches] == [34000, 24565, 16660]
    assert [b.n for b in p.branches] == [33600, 24565, 4116] and p.A_tot == 62281
    assert [b.padded for b in p.branches] == [(640, 640), (544, 544), (448, 448)]
    # other scales and flips: an upscale, an up-down flip, a flipped scale of 1 (a view of the same size, not padded)
    p = TTAPlan((40, 52), (1, 1.5, 1), (2, 3, None), stride=32, nl=3)
    assert p.branches[0].view == (2, 40, 52, 40, 52) and p.branches[1].view == (3, 60, 78, 64, 96)
    assert p.branches[2].view is None and len(p.views) == 2
    with pytest.raises(ValueError):
        TTAPlan((256, 256), (1, 0.83), (None,), stride=32, nl=4)
    with pytest.raises(ValueError):
        TTAPlan((256, 256), (1, 0.83), (None, 1), stride=32, nl=4)
    with pytest.raises(ValueError):
        TTAPlan((256, 256), (1, 0.0), (None, None), stride=32, nl=4)


def test_locate_round_trips():
    p = TTAPlan((192, 256), stride=32, nl=4)
    seen = 0
    for k, b in enumerate(p.branches):
        for a in (b.src_lo, b.src_lo + b.n // 2, b.src_lo + b.n - 1):
            i = p.index(k, a)
            assert p.locate(i) == (k, a)
            seen += 1
        assert p.index(k, b.src_lo + b.n) is None
    assert seen == 9
    assert p.locate(0) == (0, 0) and p.locate(p.A_tot - 1) == (2, p.branches[2].A - 1)
    assert p.index(2, 0) is None and p.index(0, p.branches[0].A - 1) is None  # the clipped tails
    assert all(p.index(*p.locate(i)) == i for i in range(0, p.A_tot, 97))
    with pytest.raises(IndexError):
        p.locate(p.A_tot)


def test_flow_on_the_cpu_oracle_against_the_recorded_model_output():
    """``predict_augment_ref`` (restated views, the oracle CPU model per view, restated merge) against the reference's
    own ``predict(augment=True)``; the box tolerance of branch k is 1e-3 / scale_k: the model's 1e-3 canvas-pixel
    tolerance carried through the division."""
    from oracle.model_ref import build_cpu_model
    cpu = build_cpu_model()
    x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(3))
    plan = TTAPlan((256, 256), stride=[int(s) for s in cpu.stride.tolist()], nl=cpu.model[-1].nl)
    cat, _, _ = predict_augment_ref(cpu, x, plan)
    want = golden("tta_model_256")["y"]
    assert cat.shape == want.shape and not np.isnan(cat).any()
    for b in plan.branches:
        sl = slice(b.dst, b.dst + b.n)
        ok, msg = pred_close(torch.from_numpy(cat[:, :, sl]), torch.from_numpy(want[:, :, sl]),
                             box_atol=BOX_ATOL / b.scale)
        print(f"branch scale {b.scale} flip {b.flip}: {msg}")
        assert ok, (b.scale, msg)


def test_abi_argument_checks_without_gpu():
    assert "yolosod_tta_views" in (ROOT / "include" / "yolosod_hip.h").read_text()
    lib = _hip.load_library()
    p = ctypes.c_void_p(64)
    for n in ("yolosod_tta_views", "yolosod_tta_merge"):
        assert hasattr(lib, n) and n in _hip.SIGNATURES

    def views(*a):
        rc = lib.yolosod_tta_views(*a)
        return rc, lib.yolosod_last_error()

    rc, e = views(None, 2, 3, 64, 96, 0, p, 2, 64, 96, None)
    assert rc != 0 and b"null" in e
    rc, e = views(p, 2, 3, 64, 96, 0, None, 2, 64, 96, None)
    assert rc != 0 and b"null" in e
    rc, e = views(p, 0, 3, 64, 96, 0, p, 2, 64, 96, None)
    assert rc != 0 and b"unsupported" in e
    rc, e = views(p, 2, 3, 64, 96, 0, p, 2, 64, 94, None)
    assert rc != 0 and b"width" in e
    rc, e = views(p, 2, 3, 64, 96, 2, p, 2, 64, 96, None)
    assert rc != 0 and b"bf16" in e
    rc, e = views(p, 32, 3, 64, 96, 0, p, 700, 64, 96, None)
    assert rc != 0 and b"65535" in e

    def merge(*a):
        rc = lib.yolosod_tta_merge(*a)
        return rc, lib.yolosod_last_error()

    rc, e = merge(None, 2, 10, 85, 0, 85, p, 200, 0, 1.0, 0, 96.0, 64.0, None)
    assert rc != 0 and b"null" in e
    rc, e = merge(p, 2, 0, 85, 0, 85, p, 200, 0, 1.0, 0, 96.0, 64.0, None)
    assert rc != 0 and b"nc=0" in e
    rc, e = merge(p, 2, 65, 85, 0, 85, p, 200, 0, 1.0, 0, 96.0, 64.0, None)
    assert rc != 0 and b"nc=65" in e
    rc, e = merge(p, 2, 10, 85, 1, 85, p, 200, 0, 1.0, 0, 96.0, 64.0, None)
    assert rc != 0 and b"source" in e
    rc, e = merge(p, 2, 10, 85, 0, 85, p, 200, 116, 1.0, 0, 96.0, 64.0, None)
    assert rc != 0 and b"destination" in e
    rc, e = merge(p, 2, 10, 85, 0, 85, p, 200, 0, 0.0, 0, 96.0, 64.0, None)
    assert rc != 0 and b"scale" in e
    rc, e = merge(p, 2, 10, 85, 0, 85, p, 200, 0, float("nan"), 0, 96.0, 64.0, None)
    assert rc != 0 and b"scale" in e
    rc, e = merge(p, 2, 10, 85, 0, 85, p, 200, 0, 1.0, 1, 96.0, 64.0, None)
    assert rc != 0 and b"flip" in e


def test_torch_ops_are_registered():
    ops = _hip.ops()
    assert hasattr(ops, "tta_views") and hasattr(ops, "tta_merge")


def test_no_cpu_fallback():
    from yolosod_amd.engine.predictor import DetectionPredictor
    from yolosod_amd.nn.tasks import DetectionModel
    with pytest.raises(RuntimeError, match="HIP kernel requires GPU tensors"):
        _hip.tta_views(torch.zeros(2, 3, 64, 96), [(3, 53, 79, 64, 96)])
    with pytest.raises(RuntimeError, match="HIP kernel requires GPU tensors"):
        _hip.tta_merge(torch.zeros(2, 14, 85), torch.zeros(2, 14, 85), 0, 85, 0, 1.0, None, (64, 96))
    torch.manual_seed(0)
    m = DetectionModel("yolov12-sod-fusion-v5-simple.yaml").fuse().eval()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="HIP kernel requires GPU tensors"):
        m(x, augment=True)
    with pytest.raises(RuntimeError, match="HIP kernel requires GPU tensors"):
        m.predict(x, augment=True)
    assert DetectionPredictor(m).augment is False and DetectionPredictor(m, augment=True).augment is True
