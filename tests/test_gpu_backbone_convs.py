"""GPU: the backbone C2fs' Bottleneck 3x3 convs (layers 3 / 6 / 8 / 11 of the paper YAML: ten convs) on the stride-1
fp16-split kernel (modules.S1_BACKBONE, csrc/conv3x3.hip) and its gate-free stride-2 convs (layers 7 / 10) on the
stride-2 kernel (modules.S2_BACKBONE, csrc/conv3x3s2.hip) against the MIOpen + epilogue path they replace, and the
configurations that must not take the kernels (exact_fp32_matrix(), the bf16 model)."""
import pytest
import torch

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

CFG = "yolov12-sod-fusion-v5-simple.yaml"


def _run(m, x):
    with _hip.op_timer() as t:
        y = m(x)[0]
    return y, [k for k, _ in t.durations_ms() if k[0] in ("conv3x3_backbone", "conv3x3s2_backbone")]


def test_backbone_c2f_convs_take_the_kernel(cuda, monkeypatch):
    """Ten 'conv3x3_backbone' launches (the kernel of the 'conv3x3' key; the backbone's launches carry a name of
    their own so that the censuses of the towers' and the neck's launches keep counting those) with the switch on,
    none with it off, at the backbone's channel counts, and the model output agrees with the MIOpen path within fp32
    accuracy."""
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(8)).to(cuda)
    with torch.inference_mode():
        monkeypatch.setattr(M, "S2_BACKBONE", False)
        monkeypatch.setattr(M, "S1_BACKBONE", True)
        _hip.split_range_flag(reset=True)
        y1, k1 = _run(m, x)
        assert not _hip.split_range_flag(reset=True)  # the range guard covers the new launches and stays quiet
        monkeypatch.setattr(M, "S1_BACKBONE", False)
        y0, k0 = _run(m, x)
    assert len(k1) == 10 and not k0, (len(k1), len(k0))
    extra = k1
    # (B, C, H, W) of the ten launches: 2 at L3 (32 ch, 64^2), 4 at L6 (64, 32^2), 2 at L8 (128, 16^2), 2 at L11
    assert sorted(tuple(k[1]) for k in extra) == sorted(
        [(2, 32, 64, 64)] * 2 + [(2, 64, 32, 32)] * 4 + [(2, 128, 16, 16)] * 2 + [(2, 256, 8, 8)] * 2), extra
    assert sum(1 for k in extra if isinstance(k[2], tuple) and k[2][1] == "res") == 5  # every cv2 adds the shortcut
    ok, e, _ = tol_close(y1.cpu().double(), y0.cpu().double(), 1e-3, 1e-4)
    assert ok, e


def test_backbone_stride2_convs_take_the_kernel(cuda, monkeypatch):
    """Layers 7 and 10 (128 -> 256 and 256 -> 512, no gate) run as 'conv3x3s2_backbone' launches with the switch on,
    none with it off; the model output agrees with the MIOpen path within fp32 accuracy."""
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda)
    assert [i for i, layer in enumerate(m.model) if getattr(layer, "s2_backbone", False)] == [7, 10]
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(11)).to(cuda)
    with torch.inference_mode():
        monkeypatch.setattr(M, "S1_BACKBONE", False)
        monkeypatch.setattr(M, "S2_BACKBONE", True)
        _hip.split_range_flag(reset=True)
        y1, k1 = _run(m, x)
        assert not _hip.split_range_flag(reset=True)
        monkeypatch.setattr(M, "S2_BACKBONE", False)
        y0, k0 = _run(m, x)
    assert sorted(k1) == [("conv3x3s2_backbone", (2, 128, 32, 32), (256, False, False)),
                          ("conv3x3s2_backbone", (2, 256, 16, 16), (512, False, False))], k1
    assert not k0
    ok, e, _ = tol_close(y1.cpu().double(), y0.cpu().double(), 1e-3, 1e-4)
    assert ok, e


def test_backbone_switch_inert_in_exact_fp32(cuda, monkeypatch):
    """Inside exact_fp32_matrix() no conv takes a split kernel: the switches change nothing, bit for bit."""
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda)
    x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(9)).to(cuda)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode(), _hip.exact_fp32_matrix():
            monkeypatch.setattr(M, "S1_BACKBONE", True)
            monkeypatch.setattr(M, "S2_BACKBONE", True)
            y1, k1 = _run(m, x)
            monkeypatch.setattr(M, "S1_BACKBONE", False)
            monkeypatch.setattr(M, "S2_BACKBONE", False)
            y0, k0 = _run(m, x)
    finally:
        torch.backends.cudnn.deterministic = det
    assert not k1 and not k0
    assert torch.equal(y1, y0)


def test_backbone_switch_inert_in_bf16(cuda, monkeypatch):
    """The bf16 model's convs stay on MIOpen: the switches change nothing, bit for bit."""
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda, dtype=torch.bfloat16)
    x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(10)).to(cuda).to(torch.bfloat16)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode():
            monkeypatch.setattr(M, "S1_BACKBONE", True)
            monkeypatch.setattr(M, "S2_BACKBONE", True)
            y1, k1 = _run(m, x)
            monkeypatch.setattr(M, "S1_BACKBONE", False)
            monkeypatch.setattr(M, "S2_BACKBONE", False)
            y0, k0 = _run(m, x)
    finally:
        torch.backends.cudnn.deterministic = det
    assert not k1 and not k0
    assert torch.equal(y1, y0)
