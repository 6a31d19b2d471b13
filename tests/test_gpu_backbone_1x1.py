"""GPU: the backbone's wide 1x1 convs (cv1 / cv2 of the C2fs L6 / L8 / L11 and of SPPF L13 of the paper YAML: eight
convs) on the fp16-split 1x1 kernel (modules.N1_BACKBONE, csrc/conv1x1x2.hip) against the MIOpen + bias / SiLU path
they replace, the configurations that must not take the kernel (exact_fp32_matrix(), the bf16 model) and the
predictor's split-range guard over the new launches. The paper YAML at 256^2, batch 2."""
import pytest
import torch

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

CFG = "yolov12-sod-fusion-v5-simple.yaml"
# (layer, (B, Cin, H, W), Cout) of the eight launches at 256^2, batch 2
LAUNCHES = [(6, (2, 128, 32, 32), 128), (6, (2, 256, 32, 32), 128), (8, (2, 256, 16, 16), 256),
            (8, (2, 384, 16, 16), 256), (11, (2, 512, 8, 8), 512), (11, (2, 768, 8, 8), 512),
            (13, (2, 512, 8, 8), 256), (13, (2, 1024, 8, 8), 512)]


def _run(m, x):
    """(output, the 'conv1x1x2_backbone' keys, the (Cout, H, W) of every bias_act pass)."""
    with _hip.op_timer() as t:
        y = m(x)[0]
    keys = [k for k, _ in t.durations_ms()]
    return y, [k for k in keys if k[0] == "conv1x1x2_backbone"], [k for k in keys if k[0] == "bias_act"]


@pytest.fixture(scope="module")
def model_x(cuda):
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(12)).to(cuda)
    return m, x


def test_backbone_1x1_convs_take_the_kernel(model_x, monkeypatch):
    """Eight 'conv1x1x2_backbone' launches with the switch on (a key of their own: the censuses of the neck's
    'conv1x1x2' launches keep counting those), none with it off, and the eight bias_act passes behind them are gone;
    the model output agrees with the MIOpen path within fp32 accuracy; the range guard covers the launches."""
    from yolosod_amd.nn import modules as M
    m, x = model_x
    with torch.inference_mode():
        monkeypatch.setattr(M, "N1_BACKBONE", True)
        _hip.split_range_flag(reset=True)
        y1, k1, e1 = _run(m, x)
        assert not _hip.split_range_flag(reset=True)
        monkeypatch.setattr(M, "N1_BACKBONE", False)
        y0, k0, e0 = _run(m, x)
    assert not k0
    assert sorted((tuple(k[1]), k[2][0]) for k in k1) == sorted((s, c) for _, s, c in LAUNCHES), k1
    assert not any(k[2][1] for k in k1)  # no dual store: the backbone's Bottlenecks read their slice in place
    assert len(e0) - len(e1) == 8, (len(e0), len(e1))
    ok, e, _ = tol_close(y1.cpu().double(), y0.cpu().double(), 1e-3, 1e-4)
    assert ok, e


@pytest.mark.parametrize("layers", [{6}, {8, 13}])
def test_layer_set_routes_exactly_its_layers(layers, model_x, monkeypatch):
    from yolosod_amd.nn import modules as M
    m, x = model_x
    monkeypatch.setattr(M, "N1_BACKBONE", frozenset(layers))
    with torch.inference_mode():
        _, k, _ = _run(m, x)
    assert sorted((tuple(q[1]), q[2][0]) for q in k) == sorted((s, c) for i, s, c in LAUNCHES if i in layers), k


def test_switch_inert_in_exact_fp32(model_x, monkeypatch):
    """Inside exact_fp32_matrix() no conv takes a split kernel: the switch changes nothing, bit for bit."""
    from yolosod_amd.nn import modules as M
    m, x = model_x
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode(), _hip.exact_fp32_matrix():
            monkeypatch.setattr(M, "N1_BACKBONE", True)
            y1, k1, _ = _run(m, x)
            monkeypatch.setattr(M, "N1_BACKBONE", False)
            y0, k0, _ = _run(m, x)
    finally:
        torch.backends.cudnn.deterministic = det
    assert not k1 and not k0
    assert torch.equal(y1, y0)


def test_switch_inert_in_bf16(cuda, monkeypatch):
    """The bf16 model's convs stay on MIOpen: the switch changes nothing, bit for bit."""
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda, dtype=torch.bfloat16)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(13)).to(cuda).to(torch.bfloat16)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode():
            monkeypatch.setattr(M, "N1_BACKBONE", True)
            y1, k1, _ = _run(m, x)
            monkeypatch.setattr(M, "N1_BACKBONE", False)
            y0, k0, _ = _run(m, x)
    finally:
        torch.backends.cudnn.deterministic = det
    assert not k1 and not k0
    assert torch.equal(y1, y0)


def test_predictor_guard_recovers_out_of_range_backbone_1x1_weights(cuda, monkeypatch):
    """As tests/test_gpu_split_range.py::test_predictor_guard_recovers_out_of_range_conv_weights, for a marked
    backbone conv: its weights scaled past fp16's range set the flag, and the guarded predict equals the exact run."""
    from yolosod_amd.engine.predictor import DetectionPredictor, seeded_images
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import build_model
    monkeypatch.setattr(M, "N1_BACKBONE", True)
    m = build_model(CFG, seed=0, device=cuda)
    pred = DetectionPredictor(m, conf=0.001, iou=0.7, max_det=300)
    conv = next(c for c in pred.model.modules() if isinstance(c, M.Conv) and c.n1_backbone)
    with torch.no_grad():
        conv.conv.weight.mul_(4e4)
    x = seeded_images(0, 2, 256, device=cuda)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        _hip.split_range_flag(reset=True)
        with torch.inference_mode():
            pred.predict_padded(x)
        assert _hip.split_range_flag(reset=True)  # the kernel saw its weights out of range
        with torch.inference_mode():
            g_out, g_cnt, g_idx = pred.predict_padded_guarded(x)
        assert not _hip.split_range_flag(reset=True)  # the guard consumed (and cleared) the flag
        with torch.inference_mode(), _hip.exact_fp32_matrix():
            r_out, r_cnt, r_idx = pred.predict_padded(x)
        assert not _hip.split_range_flag(reset=True)  # nothing on the exact path splits
    finally:
        torch.backends.cudnn.deterministic = det
    assert torch.isfinite(g_out).all()
    assert torch.equal(g_cnt, r_cnt) and torch.equal(g_idx, r_idx) and torch.equal(g_out, r_out)
