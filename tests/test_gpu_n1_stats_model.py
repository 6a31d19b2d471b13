"""GPU: the neck's gate-feeding wide 1x1 convs (cv2 of the C2fs L17 -> CBAM L18, L22 -> SE L23, L31 -> CA L32 of the
paper YAML) on the fp16-split 1x1 kernel with their statistics (modules.N1_STATS, yolosod_conv1x1x2_silu_stats) against
the MIOpen GEMM + bias / SiLU / statistics pass they replace, and the configurations that must not take the kernel
(exact_fp32_matrix(), the bf16 model). The paper YAML at 256^2, batch 2."""
import pytest
import torch

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

CFG = "yolov12-sod-fusion-v5-simple.yaml"
# layer: ((B, Cin, H, W), (Cout, statistics)) of its cv2 launch at 256^2, batch 2
LAUNCHES = {17: ((2, 384, 16, 16), (256, "summax")), 22: ((2, 192, 32, 32), (128, "sum")),
            31: ((2, 192, 32, 32), (128, "capool"))}
GATE_OPS = ("se", "cbam", "ca", "se_gate", "cbam_gate")


def _run(m, x):
    with _hip.op_timer() as t:
        y = m(x)[0]
    # without the weight preparations, which run once per parameter version
    return y, [k for k, _ in t.durations_ms() if not k[0].endswith("_prep")]


def _of(keys, op):
    return [k for k in keys if k[0] == op]


@pytest.fixture(scope="module")
def model_x(cuda):
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(14)).to(cuda)
    return m, x


@pytest.fixture(scope="module")
def off_run(model_x):
    """The switch at 0: the parent's launches (computed once)."""
    from yolosod_amd.nn import modules as M
    m, x = model_x
    old = M.N1_STATS
    M.N1_STATS = False
    try:
        with torch.inference_mode():
            return _run(m, x)
    finally:
        M.N1_STATS = old


def test_marked_convs(model_x):
    from yolosod_amd.nn import modules as M
    m, _ = model_x
    got = {c.n1_stats_layer: (c.conv.in_channels, c.conv.out_channels, c.emit_stats) for c in m.modules()
           if isinstance(c, M.Conv) and c.n1_stats_layer is not None}
    assert got == {i: (s[1], e[0], e[1]) for i, (s, e) in LAUNCHES.items()}
    for i in LAUNCHES:
        assert m.model[i].cv2.n1 is True and m.model[i].cv2.n1_stats_layer == i


def test_off_is_the_parents_launch_sequence(off_run):
    _, k0 = off_run
    assert not _of(k0, "conv1x1x2_stats")
    for (B, _, H, W), (cout, st) in LAUNCHES.values():  # the epilogue pass behind MIOpen's GEMM, with the statistics
        assert ("bias_act", (B, cout, H, W), st) in k0, (cout, st)


@pytest.mark.parametrize("layers", [{17, 22, 31}, {17}, {22, 31}])
def test_set_routes_exactly_its_layers_and_the_gates_use_the_statistics(layers, model_x, off_run, monkeypatch):
    from yolosod_amd.nn import modules as M
    m, x = model_x
    y0, k0 = off_run
    monkeypatch.setattr(M, "N1_STATS", True if layers == set(LAUNCHES) else frozenset(layers))
    with torch.inference_mode():
        _hip.split_range_flag(reset=True)
        y1, k1 = _run(m, x)
        assert not _hip.split_range_flag(reset=True)
    assert sorted(_of(k1, "conv1x1x2_stats")) == sorted(("conv1x1x2_stats",) + LAUNCHES[i] for i in layers)
    # the neck's other launches of the kernel keep their key and their number
    assert _of(k1, "conv1x1x2") == _of(k0, "conv1x1x2") and _of(k1, "conv1x1x2_backbone") == _of(k0, "conv1x1x2_backbone")
    # each routed conv drops its epilogue pass, and no gate launches anything it did not launch before (the SE / CBAM
    # read the attached statistics; the CA pools inside its own launch)
    assert len(_of(k0, "bias_act")) - len(_of(k1, "bias_act")) == len(layers)
    assert [k for k in k1 if k[0] in GATE_OPS] == [k for k in k0 if k[0] in GATE_OPS]
    assert len(k1) == len(k0)
    ok, e, _ = tol_close(y1.cpu().double(), y0.cpu().double(), 1e-3, 1e-4)
    assert ok, e


def test_switch_inert_in_exact_fp32(model_x, monkeypatch):
    from yolosod_amd.nn import modules as M
    m, x = model_x
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode(), _hip.exact_fp32_matrix():
            monkeypatch.setattr(M, "N1_STATS", True)
            y1, k1 = _run(m, x)
            monkeypatch.setattr(M, "N1_STATS", False)
            y0, k0 = _run(m, x)
    finally:
        torch.backends.cudnn.deterministic = det
    assert not _of(k1, "conv1x1x2_stats") and k1 == k0
    assert torch.equal(y1, y0)


def test_switch_inert_in_bf16(cuda, monkeypatch):
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda, dtype=torch.bfloat16)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(15)).to(cuda).to(torch.bfloat16)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode():
            monkeypatch.setattr(M, "N1_STATS", True)
            y1, k1 = _run(m, x)
            monkeypatch.setattr(M, "N1_STATS", False)
            y0, k0 = _run(m, x)
    finally:
        torch.backends.cudnn.deterministic = det
    assert not _of(k1, "conv1x1x2_stats") and k1 == k0
    assert torch.equal(y1, y0)
