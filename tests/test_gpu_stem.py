"""GPU: the stem kernel (csrc/stem.hip: layer 0, Conv 3 -> 32, 3x3 / stride 2 / pad 1, SiLU, plus the plane sums of the
SE that follows) against the exact (fp64) conv + bias + SiLU of the same fp32 weights, next to the MIOpen fp32 path's own
error; its statistics, determinism, the shapes it refuses (stem_ok) and the model routing (YOLOSOD_STEM_HIP)."""
import pytest
import torch
import torch.nn.functional as F

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

# Hout * Wout = 129 * 128 = 16512: _hip.plane_parts gives 2 parts of 8256 floats, and 8256 % 128 = 64 - the segment
# boundary falls inside an output row (asserted in the test)
SPLIT_ROW_SHAPE = (1, 3, 258, 256)
SHAPES = [(2, 3, 64, 64), (1, 3, 40, 56), (2, 3, 24, 104), SPLIT_ROW_SHAPE, (2, 3, 640, 640)]


def _inputs(shape, cout=32):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    # large border values: a missing top / left zero pad (or a read past the right / bottom edge) shows at once
    x[:, :, 0, :] *= 4.0
    x[:, :, :, 0] *= 4.0
    x[:, :, -1, :] *= 4.0
    x[:, :, :, -1] *= 4.0
    w = torch.randn(cout, shape[1], 3, 3, generator=g) * (1.0 / (3 * shape[1] ** 0.5))
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b


def _ref64(x, w, b):
    return F.silu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1))


class _FakeConv:
    """The attributes stem_ok reads of a fused nn.Conv2d."""

    def __init__(self, w, b):
        self.weight, self.bias = w, b
        self.in_channels, self.out_channels = w.shape[1], w.shape[0]
        self.kernel_size, self.stride, self.padding, self.dilation, self.groups = (3, 3), (2, 2), (1, 1), (1, 1), 1
        self.padding_mode = "zeros"


@pytest.fixture(scope="module")
def runs(cuda):
    """shape -> (y on the GPU, fp64 reference, MIOpen fp32 output), computed once."""
    cache = {}

    def get(shape):
        if shape not in cache:
            x, w, b = _inputs(shape)
            xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
            assert _hip.stem_ok(xd, _FakeConv(wd, bd))
            y = _hip.stem_conv(xd, wd, bd)
            miopen = F.silu(F.conv2d(xd, wd, bd, stride=2, padding=1)).cpu().double()
            cache[shape] = (y, _ref64(x, w, b), miopen, (xd, wd, bd))
        return cache[shape]

    return get


@pytest.mark.parametrize("shape", SHAPES)
def test_stem_matches_fp64(shape, runs):
    y, ref, miopen, _ = runs(shape)
    yd = y.cpu().double()
    err, err_m = float((yd - ref).abs().max()), float((miopen - ref).abs().max())
    print(f"stem {shape}: max abs err {err:.3g} (MIOpen fp32 {err_m:.3g})")
    ok, e, ratio = tol_close(yd, ref, 5e-5, 1e-4)
    assert ok, f"{shape}: max abs err {e:.3g} (MIOpen fp32 {err_m:.3g})"
    # both sides compute exact fp32 products and differ only in the summation order of the 27 of them
    assert err <= 2 * err_m + 1e-6, (err, err_m)


def test_split_row_shape_splits_a_row():
    _, _, H, W = SPLIT_ROW_SHAPE
    parts, seg = _hip.plane_parts((H // 2) * (W // 2))
    assert parts >= 2 and seg % (W // 2) != 0, (parts, seg)


@pytest.mark.parametrize("shape", SHAPES)
def test_stem_plane_sums(shape, runs):
    """psum summed over the parts = the fp64 sum of the kernel's own stored output, per part too."""
    y, _, _, _ = runs(shape)
    st = y._ys_plane_stats
    B, C, Ho, Wo = y.shape
    assert st.shape == tuple(y.shape) and st.pmax is None and st.parts == _hip.plane_parts(Ho * Wo)[0]
    yd = y.double().cpu()
    s = st.psum.view(B, C, st.parts).double().cpu()
    ok, e, _ = tol_close(s.sum(-1), yd.sum((2, 3)), 1e-6, 1e-5)
    print(f"stem {shape}: plane sums max abs err {e:.3g}")
    assert ok, e
    seg = _hip.plane_parts(Ho * Wo)[1]
    flat = yd.reshape(B, C, Ho * Wo)
    per = torch.stack([flat[:, :, k * seg:(k + 1) * seg].sum(-1) for k in range(st.parts)], -1)
    ok, e, _ = tol_close(s, per, 1e-6, 1e-5)
    assert ok, f"per-part sums: {e:.3g}"


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), SPLIT_ROW_SHAPE])
def test_stem_stats_feed_se(shape, runs, cuda):
    """SE consuming the kernel's statistics = SE running its own statistics pass on the same tensor."""
    import recipes
    from yolosod_amd.nn import modules as M
    y, _, _, _ = runs(shape)
    plain = y.clone()  # no _ys_plane_stats
    assert getattr(plain, "_ys_plane_stats", None) is None
    se = M.SE_Block(4)
    se._maybe_build(y.shape[1], None)
    recipes.perturb_(se, 3)
    se.to(cuda).eval()
    with torch.inference_mode():
        a = se(plain)
        b = se(y)
    ok, err, _ = tol_close(b.cpu(), a.cpu(), 1e-6, 1e-5)
    assert ok, err


def test_stem_deterministic(runs):
    y, _, _, (xd, wd, bd) = runs(SPLIT_ROW_SHAPE)
    y2 = _hip.stem_conv(xd, wd, bd)
    assert torch.equal(y, y2) and torch.equal(y._ys_plane_stats.psum, y2._ys_plane_stats.psum)


def _fused_stem(cin, cuda):
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import _fuse_conv_and_bn
    torch.manual_seed(5)
    m = M.Conv(cin, 32, 3, 2)
    m.conv = _fuse_conv_and_bn(m.conv, m.bn)
    delattr(m, "bn")
    m.forward = m.forward_fuse
    m.emit_stats, m.stem = "sum", True
    return m.to(cuda).eval()


@pytest.mark.parametrize("shape,dtype", [((1, 3, 40, 56), torch.bfloat16), ((1, 3, 41, 56), torch.float32),
                                         ((1, 3, 40, 52), torch.float32), ((1, 4, 40, 56), torch.float32)])
def test_stem_ok_refuses_and_falls_back(shape, dtype, cuda, monkeypatch):
    """bf16, odd H, Wout % 4 != 0 and Cin = 4 keep the MIOpen + epilogue path: no stem launch, the switch-off result."""
    from yolosod_amd.nn import modules as M
    m = _fused_stem(shape[1], cuda).to(dtype)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(cuda).to(dtype)
    assert not _hip.stem_ok(x, m.conv)
    with torch.inference_mode():
        monkeypatch.setattr(M, "STEM_HIP", True)
        with _hip.op_timer() as t:
            y1 = m(x)
        assert all(k[0] != "stem" for k, _ in t.durations_ms())
        monkeypatch.setattr(M, "STEM_HIP", False)
        y0 = m(x)
    assert torch.equal(y1, y0)


def test_stem_ok_accepts_and_refuses_cpu(cuda):
    m = _fused_stem(3, cuda)
    assert _hip.stem_ok(torch.zeros(1, 3, 40, 56, device=cuda), m.conv)
    assert not _hip.stem_ok(torch.zeros(1, 3, 40, 56), m.conv)


def test_bf16_model_keeps_todays_path(cuda, monkeypatch):
    from yolosod_amd.nn import modules as M
    from yolosod_amd.nn.tasks import build_model
    m = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda, dtype=torch.bfloat16)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(4)).to(cuda).bfloat16()
    torch.backends.cudnn.deterministic = True  # MIOpen's bf16 convolutions repeat bit for bit only with this
    try:
        with torch.inference_mode():
            monkeypatch.setattr(M, "STEM_HIP", True)
            with _hip.op_timer() as t:
                y1 = m(x)[0]
            assert all(k[0] != "stem" for k, _ in t.durations_ms())
            monkeypatch.setattr(M, "STEM_HIP", False)
            y0 = m(x)[0]
    finally:
        torch.backends.cudnn.deterministic = False
    assert torch.equal(y1, y0), float((y1 - y0).abs().max())


@pytest.fixture(scope="module")
def paper_model(cuda):
    from yolosod_amd.nn.tasks import build_model
    return build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda)


@pytest.mark.parametrize("size", [256, 640])
def test_model_takes_the_stem_kernel(size, paper_model, cuda, monkeypatch):
    """Layer 0 routes to the kernel (one 'stem' launch, no statistics epilogue at its output shape) and the model
    matches the MIOpen + epilogue path (YOLOSOD_STEM_HIP=0) within fp32 accuracy."""
    from yolosod_amd.nn import modules as M
    m = paper_model
    x = torch.rand(2, 3, size, size, generator=torch.Generator().manual_seed(4)).to(cuda)
    with torch.inference_mode():
        monkeypatch.setattr(M, "STEM_HIP", True)
        with _hip.op_timer() as t:
            y = m(x)[0]
        keys = [k for k, _ in t.durations_ms()]
        monkeypatch.setattr(M, "STEM_HIP", False)
        with _hip.op_timer() as t0:
            y0 = m(x)[0]
        keys0 = [k for k, _ in t0.durations_ms()]
    l0 = (2, 32, size // 2, size // 2)

    def l0_stats(ks):
        return [k for k in ks if k[0] == "bias_act" and tuple(k[1]) == l0 and isinstance(k[2], str) and "sum" in k[2]]

    assert [k for k in keys if k[0] == "stem"] == [("stem", (2, 3, size, size), (32, "sum"))]
    assert not l0_stats(keys)
    assert not [k for k in keys0 if k[0] == "stem"] and len(l0_stats(keys0)) == 1
    ok, e, _ = tol_close(y.cpu().double(), y0.cpu().double(), 1e-3, 1e-4)
    print(f"model {size}: stem kernel vs MIOpen path max abs diff {e:.3g}")
    assert ok, e
