"""GPU: the 32-channel C2f Bottleneck as one launch (csrc/conv3x3.hip, bottleneck3x3_c32_kernel: both 3x3 convs, the
intermediate map in LDS) against the two launches of the stride-1 fp16-split kernel it replaces: bit-identical on
every shape with and without the shortcut and in place in a concat buffer, the second conv's zero padding with nonzero
biases, the fp64 bound of tests/test_gpu_conv3x3.py, the split-range flag, and the model's routing."""
import pytest
import torch
import torch.nn.functional as F

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

SHAPES = [(2, 32, 8, 32),      # one exact tile
          (1, 32, 3, 4),       # smaller than the halo
          (2, 32, 12, 20), (2, 32, 6, 40),  # the other tile geometries' footprints
          (2, 32, 24, 44),     # ragged in both directions, W % 4 == 0
          (3, 32, 40, 36),
          (6, 32, 160, 160)]   # 600 tiles: a workgroup walks several, the read-ahead crosses tiles and images


class forced:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_bottleneck3x3_fuse(self.mode)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_bottleneck3x3_fuse(self.old)


def _params(shape, cuda, scale=1.0):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    w1 = torch.randn(32, 32, 3, 3, generator=g) * (scale / (3 * 32 ** 0.5))
    w2 = torch.randn(32, 32, 3, 3, generator=g) * (1.0 / (3 * 32 ** 0.5))
    b1 = torch.randn(32, generator=g) * 0.5 + 0.25  # nonzero: SiLU(b1) != 0 is what a wrong padding would show
    b2 = torch.randn(32, generator=g) * 0.5 - 0.25
    return [t.to(cuda) for t in (x, w1, b1, w2, b2)]


def _pair(x, b1, p1, b2, p2, res, out=None):
    t = _hip.conv3x3_silu(x, b1, lambda: p1, 32)
    return _hip.conv3x3_silu(t, b2, lambda: p2, 32, out=out, res=x if res else None)


def _fused(x, b1, p1, b2, p2, res, out=None):
    return _hip.bottleneck3x3_silu(x, b1, lambda: p1, b2, lambda: p2, out=out, res=x if res else None)


@pytest.fixture(scope="module")
def cases(cuda):
    """Per shape: the operands, the prepared blocks and the pair's outputs (computed once, not modified)."""
    out = {}
    for shape in SHAPES:
        x, w1, b1, w2, b2 = _params(shape, cuda)
        p1, p2 = _hip.conv3x3_prepare(w1), _hip.conv3x3_prepare(w2)
        out[shape] = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, p1=p1, p2=p2,
                          pair={res: _pair(x, b1, p1, b2, p2, res) for res in (False, True)})
    return out


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_equals_the_pair(shape, res, cases, cuda):
    c = cases[shape]
    _hip.split_range_flag(reset=True)
    y = _fused(c["x"], c["b1"], c["p1"], c["b2"], c["p2"], res)
    ref = c["pair"][res]
    assert torch.equal(y, ref), f"{shape} res={res}: max |d| {float((y - ref).abs().max()):.3g}"
    assert not _hip.split_range_flag(reset=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_in_place_in_a_concat_buffer(shape, cases, cuda):
    """Input z[:, 32:64], output z[:, 64:96] of one 96-channel buffer (C2f.forward's slices); every other channel and
    a neighbouring image are NaN before and after."""
    c = cases[shape]
    B, _, H, W = shape
    z = torch.full((B + 1, 96, H, W), float("nan"), device=cuda)
    z[:B, 32:64] = c["x"]
    _fused(z[:B, 32:64], c["b1"], c["p1"], c["b2"], c["p2"], True, out=z[:B, 64:96])
    y = z[:B, 64:96]
    assert torch.isfinite(y).all()
    assert torch.equal(y, c["pair"][True])
    assert torch.equal(z[:B, 32:64], c["x"])
    assert torch.isnan(z[:B, :32]).all() and torch.isnan(z[B]).all()


def test_padding_is_zero_not_silu_of_bias(cuda):
    """Zero input, W1 = 0, b1 = 3: the intermediate is SiLU(3) inside the image and zero outside it. With W2 summing
    the nine taps of one channel the interior sees nine of them, an edge six and a corner four."""
    B, H, W = 1, 20, 40
    x = torch.zeros(B, 32, H, W, device=cuda)
    w1 = torch.zeros(32, 32, 3, 3, device=cuda)
    b1 = torch.full((32,), 3.0, device=cuda)
    w2 = torch.zeros(32, 32, 3, 3, device=cuda)
    w2[:, 5] = 1.0  # one input channel hot
    b2 = torch.linspace(-0.5, 0.5, 32, device=cuda)
    p1, p2 = _hip.conv3x3_prepare(w1), _hip.conv3x3_prepare(w2)
    for res in (False, True):
        ref = _pair(x, b1, p1, b2, p2, res)
        y = _fused(x, b1, p1, b2, p2, res)
        for iy, ix in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 17), (H - 1, 33), (9, 0), (8, W - 1),
                       (7, 31), (7, 32), (8, 31)):
            assert torch.equal(y[:, :, iy, ix], ref[:, :, iy, ix]), (res, iy, ix)
        assert torch.equal(y, ref)
        s3 = float(F.silu(torch.tensor(3.0)))
        want = F.silu(torch.tensor([4 * s3, 6 * s3, 9 * s3]) + float(b2[0]))
        got = torch.stack([y[0, 0, 0, 0], y[0, 0, 0, 17], y[0, 0, 9, 17]]).cpu()
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (got, want)
        assert not torch.equal(y[:, :, 0, 0], y[:, :, 9, 17]) and not torch.equal(y[:, :, 0, 17], y[:, :, 9, 17])


@pytest.mark.parametrize("shape", [(2, 32, 24, 44), (3, 32, 40, 36)])
def test_fused_matches_fp64(shape, cases, cuda):
    """The bound of tests/test_gpu_conv3x3.py against a double-precision reference of the pair, next to the error of
    the fp32 library convolution doing the same two steps."""
    c = cases[shape]
    x, w1, b1, w2, b2 = (c[k] for k in ("x", "w1", "b1", "w2", "b2"))
    xd = x.cpu().double()
    t = F.silu(F.conv2d(xd, w1.cpu().double(), b1.cpu().double(), padding=1))
    ref = xd + F.silu(F.conv2d(t, w2.cpu().double(), b2.cpu().double(), padding=1))
    y = _fused(x, b1, c["p1"], b2, c["p2"], True).cpu().double()
    mi = (x + F.silu(F.conv2d(F.silu(F.conv2d(x, w1, b1, padding=1)), w2, b2, padding=1))).cpu().double()
    err, err_m = float((y - ref).abs().max()), float((mi - ref).abs().max())
    print(f"{shape}: max abs err {err:.3g} (fp32 library conv {err_m:.3g})")
    ok, e, _ = tol_close(y, ref, 5e-5, 1e-4)
    assert ok, f"{shape}: max abs err {e:.3g} (fp32 library conv {err_m:.3g})"
    assert err <= 8 * err_m + 1e-5, (err, err_m)


def test_split_range_flag(cuda):
    shape = (2, 32, 24, 44)
    x, w1, b1, w2, b2 = _params(shape, cuda)
    p1, p2 = _hip.conv3x3_prepare(w1), _hip.conv3x3_prepare(w2)
    _hip.split_range_flag(reset=True)
    _fused(x, b1, p1, b2, p2, True)
    assert not _hip.split_range_flag(reset=True)
    xb = x.clone()
    xb[1, 7, 13, 21] = 1e6  # the input leaves fp16's range
    _fused(xb, b1, p1, b2, p2, True)
    assert _hip.split_range_flag(reset=True)
    # an in-range input whose intermediate leaves it: 64 W1 = 57600 is finite in fp16, SiLU(conv) ~ 900 * 288 * 0.8
    wb = torch.full_like(w1, 900.0)
    pb = _hip.conv3x3_prepare(wb)
    xp = x.abs()
    assert not _hip.split_range_flag(reset=True)
    t = _hip.conv3x3_silu(xp, b1, lambda: pb, 32)
    assert not _hip.split_range_flag(reset=True) and float(t.max()) > 65504.0
    _hip.conv3x3_silu(t, b2, lambda: p2, 32, res=xp)  # the pair's second launch stages the intermediate
    assert _hip.split_range_flag(reset=True)
    _fused(xp, b1, pb, b2, p2, True)
    assert _hip.split_range_flag(reset=True)
    # a prepared block whose own flag is up is re-reported, whichever conv it belongs to
    big = _hip.conv3x3_prepare(w2 * 2e4)
    _hip.split_range_flag(reset=True)
    _fused(x, b1, p1, b2, big, False)
    assert _hip.split_range_flag(reset=True)
    _fused(x, b1, big, b2, p2, False)
    assert _hip.split_range_flag(reset=True)


def _census(m, x):
    with _hip.op_timer() as t:
        y = m(x)[0]
    keys = [k[0] for k, _ in t.durations_ms()]
    return y, {k: keys.count(k) for k in ("bottleneck3x3", "bottleneck3x3_backbone", "conv3x3", "conv3x3_backbone")}


def test_model_routing(cuda):
    """Batch 2 at 256^2 (P2 maps of 64^2, 1 MB): forced on, the two P2 Bottlenecks are one launch each and the output
    is the two-launch model's bit for bit; with nothing forced no launch fuses at this size; inert in
    exact_fp32_matrix() and in bf16."""
    from yolosod_amd.nn.tasks import build_model
    m = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda)
    mb = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda, dtype=torch.bfloat16)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(7)).to(cuda)
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode():
            with forced(0):
                y0, n0 = _census(m, x)
            with forced(1):
                y1, n1 = _census(m, x)
                with _hip.exact_fp32_matrix():
                    _, ne = _census(m, x)
                _, nb = _census(mb, x.to(torch.bfloat16))
            _, na = _census(m, x)
    finally:
        torch.backends.cudnn.deterministic = False
    assert torch.equal(y1, y0), float((y1 - y0).abs().max())
    assert n0["bottleneck3x3"] == 0 and n0["bottleneck3x3_backbone"] == 0
    assert n1["bottleneck3x3"] == 1 and n1["bottleneck3x3_backbone"] == 1
    assert n0["conv3x3"] - n1["conv3x3"] == 2 and n0["conv3x3_backbone"] - n1["conv3x3_backbone"] == 2
    assert na == n0  # automatic: below the size threshold the two launches stay
    assert ne["bottleneck3x3"] == 0 and ne["bottleneck3x3_backbone"] == 0
    assert nb["bottleneck3x3"] == 0 and nb["bottleneck3x3_backbone"] == 0
