"""GPU: the statistics forms of the fp16-split 1x1 conv kernel (csrc/conv1x1x2.hip, yolosod_conv1x1x2_silu_stats):
the conv launch that also emits its output's per-plane sum (+ max) for the SE / CBAM gate behind it, in every routed
form (workgroups of 128 and, for Cout % 256 == 0, of 256 output channels; forced through
yolosod_debug_set_conv1x1x2_form).

Bounds, from the arithmetic alone: the stored output is the plain form's, bit for bit; the max is the max of the
stored values, bit for bit; the plane sum is HW fp32 additions of the stored values in some fixed order, so it differs
from their fp64 sum by at most HW * 2^-24 * sum|out| (every partial sum is at most sum|out| in magnitude and rounds
with relative error 2^-24). A pixel or a tile missed or counted twice is orders of magnitude above that.

The layer-31 conv ("capool") runs the plain launch and the CA_Block behind it pools the finished output itself (its
own path, tests/test_gpu_ops.py): there is no pool pass of this change's to test here, only the launch key."""
import pytest
import torch

from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

G128, G256, B1 = 1, 2, 4 * 1
CHANNELS = [(192, 128), (384, 256), (128, 128)]  # a last stage of 64 / 128 of 128 channels (two / three stages); one
# one tile; a 36-pixel last tile; 3.75 tiles; 6.25 tiles; 3.75 tiles of 40-wide rows
MAPS = [(8, 8), (10, 10), (12, 20), (20, 20), (6, 40)]


class _Form:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_conv1x1x2_form(self.form)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_conv1x1x2_form(self.old)
        return False


def _forms(cout):
    return [G128 + B1] + ([G256 + B1] if cout % 256 == 0 else [])


def _case(B, cin, cout, H, W, cuda):
    g = torch.Generator().manual_seed(1000 * cin + 10 * H + W + B)
    x = torch.randn(B, cin, H, W, generator=g).to(cuda)
    w = (torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin ** 0.5)).to(cuda)
    b = (torch.randn(cout, generator=g) * 0.1).to(cuda)
    return x, b, _hip.conv1x1x2_prepare(w)


def _stats(y):
    """(plane totals [B, C], k > 0 entries, the same for the maxes or None) of the PlaneStats attached to y."""
    st = y._ys_plane_stats
    B, C, H, W = y.shape
    assert st.shape == tuple(y.shape) and st.parts == _hip.plane_parts(H * W)[0]
    ps = st.psum.view(B, C, st.parts)
    pm = None if st.pmax is None else st.pmax.view(B, C, st.parts)
    return ps[:, :, 0], ps[:, :, 1:], None if pm is None else pm[:, :, 0], None if pm is None else pm[:, :, 1:]


def _check_stats(y, stats, what):
    B, C, H, W = y.shape
    s0, srest, m0, mrest = _stats(y)
    y64 = y.double()
    ref = y64.sum((2, 3))
    bound = H * W * 2.0 ** -24 * y64.abs().sum((2, 3))
    err = (s0.double() - ref).abs()
    print(what, "sum err / bound max", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all()), (what, float(err.max()), float(bound.min()))
    assert bool((srest == 0).all()), what
    if stats == "summax":
        assert torch.equal(m0, y.amax((2, 3))), what
        assert bool((mrest == float("-inf")).all()), what
    else:
        assert m0 is None, what


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("stats", ["sum", "summax"])
def test_output_bit_identical_and_statistics_of_the_stored_values(cin, cout, stats, cuda):
    lib = _hip.load_library()
    for H, W in MAPS + [(40, 40)]:
        B = 3 if (H, W) == (40, 40) else 2
        x, b, prep = _case(B, cin, cout, H, W, cuda)
        for form in _forms(cout):
            with _Form(form):
                assert lib.yolosod_debug_conv1x1x2_form(B, cout, H, W) == form
                y0 = _hip.conv1x1x2_silu(x, b, lambda: prep, cout)
                with _hip.op_timer() as t:
                    y = _hip.conv1x1x2_silu(x, b, lambda: prep, cout, stats=stats)
            assert [k for k, _ in t.durations_ms()] == [("conv1x1x2_stats", (B, cin, H, W), (cout, stats))]
            assert torch.equal(y, y0), (form, H, W)
            _check_stats(y, stats, (form, cin, cout, H, W))
    assert lib.yolosod_debug_set_conv1x1x2_form(0) == 0


@pytest.mark.parametrize("H,W", [(8, 8), (10, 10), (20, 20)])
def test_clamped_pixels_are_not_counted(H, W, cuda):
    """Zero weights and bias -5: every stored value is SiLU(-5) < 0, so a lane that counted nothing must not leave a
    0 in the max, and the sum is HW times that value. Then an input that is zero except the last pixel of every
    channel, with one-hot weight rows: on a ragged last tile the staging repeats that pixel for the pixels past HW,
    and the plane sum must hold it once."""
    cin, cout, B = 192, 256, 2
    HW = H * W
    x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(5)).to(cuda)
    prep0 = _hip.conv1x1x2_prepare(torch.zeros(cout, cin, 1, 1, device=cuda))
    bias = torch.full((cout,), -5.0, device=cuda)
    xl = torch.zeros(B, cin, H, W, device=cuda)
    xl[:, :, H - 1, W - 1] = 3.0
    w1 = torch.zeros(cout, cin, 1, 1, device=cuda)
    w1[torch.arange(cout), torch.arange(cout) % cin] = 1.0
    prep1 = _hip.conv1x1x2_prepare(w1)
    zero = torch.zeros(cout, device=cuda)
    for form in _forms(cout):
        with _Form(form):
            y = _hip.conv1x1x2_silu(x, bias, lambda: prep0, cout, stats="summax")
            yl = _hip.conv1x1x2_silu(xl, zero, lambda: prep1, cout, stats="summax")
        v = y[0, 0, 0, 0]
        assert float(v) < 0 and bool((y == v).all())
        s0, _, m0, _ = _stats(y)
        assert bool((m0 == v).all()), form
        assert bool(((s0.double() - HW * float(v)).abs() <= HW * 2.0 ** -24 * HW * abs(float(v))).all()), form
        # one non-zero stored value per plane (SiLU(0) = 0): the sum and the max are that value exactly
        assert int((yl != 0).sum()) == B * cout and bool((yl[:, :, H - 1, W - 1] > 2.8).all())
        s1, _, m1, _ = _stats(yl)
        assert torch.equal(s1, yl[:, :, H - 1, W - 1]) and torch.equal(m1, yl[:, :, H - 1, W - 1]), form


@pytest.mark.parametrize("cin,cout", [(192, 128), (384, 256)])
def test_channel_slices_between_nan(cin, cout, cuda):
    """Input and output as channel slices of buffers whose other channels, and a neighbouring image, are NaN."""
    B, H, W = 2, 10, 10
    x, b, prep = _case(B, cin, cout, H, W, cuda)
    xb = torch.full((B + 1, cin + 64, H, W), float("nan"), device=cuda)
    xb[:B, 32:32 + cin] = x
    xs = xb[:B, 32:32 + cin]
    for form in _forms(cout):
        for stats in ("sum", "summax"):
            z = torch.full((B + 1, cout + 256, H, W), float("nan"), device=cuda)
            with _Form(form):
                y0 = _hip.conv1x1x2_silu(x, b, lambda: prep, cout, stats=stats)
                y = _hip.conv1x1x2_silu(xs, b, lambda: prep, cout, out=z[:B, 128:128 + cout], stats=stats)
            assert torch.isfinite(y).all() and torch.equal(y, y0), (form, stats)
            assert torch.isnan(z[:B, :128]).all() and torch.isnan(z[:B, 128 + cout:]).all() and torch.isnan(z[B]).all()
            a, c = _stats(y0), _stats(y)
            assert torch.isfinite(c[0]).all() and torch.equal(a[0], c[0]), (form, stats)
            if stats == "summax":
                assert torch.isfinite(c[2]).all() and torch.equal(a[2], c[2]), (form, stats)


def test_split_range_flag(cuda):
    """1e6 (beyond fp16) in the last channel of the last image raises the split-range flag; otherwise it stays clear."""
    B, cin, cout, H, W = 2, 192, 256, 10, 10
    x, b, prep = _case(B, cin, cout, H, W, cuda)
    big = x.clone()
    big[B - 1, cin - 1, H - 1, W - 1] = 1e6
    for form in _forms(cout):
        for stats in ("sum", "summax"):
            with _Form(form):
                _hip.split_range_flag(reset=True)
                _hip.conv1x1x2_silu(x, b, lambda: prep, cout, stats=stats)
                assert not _hip.split_range_flag(reset=True), (form, stats)
                _hip.conv1x1x2_silu(big, b, lambda: prep, cout, stats=stats)
                assert _hip.split_range_flag(reset=True), (form, stats)


def test_statistics_independent_of_the_batch(cuda):
    B, cin, cout, H, W = 3, 384, 256, 12, 20
    x, b, prep = _case(B, cin, cout, H, W, cuda)
    for form in _forms(cout):
        with _Form(form):
            y3 = _hip.conv1x1x2_silu(x, b, lambda: prep, cout, stats="summax")
            y1 = _hip.conv1x1x2_silu(x[:1].contiguous(), b, lambda: prep, cout, stats="summax")
        a, c = _stats(y3), _stats(y1)
        assert torch.equal(y3[:1], y1) and torch.equal(a[0][:1], c[0]) and torch.equal(a[2][:1], c[2]), form


def test_gates_read_the_attached_statistics(cuda):
    """SE / CBAM fed the kernel's output use its statistics (no statistics pass of their own) and give what they give
    on the same tensor without them, within the rounding of the plane mean (another addition order)."""
    B, cin, cout, H, W = 2, 192, 128, 12, 20
    x, b, prep = _case(B, cin, cout, H, W, cuda)
    g = torch.Generator().manual_seed(3)
    hid = cout // 16
    fc1_w, fc1_b = (torch.randn(hid, cout, generator=g) * 0.1).to(cuda), torch.zeros(hid, device=cuda)
    fc2_w, fc2_b = (torch.randn(cout, hid, generator=g) * 0.1).to(cuda), torch.zeros(cout, device=cuda)
    y = _hip.conv1x1x2_silu(x, b, lambda: prep, cout, stats="sum")
    assert _hip._pre_stats(y, False) is not None and _hip._pre_stats(y, True) is None
    o1 = _hip.se_forward(y, fc1_w, fc1_b, fc2_w, fc2_b)
    o0 = _hip.se_forward(y.clone(), fc1_w, fc1_b, fc2_w, fc2_b)
    assert float((o1 - o0).abs().max()) <= 1e-5
    ym = _hip.conv1x1x2_silu(x, b, lambda: prep, cout, stats="summax")
    assert _hip._pre_stats(ym, True) is not None


def test_capool_is_the_plain_launch_under_the_statistics_key(cuda):
    B, cin, cout, H, W = 2, 192, 128, 8, 12
    x, b, prep = _case(B, cin, cout, H, W, cuda)
    y0 = _hip.conv1x1x2_silu(x, b, lambda: prep, cout)
    with _hip.op_timer() as t:
        y = _hip.conv1x1x2_silu(x, b, lambda: prep, cout, stats="capool")
    assert [k for k, _ in t.durations_ms()] == [("conv1x1x2_stats", (B, cin, H, W), (cout, "capool"))]
    assert torch.equal(y, y0) and not hasattr(y, "_ys_ca_pool") and not hasattr(y, "_ys_plane_stats")


def test_bad_arguments_are_errors(cuda):
    x, b, prep = _case(2, 192, 128, 8, 8, cuda)
    with pytest.raises(RuntimeError):
        _hip.conv1x1x2_silu(x, b, lambda: prep, 128, stats="mean")
    with pytest.raises(RuntimeError):
        _hip.conv1x1x2_silu(x, b, lambda: prep, 128, stats="sum", out2=torch.empty(2, 64, 8, 8, device=cuda), c2lo=64)
