"""GPU: the halo staging of the persistent 3x3 conv kernel (csrc/conv3x3.hip): aligned groups of four pixels, one
16-byte buffer load per channel, placed into the LDS planes pixel by pixel. Every form (three tile geometries x two
output group widths, forced through yolosod_debug_set_conv3x3_form) is checked for

- placement, independent of any summation order: with one weight of 1.0 per output channel (tap t of input channel
  pi(o)), every other product is an exact zero, so tap t's output is the centre tap's output moved by the tap offset,
  bit for bit, and exactly 0 where the source pixel is outside the image;
- no leak through the overhang: the groups before and after a tile row, the rows above and below the image and the
  channels past the last chunk read memory that is not the input (NaN here) and must not reach the output;
- the split-range flag: a value beyond fp16's range in the last staged corner positions is still seen."""
import functools

import pytest
import torch
import torch.nn.functional as F

from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

GEOS = (1, 2, 3)   # 32 x 8, 20 x 12 (4 x 4 blocks), 40 x 6 (8 x 2 blocks)
G64, G32 = 1, 2
# (B, H, W): smaller than any tile, one exact tile of each geometry, ragged in both directions, the narrowest legal
# width (tile overhang on every side)
PLACE_SHAPES = [(2, 8, 8), (2, 8, 32), (2, 12, 20), (2, 6, 40), (2, 24, 44), (1, 3, 4)]
CHANNELS = [(32, 32), (32, 64), (64, 32), (64, 64)]   # (Cin, Cout)


def _forms(cout):
    return [g + 4 * grp for g in GEOS for grp in ((G32,) if cout == 32 else (G64, G32))]


class _forced:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_conv3x3_form(self.form)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_conv3x3_form(self.old)


@functools.lru_cache(maxsize=None)
def _pi(cin, cout):
    """Input channel of output channel o (a fixed draw; both 32-channel chunks of Cin 64 are hit)."""
    g = torch.Generator().manual_seed(100 * cin + cout)
    pi = torch.cat([torch.randperm(cin, generator=g) for _ in range((cout + cin - 1) // cin)])[:cout]
    assert cin == 32 or (bool((pi < 32).any()) and bool((pi >= 32).any()))
    return pi


@functools.lru_cache(maxsize=None)
def _tap_prep(cin, cout, t):
    w = torch.zeros(cout, cin, 3, 3)
    w[torch.arange(cout), _pi(cin, cout), t // 3, t % 3] = 1.0
    return _hip.conv3x3_prepare(w.to("cuda:0"))


@pytest.mark.parametrize("shape", PLACE_SHAPES)
def test_every_tap_places_every_pixel(shape, cuda):
    B, H, W = shape
    for cin, cout in CHANNELS:
        g = torch.Generator().manual_seed(B + H + W + cin + cout)
        x = torch.randn(B, cin, H, W, generator=g).to(cuda)
        bias = torch.zeros(cout, device=cuda)
        want_c = F.silu(x[:, _pi(cin, cout).to(cuda)])
        for form in _forms(cout):
            with _forced(form):
                assert _hip.load_library().yolosod_debug_conv3x3_form(B, cout, H, W) == form
                ys = [_hip.conv3x3_silu(x, bias, functools.partial(_tap_prep, cin, cout, t), cout) for t in range(9)]
            yc = ys[4]
            # the centre tap is SiLU of the selected channel: the two-term split keeps 22 bits and the hardware
            # exp2 / rcp SiLU ~2^-22 relative (the bound of tests/test_gpu_conv3x3_forms.py)
            assert torch.allclose(yc, want_c, rtol=1e-4, atol=5e-5), (shape, cin, cout, form)
            ypad = F.pad(yc, (1, 1, 1, 1))   # 0 where the source pixel is outside the image
            for t in range(9):
                dy, dx = t // 3 - 1, t % 3 - 1
                want = ypad[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                assert torch.equal(ys[t], want), f"{shape} Cin {cin} Cout {cout} form {form}: tap {t} misplaced"


@pytest.mark.parametrize("hw", [(24, 44), (8, 8)])
@pytest.mark.parametrize("cin", [32, 64])
def test_nothing_leaks_through_the_overhang(hw, cin, cuda):
    """Input and residual as channel slices of wider buffers whose other channels, and one image before and after,
    are NaN: finite, and bit for bit the result on packed copies."""
    B, (H, W) = 2, hw
    nan = float("nan")
    for cout in (32, 64):
        g = torch.Generator().manual_seed(H + W + cin + cout)
        x = torch.randn(B, cin, H, W, generator=g).to(cuda)
        r = torch.randn(B, cout, H, W, generator=g).to(cuda)
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (3 * cin ** 0.5))).to(cuda)
        bias = (torch.randn(cout, generator=g) * 0.1).to(cuda)
        prep = _hip.conv3x3_prepare(w)
        xbuf = torch.full((B + 2, cin + 64, H, W), nan, device=cuda)
        xbuf[1:B + 1, 32:32 + cin] = x
        rbuf = torch.full((B + 2, cout + 64, H, W), nan, device=cuda)
        rbuf[1:B + 1, 32:32 + cout] = r
        xs, rs = xbuf[1:B + 1, 32:32 + cin], rbuf[1:B + 1, 32:32 + cout]
        for form in _forms(cout):
            with _forced(form):
                y0 = _hip.conv3x3_silu(x, bias, lambda: prep, cout)
                y0r = _hip.conv3x3_silu(x, bias, lambda: prep, cout, res=r)
                y = _hip.conv3x3_silu(xs, bias, lambda: prep, cout)
                yr = _hip.conv3x3_silu(xs, bias, lambda: prep, cout, res=rs)
            assert torch.isfinite(y).all() and torch.isfinite(yr).all(), (hw, cin, cout, form)
            assert torch.equal(y, y0) and torch.equal(yr, y0r), (hw, cin, cout, form)
            assert torch.equal(y0r, y0 + r), (hw, cin, cout, form)


@pytest.mark.parametrize("shape", [(2, 24, 44), (2, 8, 8), (1, 3, 4)])
def test_range_flag_sees_the_corners(shape, cuda):
    """One value of 1e6 (beyond fp16) at an image corner, in the last channel of the last chunk of the last image."""
    B, H, W = shape
    cin, cout = 64, 64
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(B, cin, H, W, generator=g).to(cuda)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (3 * cin ** 0.5))).to(cuda)
    bias = torch.zeros(cout, device=cuda)
    prep = _hip.conv3x3_prepare(w)
    _hip.split_range_flag(reset=True)
    for form in _forms(cout):
        with _forced(form):
            _hip.conv3x3_silu(x, bias, lambda: prep, cout)
            assert not _hip.split_range_flag(reset=True), (shape, form)
            for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
                xb = x.clone()
                xb[B - 1, cin - 1, cy, cx] = 1e6
                _hip.conv3x3_silu(xb, bias, lambda: prep, cout)
                assert _hip.split_range_flag(reset=True), (shape, form, cy, cx)
