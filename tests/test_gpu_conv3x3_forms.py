"""GPU: the forms of the persistent 3x3 conv kernel (csrc/conv3x3.hip): three tile geometries (the 32 x 8 tile of
16 x 1 pixel blocks, the 20 x 12 tile of 4 x 4 blocks, the 40 x 6 tile of 8 x 2 blocks) x two output group widths
(64 / 32 channels), forced through yolosod_debug_set_conv3x3_form. The order of an output element's additions does
not depend on the form, so every form must give the 32 x 8 / 64-channel-group result bit for bit (Cout 32 has only
32-channel groups: its 32 x 8 form is the reference there), and that result must keep the fp64 bound of
tests/test_gpu_conv3x3.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, H, W): 20^2 and 40^2 maps, a ragged last tile row, ragged on both edges, an image smaller than a
# tile, one block
SHAPES = [(2, 32, 32, 20, 20), (2, 64, 64, 20, 20), (1, 32, 128, 40, 40), (2, 32, 64, 12, 20), (1, 32, 64, 44, 36),
          (3, 64, 64, 8, 8), (1, 32, 64, 4, 4)]
GEOS = (1, 2, 3)   # 32 x 8, 20 x 12 (4 x 4 blocks), 40 x 6 (8 x 2 blocks)
G64, G32 = 1, 2


def _forms(cout):
    return [g + 4 * grp for g in GEOS for grp in ((G32,) if cout == 32 else (G64, G32))]


def _ref_form(cout):
    return 1 + 4 * (G32 if cout == 32 else G64)


class _forced:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_conv3x3_form(self.form)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_conv3x3_form(self.old)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, the fp64 reference, MIOpen's fp32 error and the reference form's output of one shape (computed once)."""
    B, cin, cout, H, W = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (3 * cin ** 0.5))
    b = torch.randn(cout, generator=g) * 0.1
    r = torch.randn(B, cout, H, W, generator=g)
    ref = F.silu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    xd, wd, bd, rd = x.to(dev), w.to(dev), b.to(dev), r.to(dev)
    err_m = float((F.silu(F.conv2d(xd, wd, bd, padding=1)).cpu().double() - ref).abs().max())
    prep = _hip.conv3x3_prepare(wd)
    with _forced(_ref_form(cout)):
        y0 = _hip.conv3x3_silu(xd, bd, lambda: prep, cout)
    return xd, bd, rd, prep, ref, err_m, y0


@pytest.mark.parametrize("shape", SHAPES)
def test_forms_match_fp64_and_each_other(shape, cuda):
    cout = shape[2]
    xd, bd, _, prep, ref, err_m, y0 = _case(shape)
    for form in _forms(cout):
        with _forced(form):
            assert _hip.load_library().yolosod_debug_conv3x3_form(shape[0], cout, shape[3], shape[4]) == form
            y = _hip.conv3x3_silu(xd, bd, lambda: prep, cout)
            y2 = _hip.conv3x3_silu(xd, bd, lambda: prep, cout)
        yc = y.cpu().double()
        err = float((yc - ref).abs().max())
        print(f"{shape} form {form}: max abs err {err:.3g} (MIOpen fp32 {err_m:.3g})")
        ok, e, _ = tol_close(yc, ref, 5e-5, 1e-4)
        assert ok, f"{shape} form {form}: max abs err {e:.3g} (MIOpen fp32 {err_m:.3g})"
        assert err <= 8 * err_m + 1e-5, (form, err, err_m)
        assert torch.equal(y, y0), f"{shape}: form {form} differs from the 32 x 8 form"
        assert torch.equal(y, y2), f"{shape}: form {form} is not deterministic"


@pytest.mark.parametrize("shape", [(2, 64, 64, 20, 20), (1, 32, 64, 44, 36)])
def test_forms_residual_and_slices_bit_identical(shape, cuda):
    """Residual, output into a concat slice, input (and residual) read from a channel slice: each bit-identical to
    the packed result (the residual is one separately rounded add after the activation)."""
    B, cin, cout, H, W = shape
    xd, bd, rd, prep, _, _, y0 = _case(shape)
    xbuf = torch.randn(B, cin + 96, H, W, device=cuda)
    xbuf[:, 32:32 + cin] = xd
    rbuf = torch.randn(B, cout + 32, H, W, device=cuda)
    rbuf[:, 32:] = rd
    for form in _forms(cout):
        with _forced(form):
            y_res = _hip.conv3x3_silu(xd, bd, lambda: prep, cout, res=rd)
            obuf = torch.full((B, cout + 64, H, W), float("nan"), device=cuda)
            _hip.conv3x3_silu(xd, bd, lambda: prep, cout, out=obuf[:, 32:32 + cout])
            y_xs = _hip.conv3x3_silu(xbuf[:, 32:32 + cin], bd, lambda: prep, cout)
            y_all = _hip.conv3x3_silu(xbuf[:, 32:32 + cin], bd, lambda: prep, cout, res=rbuf[:, 32:])
        assert torch.equal(y_res, y0 + rd), form
        assert torch.equal(obuf[:, 32:32 + cout], y0), form
        assert torch.isnan(obuf[:, :32]).all() and torch.isnan(obuf[:, 32 + cout:]).all(), form
        assert torch.equal(y_xs, y0), form
        assert torch.equal(y_all, y0 + rd), form


def test_automatic_choice_takes_32_channel_groups_when_underfilled(cuda):
    """One image of 44 x 36 with 64 outputs is a handful of 64-channel work items for hundreds of workgroup slots: the
    automatic choice launches 32-channel groups (and a small-map geometry) and equals the forced 32 x 8 / 64 form."""
    shape = (1, 32, 64, 44, 36)
    xd, bd, _, prep, _, _, y0 = _case(shape)
    lib = _hip.load_library()
    with _forced(0):
        form = lib.yolosod_debug_conv3x3_form(1, 64, 44, 36)
        y = _hip.conv3x3_silu(xd, bd, lambda: prep, 64)
    assert form >> 2 == G32 and form & 3 in (2, 3), form
    assert torch.equal(y, y0)
    with _forced(0):  # a full grid keeps 64-channel groups; P2 / P3 maps keep the 32 x 8 tile
        assert lib.yolosod_debug_conv3x3_form(32, 64, 160, 160) == 1 + 4 * G64
        assert lib.yolosod_debug_conv3x3_form(32, 128, 80, 80) == 1 + 4 * G64
        assert lib.yolosod_debug_conv3x3_form(32, 32, 160, 160) == 1 + 4 * G32


def test_forced_64_channel_groups_refuse_32_outputs(cuda):
    xd, bd, _, prep, _, _, _ = _case((2, 32, 32, 20, 20))
    with _forced(1 + 4 * G64):
        with pytest.raises(RuntimeError):
            _hip.conv3x3_silu(xd, bd, lambda: prep, 32)
