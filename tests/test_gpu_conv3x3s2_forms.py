"""GPU: the forms of the tiled stride-2 3x3 conv kernel (csrc/conv3x3s2.hip, conv3x3s2_t2_kernel): three tile
geometries (the 32 x 2 output tile of 16 x 1 pixel blocks, the 40 x 2 tile of 8 x 2 blocks, the 20 x 4 tile of 4 x 4
blocks) x two output group widths (128 / 64 channels), forced through yolosod_debug_set_conv3x3s2_form. The order of
an output element's additions does not depend on the form, so every form must give the 32 x 2 tile's result bit for
bit, and the automatic form must keep the fp64 bound of tests/test_gpu_conv3x3s2.py. (Cout 64 has 64-channel groups
only; Cout 64 from Cin 32 runs the register-weight kernel, which has one form.)"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

# input (H, W) at batch 2: an output smaller than any tile; exactly one column of 20 x 4 tiles; exactly one column of
# 40 x 2 tiles; odd Ho with ragged last tiles in both directions; two 40-wide tiles with the second ragged
SIZES = [(8, 8), (40, 40), (80, 80), (38, 72), (24, 88)]
CHANNELS = [(32, 64), (96, 64), (32, 128), (96, 128), (32, 256), (96, 256)]  # one / several chunks x the group loop
GEOS = (1, 2, 3)  # 32 x 2, 40 x 2 (8 x 2 blocks), 20 x 4 (4 x 4 blocks)
G128, G64 = 1, 2
CFG = "yolov12-sod-fusion-v5-simple.yaml"


def _forms(cout):
    return [g + 4 * grp for g in GEOS for grp in ((G64,) if cout == 64 else (G128, G64))]


def _ref_form(cout):
    return 1 + 4 * (G64 if cout == 64 else G128)  # the 32 x 2 tile in the group width the kernel had before the forms


class _forced:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_conv3x3s2_form(self.form)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_conv3x3s2_form(self.old)


def _gated(x, gc, gp):
    y = x
    if gc is not None:
        y = y * gc[:, :, None, None]
    if gp is not None:
        y = y * gp[:, None]
    return y


@functools.lru_cache(maxsize=None)
def _case(size, cin, cout, gates):
    """Inputs, the fp64 reference, MIOpen's fp32 error and the 32 x 2 form's output of one case (computed once)."""
    H, W = size
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(H + W + cin + cout + len(gates))
    x = torch.randn(2, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (3 * cin ** 0.5))
    b = torch.randn(cout, generator=g) * 0.1
    gc = torch.sigmoid(torch.randn(2, cin, generator=g)) if "c" in gates else None
    gp = torch.sigmoid(torch.randn(2, H, W, generator=g)) if "p" in gates else None
    xg = _gated(x, gc, gp)  # fp32 products, as the reference's gate output
    ref = F.silu(F.conv2d(xg.double(), w.double(), b.double(), stride=2, padding=1))
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    xd, wd, bd, gcd, gpd = d(x), d(w), d(b), d(gc), d(gp)
    err_m = float((F.silu(F.conv2d(d(xg), wd, bd, stride=2, padding=1)).cpu().double() - ref).abs().max())
    prep = _hip.conv3x3s2_prepare(wd)
    with _forced(_ref_form(cout)):
        y0 = _hip.conv3x3s2_silu(xd, bd, lambda: prep, cout, gcd, gpd)
    return xd, bd, gcd, gpd, prep, ref, err_m, y0


def _check_case(size, cin, cout, gates):
    xd, bd, gcd, gpd, prep, ref, err_m, y0 = _case(size, cin, cout, gates)
    lib = _hip.load_library()
    for form in _forms(cout):
        with _forced(form):
            assert lib.yolosod_debug_conv3x3s2_form(2, cout, size[0], size[1]) == form
            y = _hip.conv3x3s2_silu(xd, bd, lambda: prep, cout, gcd, gpd)
            y2 = _hip.conv3x3s2_silu(xd, bd, lambda: prep, cout, gcd, gpd)
        assert torch.equal(y, y0), f"{size} {cin}->{cout} {gates}: form {form} differs from the 32 x 2 form"
        assert torch.equal(y, y2), f"{size} {cin}->{cout} {gates}: form {form} is not deterministic"
    with _forced(0):
        ya = _hip.conv3x3s2_silu(xd, bd, lambda: prep, cout, gcd, gpd)
    assert torch.equal(ya, y0), f"{size} {cin}->{cout} {gates}: the automatic form differs from the 32 x 2 form"
    yc = ya.cpu().double()
    assert yc.shape == ref.shape
    err = float((yc - ref).abs().max())
    print(f"{size} {cin}->{cout} {gates}: max abs err {err:.3g} (MIOpen fp32 {err_m:.3g})")
    ok, e, _ = tol_close(yc, ref, 5e-5, 1e-4)
    assert ok, f"{size} {cin}->{cout} {gates}: max abs err {e:.3g} (MIOpen fp32 {err_m:.3g})"
    assert err <= 8 * err_m + 1e-5, (err, err_m)


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("size", SIZES)
def test_forms_match_fp64_and_each_other(size, cin, cout, cuda):
    _check_case(size, cin, cout, "")


@pytest.mark.parametrize("gates", ["c", "p", "cp"])
@pytest.mark.parametrize("size,cin,cout", [((8, 8), 96, 64), ((40, 40), 32, 128), ((80, 80), 96, 128),
                                           ((38, 72), 96, 256), ((24, 88), 96, 64)])
def test_forms_apply_the_gates_alike(size, cin, cout, gates, cuda):
    _check_case(size, cin, cout, gates)


@pytest.mark.parametrize("size,cin,cout", [((38, 72), 96, 128), ((24, 88), 32, 256), ((40, 40), 96, 64)])
def test_forms_into_concat_slice(size, cin, cout, cuda):
    """out= a channel slice of a concat buffer: bit-identical in every form, the other channels keep their fill."""
    xd, bd, _, _, prep, _, _, y0 = _case(size, cin, cout, "")
    Ho, Wo = y0.shape[2:]
    for form in _forms(cout):
        buf = torch.full((2, cout + 96, Ho, Wo), -7.5, device=cuda)
        with _forced(form):
            _hip.conv3x3s2_silu(xd, bd, lambda: prep, cout, out=buf[:, 32:32 + cout])
        assert torch.equal(buf[:, 32:32 + cout], y0), form
        assert (buf[:, :32] == -7.5).all() and (buf[:, 32 + cout:] == -7.5).all(), form


@pytest.mark.parametrize("geo", [2, 3])
def test_new_forms_raise_the_range_flag(geo, cuda):
    """One input value beyond fp16's range, in the last (ragged) tile of a new geometry, sets the range flag; the same
    launch without it leaves the flag clear."""
    xd, bd, _, _, prep, _, _, _ = _case((38, 72), 96, 128, "")
    with _forced(geo):
        _hip.split_range_flag(reset=True)
        _hip.conv3x3s2_silu(xd, bd, lambda: prep, 128)
        assert not _hip.split_range_flag(reset=True)
        bad = xd.clone()
        bad[1, 95, 37, 71] = 1e6
        _hip.conv3x3s2_silu(bad, bd, lambda: prep, 128)
        assert _hip.split_range_flag(reset=True)


def test_automatic_form_of_the_model_shapes(cuda):
    """The five gate-free stride-2 launches of the n640 step at batch 32 (input shapes) and the gated L5 shape: 40-wide
    outputs on the 40 x 2 tile, 20-wide outputs on the 20 x 4 tile, 80-wide outputs on the 32 x 2 tile; 128-channel
    groups throughout (the measurements behind the rule: DESIGN.md, the section on the stride-2 forms)."""
    lib = _hip.load_library()
    with _forced(0):
        assert lib.yolosod_debug_conv3x3s2_form(32, 256, 80, 80) == 2 + 4 * G128    # L7, L33
        assert lib.yolosod_debug_conv3x3s2_form(32, 512, 40, 40) == 3 + 4 * G128    # L10, L36
        assert lib.yolosod_debug_conv3x3s2_form(32, 128, 160, 160) == 1 + 4 * G128  # L29, L5
        assert lib.yolosod_debug_conv3x3s2_form(32, 64, 160, 160) == 1 + 4 * G64
        assert lib.yolosod_debug_conv3x3s2_form(32, 128, 80, 78) == 0               # output width 39
    with _forced(3 + 4 * G64):
        assert lib.yolosod_debug_conv3x3s2_form(32, 256, 80, 80) == 3 + 4 * G64
    assert lib.yolosod_debug_set_conv3x3s2_form(99) == 0 and lib.yolosod_debug_set_conv3x3s2_form(0) == 0  # ignored


def test_model_output_does_not_depend_on_the_form(cuda):
    """The fp32 model at 256^2, batch 2: the 32 x 2 tile forced against the automatic choice, bit for bit."""
    from yolosod_amd.nn.tasks import build_model
    m = build_model(CFG, seed=0, device=cuda)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(17)).to(cuda)
    lib = _hip.load_library()
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True  # MIOpen's split-K solvers add with atomics otherwise
    try:
        with torch.inference_mode():
            with _forced(1):
                y0 = m(x)[0]
                y1 = m(x)[0]
            with _forced(0):
                # the automatic choice takes a new geometry for the backbone's stride-2 convs at this size
                assert lib.yolosod_debug_conv3x3s2_form(2, 256, 32, 32) & 3 != 1
                assert lib.yolosod_debug_conv3x3s2_form(2, 512, 16, 16) & 3 != 1
                ya = m(x)[0]
    finally:
        torch.backends.cudnn.deterministic = det
    assert torch.equal(y1, y0)  # the model itself repeats bit for bit
    assert torch.equal(ya, y0)
