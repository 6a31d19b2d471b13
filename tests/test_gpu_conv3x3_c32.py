"""GPU: the two further forms of the persistent 3x3 conv kernel's 32-channel output group (csrc/conv3x3.hip, F 1 / F 2;
form ids geometry + 4 * 3 and geometry + 4 * 4 of yolosod_debug_set_conv3x3_form) for Cin 32 -> Cout 32, layer 3's and
the neck's P2 Bottleneck convs: the wave's whole weight set resident in registers, and both 16-channel blocks on every
wave (four block slots each instead of eight). Neither changes the order of an output element's additions, so each
must equal today's 32-channel form (groups 2) of the same geometry bit for bit - plain, with the shortcut, and with
input / residual / output as channel slices of buffers that hold NaN everywhere else."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

C = 32
# (B, H, W): one 32 x 8 tile; ragged in both directions; the 20 x 12 and 40 x 6 geometries' own tiles; smaller than a
# block; several tiles per image at batch 3; and 600 tiles of 32 x 8, more than the 512 workgroup slots of 256 CUs, so
# that workgroups walk several items and the resident weights outlive a tile
SHAPES = [(2, 8, 32), (2, 24, 44), (2, 12, 20), (2, 6, 40), (1, 3, 4), (3, 40, 36), (6, 160, 160)]
GEOS = (1, 2, 3)
G32, RESIDENT, BOTH = 2, 3, 4


class _forced:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_conv3x3_form(self.form)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_conv3x3_form(self.old)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs of one shape and, per geometry, the outputs (plain, + shortcut) of today's 32-channel form."""
    B, H, W = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    w = (torch.randn(C, C, 3, 3, generator=g) * (1.0 / (3 * C ** 0.5))).to(dev)
    b = (torch.randn(C, generator=g) * 0.1).to(dev)
    r = torch.randn(B, C, H, W, generator=g).to(dev)
    prep = _hip.conv3x3_prepare(w)
    old = {}
    for geo in GEOS:
        with _forced(geo + 4 * G32):
            old[geo] = (_hip.conv3x3_silu(x, b, lambda: prep, C), _hip.conv3x3_silu(x, b, lambda: prep, C, res=r))
    return x, w, b, r, prep, old


@pytest.mark.parametrize("shape", SHAPES)
def test_new_forms_equal_the_old_form(shape, cuda):
    B, H, W = shape
    x, _, b, r, prep, old = _case(shape)
    lib = _hip.load_library()
    for geo in GEOS:
        for grp in (RESIDENT, BOTH):
            with _forced(geo + 4 * grp):
                assert lib.yolosod_debug_conv3x3_form_ex(B, C, C, H, W) == geo + 4 * grp
                y = _hip.conv3x3_silu(x, b, lambda: prep, C)
                y_res = _hip.conv3x3_silu(x, b, lambda: prep, C, res=r)
            assert torch.equal(y, old[geo][0]), (shape, geo, grp)
            assert torch.equal(y_res, old[geo][1]), (shape, geo, grp)


@pytest.mark.parametrize("shape", SHAPES[:6])
def test_new_forms_on_channel_slices_between_nan(shape, cuda):
    """Input, residual and output are channels 32 .. 63 of images 1 .. B of buffers whose other channels and images
    are NaN: nothing outside the slices is read into the result or written."""
    B, H, W = shape
    x, _, b, r, prep, old = _case(shape)
    nan = float("nan")
    xbuf = torch.full((B + 2, 3 * C, H, W), nan, device=cuda)
    rbuf = torch.full((B + 2, 3 * C, H, W), nan, device=cuda)
    xbuf[1:B + 1, C:2 * C] = x
    rbuf[1:B + 1, C:2 * C] = r
    for geo in GEOS:
        for grp in (RESIDENT, BOTH):
            obuf = torch.full((B + 2, 3 * C, H, W), nan, device=cuda)
            with _forced(geo + 4 * grp):
                _hip.conv3x3_silu(xbuf[1:B + 1, C:2 * C], b, lambda: prep, C, out=obuf[1:B + 1, C:2 * C],
                                  res=rbuf[1:B + 1, C:2 * C])
            y = obuf[1:B + 1, C:2 * C]
            assert torch.isfinite(y).all(), (shape, geo, grp)
            assert torch.equal(y, old[geo][1]), (shape, geo, grp)
            obuf[1:B + 1, C:2 * C] = nan
            assert torch.isnan(obuf).all(), (shape, geo, grp)


def test_new_forms_match_fp64(cuda):
    """The bound of tests/test_gpu_conv3x3.py for this kernel (5e-5 + 1e-4 |ref|, and within 8 x MIOpen's fp32 error)."""
    shape = (2, 24, 44)
    x, w, b, _, prep, _ = _case(shape)
    ref = F.silu(F.conv2d(x.cpu().double(), w.cpu().double(), b.cpu().double(), padding=1))
    err_m = float((F.silu(F.conv2d(x, w, b, padding=1)).cpu().double() - ref).abs().max())
    for grp in (RESIDENT, BOTH):
        with _forced(1 + 4 * grp):
            y = _hip.conv3x3_silu(x, b, lambda: prep, C).cpu().double()
        err = float((y - ref).abs().max())
        print(f"groups {grp}: max abs err {err:.3g} (MIOpen fp32 {err_m:.3g})")
        ok, e, _ = tol_close(y, ref, 5e-5, 1e-4)
        assert ok, (grp, e, err_m)
        assert err <= 8 * err_m + 1e-5, (grp, err, err_m)


def test_new_forms_raise_the_split_range_flag(cuda):
    """1e6 in the last channel of the last image is beyond fp16's range: flagged; the flag stays clear otherwise."""
    x, _, b, _, prep, _ = _case((2, 24, 44))
    big = x.clone()
    big[-1, -1] = 1e6
    for grp in (RESIDENT, BOTH):
        with _forced(1 + 4 * grp):
            _hip.split_range_flag(reset=True)
            _hip.conv3x3_silu(x, b, lambda: prep, C)
            assert not _hip.split_range_flag(reset=True), grp
            _hip.conv3x3_silu(big, b, lambda: prep, C)
            assert _hip.split_range_flag(reset=True), grp


def test_two_input_chunks_keep_an_old_form(cuda):
    """Cin 64 -> Cout 32 has two input chunks (a weight set per chunk: nothing to keep resident): the automatic choice
    and a forced resident-weights form both report - and run - today's 32-channel form."""
    B, H, W = 2, 24, 44
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 64, H, W, generator=g).to(cuda)
    w = (torch.randn(C, 64, 3, 3, generator=g) * (1.0 / 24)).to(cuda)
    b = (torch.randn(C, generator=g) * 0.1).to(cuda)
    prep = _hip.conv3x3_prepare(w)
    lib = _hip.load_library()
    with _forced(0):
        auto = lib.yolosod_debug_conv3x3_form_ex(B, 64, C, H, W)
        assert auto >> 2 == G32 and auto == lib.yolosod_debug_conv3x3_form(B, C, H, W), auto
    with _forced(1 + 4 * G32):
        y0 = _hip.conv3x3_silu(x, b, lambda: prep, C)
    with _forced(1 + 4 * RESIDENT):
        assert lib.yolosod_debug_conv3x3_form_ex(B, 64, C, H, W) == 1 + 4 * G32
        y = _hip.conv3x3_silu(x, b, lambda: prep, C)
    assert torch.equal(y, y0)
