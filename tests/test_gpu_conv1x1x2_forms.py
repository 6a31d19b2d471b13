"""GPU: the forms of the fp16-split 1x1 conv kernel (csrc/conv1x1x2.hip) - workgroups of 256 output channels (a wave
owns four 16-channel blocks) and the double-buffered staging, each forced through yolosod_debug_set_conv1x1x2_form.
No form changes the order of an output element's additions, so every form must be torch.equal to the single-buffered
128-channel form (the only one before the forms existed), with every option of the launch: dual store, channel-slice
input and output, a virtual concat and its upsampled first part. The fp64 bound and the split-range flag are those of
tests/test_gpu_conv1x1x2.py and tests/test_gpu_split_range.py."""
import pytest
import torch
import torch.nn.functional as F

from oplib import tol_close
from yolosod_amd import _hip

pytestmark = pytest.mark.gpu

G128, G256, B1, B2 = 1, 2, 4 * 1, 4 * 2
OLD = G128 + B1
NEW = [G256 + B1, G128 + B2, G256 + B2]
# (shape, cout): one tile and one group; three stages and a 16-pixel tail tile; two groups and seven tiles with a
# tail; Cin below one stage (padded channels read 0); HW 16 with eight stages
SHAPES = [((2, 256, 8, 8), 256), ((1, 384, 12, 12), 256), ((2, 768, 20, 20), 512), ((3, 96, 8, 8), 256),
          ((1, 1024, 4, 4), 512)]


class _Form:
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = _hip.load_library().yolosod_debug_set_conv1x1x2_form(self.form)

    def __exit__(self, *exc):
        _hip.load_library().yolosod_debug_set_conv1x1x2_form(self.old)
        return False


def _case(shape, cout, cuda):
    g = torch.Generator().manual_seed(sum(shape) + cout)
    cin = shape[1]
    x = torch.randn(shape, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b


@pytest.mark.parametrize("shape,cout", SHAPES)
def test_forms_bit_identical_with_and_without_dual_store(shape, cout, cuda):
    x, w, b = _case(shape, cout, cuda)
    xd, bd, prep = x.to(cuda), b.to(cuda), _hip.conv1x1x2_prepare(w.to(cuda))
    B, _, H, W = shape
    lib = _hip.load_library()
    with _Form(OLD):
        assert lib.yolosod_debug_conv1x1x2_form(B, cout, H, W) == OLD
        y0 = _hip.conv1x1x2_silu(xd, bd, lambda: prep, cout)
    for form in NEW:
        with _Form(form):
            assert lib.yolosod_debug_conv1x1x2_form(B, cout, H, W) == form
            y = _hip.conv1x1x2_silu(xd, bd, lambda: prep, cout)
            t = torch.full((B, cout // 2, H, W), float("nan"), device=cuda)
            y2 = _hip.conv1x1x2_silu(xd, bd, lambda: prep, cout, out2=t, c2lo=cout // 2)
        assert torch.equal(y, y0), (form, float((y - y0).abs().max()))
        assert torch.equal(y2, y0) and torch.equal(t, y0[:, cout // 2:]), form
    assert lib.yolosod_debug_set_conv1x1x2_form(0) == 0  # every forced form was restored


@pytest.mark.parametrize("shape,cout", [SHAPES[1], SHAPES[2]])
def test_forms_match_fp64(shape, cout, cuda):
    """The bound of tests/test_gpu_conv1x1x2.py::test_conv1x1x2_matches_fp64, for every form."""
    x, w, b = _case(shape, cout, cuda)
    ref = F.silu(F.conv2d(x.double(), w.double(), b.double()))
    wd = w.to(cuda)
    miopen = F.silu(F.conv2d(x.to(cuda), wd, b.to(cuda))).cpu().double()
    err_m = float((miopen - ref).abs().max())
    prep = _hip.conv1x1x2_prepare(wd)
    for form in [OLD] + NEW:
        with _Form(form):
            y = _hip.conv1x1x2_silu(x.to(cuda), b.to(cuda), lambda: prep, cout).cpu().double()
        err = float((y - ref).abs().max())
        ok, e, _ = tol_close(y, ref, 5e-5, 1e-4)
        assert ok, f"form {form} {shape}: max abs err {e:.3g} (MIOpen fp32 {err_m:.3g})"
        assert err <= 8 * err_m + 1e-5, (form, err, err_m)


def test_forms_slices_bit_identical(cuda):
    """Input as a channel slice, output as a channel slice between NaN channels: the forms write the same values and
    nothing else."""
    g = torch.Generator().manual_seed(9)
    xb = torch.randn(2, 320, 12, 20, generator=g).to(cuda)
    x = xb[:, 32:288]  # 256 channels, batch stride 320 * HW
    w = (torch.randn(256, 256, generator=g) * 0.06).to(cuda)
    b = (torch.randn(256, generator=g) * 0.1).to(cuda)
    prep = _hip.conv1x1x2_prepare(w)
    with _Form(OLD):
        y0 = _hip.conv1x1x2_silu(x.contiguous(), b, lambda: prep, 256)
    for form in NEW:
        z = torch.full((2, 512, 12, 20), float("nan"), device=cuda)
        t = torch.full((2, 128, 12, 20), float("nan"), device=cuda)
        with _Form(form):
            _hip.conv1x1x2_silu(x, b, lambda: prep, 256, out=z[:, 128:384], out2=t, c2lo=128)
        assert torch.equal(z[:, 128:384], y0) and torch.equal(t, y0[:, 128:]), form
        assert torch.isnan(z[:, :128]).all() and torch.isnan(z[:, 384:]).all(), form


@pytest.mark.parametrize("shape,k1,cout", [((2, 384, 12, 20), 128, 256), ((1, 768, 20, 20), 256, 512)])
def test_forms_virtual_concat_bit_identical(shape, k1, cout, cuda):
    """A CatView split at k1 (the second part a channel slice), as it is and with its first part the quarter-size
    source of a nearest 2x upsample, against the materialised concat in the old form."""
    g = torch.Generator().manual_seed(k1 + cout)
    B, cin, H, W = shape
    a = torch.randn(B, k1, H, W, generator=g).to(cuda)
    a4 = torch.randn(B, k1, H // 2, W // 2, generator=g).to(cuda)
    bb = torch.randn(B, cin - k1 + 64, H, W, generator=g).to(cuda)[:, 32:32 + cin - k1]
    w = (torch.randn(cout, cin, generator=g) * (1.0 / cin ** 0.5)).to(cuda)
    b = (torch.randn(cout, generator=g) * 0.1).to(cuda)
    prep = _hip.conv1x1x2_prepare(w)
    cv, cvu = _hip.CatView([a, bb]), _hip.CatView([a4, bb], up0=True)
    with _Form(OLD):
        y0 = _hip.conv1x1x2_silu(cv.materialize(), b, lambda: prep, cout)
        yu0 = _hip.conv1x1x2_silu(cvu.materialize(), b, lambda: prep, cout)
    for form in NEW:
        with _Form(form):
            t = torch.empty((B, cout // 2, H, W), device=cuda)
            y = _hip.conv1x1x2_silu(cv, b, lambda: prep, cout, out2=t, c2lo=cout // 2)
            yu = _hip.conv1x1x2_silu(cvu, b, lambda: prep, cout)
        assert torch.equal(y, y0) and torch.equal(t, y0[:, cout // 2:]), form
        assert torch.equal(yu, yu0), form


def test_forms_split_range_flag(cuda):
    """An input of 1e6 (beyond fp16) sets the split-range flag in every form; an ordinary input leaves it clear."""
    x, w, b = _case((2, 256, 8, 8), 256, cuda)
    xd, bd, prep = x.to(cuda), b.to(cuda), _hip.conv1x1x2_prepare(w.to(cuda))
    big = xd.clone()
    big[1, 200, 5, 3] = 1e6
    for form in [OLD] + NEW:
        with _Form(form):
            _hip.split_range_flag(reset=True)
            _hip.conv1x1x2_silu(xd, bd, lambda: prep, 256)
            assert not _hip.split_range_flag(reset=True), form
            _hip.conv1x1x2_silu(big, bd, lambda: prep, 256)
            assert _hip.split_range_flag(reset=True), form


def test_automatic_form(cuda):
    """Nothing forced: 256-channel groups for Cout 512 on maps up to 20 x 20 when the 128-channel items exceed the
    workgroup slots (the bench step's three shapes at batch 32), the old form everywhere else."""
    lib = _hip.load_library()
    assert lib.yolosod_debug_set_conv1x1x2_form(0) == 0
    assert lib.yolosod_debug_conv1x1x2_form(32, 512, 20, 20) == G256 + B1
    for B, cout, side in [(2, 512, 20), (32, 256, 20), (32, 512, 40), (32, 256, 40), (32, 128, 80), (32, 1024, 20)]:
        assert lib.yolosod_debug_conv1x1x2_form(B, cout, side, side) == OLD, (B, cout, side)


def test_256_form_forced_on_cout_128_runs_the_old_form(cuda):
    x, w, b = _case((2, 256, 12, 12), 128, cuda)
    xd, bd, prep = x.to(cuda), b.to(cuda), _hip.conv1x1x2_prepare(w.to(cuda))
    lib = _hip.load_library()
    with _Form(OLD):
        y0 = _hip.conv1x1x2_silu(xd, bd, lambda: prep, 128)
    with _Form(G256 + B1):
        assert lib.yolosod_debug_conv1x1x2_form(2, 128, 12, 12) == OLD
        assert lib.yolosod_debug_conv1x1x2_form(2, 384, 12, 12) == OLD      # Cout % 256 != 0
        assert lib.yolosod_debug_conv1x1x2_form(2, 64, 12, 12) == OLD       # the 64-channel group has one form
        assert lib.yolosod_debug_conv1x1x2_form(2, 256, 12, 12) == G256 + B1
        y = _hip.conv1x1x2_silu(xd, bd, lambda: prep, 128)
    with _Form(G256 + B2):
        assert lib.yolosod_debug_conv1x1x2_form(2, 128, 12, 12) == G128 + B2  # the buffers field still applies
        y2 = _hip.conv1x1x2_silu(xd, bd, lambda: prep, 128)
    assert torch.equal(y, y0) and torch.equal(y2, y0)
    assert lib.yolosod_debug_conv1x1x2_form(2, 100, 12, 12) == 0 and lib.yolosod_debug_conv1x1x2_form(2, 128, 3, 3) == 0
    old = lib.yolosod_debug_set_conv1x1x2_form(3)  # not a form: ignored
    assert old == 0 and lib.yolosod_debug_set_conv1x1x2_form(0) == 0
