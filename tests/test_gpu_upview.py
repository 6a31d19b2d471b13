"""GPU: a nearest 2x Upsample read in place by the 1x1 kernel that consumes its Concat (_hip.CatView(up0=True),
tasks.UPVIEW): both CatView kernels against the materialised upsample + concat, bit for bit, and the model routing."""
import pytest
import torch
import torch.nn.functional as F

from yolosod_amd import _hip

pytestmark = pytest.mark.gpu


def _parts(B, c0, c1, H, W, g, cuda):
    src = torch.randn(B, c0, H // 2, W // 2, generator=g).to(cuda)
    skip = torch.randn(B, c1 + 64, H, W, generator=g).to(cuda)[:, 32:32 + c1]  # a channel slice: its own batch stride
    full = torch.cat([F.interpolate(src, scale_factor=2, mode="nearest"), skip], 1)
    return src, skip, full


@pytest.mark.parametrize("B,c0,c1,H,W", [(2, 64, 64, 16, 24), (2, 64, 64, 32, 48), (1, 32, 64, 16, 24)])
def test_thin_kernel_reads_the_upsample_in_place(B, c0, c1, H, W, cuda):
    g = torch.Generator().manual_seed(c0 + H)
    src, skip, full = _parts(B, c0, c1, H, W, g, cuda)
    cin = c0 + c1
    w = (torch.randn(64, cin, generator=g) * (1.0 / cin ** 0.5)).to(cuda)
    b = (torch.randn(64, generator=g) * 0.1).to(cuda)
    y0 = _hip.conv1x1_thin(full, w, b)
    cv = _hip.CatView([src, skip], up0=True)
    assert tuple(cv.shape) == (B, cin, H, W) and _hip.conv1x1_thin_ok(cv, 64)
    assert torch.equal(cv.materialize(), full)
    assert torch.equal(_hip.conv1x1_thin(cv, w, b), y0)
    buf = torch.zeros((B, 96, H, W), device=cuda)  # out as a concat slice, plus the dual store
    t = torch.empty((B, 32, H, W), device=cuda)
    _hip.conv1x1_thin(cv, w, b, out=buf[:, 16:80], out2=t, c2lo=32)
    assert torch.equal(buf[:, 16:80], y0) and torch.equal(t, y0[:, 32:])
    assert not buf[:, :16].any() and not buf[:, 80:].any()


@pytest.mark.parametrize("B,c0,c1,cout,H,W", [(2, 128, 128, 128, 8, 12), (2, 256, 256, 256, 4, 20)])
def test_wide_kernel_reads_the_upsample_in_place(B, c0, c1, cout, H, W, cuda):
    g = torch.Generator().manual_seed(c0 + cout)
    src, skip, full = _parts(B, c0, c1, H, W, g, cuda)
    cin = c0 + c1
    w = (torch.randn(cout, cin, generator=g) * (1.0 / cin ** 0.5)).to(cuda)
    b = (torch.randn(cout, generator=g) * 0.1).to(cuda)
    prep = _hip.conv1x1x2_prepare(w)
    y0 = _hip.conv1x1x2_silu(full, b, lambda: prep, cout)
    cv = _hip.CatView([src, skip], up0=True)
    assert _hip.conv1x1x2_ok(cv, torch.nn.Conv2d(cin, cout, 1))
    assert torch.equal(_hip.conv1x1x2_silu(cv, b, lambda: prep, cout), y0)
    buf = torch.zeros((B, cout + 64, H, W), device=cuda)  # out as a concat slice, plus the dual store
    t = torch.empty((B, cout // 2, H, W), device=cuda)
    _hip.conv1x1x2_silu(cv, b, lambda: prep, cout, out=buf[:, 32:32 + cout], out2=t, c2lo=cout // 2)
    assert torch.equal(buf[:, 32:32 + cout], y0) and torch.equal(t, y0[:, cout // 2:])
    assert not buf[:, :32].any() and not buf[:, 32 + cout:].any()


def test_catview_checks_the_upsampled_part():
    a, b = torch.zeros(1, 4, 4, 6), torch.zeros(1, 8, 8, 12)
    assert tuple(_hip.CatView([a, b], up0=True).shape) == (1, 12, 8, 12)
    with pytest.raises(ValueError):
        _hip.CatView([a, b])
    with pytest.raises(ValueError):
        _hip.CatView([b, b], up0=True)


@pytest.fixture(scope="module")
def paper_model(cuda):
    from yolosod_amd.nn.tasks import build_model
    return build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=cuda)


@pytest.mark.parametrize("size", [256, 640])
def test_model_upview_bit_identical(size, paper_model, cuda, monkeypatch):
    """tasks.UPVIEW on: no upsample2x launch, the same output bit for bit as with the upsample written out, and as
    with the concat buffers (YOLOSOD_CATVIEW=0, where the switch has nothing to act on)."""
    from yolosod_amd.nn import tasks as T
    m = paper_model
    x = torch.rand(2, 3, size, size, generator=torch.Generator().manual_seed(8)).to(cuda)
    torch.backends.cudnn.deterministic = True
    try:
        with torch.inference_mode():
            monkeypatch.setattr(T, "UPVIEW", True)
            with _hip.op_timer() as t:
                y = m(x)[0]
            keys = [k for k, _ in t.durations_ms()]
            monkeypatch.setattr(T, "UPVIEW", False)
            with _hip.op_timer() as t0:
                y0 = m(x)[0]
            keys0 = [k for k, _ in t0.durations_ms()]
            monkeypatch.setattr(T, "UPVIEW", True)
            monkeypatch.setattr(T, "CATVIEW", False)
            y1 = m(x)[0]
    finally:
        torch.backends.cudnn.deterministic = False
    assert not [k for k in keys if k[0] == "upsample2x"]
    assert len([k for k in keys0 if k[0] == "upsample2x"]) == 3
    assert torch.equal(y, y0), float((y - y0).abs().max())
    assert torch.equal(y, y1), float((y - y1).abs().max())
