"""CPU: the raw-frame front door without a GPU - LetterBox geometry (yolo-sod_amd/data/augment.py) on hand-checked
cases and against scale_boxes' own gain / pad, the integer bilinear definition (tests/ingest_ref.py) against exact
bilinear interpolation, and the two C-ABI entry points' host-side argument checks."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ingest_ref import resize_u8
from yolosod_amd import _hip
from yolosod_amd.data.augment import LetterBox
from yolosod_amd.utils.ops import scale_boxes

# (frame (h, w), LetterBox kwargs)
GEOM_CASES = [
    ((1080, 1920), dict(new_shape=(640, 640), auto=True)),
    ((1080, 1920), dict(new_shape=(640, 640), auto=False)),
    ((60, 100), dict(new_shape=(128, 128), auto=True)),
    ((40, 50), dict(new_shape=(128, 128), scaleup=False)),
    ((100, 60), dict(new_shape=(128, 128))),
    ((100, 60), dict(new_shape=(128, 128), auto=True)),
    ((60, 100), dict(new_shape=(128, 128), center=False)),
    ((765, 1360), dict(new_shape=(640, 640))),
    ((1500, 2000), dict(new_shape=(640, 640), auto=True)),
]


def test_letterbox_geometry_hand_checked():
    g = LetterBox((640, 640), auto=True).geometry((1080, 1920))
    assert g == (360, 640, 12, 0, 384, 640)
    g = LetterBox((640, 640), auto=False).geometry((1080, 1920))
    assert g == (360, 640, 140, 0, 640, 640)
    nh, nw, top, left, oh, ow = LetterBox((128, 128), auto=True).geometry((60, 100))
    assert (nh, nw, top, left, oh, ow) == (77, 128, 9, 0, 96, 128) and oh - nh - top == 10
    # scaleup=False: a small frame is not enlarged
    nh, nw, top, left, oh, ow = LetterBox((128, 128), scaleup=False).geometry((40, 50))
    assert (nh, nw) == (40, 50) and (top, left, oh, ow) == (44, 39, 128, 128)
    # portrait: the padding lands left / right
    nh, nw, top, left, oh, ow = LetterBox((128, 128)).geometry((100, 60))
    assert (nh, nw, top) == (128, 77, 0) and left == 25 and ow - nw - left == 26 and (oh, ow) == (128, 128)
    # center=False: the frame sits in the top-left corner
    nh, nw, top, left, oh, ow = LetterBox((128, 128), center=False).geometry((60, 100))
    assert (top, left) == (0, 0) and (nh, nw, oh, ow) == (77, 128, 128, 128)
    assert LetterBox(640).new_shape == (640, 640)
    with pytest.raises(NotImplementedError):
        LetterBox((640, 640), scaleFill=True)


@pytest.mark.parametrize("shape,kw", [c for c in GEOM_CASES if c[1].get("center", True) and c[1].get("scaleup", True)])
def test_letterbox_agrees_with_scale_boxes(shape, kw):
    """scale_boxes recomputes gain and pad from the two shapes (ratio_pad=None); with them the canvas corners of the
    resized region map to within 1 px of the frame's corners. That recomputation assumes a centred, scaled-up
    letterbox (the predictor's): with scaleup=False on a small frame or center=False the reference itself needs an
    explicit ratio_pad, so those two geometry cases are not part of this check."""
    nh, nw, top, left, oh, ow = LetterBox(**kw).geometry(shape)
    corners = torch.tensor([[left, top, left + nw, top + nh]], dtype=torch.float32)
    # clip_boxes would hide an overshoot: the unclipped arithmetic, then the clipped call
    gain = min(oh / shape[0], ow / shape[1])
    pad = (round((ow - shape[1] * gain) / 2 - 0.1), round((oh - shape[0] * gain) / 2 - 0.1))
    raw = (corners - torch.tensor([pad[0], pad[1], pad[0], pad[1]], dtype=torch.float32)) / gain
    want = torch.tensor([[0.0, 0.0, shape[1], shape[0]]])
    assert float((raw - want).abs().max()) <= 1.0, (raw, want)
    got = scale_boxes((oh, ow), corners.clone(), shape)
    assert float((got - want).abs().max()) <= 1.0, (got, want)


@pytest.mark.parametrize("src,dst", [((37, 53), (23, 33)), ((9, 7), (20, 16)), ((13, 29), (40, 88)), ((2, 3), (7, 5)),
                                     ((1, 1), (4, 4))])
def test_integer_bilinear_is_within_its_bound_of_exact_bilinear(src, dst):
    """0.5 (the final rounding) + 2 * 255 * 2^-12 (two 11-bit coefficients, each off by at most 2^-12 of a 255 range)
    = 0.625 grey levels from bilinear interpolation in float64 (half-pixel centres, edge replicate, no antialias)."""
    img = np.random.default_rng(src[0] * 100 + src[1]).integers(0, 256, (*src, 3), dtype=np.uint8)
    got = resize_u8(img, *dst).astype(np.float64)
    x = torch.from_numpy(img).permute(2, 0, 1)[None].double()
    ref = F.interpolate(x, size=dst, mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    err = float(np.abs(got - ref).max())
    print(f"{src}->{dst}: max |integer - exact| = {err:.4f} grey levels")
    assert err <= 0.625, err


def test_integer_bilinear_is_the_identity_at_equal_size():
    img = np.random.default_rng(3).integers(0, 256, (17, 23, 3), dtype=np.uint8)
    assert np.array_equal(resize_u8(img, 17, 23), img)


def test_abi_exports_and_validates_the_ingest_entry_points():
    lib = _hip.load_library()
    for n in ("yolosod_letterbox_ingest", "yolosod_scale_boxes"):
        assert hasattr(lib, n) and n in _hip.SIGNATURES
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its host checks first
    rc = lib.yolosod_letterbox_ingest(None, 1, None, 3 * 64 * 96, 64, 96, 0, 114, None)
    assert rc != 0 and b"null" in lib.yolosod_last_error()
    rc = lib.yolosod_letterbox_ingest(p, 1, p, 3 * 64 * 30, 64, 30, 0, 114, None)
    assert rc != 0 and b"out_w" in lib.yolosod_last_error()
    rc = lib.yolosod_letterbox_ingest(p, 0, p, 3 * 64 * 96, 64, 96, 0, 114, None)
    assert rc != 0 and b"B=0" in lib.yolosod_last_error()
    rc = lib.yolosod_scale_boxes(None, None, 1, 8, None, None)
    assert rc != 0 and b"null" in lib.yolosod_last_error()
    rc = lib.yolosod_scale_boxes(p, p, 1, 0, p, None)
    assert rc != 0 and b"D=0" in lib.yolosod_last_error()
    rc = lib.yolosod_scale_boxes(p, p, 0, 8, p, None)
    assert rc != 0 and b"B=0" in lib.yolosod_last_error()


def test_wrapper_refuses_cpu_frames():
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.letterbox_ingest([torch.zeros(8, 8, 3, dtype=torch.uint8)], (64, 96), [(64, 64, 0, 16, 64, 96)])
