"""CPU: the NV12 front door without a GPU - the coefficient table against its rounding rule, the int32 head-room and
the colour accuracy of the integer conversion over all 2^24 (Y, U, V) triples (tests/nv12_ref.py), NV12Frame (views,
crops, parities), the C entry point's host-side argument checks, and what the wrapper and frames_to_device refuse."""
import ctypes
from decimal import ROUND_HALF_UP, Decimal

import numpy as np
import pytest
import torch

from nv12_ref import COEF, accumulators, make_nv12, nv12_to_bgr_u8, yuv_to_bgr_u8
from yolosod_amd import _hip
from yolosod_amd.data import NV12Frame
from yolosod_amd.data.nv12 import NV12_COEF, NV12_CONSTANTS, NV12_MATRICES

MATRICES = ("bt601", "bt709", "bt601_full", "bt709_full")


def _triples(y_lo, y_hi):
    """(Y, U, V) broadcastable over [y_hi - y_lo, 256, 256]."""
    return (np.arange(y_lo, y_hi, dtype=np.int64)[:, None, None], np.arange(256, dtype=np.int64)[None, :, None],
            np.arange(256, dtype=np.int64)[None, None, :])


def test_the_coefficient_table_is_the_rounding_rule_on_the_textbook_constants():
    assert NV12_MATRICES == MATRICES and tuple(NV12_COEF) == MATRICES
    for name in MATRICES:
        yoff, *consts = NV12_CONSTANTS[name]
        want = [yoff]
        for c in consts:
            d = Decimal(str(c))
            assert -d.as_tuple().exponent <= 3, (name, c)  # three decimals
            mag = (abs(d) * (1 << 20)).quantize(Decimal(1), rounding=ROUND_HALF_UP)  # half away from zero
            want.append(int(mag) if d >= 0 else -int(mag))
        assert tuple(want) == NV12_COEF[name] == COEF[name], name


@pytest.mark.parametrize("matrix", MATRICES)
def test_accumulators_stay_inside_int32_on_all_triples(matrix):
    worst = 0
    for lo in range(0, 256, 32):
        for a in accumulators(*_triples(lo, lo + 32), matrix):
            worst = max(worst, int(np.abs(a).max()), int(np.abs(a - (1 << 19)).max()))
    print(f"{matrix}: largest accumulator magnitude {worst}")
    assert worst < 2 ** 31
    assert worst <= 573_487_137


def test_bt601_full_is_within_one_grey_level_of_pil_on_all_triples():
    Image = pytest.importorskip("PIL.Image", reason="PIL is not installed")
    Y, U, V = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8),
                          np.arange(256, dtype=np.uint8), indexing="ij")
    ycc = np.stack([Y, U, V], -1).reshape(4096, 4096, 3)
    rgb = np.asarray(Image.fromarray(ycc, mode="YCbCr").convert("RGB")).astype(np.int16)
    got = yuv_to_bgr_u8(ycc[..., 0], ycc[..., 1], ycc[..., 2], "bt601_full")[..., ::-1].astype(np.int16)
    d = np.abs(got - rgb)
    print(f"bt601_full vs PIL: max {int(d.max())}, share differing by 1: {float((d == 1).mean()):.3f}")
    assert int(d.max()) <= 1


def test_bt601_is_within_one_grey_level_of_the_float_formula_on_all_triples():
    yoff, cy, cvr, cug, cvg, cub = NV12_CONSTANTS["bt601"]
    worst = 0
    for lo in range(0, 256, 32):
        Y, U, V = _triples(lo, lo + 32)
        y = cy * np.maximum(Y - yoff, 0).astype(np.float64)
        u, v = (U - 128).astype(np.float64), (V - 128).astype(np.float64)
        chans = np.broadcast_arrays(y + cub * u, y + cvg * v + cug * u, y + cvr * v)  # B, G, R
        want = np.stack([np.clip(np.rint(a), 0, 255) for a in chans], -1)
        got = yuv_to_bgr_u8(Y, U, V, "bt601").astype(np.float64)
        worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1, worst


# ---- NV12Frame ---------------------------------------------------------------------------------------------------
def test_from_packed_makes_the_two_views():
    y, uv = make_nv12(6, 8, 1)
    buf = np.concatenate([y, uv.reshape(3, 8)])
    for b in (buf, torch.from_numpy(buf.copy())):
        f = NV12Frame.from_packed(b, matrix="bt709")
        assert f.shape == (6, 8) and f.matrix == "bt709" and f.parity == (0, 0)
        assert np.array_equal(f.y.numpy(), y) and np.array_equal(f.uv.numpy(), uv)
        assert f.uv.stride() == (8, 2, 1) and f.y.stride() == (8, 1)
    t = torch.from_numpy(buf.copy())
    f = NV12Frame.from_packed(t)
    assert f.y.data_ptr() == t.data_ptr() and f.uv.data_ptr() == t.data_ptr() + 48  # views, no copy
    # a pitched packed buffer: 8 columns of a 12-wide allocation
    wide = torch.zeros(9, 12, dtype=torch.uint8)
    wide[:, :8] = torch.from_numpy(buf)
    f = NV12Frame.from_packed(wide[:, :8])
    assert f.uv.stride() == (12, 2, 1) and np.array_equal(f.uv.numpy(), uv) and np.array_equal(f.y.numpy(), y)
    with pytest.raises(ValueError):
        NV12Frame.from_packed(np.zeros((8, 8), dtype=np.uint8))  # 8 is no 3h/2


def test_constructor_refusals():
    y, uv = make_nv12(6, 8, 2)
    assert NV12Frame(y, uv).matrix == "bt601"
    with pytest.raises(ValueError, match="even"):
        NV12Frame(y[:5], uv)
    with pytest.raises(ValueError, match="even"):
        NV12Frame(y[:, :7], uv)
    with pytest.raises(ValueError, match="uv must be"):
        NV12Frame(y, uv[:2])
    with pytest.raises(ValueError, match="uv must be"):
        NV12Frame(y, uv.reshape(3, 8))
    with pytest.raises(TypeError, match="uint8"):
        NV12Frame(y.astype(np.int16), uv)
    with pytest.raises(TypeError, match="uint8"):
        NV12Frame(torch.from_numpy(y), torch.from_numpy(uv).float())
    with pytest.raises(ValueError, match="matrix"):
        NV12Frame(y, uv, matrix="bt2020")
    f = NV12Frame(y, uv)
    for rect in [(0, 0, 0, 4), (2, 2, 2, 4), (0, 0, 7, 4), (-1, 0, 3, 3), (0, 5, 3, 9)]:
        with pytest.raises(ValueError, match="crop"):
            f.crop(*rect)


@pytest.mark.parametrize("matrix", ["bt601", "bt709_full"])
def test_crop_then_convert_is_convert_then_slice(matrix):
    """All four origin parities, even and odd extents, down to one pixel, and up to the surface's last row / column."""
    y, uv = make_nv12(12, 16, 3)
    f = NV12Frame(y, uv, matrix)
    full = nv12_to_bgr_u8(y, uv, matrix)
    seen = set()
    for y0, x0, y1, x1 in [(0, 0, 12, 16), (2, 4, 8, 10), (1, 4, 8, 9), (2, 3, 7, 16), (3, 5, 12, 16), (5, 7, 6, 8),
                           (11, 15, 12, 16), (1, 1, 2, 2), (4, 1, 5, 16), (3, 6, 12, 7)]:
        v = f.crop(y0, x0, y1, x1)
        assert v.shape == (y1 - y0, x1 - x0) and v.parity == (y0 & 1, x0 & 1) and v.matrix == matrix
        assert v.y.data_ptr() == f.y.data_ptr() + y0 * 16 + x0, "y is no view"
        assert v.uv.data_ptr() == f.uv.data_ptr() + (y0 >> 1) * 16 + 2 * (x0 >> 1), "uv does not start at the pair"
        got = nv12_to_bgr_u8(v.y.numpy(), v.uv.numpy(), matrix, *v.parity)
        assert np.array_equal(got, full[y0:y1, x0:x1]), (y0, x0, y1, x1)
        seen.add(v.parity)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_crops_compose():
    y, uv = make_nv12(20, 24, 4)
    f = NV12Frame(y, uv)
    full = nv12_to_bgr_u8(y, uv)
    for (a, b) in [((3, 5, 19, 23), (2, 2, 9, 11)), ((1, 1, 20, 24), (1, 1, 18, 22)), ((2, 3, 15, 20), (1, 0, 2, 17)),
                   ((5, 4, 16, 21), (0, 1, 11, 2))]:
        v = f.crop(*a).crop(*b)
        y0, x0 = a[0] + b[0], a[1] + b[1]
        w = f.crop(y0, x0, a[0] + b[2], a[1] + b[3])
        assert v.parity == w.parity == (y0 & 1, x0 & 1) and v.shape == w.shape
        assert v.y.data_ptr() == w.y.data_ptr() and v.uv.data_ptr() == w.uv.data_ptr()
        assert tuple(v.uv.shape) == tuple(w.uv.shape)
        got = nv12_to_bgr_u8(v.y.numpy(), v.uv.numpy(), "bt601", *v.parity)
        assert np.array_equal(got, full[y0:a[0] + b[2], x0:a[1] + b[3]])


# ---- entry point, wrapper, frames_to_device ------------------------------------------------------------------------
def test_abi_exports_and_validates_the_nv12_entry_point():
    lib = _hip.load_library()
    fn = lib.yolosod_letterbox_ingest_nv12
    assert "yolosod_letterbox_ingest_nv12" in _hip.SIGNATURES
    assert _hip.SIGNATURES["yolosod_letterbox_ingest_nv12"] == _hip.SIGNATURES["yolosod_letterbox_ingest"]
    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its host checks first
    n = 3 * 64 * 96

    def err(rc):
        assert rc != 0
        return lib.yolosod_last_error()

    assert b"null" in err(fn(None, 1, None, n, 64, 96, 0, 114, None))
    assert b"null" in err(fn(p, 1, None, n, 64, 96, 0, 114, None))
    assert b"B=0" in err(fn(p, 0, p, n, 64, 96, 0, 114, None))
    assert b"B=65536" in err(fn(p, 65536, p, n, 64, 96, 0, 114, None))
    assert b"out_w" in err(fn(p, 1, p, 3 * 64 * 30, 64, 30, 0, 114, None))
    assert b"canvas" in err(fn(p, 1, p, 3 * 64 * 16388, 64, 16388, 0, 114, None))
    assert b"canvas" in err(fn(p, 1, p, 3 * 16385 * 96, 16385, 96, 0, 114, None))
    assert b"batch stride" in err(fn(p, 2, p, n + 2, 64, 96, 0, 114, None))
    assert b"batch stride" in err(fn(p, 2, p, n - 4, 64, 96, 0, 114, None))
    assert b"aligned" in err(fn(p, 1, ctypes.c_void_p(264), n, 64, 96, 0, 114, None))
    assert b"out_bf16" in err(fn(p, 1, p, n, 64, 96, 2, 114, None))
    assert b"pad_value" in err(fn(p, 1, p, n, 64, 96, 0, 256, None))
    assert b"pad_value" in err(fn(p, 1, p, n, 64, 96, 0, -1, None))
    for m in (lib.yolosod_last_error(),):
        assert m.startswith(b"letterbox_ingest_nv12")
    assert lib.yolosod_abi_version() == 1


def test_wrapper_refuses_cpu_frames_and_other_items():
    y, uv = make_nv12(8, 8, 5)
    g = [(64, 64, 0, 16, 64, 96)]
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.letterbox_ingest_nv12([NV12Frame(y, uv)], (64, 96), g)
    with pytest.raises(TypeError, match="NV12Frame"):
        _hip.letterbox_ingest_nv12([torch.zeros(8, 8, 3, dtype=torch.uint8)], (64, 96), g)
    with pytest.raises(RuntimeError, match="canvas"):
        _hip.letterbox_ingest_nv12([NV12Frame(y, uv)], (64, 30), [(30, 30, 17, 0, 64, 30)])
    with pytest.raises(RuntimeError, match="geometries"):
        _hip.letterbox_ingest_nv12([NV12Frame(y, uv)], (64, 96), g * 2)
    # strides the kernel does not take: a y with element stride 2, a uv with pixel stride 4
    y2 = torch.zeros(8, 16, dtype=torch.uint8)[:, ::2]
    with pytest.raises(RuntimeError, match="element stride"):
        _hip.letterbox_ingest_nv12([NV12Frame(y2, uv)], (64, 96), g)
    uv2 = torch.zeros(4, 8, 2, dtype=torch.uint8)[:, ::2]
    with pytest.raises(RuntimeError, match="pixel stride"):
        _hip.letterbox_ingest_nv12([NV12Frame(y, uv2)], (64, 96), g)
    uv3 = torch.zeros(4, 2, 4, dtype=torch.uint8).permute(0, 2, 1)[:, :, :2]
    with pytest.raises(RuntimeError, match="channel stride"):
        _hip.letterbox_ingest_nv12([NV12Frame(y, uv3)], (64, 96), g)


def test_frames_to_device_refuses_a_list_that_mixes_bgr_and_nv12():
    from yolosod_amd.engine.predictor import frames_to_device
    y, uv = make_nv12(8, 8, 6)
    bgr = np.zeros((8, 8, 3), dtype=np.uint8)
    for frames in ([NV12Frame(y, uv), bgr], [bgr, NV12Frame(y, uv)]):
        with pytest.raises(TypeError, match="mixes BGR arrays and NV12Frame"):
            frames_to_device(frames, "cpu")


def test_frames_to_device_packs_planes_and_leaves_bgr_lists_as_they_were(monkeypatch):
    """Without a GPU the pinned staging buffer is an ordinary one: the packing, the slots and the views are the same."""
    from yolosod_amd.engine.predictor import frames_to_device
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **k: self)
    rng = np.random.default_rng(7)
    bgr = [rng.integers(0, 256, s, dtype=np.uint8) for s in [(5, 7, 3), (8, 8, 3), (3, 2, 3)]]
    ts = frames_to_device([bgr[0], torch.from_numpy(bgr[1]), bgr[2][::-1]], "cpu")
    assert [t.dtype for t in ts] == [torch.uint8] * 3
    for t, want in zip(ts, [bgr[0], bgr[1], bgr[2][::-1]]):
        assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), want) and t.is_contiguous()
    base = ts[0].data_ptr()
    assert [t.data_ptr() - base for t in ts] == [0, 112, 112 + 192], "16-byte aligned slots of one buffer"
    with pytest.raises(RuntimeError, match=r"\[h, w, 3\]"):
        frames_to_device([np.zeros((4, 4), dtype=np.uint8)], "cpu")
    # NV12: both planes of every frame in one buffer, crops keep their parity, the matrix travels
    y, uv = make_nv12(10, 12, 8)
    a = NV12Frame(y, uv, "bt709")
    b = NV12Frame(*make_nv12(4, 6, 9)).crop(1, 1, 4, 6)
    out = frames_to_device([a, b], "cpu")
    assert all(isinstance(f, NV12Frame) for f in out)
    assert out[0].matrix == "bt709" and out[1].parity == (1, 1) and out[1].shape == (3, 5)
    for f, src in zip(out, (a, b)):
        assert torch.equal(f.y, src.y) and torch.equal(f.uv, src.uv)
        assert f.y.data_ptr() % 16 == out[0].y.data_ptr() % 16 and f.uv.data_ptr() % 16 == out[0].y.data_ptr() % 16
    assert out[0].uv.data_ptr() - out[0].y.data_ptr() == 128  # 120 bytes of Y in a 16-byte slot
