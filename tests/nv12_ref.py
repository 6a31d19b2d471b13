"""Test helper: the CPU restatement of the NV12 front door (``csrc/ingest_nv12.hip``) - the integer colour conversion
in numpy int64 (so it cannot share an overflow with the kernel's int32), followed by ``tests/ingest_ref.py`` on the
converted frames. The product has no CPU path; this file is the definition the kernel is tested against.

Pixel (r, c) of a view with origin parities (py, px) takes Y[r][c] and UV[(r + py) >> 1][(c + px) >> 1]:
    y = max(Y - YOFF, 0) CY;  u = U - 128;  v = V - 128
    R = sat((y + CVR v + 2^19) >> 20);  G = sat((y + CVG v + CUG u + 2^19) >> 20);  B = sat((y + CUB u + 2^19) >> 20)
"""
from __future__ import annotations

import numpy as np

from ingest_ref import ingest_ref

# name -> (YOFF, CY, CVR, CUG, CVG, CUB): the issue's table, written out here on its own
COEF = {
    "bt601": (16, 1220542, 1673527, -409993, -852492, 2116026),
    "bt709": (16, 1220542, 1880097, -223347, -558891, 2214593),
    "bt601_full": (0, 1048576, 1470104, -360710, -748683, 1858077),
    "bt709_full": (0, 1048576, 1651507, -196084, -490734, 1946157),
}


def accumulators(Y, U, V, matrix):
    """The three int64 accumulators (R, G, B) before the shift, for broadcastable integer arrays."""
    yoff, cy, cvr, cug, cvg, cub = COEF[matrix]
    y = np.maximum(np.asarray(Y, dtype=np.int64) - yoff, 0) * cy
    u, v = np.asarray(U, dtype=np.int64) - 128, np.asarray(V, dtype=np.int64) - 128
    return y + cvr * v + (1 << 19), y + cvg * v + cug * u + (1 << 19), y + cub * u + (1 << 19)


def yuv_to_bgr_u8(Y, U, V, matrix):
    """uint8 [..., 3] in B, G, R order."""
    r, g, b = np.broadcast_arrays(*accumulators(Y, U, V, matrix))
    return np.stack([np.clip(a >> 20, 0, 255) for a in (b, g, r)], axis=-1).astype(np.uint8)


def nv12_to_bgr_u8(y, uv, matrix="bt601", py=0, px=0):
    """[h, w, 3] uint8 BGR of the view ``y`` [h, w] whose chroma ``uv`` [.., .., 2] starts at the pair of its first
    pixel; (py, px) are the parities of the view's origin on its surface."""
    y, uv = np.asarray(y), np.asarray(uv)
    h, w = y.shape
    rr, cc = (np.arange(h) + py) >> 1, (np.arange(w) + px) >> 1
    c = uv[rr][:, cc]
    return yuv_to_bgr_u8(y, c[..., 0], c[..., 1], matrix)


def make_nv12(h, w, seed):
    """Seeded (y [h, w], uv [h/2, w/2, 2]) uint8 over the whole byte range."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8)


def frame_to_bgr_u8(f):
    """An ``NV12Frame`` (planes anywhere) converted on the CPU."""
    return nv12_to_bgr_u8(f.y.cpu().numpy(), f.uv.cpu().numpy(), f.matrix, *f.parity)


def ingest_nv12_ref(frames, geoms, pad=114):
    """``ingest_ref`` on the converted frames; ``frames`` are (y, uv, matrix[, py, px]) tuples."""
    return ingest_ref([nv12_to_bgr_u8(*f) for f in frames], geoms, pad)
