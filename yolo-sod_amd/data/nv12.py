"""NV12 frames: what a hardware video decoder writes (a full-resolution Y plane, then a half-resolution plane of
interleaved U, V pairs, each with a row pitch that may exceed the picture). :class:`NV12Frame` holds the two planes as
views, remembers which colour matrix the stream uses, and crops without copying; ``_hip.letterbox_ingest_nv12``
(``csrc/ingest_nv12.hip``) takes a list of them straight to the model's input tensor. There is no host conversion.

The conversion is defined in integers (one result on every machine). Pixel (r, c) takes ``Y[r][c]`` and the pair
``UV[r >> 1][c >> 1]`` (replicated over its 2 x 2 block, no chroma interpolation) and, in int32 arithmetic with an
arithmetic right shift and saturation to [0, 255]::

    y = max(Y - YOFF, 0) * CY;  u = U - 128;  v = V - 128
    R = sat((y + CVR v + 2^19) >> 20);  G = sat((y + CVG v + CUG u + 2^19) >> 20);  B = sat((y + CUB u + 2^19) >> 20)

:data:`NV12_COEF` is the table of the four matrices: each coefficient is the three-decimal textbook constant
(:data:`NV12_CONSTANTS`) times 2^20, rounded half away from zero. ``bt601`` are OpenCV's BT.601 constants."""
from __future__ import annotations

import torch

# name -> (YOFF, luma gain, V -> R, U -> G, V -> G, U -> B) as the textbooks print them
NV12_CONSTANTS = {
    "bt601": (16, 1.164, 1.596, -0.391, -0.813, 2.018),
    "bt709": (16, 1.164, 1.793, -0.213, -0.533, 2.112),
    "bt601_full": (0, 1.0, 1.402, -0.344, -0.714, 1.772),
    "bt709_full": (0, 1.0, 1.575, -0.187, -0.468, 1.856),
}
# name -> (YOFF, CY, CVR, CUG, CVG, CUB); the kernel's constant table holds the same rows in this order
NV12_COEF = {
    "bt601": (16, 1220542, 1673527, -409993, -852492, 2116026),
    "bt709": (16, 1220542, 1880097, -223347, -558891, 2214593),
    "bt601_full": (0, 1048576, 1470104, -360710, -748683, 1858077),
    "bt709_full": (0, 1048576, 1651507, -196084, -490734, 1946157),
}
NV12_MATRICES = tuple(NV12_COEF)  # the matrix id the kernel reads is the index here


def _plane(a, name):
    if not isinstance(a, torch.Tensor):
        import numpy as np
        a = np.asarray(a)
        if a.dtype != np.uint8:
            raise TypeError(f"NV12Frame: {name} must be uint8, got {a.dtype}")
        if any(s < 0 for s in a.strides):
            a = np.ascontiguousarray(a)
        a = torch.from_numpy(a)
    if a.dtype != torch.uint8:
        raise TypeError(f"NV12Frame: {name} must be uint8, got {a.dtype}")
    return a


class NV12Frame:
    """One NV12 frame, or a rectangular view of one.

    ``NV12Frame(y, uv, matrix="bt601")``: ``y`` uint8 [h, w] and ``uv`` uint8 [h/2, w/2, 2] (U at channel 0, V at
    channel 1), numpy arrays or torch tensors, on the CPU or on the GPU; h and w even. The planes are kept as views:
    element stride 1 in ``y``, pixel stride 2 and channel stride 1 in ``uv``, any row pitch (``_hip`` checks the
    strides when the frame is ingested). ``matrix`` names a row of :data:`NV12_COEF`.

    ``shape`` is ``(h, w)``. :meth:`crop` gives a view frame of any extents >= 1 at any origin: its ``y`` is the
    slice, its ``uv`` starts at the chroma pair of the first pixel, and ``parity`` = (y0 & 1, x0 & 1) on the surface
    says whether that pair's first row / column lies outside the view. Crops compose."""

    __slots__ = ("y", "uv", "matrix", "parity")

    def __init__(self, y, uv, matrix="bt601"):
        y, uv = _plane(y, "y"), _plane(uv, "uv")
        if y.dim() != 2:
            raise ValueError(f"NV12Frame: y must be [h, w], got {tuple(y.shape)}")
        h, w = int(y.shape[0]), int(y.shape[1])
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"NV12Frame: h and w must be even and >= 2, got {h}x{w}")
        if tuple(uv.shape) != (h // 2, w // 2, 2):
            raise ValueError(f"NV12Frame: uv must be [{h // 2}, {w // 2}, 2] for a {h}x{w} frame, got "
                             f"{tuple(uv.shape)}")
        if matrix not in NV12_COEF:
            raise ValueError(f"NV12Frame: unknown matrix {matrix!r} (one of {', '.join(NV12_MATRICES)})")
        self.y, self.uv, self.matrix, self.parity = y, uv, matrix, (0, 0)

    @classmethod
    def _view(cls, y, uv, matrix, parity):
        f = object.__new__(cls)
        f.y, f.uv, f.matrix, f.parity = y, uv, matrix, parity
        return f

    @classmethod
    def from_packed(cls, buf, matrix="bt601"):
        """The usual contiguous layout: ``buf`` uint8 [3h/2, w], h rows of Y, then h/2 rows of w/2 U, V pairs."""
        buf = _plane(buf, "buf")
        if buf.dim() != 2 or buf.shape[0] % 3 or buf.shape[1] % 2 or buf.shape[0] < 3:
            raise ValueError(f"NV12Frame.from_packed: expected [3h/2, w] with even h and w, got {tuple(buf.shape)}")
        if buf.shape[1] > 1 and buf.stride(1) != 1:
            raise ValueError(f"NV12Frame.from_packed: element stride {buf.stride(1)} (1 expected)")
        h, w = int(buf.shape[0]) // 3 * 2, int(buf.shape[1])
        uv = buf[h:].as_strided((h // 2, w // 2, 2), (buf.stride(0), 2, 1), buf[h:].storage_offset())
        return cls(buf[:h], uv, matrix)

    @property
    def shape(self):
        return (int(self.y.shape[0]), int(self.y.shape[1]))

    @property
    def device(self):
        return self.y.device

    def crop(self, y0, x0, y1, x1):
        """The view [y0, y1) x [x0, x1) of this frame (or view) as a frame; extents >= 1, inside the frame."""
        h, w = self.shape
        y0, x0, y1, x1 = int(y0), int(x0), int(y1), int(x1)
        if not (0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w):
            raise ValueError(f"NV12Frame.crop: ({y0}, {x0}, {y1}, {x1}) is no rectangle inside {h}x{w}")
        py, px = self.parity
        uv = self.uv[(y0 + py) >> 1:((y1 - 1 + py) >> 1) + 1, (x0 + px) >> 1:((x1 - 1 + px) >> 1) + 1]
        return NV12Frame._view(self.y[y0:y1, x0:x1], uv, self.matrix, ((y0 + py) & 1, (x0 + px) & 1))

    def to(self, device, non_blocking=False):
        """The frame with both planes on ``device`` (itself if they are there already)."""
        device = torch.device(device)
        if self.y.device == device and self.uv.device == device:
            return self
        return NV12Frame._view(self.y.to(device, non_blocking=non_blocking),
                               self.uv.to(device, non_blocking=non_blocking), self.matrix, self.parity)

    def __repr__(self):
        h, w = self.shape
        return f"NV12Frame({h}x{w}, {self.matrix}, parity={self.parity}, device={self.y.device})"
