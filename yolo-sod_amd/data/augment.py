"""Letterbox geometry (``ultralytics/data/augment.py`` ``LetterBox`` of Ultralytics 8.3.63, the transform the
reference predictor's ``pre_transform`` applies, ``engine/predictor.py:145-161``).

Only the geometry lives here, as host arithmetic on shapes: the pixels are resized, padded, flipped to RGB and scaled
by one HIP launch (``_hip.letterbox_ingest``, ``csrc/ingest.hip``). There is no host resize."""
from __future__ import annotations


class LetterBox:
    """Resize keeping the aspect ratio, pad to ``new_shape`` (or, ``auto``, to the smallest rectangle whose sides are
    multiples of ``stride``) with border value 114.

    ``geometry((h, w))`` -> ``(new_h, new_w, top, left, out_h, out_w)``: the frame is resized to ``new_h x new_w`` and
    sits at ``(top, left)`` of an ``out_h x out_w`` canvas."""

    pad_value = 114

    def __init__(self, new_shape=(640, 640), auto=False, scaleFill=False, scaleup=True, center=True, stride=32):
        if scaleFill:
            raise NotImplementedError("LetterBox(scaleFill=True) (stretch without padding) is not on this path")
        if isinstance(new_shape, int):
            new_shape = (new_shape, new_shape)
        self.new_shape = (int(new_shape[0]), int(new_shape[1]))
        self.auto, self.scaleup, self.center, self.stride = bool(auto), bool(scaleup), bool(center), int(stride)

    def geometry(self, shape):
        h, w = int(shape[0]), int(shape[1])
        H, W = self.new_shape
        r = min(H / h, W / w)
        if not self.scaleup:
            r = min(r, 1.0)
        new_w, new_h = int(round(w * r)), int(round(h * r))
        dw, dh = W - new_w, H - new_h
        if self.auto:  # minimal rectangle
            dw, dh = dw % self.stride, dh % self.stride
        if self.center:
            dw, dh = dw / 2, dh / 2
        top, bottom = (int(round(dh - 0.1)) if self.center else 0), int(round(dh + 0.1))
        left, right = (int(round(dw - 0.1)) if self.center else 0), int(round(dw + 0.1))
        return new_h, new_w, top, left, new_h + top + bottom, new_w + left + right
