"""Generate the test-time augmentation fixtures by running the REFERENCE (``make_golden.import_reference``):
``python tests/golden/make_tta_golden.py``. Data only - seeds, shapes and recorded outputs:

  tests/golden/tta_scale_img.npz   ``scale_img(x.flip(f) if f else x, ratio, gs=32)`` (utils/torch_utils.py:423-432) for
                                   the small cases of tests/test_gpu_tta.py, x = rand(2, 3, H, W) from a seeded generator
  tests/golden/tta_descale.npz     ``DetectionModel._descale_pred`` (nn/tasks.py:398-407) on a random [2, 14, 85]
  tests/golden/tta_model_256.npz   ``predict(x, augment=True)`` of the seed-0 fused paper model on rand(1, 3, 256, 256)
                                   (seed 3): [1, 14, 10297]
"""
from __future__ import annotations

import numpy as np
import torch

from make_golden import HERE, REF, import_reference

# (H, W, ratio, flip), x = rand(2, 3, H, W) with seed 100 + case index
SCALE_IMG_CASES = [(64, 96, 0.83, 3), (64, 96, 0.67, None), (40, 50, 0.83, 2), (40, 50, 1.5, 3), (64, 64, 0.5, None)]
DESCALE_CASES = [(None, 1), (3, 0.83), (2, 0.67), (3, 1.5)]
DESCALE_IMG = (64, 96)


def case_input(i: int, h: int, w: int) -> torch.Tensor:
    return torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(100 + i))


def descale_input() -> torch.Tensor:
    g = torch.Generator().manual_seed(7)
    p = torch.rand(2, 14, 85, generator=g)
    p[:, :4] = p[:, :4] * 120 - 10
    return p


def main():
    _, tasks, _ = import_reference()
    from ultralytics.utils.torch_utils import scale_img
    out = {}
    for i, (h, w, r, f) in enumerate(SCALE_IMG_CASES):
        x = case_input(i, h, w)
        y = scale_img(x.flip(f) if f else x, r, gs=32)
        out[f"y{i}"] = y.numpy()
        print("scale_img", (h, w, r, f), tuple(y.shape))
    np.savez_compressed(HERE / "tta_scale_img.npz", **out)

    out = {}
    for i, (f, s) in enumerate(DESCALE_CASES):
        out[f"y{i}"] = tasks.DetectionModel._descale_pred(descale_input(), f, s, DESCALE_IMG).numpy()
    np.savez_compressed(HERE / "tta_descale.npz", **out)

    torch.manual_seed(0)
    m = tasks.DetectionModel(str(REF / "ultralytics/cfg/models/new/yolov12-sod-fusion-v5-simple.yaml"), verbose=False)
    m.fuse(verbose=False)
    m.eval()
    x = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(3))
    with torch.inference_mode():
        y, none = m.predict(x, augment=True)
    assert none is None
    print("predict(augment=True)", tuple(y.shape))
    np.savez_compressed(HERE / "tta_model_256.npz", x_seed=np.array(3), y=y.numpy())


if __name__ == "__main__":
    main()
