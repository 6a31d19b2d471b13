"""Five launches of the neck's L22 cv2 (192 -> 128 at 80^2, batch 32, statistics "sum") for a rocprofv3 --pmc pass of
its own (FETCH_SIZE WRITE_SIZE; no tracing in the same run): python scripts/c1_stats_pmc.py new | old
new: the fp16-split kernel's statistics form + the tile reduce; old: F.conv2d + bias_act(stats="sum"). GPU only."""
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402

dev = torch.device("cuda", 0)
torch.backends.cudnn.deterministic = True
cin, cout, side = 192, 128, 80
x = torch.randn(32, cin, side, side, device=dev)
w = torch.randn(cout, cin, 1, 1, device=dev) * (1.0 / cin ** 0.5)
b = torch.randn(cout, device=dev) * 0.1
out = torch.empty(32, cout, side, side, device=dev)
prep = _hip.conv1x1x2_prepare(w)
with torch.inference_mode():
    for _ in range(5):
        if sys.argv[1] == "new":
            _hip.conv1x1x2_silu(x, b, lambda: prep, cout, out=out, stats="sum")
        else:
            _hip.bias_act(F.conv2d(x, w), b, 1, out=out, stats="sum")
torch.cuda.synchronize()
print("ok")
