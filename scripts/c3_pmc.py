"""A few launches of one stride-1 3x3 conv at 32 x Cin x 160 x 160 on the fp16-split kernel, for rocprofv3 --pmc passes:
python scripts/c3_pmc.py [cin cout [form]]   (default 64 64: the P2 Detect tower conv; 32 32: layer 3 / layer 27;
form: yolosod_debug_set_conv3x3_form, 0 = the automatic choice). GPU only."""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402

dev = torch.device("cuda", 0)
cin, cout = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (64, 64)
form = int(sys.argv[3]) if len(sys.argv) > 3 else 0
B, H, W = 32, 160, 160
x = torch.randn(B, cin, H, W, device=dev)
w = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
b = torch.randn(cout, device=dev) * 0.1
prep = _hip.conv3x3_prepare(w)
_hip.load_library().yolosod_debug_set_conv3x3_form(form)
for _ in range(5):
    _hip.conv3x3_silu(x, b, lambda: prep, cout)
torch.cuda.synchronize()
print("ok")
