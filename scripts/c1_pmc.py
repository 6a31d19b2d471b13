"""A few launches of one wide 1x1 conv at batch 32 on the fp16-split kernel in each of its forms, for rocprofv3 --pmc
passes (the forms are different instances of conv1x1_x2_kernel<DUAL, 64, CPW, DB>, so the counters separate by kernel
name): python scripts/c1_pmc.py [cin cout side]   (default 768 512 20; 384 256 40: the neck's P4 shape). GPU only."""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402

dev = torch.device("cuda", 0)
cin, cout, side = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (768, 512, 20)
x = torch.randn(32, cin, side, side, device=dev)
w = torch.randn(cout, cin, device=dev) * (1.0 / cin ** 0.5)
b = torch.randn(cout, device=dev) * 0.1
prep = _hip.conv1x1x2_prepare(w)
lib = _hip.load_library()
for form in (5, 6, 9, 10):  # groups 128 / 256 + 4 * buffers 1 / 2
    lib.yolosod_debug_set_conv1x1x2_form(form)
    for _ in range(5):
        _hip.conv1x1x2_silu(x, b, lambda: prep, cout)
lib.yolosod_debug_set_conv1x1x2_form(0)
torch.cuda.synchronize()
print("ok")
