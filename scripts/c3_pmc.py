"""A few launches of one stride-1 3x3 conv at 32 x Cin x 160 x 160 on the fp16-split kernel, for rocprofv3 --pmc passes:
python scripts/c3_pmc.py [cin cout [form]]   (default 64 64: the P2 Detect tower conv; 32 32: layer 3 / layer 27;
form: yolosod_debug_set_conv3x3_form, 0 = the automatic choice), or
python scripts/c3_pmc.py bottleneck fused|pair [B]   the 32-channel Bottleneck with the shortcut in place in a
96-channel buffer, as one launch or as its two conv launches, or
python scripts/c3_pmc.py head fused|pair   the P2 box tower's last conv with the head's tail in its epilogue, or the conv
launch followed by the head kernel on that level. GPU only."""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402

dev = torch.device("cuda", 0)
if len(sys.argv) > 2 and sys.argv[1] == "bottleneck":
    B, H, W = int(sys.argv[3]) if len(sys.argv) > 3 else 32, 160, 160
    z = torch.randn(B, 96, H, W, device=dev)
    t = torch.empty(B, 32, H, W, device=dev)
    x, y = z[:, 32:64], z[:, 64:96]
    w1, w2 = (torch.randn(32, 32, 3, 3, device=dev) * 0.05 for _ in range(2))
    b1, b2 = (torch.randn(32, device=dev) * 0.1 for _ in range(2))
    p1, p2 = _hip.conv3x3_prepare(w1), _hip.conv3x3_prepare(w2)
    for _ in range(5):
        if sys.argv[2] == "fused":
            _hip.bottleneck3x3_silu(x, b1, lambda: p1, b2, lambda: p2, out=y, res=x)
        else:
            _hip.conv3x3_silu(x, b1, lambda: p1, 32, out=t)
            _hip.conv3x3_silu(t, b2, lambda: p2, 32, out=y, res=x)
    torch.cuda.synchronize()
    print("ok")
    sys.exit(0)
if len(sys.argv) > 2 and sys.argv[1] == "head":
    # the P2 box tower from its second conv on: the fused launch (conv + 1x1 conv + decode), or the conv launch and the
    # head kernel on that level (which also reads the class features: half of its traffic is the box tower's)
    B, H, W, nc = 32, 160, 160, 10
    x = torch.randn(B, 64, H, W, device=dev)
    w = torch.randn(64, 64, 3, 3, device=dev) * 0.04
    b = torch.randn(64, device=dev) * 0.1
    hw, hb = torch.randn(64, 64, device=dev) * 0.25, torch.randn(64, device=dev)
    cw, cb = torch.randn(nc, 64, device=dev) * 0.2, torch.randn(nc, device=dev) - 2.0
    p, hp = _hip.conv3x3_prepare(w), _hip.detect_head_prepare(hw, 64)
    y = torch.empty(B, 4 + nc, H * W, device=dev)
    fb, fc = torch.empty(B, 64, H, W, device=dev), torch.randn(B, 64, H, W, device=dev)
    for _ in range(5):
        if sys.argv[2] == "fused":
            _hip.conv3x3_head(x, b, lambda: p, lambda: hp, hb, 1, nc, 4.0, y, 0)
        else:
            _hip.conv3x3_silu(x, b, lambda: p, 64, out=fb)
            _hip.detect_head_into(y, 0, 1, [fb], [fc], [hw], [hb], [cw], [cb], [4.0], nc)
    torch.cuda.synchronize()
    print("ok")
    sys.exit(0)
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
