"""Micro-benchmark: the gate-consumer stride-2 convs at the n640 / m640 shapes on the fused kernel (gate applied at
staging) vs what it replaces: the gate's apply pass + MIOpen conv (no bias) + the HIP bias / SiLU epilogue. GPU only.
python scripts/bench_conv3x3s2.py [forms]; "forms" times every form of the tiled kernel on the stride-2
launch shapes of the n640 step; YOLOSOD_LIB_AB=<lib> times another build of the library (one form if it predates the
hook)."""
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402

dev = torch.device("cuda", 0)
# (input shape, Cout, gates): SE L1 -> L2 and CBAM L4 -> L5 (n640, n1280), SE L1 -> L2 (m640 shape)
SHAPES = [((32, 32, 320, 320), 64, "c"), ((32, 64, 160, 160), 128, "cp"), ((8, 32, 640, 640), 64, "c"),
          ((8, 64, 320, 320), 128, "cp"), ((64, 64, 320, 320), 128, "c")]


def timed(fn, reps=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


FORMS_MODE = len(sys.argv) > 1 and sys.argv[1] == "forms"
if FORMS_MODE:
    # the five gate-free launches of the n640 step at bs 32 (L7, L10, L29, L33 and L36 into their concat slices:
    # (input shape, Cout, channels of the output buffer)) and the gated L5 launch; every form per shape
    # (yolosod_debug_set_conv3x3s2_form: geometry + 4 groups), each timed twice and the automatic choice
    # again at the end (the spread of the script)
    lib = _hip.load_library()
    CASES = [("L7", (32, 128, 80, 80), 256, 256, ""), ("L10", (32, 256, 40, 40), 512, 512, ""),
             ("L29", (32, 64, 160, 160), 128, 384, ""), ("L33", (32, 128, 80, 80), 256, 768, ""),
             ("L36", (32, 256, 40, 40), 512, 1024, ""), ("L5", (32, 64, 160, 160), 128, 128, "cp")]
    has = hasattr(lib, "yolosod_debug_set_conv3x3s2_form")
    FORMS = [0] + [g + 4 * grp for grp in (1, 2) for g in (1, 2, 3)] if has else [0]
    GEO = {1: "32x2", 2: "40x2", 3: "20x4"}
    for name, shape, cout, cbuf, gates in CASES:
        B, cin, H, W = shape
        x = torch.randn(shape, device=dev)
        w = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
        b = torch.randn(cout, device=dev) * 0.1
        gc = torch.sigmoid(torch.randn(B, cin, device=dev)) if "c" in gates else None
        gp = torch.sigmoid(torch.randn(B, H, W, device=dev)) if "p" in gates else None
        buf = torch.zeros(B, cbuf, H // 2, W // 2, device=dev)
        out = buf[:, cbuf - cout:]
        prep = _hip.conv3x3s2_prepare(w)
        gf = 2 * B * (H // 2) * (W // 2) * cout * cin * 9 / 1e9
        line = f"{name:4s} {str(shape):20s} -> {cout:3d} in {cbuf:4d} {gates or '-':2s}"
        run = lambda: _hip.conv3x3s2_silu(x, b, lambda: prep, cout, gc, gp, out=out)  # noqa: E731
        timed(run, 100)  # the first timing of a shape read 5 - 10 % high without it (clocks, caches)
        for form in FORMS + [0]:  # the automatic choice first and last
            if has:
                lib.yolosod_debug_set_conv3x3s2_form(form)
            t1, t2 = timed(run, 50), timed(run, 50)
            label = "kernel"
            if has:
                f = lib.yolosod_debug_conv3x3s2_form(B, cout, H, W)
                label = f"{'auto=' if form == 0 else ''}{GEO[f & 3]}/g{256 >> (f >> 2)}"
            line += f"   {label} {t1:6.3f} {t2:6.3f} ms ({gf / min(t1, t2):5.1f} TF/s)"
        if has:
            lib.yolosod_debug_set_conv3x3s2_form(0)
        print(line, flush=True)
    sys.exit(0)

for shape, cout, gates in SHAPES:
    B, cin, H, W = shape
    x = torch.randn(shape, device=dev)
    w = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
    b = torch.randn(cout, device=dev) * 0.1
    gc = torch.sigmoid(torch.randn(B, cin, device=dev))
    gp = torch.sigmoid(torch.randn(B, H, W, device=dev)) if "p" in gates else None
    prep = _hip.conv3x3s2_prepare(w)
    t_f = timed(lambda: _hip.conv3x3s2_silu(x, b, lambda: prep, cout, gc, gp))
    t_n = timed(lambda: _hip.conv3x3s2_silu(x, b, lambda: prep, cout))

    def unfused():
        xg = x * gc[:, :, None, None]
        if gp is not None:
            xg = xg * gp[:, None]
        return _hip.bias_act(F.conv2d(xg, w, None, stride=2, padding=1), b, 1)

    t_u = timed(unfused)
    t_c = timed(lambda: _hip.bias_act(F.conv2d(x, w, None, stride=2, padding=1), b, 1))
    gf = 2 * B * ((H + 1) // 2) * ((W + 1) // 2) * cout * cin * 9 / 1e9
    gb = (x.numel() + B * cout * ((H + 1) // 2) * ((W + 1) // 2)) * 4 / 1e9
    print(f"{str(shape):22s} Cout {cout:3d} gates {gates:2s}  fused {t_f:7.3f} ms ({gf / t_f:6.1f} TF/s, "
          f"{gb / t_f:5.2f} TB/s)  no-gate {t_n:7.3f}  |  torch apply + MIOpen + epilogue {t_u:7.3f} "
          f"(MIOpen + epilogue alone {t_c:7.3f})", flush=True)
