"""Micro-benchmark: the stride-1 3x3 convs of the n640 step (bs 32) - the Detect towers and the backbone's / neck's C2f
Bottleneck convs (Cout 32 .. 256, with and without the shortcut) - on the fp16-split kernel vs MIOpen (F.conv2d without
bias + the HIP bias / SiLU (+ shortcut) epilogue, as the executor runs it). GPU only.
python scripts/bench_conv3x3.py [forms | bottleneck [H [batches]] | head [rounds]]; YOLOSOD_LIB_AB=<lib> times another build of the library."""
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402

dev = torch.device("cuda", 0)
SHAPES = [(32, 64, 160, 160), (32, 128, 80, 80), (32, 64, 80, 80), (32, 256, 40, 40), (32, 64, 40, 40),
          (32, 512, 20, 20), (32, 64, 20, 20)]


def timed(fn, reps=50):
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


if len(sys.argv) > 1 and sys.argv[1] == "bottleneck":
    # the 32-channel Bottleneck (32 -> 32 -> 32 with the shortcut) in place in a C2f's 96-channel buffer, input
    # z[:, 32:64] and output z[:, 64:96]: the fused launch against the two conv launches (each timed alone, their sum,
    # and the two back to back); python scripts/bench_conv3x3.py bottleneck [H [batches]], every batch twice,
    # alternating the two sides
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 160
    batches = [int(a) for a in sys.argv[3].split(",")] if len(sys.argv) > 3 else [2, 4, 8, 16, 32]
    for B in batches * 2:
        z = torch.randn(B, 96, H, H, device=dev)
        t = torch.empty(B, 32, H, H, device=dev)
        x, y = z[:, 32:64], z[:, 64:96]
        w1, w2 = (torch.randn(32, 32, 3, 3, device=dev) * 0.05 for _ in range(2))
        b1, b2 = (torch.randn(32, device=dev) * 0.1 for _ in range(2))
        p1, p2 = _hip.conv3x3_prepare(w1), _hip.conv3x3_prepare(w2)
        cv1 = lambda: _hip.conv3x3_silu(x, b1, lambda: p1, 32, out=t)  # noqa: E731
        cv2 = lambda: _hip.conv3x3_silu(t, b2, lambda: p2, 32, out=y, res=x)  # noqa: E731
        fused = lambda: _hip.bottleneck3x3_silu(x, b1, lambda: p1, b2, lambda: p2, out=y, res=x)  # noqa: E731
        cv1(), cv2()
        y0 = y.clone()
        fused()
        same = torch.equal(y, y0)
        row = []
        for _ in range(2):
            t1, t2 = timed(cv1), timed(cv2)
            row.append((timed(fused), t1, t2, timed(lambda: (cv1(), cv2()))))
        mb = B * 32 * H * H * 4 / 1e6
        print(f"B {B:2d} x 32 x {H}^2 ({mb:6.1f} MB/map) equal {same}  " + "   ".join(
            f"fused {f:.4f}  cv1 {a:.4f} + cv2 {b:.4f} = {a + b:.4f}  pair back-to-back {p:.4f} ms"
            for f, a, b, p in row), flush=True)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "head":
    # a Detect level's two towers from their second conv on: the two fused launches (conv + 1x1 conv + decode, box and
    # class) against the two conv launches + the head kernel on that level alone, alternating the sides, four timings
    # per side; the spread is the largest difference between two timings of one side at one size.
    # python scripts/bench_conv3x3.py head [rounds]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    nc, strides = 10, [4.0, 8.0, 16.0, 32.0]
    rows, spread = [], 0.0
    for B, H, li in ((32, 160, 0), (32, 80, 1), (32, 40, 2), (32, 20, 3), (8, 320, 0)):
        x = torch.randn(B, 64, H, H, device=dev)
        ws = [torch.randn(64, 64, 3, 3, device=dev) * 0.04 for _ in range(2)]
        bs = [torch.randn(64, device=dev) * 0.1 for _ in range(2)]
        hw = [torch.randn(64, 64, device=dev) * 0.25, torch.randn(nc, 64, device=dev) * 0.2]
        hb = [torch.randn(64, device=dev), torch.randn(nc, device=dev) - 2.0]
        ps = [_hip.conv3x3_prepare(w) for w in ws]
        hps = [_hip.detect_head_prepare(hw[0], 64), _hip.detect_head_prepare(hw[1], nc)]
        sizes = [(4, 4)] * 4
        sizes[li] = (H, H)
        a_off = 16 * li
        A = 16 * 3 + H * H
        y = torch.full((B, 4 + nc, A), float("nan"), device=dev)
        fb, fc = (torch.empty(B, 64, H, H, device=dev) for _ in range(2))
        fbs = [fb if i == li else sizes[i] for i in range(4)]
        fcs = [fc if i == li else None for i in range(4)]

        def pair():
            _hip.conv3x3_silu(x, bs[0], lambda: ps[0], 64, out=fb)
            _hip.conv3x3_silu(x, bs[1], lambda: ps[1], 64, out=fc)
            _hip.detect_head_into(y, li, li + 1, fbs, fcs, [hw[0]] * 4, [hb[0]] * 4, [hw[1]] * 4, [hb[1]] * 4, strides, nc)

        def fused():
            for m in (1, 2):
                _hip.conv3x3_head(x, bs[m - 1], lambda: ps[m - 1], lambda: hps[m - 1], hb[m - 1], m, nc, strides[li], y,
                                  a_off)

        auto = _hip.conv3x3_head_fused(B, H, H)
        # the fused side runs 64-channel groups on every shape; the conv side its automatic form
        pair()
        y0 = y.clone()
        y.fill_(float("nan"))
        fused()
        same = torch.equal(torch.nan_to_num(y, nan=-1.0), torch.nan_to_num(y0, nan=-1.0))
        for _ in range(3):  # both sides warm (clocks, caches, the allocator) before the first timing
            timed(fused, 20), timed(pair, 20)
        tf, tp = [], []
        for _ in range(rounds):
            tf.append(timed(fused))
            tp.append(timed(pair))
        spread = max(spread, max(tf) - min(tf), max(tp) - min(tp))
        rows.append((B, H, auto, same, tf, tp))
    print(f"spread (largest difference between two timings of one side at one size): {spread:.4f} ms")
    for B, H, auto, same, tf, tp in rows:
        wins = min(tp) - max(tf) > spread
        print(f"B {B:2d} x 64 x {H:3d}^2  equal {same}  automatic route {'fused' if auto else 'pair '}  "
              f"fused {' '.join(f'{t:.4f}' for t in tf)}   conv + conv + head {' '.join(f'{t:.4f}' for t in tp)} ms   "
              f"every fused timing beats every pair timing by more than the spread: {wins}", flush=True)
    sys.exit(0)

# every stride-1 3x3 launch shape of the n640 step at bs 32: (input shape, Cout, residual). Detect towers (Cout 64),
# then the C2f Bottleneck convs of the backbone (L3 / L6 / L8 / L11) and the neck (cv1 plain, cv2 + shortcut)
CASES = [(s, 64, False) for s in SHAPES]
for c, hw in ((32, 160), (64, 80), (128, 40), (256, 20)):
    CASES += [((32, c, hw, hw), c, False), ((32, c, hw, hw), c, True)]
# forms of the persistent kernel (yolosod_debug_set_conv3x3_form: geometry + 4 groups), when the library has the hook
# (an older library given by YOLOSOD_LIB_AB has one form): "forms" as the first argument times every form per shape
lib = _hip.load_library()
FORMS = [0]
if len(sys.argv) > 1 and sys.argv[1] == "forms" and hasattr(lib, "yolosod_debug_set_conv3x3_form"):
    FORMS = [0] + [g + 4 * grp for g in (1, 2, 3) for grp in (1, 2)]
    if hasattr(lib, "yolosod_debug_conv3x3_form_ex"):  # Cin 32 -> Cout 32: resident weights (3), both blocks per wave (4)
        FORMS += [g + 4 * grp for g in (1, 2, 3) for grp in (3, 4)]
GEO = {1: "32x8", 2: "20x12", 3: "40x6"}
GRP = {1: "g64", 2: "g32", 3: "g32r", 4: "g32b"}

for shape, cout, res in CASES:
    B, cin, H, W = shape
    x = torch.randn(shape, device=dev)
    w = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
    b = torch.randn(cout, device=dev) * 0.1
    r = torch.randn(B, cout, H, W, device=dev) if res else None
    prep = _hip.conv3x3_prepare(w)
    gf = 2 * B * H * W * cout * cin * 9 / 1e9
    t_m = timed(lambda: _hip.bias_act(F.conv2d(x, w, None, padding=1), b, 1, res=r))
    line = f"{str(shape):22s} -> {cout:3d}{' +res' if res else '     '}  MIOpen+epilogue {t_m:7.3f} ms ({gf / t_m:6.1f} TF/s)"
    for form in FORMS:
        if form and (cout == 32 and form >> 2 == 1 or form >> 2 > 2 and (cout, cin) != (32, 32)):
            continue
        if len(FORMS) > 1:
            lib.yolosod_debug_set_conv3x3_form(form)
        t_k = timed(lambda: _hip.conv3x3_silu(x, b, lambda: prep, cout, res=r))
        name = "kernel"
        if hasattr(lib, "yolosod_debug_conv3x3_form_ex"):
            f = lib.yolosod_debug_conv3x3_form_ex(B, cin, cout, H, W)
            name = f"{'auto=' if form == 0 else ''}{GEO[f & 3]}/{GRP[f >> 2]}"
        elif hasattr(lib, "yolosod_debug_conv3x3_form"):
            f = lib.yolosod_debug_conv3x3_form(B, cout, H, W)
            name = f"{'auto=' if form == 0 else ''}{GEO[f & 3]}/{GRP[f >> 2]}"
        line += f"   {name} {t_k:6.3f} ms ({gf / t_k:5.1f} TF/s)"
    if len(FORMS) > 1:
        lib.yolosod_debug_set_conv3x3_form(0)
    print(line, flush=True)
