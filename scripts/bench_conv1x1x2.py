"""Times the fp16-split 1x1 kernel (yolosod_conv1x1x2_silu) on the neck's n1 conv shapes of the n640 model at bs=32
(MIOpen conv + HIP bias/SiLU beside it). GPU only; one line per distinct (shape, Cout)."""
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402
from yolosod_amd.nn import modules as M  # noqa: E402
from yolosod_amd.nn.tasks import build_model  # noqa: E402


def timeit(fn, iters=30):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    bs = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    dev = torch.device("cuda")
    model = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=dev)
    shapes = {}

    def hook(mod, inp):
        if mod.n1:
            c = mod.conv
            shapes[(tuple(inp[0].shape), c.out_channels)] = (c.weight.detach(), c.bias.detach())

    hs = [m.register_forward_pre_hook(hook) for m in model.modules() if isinstance(m, M.Conv)]
    with torch.inference_mode():
        model(torch.rand(bs, 3, 640, 640, device=dev))
    for h in hs:
        h.remove()
    tot_a = tot_b = 0.0
    with torch.inference_mode():
        for (shape, cout), (w, b) in sorted(shapes.items(), key=lambda kv: -kv[0][0][2]):
            x = torch.randn(shape, device=dev)
            blk = _hip.conv1x1x2_prepare(w)
            out = torch.empty((shape[0], cout, shape[2], shape[3]), device=dev)
            out2 = torch.empty((shape[0], cout // 2, shape[2], shape[3]), device=dev)
            ta = timeit(lambda: _hip.bias_act(F.conv2d(x, w), b, 1))
            tb = timeit(lambda: _hip.conv1x1x2_silu(x, b, lambda: blk, cout, out=out))
            td = timeit(lambda: _hip.conv1x1x2_silu(x, b, lambda: blk, cout, out=out, out2=out2, c2lo=cout // 2))
            flops = 2.0 * shape[0] * shape[2] * shape[3] * shape[1] * cout
            byt = 4.0 * shape[0] * shape[2] * shape[3] * (shape[1] + cout)
            print(f"{str(shape):24s} -> {cout:5d}  miopen+epi {ta:7.3f} ms  x2 {tb:7.3f} ms "
                  f"({flops / tb / 1e9:6.1f} TF/s, {byt / tb / 1e6:6.0f} GB/s)  dual {td:7.3f} ms", flush=True)
            tot_a += ta
            tot_b += tb
    print(f"total n1 shapes: miopen+epi {tot_a:.3f} ms  x2 {tot_b:.3f} ms")


def forms():
    """python scripts/bench_conv1x1x2.py forms: every form of the kernel (yolosod_debug_set_conv1x1x2_form: groups +
    4 buffers) forced on the neck's n1 shapes and the backbone's eight wide 1x1 shapes of the n640 step at bs 32; a
    library given by YOLOSOD_LIB_AB that predates the hook has its one form. One line per (shape, Cout, form): run it
    twice per library, alternating the libraries, and compare across the runs."""
    dev = torch.device("cuda")
    lib = _hip.load_library()
    model = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=dev)
    # the launches of one step with every marked conv routed (C2f calls its cv1 without a module hook: the op_timer
    # keys (op, input shape, (Cout, dual store, ...)) see every launch)
    M.N1_BACKBONE = True
    with torch.inference_mode(), _hip.op_timer() as rec:
        model(torch.rand(32, 3, 640, 640, device=dev))
    shapes = {}
    for k, _ in rec.durations_ms():
        if k[0] in ("conv1x1x2", "conv1x1x2_backbone") and k[2][0] % 128 == 0:
            who = "backbone" if k[0].endswith("_backbone") else "neck"
            where = shapes.setdefault((tuple(k[1]), k[2][0]), who)
            if who not in where:
                shapes[(tuple(k[1]), k[2][0])] = "both"
    del model
    has = hasattr(lib, "yolosod_debug_set_conv1x1x2_form")
    g = torch.Generator().manual_seed(0)
    with torch.inference_mode():
        for (shape, cout), where in sorted(shapes.items(), key=lambda kv: (-kv[0][0][2], kv[0][1], kv[0][0][1])):
            B, cin, H, W = shape
            x = torch.randn(shape, device=dev)
            w = (torch.randn(cout, cin, generator=g) * (1.0 / cin ** 0.5)).to(dev)
            b = (torch.randn(cout, generator=g) * 0.1).to(dev)
            blk = _hip.conv1x1x2_prepare(w)
            out = torch.empty((B, cout, H, W), device=dev)
            for form in ((5, 6, 9, 10) if has else (0,)):
                if has:
                    lib.yolosod_debug_set_conv1x1x2_form(form)
                    if lib.yolosod_debug_conv1x1x2_form(B, cout, H, W) != form:
                        continue  # the shape does not take the form
                t = timeit(lambda: _hip.conv1x1x2_silu(x, b, lambda: blk, cout, out=out), iters=50)
                print(f"{where:8s} {cin:5d} -> {cout:4d} at {H:3d}^2  form {form:2d}  {t:7.4f} ms", flush=True)
            if has:
                lib.yolosod_debug_set_conv1x1x2_form(0)


def stats():
    """python scripts/bench_conv1x1x2.py stats: the three gate-feeding neck convs of the n640 step at bs 32 (cv2 of the
    C2fs L17 / L22 / L31) - the new launch (yolosod_conv1x1x2_silu_stats; before the CA: the plain launch, and the CA
    pooling the map itself) against the sequence it replaces, F.conv2d + bias_act(stats=...), under
    cudnn.deterministic. The L31 pair is timed with the CA_Block's own launch behind it on both sides, since the pool
    moves into that launch. Each side twice per run; run it twice. A layer is kept only if every timing of the new form
    beats every timing of the old sequence by more than the spread (the largest difference between two timings of one
    side on one shape)."""
    dev = torch.device("cuda")
    torch.backends.cudnn.deterministic = True
    g = torch.Generator().manual_seed(0)
    spread = 0.0
    rows = []
    with torch.inference_mode():
        for layer, cin, cout, side, st in ((17, 384, 256, 40, "summax"), (22, 192, 128, 80, "sum"),
                                           (31, 192, 128, 80, "capool")):
            B = 32
            x = torch.randn(B, cin, side, side, device=dev)
            w = (torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin ** 0.5)).to(dev)
            b = (torch.randn(cout, generator=g) * 0.1).to(dev)
            blk = _hip.conv1x1x2_prepare(w)
            out = torch.empty((B, cout, side, side), device=dev)
            tail = lambda y: y  # noqa: E731
            if st == "capool":
                mip = max(8, cout // 32)
                cw = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(dev)  # noqa: E731
                ca = (cw(mip, cout, 1, 1), cw(mip), torch.ones(mip, device=dev), cw(mip), cw(mip),
                      torch.ones(mip, device=dev), 1e-5, cw(cout, mip, 1, 1), cw(cout), cw(cout, mip, 1, 1), cw(cout))
                tail = lambda y: _hip.ca_forward(y, *ca)  # noqa: E731
            old = lambda: tail(_hip.bias_act(F.conv2d(x, w), b, 1, out=out, stats=st))  # noqa: E731
            new = lambda: tail(_hip.conv1x1x2_silu(x, b, lambda: blk, cout, out=out, stats=st))  # noqa: E731
            to, tn = [], []
            for _ in range(2):
                to.append(timeit(old, iters=50))
                tn.append(timeit(new, iters=50))
            spread = max(spread, max(to) - min(to), max(tn) - min(tn))
            rows.append((layer, cin, cout, side, st, to, tn))
    for layer, cin, cout, side, st, to, tn in rows:
        keep = min(to) - max(tn) > spread
        print(f"L{layer} {cin:4d} -> {cout:4d} at {side}^2 {st:7s}  old {min(to):.4f} - {max(to):.4f} ms  "
              f"new {min(tn):.4f} - {max(tn):.4f} ms  {'KEEP' if keep else 'no gain'}"
              + ("  (with the CA launch on both sides)" if st == "capool" else ""), flush=True)
    print(f"spread {spread:.4f} ms")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "forms":
        forms()
    elif len(sys.argv) > 1 and sys.argv[1] == "stats":
        stats()
    else:
        main()
