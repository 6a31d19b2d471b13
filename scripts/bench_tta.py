"""Times test-time augmentation (nn/tasks.py DetectionModel._predict_augment, csrc/tta.hip) at n640 fp32 bs 32: views
of 544 x 544 (scale 0.83, flipped left-right) and 448 x 448 (scale 0.67), branches of 34000 / 24565 / 16660 anchors of
which 33600 + 24565 + 4116 = 62281 are kept. GPU only.

  views  the one launch that makes both views against the torch ops a user would write today, per view: ``flip`` +
         ``F.interpolate(bilinear)`` + ``F.pad(value=0.447)`` (the reference's ``scale_img``). "kernel" = the C-ABI
         launch on outputs and a descriptor table made once, "wrapper" = _hip.tta_views (allocates the views; the table
         is cached per output addresses). Bytes for the share of the HBM roof: x read once, the views written once.
         Two copies of x alternate, so that input + output (about 350 MB per call) never sit in the 256 MiB Infinity
         Cache whole.
  merge  the three launches that de-scale / de-flip / clip / concatenate against the reference's sequence: an in-place
         divide, ``split``, a subtract and a ``cat`` per branch (``_descale_pred``), slices (``_clip_augmented``) and
         the final ``cat``. Bytes: the kept anchors read once, ``cat`` written once. Two sets of branch outputs alternate.
  step   DetectionPredictor.predict_padded on a [32, 3, 640, 640] tensor with ``augment`` off and on (seed-0 paper
         model, conf 0.25: random weights leave NMS empty, as in bench.py).

Times are HIP events on the stream over windows of at least 0.3 s after a warm-up, each taken twice, alternating.

  python scripts/bench_tta.py [--iters 20] [--out FILE.json] [--skip-step]"""
import argparse
import json
import os
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("MIOPEN_USER_DB_PATH", str(ROOT / "yolo-sod_amd" / "miopen_db"))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402
from yolosod_amd.data.tta import TTAPlan  # noqa: E402
from yolosod_amd.engine.predictor import DetectionPredictor  # noqa: E402

HBM_ROOF = 6.3e12  # achievable bytes / s
B, C, IMGSZ, NC, NL, STRIDE = 32, 3, 640, 10, 4, 32


def timeit(fn, iters, warmup=3, min_ms=300.0):
    """ms per call: events on the stream around a window of at least ``iters`` calls and ``min_ms`` of GPU time."""
    for i in range(warmup):
        fn(i)
    while True:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for i in range(iters):
            fn(i)
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e)
        if ms >= min_ms:
            return ms / iters
        iters = int(iters * min(20.0, 1.25 * min_ms / max(ms, 1e-3))) + 1


def twice(fns, iters):
    """{name: [ms, ms]} with the candidates alternating."""
    runs = {k: [] for k in fns}
    for _ in range(2):
        for k, fn in fns.items():
            runs[k].append(timeit(fn, iters))
    return runs


def torch_views(x, plan):
    """The views with torch ops, as the reference makes them (x.flip + scale_img)."""
    out = []
    for b in plan.branches:
        if b.view is None:
            continue
        xi = x.flip(b.flip) if b.flip else x
        xi = F.interpolate(xi, size=b.resized, mode="bilinear", align_corners=False)
        out.append(F.pad(xi, [0, b.padded[1] - b.resized[1], 0, b.padded[0] - b.resized[0]], value=0.447))
    return out


def bench_views(dev, iters, plan):
    g = torch.Generator(device=dev).manual_seed(0)
    xs = [torch.rand((B, C, IMGSZ, IMGSZ), generator=g, device=dev) for _ in range(2)]
    outs = [torch.empty((B, C, v[3], v[4]), device=dev) for v in plan.views]
    geom = [(_hip.TTA_FLIPS[v[0]], *v[1:]) for v in plan.views]
    desc = torch.tensor([[t.data_ptr(), *g_, 0, 0] for t, g_ in zip(outs, geom)], dtype=torch.int64).to(dev)
    lib = _hip.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    max_ph, max_pw = max(v[3] for v in plan.views), max(v[4] for v in plan.views)
    cache = {}

    def kernel(i):
        rc = lib.yolosod_tta_views(xs[i % 2].data_ptr(), B, C, IMGSZ, IMGSZ, 0, desc.data_ptr(), len(outs), max_ph,
                                   max_pw, st)
        assert rc == 0

    kernel(0)
    got = _hip.tta_views(xs[0], plan.views, cache=cache)
    ref = torch_views(xs[0], plan)
    assert all(torch.equal(a, b) for a, b in zip(outs, got)), "the prebuilt table differs from the wrapper's"
    diff = max(float((a - b).abs().max()) for a, b in zip(got, ref))
    del got, ref
    runs = twice({"kernel": kernel, "wrapper": lambda i: _hip.tta_views(xs[i % 2], plan.views, cache=cache),
                  "torch": lambda i: torch_views(xs[i % 2], plan)}, iters)
    t_k, t_w, t_t = (sum(v) / 2 for v in (runs["kernel"], runs["wrapper"], runs["torch"]))
    byt = xs[0].numel() * 4 + sum(t.numel() for t in outs) * 4
    r = dict(case="views", x=[B, C, IMGSZ, IMGSZ], views=[list(v[1:]) for v in plan.views], bytes=byt, kernel_ms=t_k,
             wrapper_ms=t_w, torch_ms=t_t, runs_ms=runs, speedup_vs_torch=t_t / t_w,
             hbm_roof_fraction=byt / HBM_ROOF / (t_k * 1e-3), max_abs_diff_vs_torch=diff)
    print(json.dumps(r), flush=True)
    return [r]


def torch_merge(ys, plan, undo):
    """The reference's _descale_pred per branch, _clip_augmented and torch.cat. ``undo``: divide by 1 / scale instead
    (the in-place divide would otherwise compound over the timed calls)."""
    out = []
    for p, b in zip(ys, plan.branches):
        p[:, :4] /= (1.0 / b.scale) if undo else b.scale
        x, y, wh, cls = p.split((1, 1, 2, p.shape[1] - 4), 1)
        if b.flip == 2:
            y = plan.shape[0] - y
        elif b.flip == 3:
            x = plan.shape[1] - x
        out.append(torch.cat((x, y, wh, cls), 1))
    g = sum(4 ** k for k in range(plan.nl))
    i = (out[0].shape[-1] // g) * 1
    out[0] = out[0][..., :-i]
    i = (out[-1].shape[-1] // g) * 4 ** (plan.nl - 1)
    out[-1] = out[-1][..., i:]
    return torch.cat(out, -1)


def bench_merge(dev, iters, plan):
    g = torch.Generator(device=dev).manual_seed(1)
    sets = []
    for _ in range(2):
        ys = []
        for b in plan.branches:
            y = torch.empty((B, 4 + NC, b.A), device=dev)
            y[:, :4] = torch.rand((B, 4, b.A), generator=g, device=dev) * IMGSZ * b.scale
            y[:, 4:] = torch.rand((B, NC, b.A), generator=g, device=dev)
            ys.append(y)
        sets.append(ys)
    cat = torch.empty((B, 4 + NC, plan.A_tot), device=dev)

    def kernel(i):
        for k, y in enumerate(sets[i % 2]):
            plan.merge(k, y, cat)

    kernel(0)
    ref = torch_merge([y.clone() for y in sets[0]], plan, False)
    same = bool(torch.equal(ref, cat))
    diff = float((ref - cat).abs().max())
    del ref
    runs = twice({"kernel": kernel, "torch": lambda i: torch_merge(sets[i % 2], plan, bool((i // 2) & 1))}, iters)
    t_k, t_t = (sum(v) / 2 for v in (runs["kernel"], runs["torch"]))
    byt = 2 * cat.numel() * 4
    r = dict(case="merge", branches=[[b.A, b.src_lo, b.n, b.dst] for b in plan.branches], A_tot=plan.A_tot, nc=NC,
             bytes=byt, kernel_ms=t_k, torch_ms=t_t, runs_ms=runs, speedup_vs_torch=t_t / t_k,
             hbm_roof_fraction=byt / HBM_ROOF / (t_k * 1e-3), torch_equals_fused=same, max_abs_diff_vs_torch=diff)
    print(json.dumps(r), flush=True)
    return [r]


def bench_step(dev, iters):
    from yolosod_amd.nn.tasks import build_model
    model = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=dev)
    x = torch.rand((B, C, IMGSZ, IMGSZ), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    off = DetectionPredictor(model, conf=0.25, iou=0.7)
    on = DetectionPredictor(model, conf=0.25, iou=0.7, augment=True)
    with torch.inference_mode():
        runs = twice({"augment_off": lambda i: off.predict_padded(x), "augment_on": lambda i: on.predict_padded(x)},
                     iters)
        with _hip.op_timer(lambda key: key[0] in ("tta_views", "tta_merge")) as t:
            on.predict_padded(x)
        own = {}
        for key, ms in t.durations_ms():
            own[key[0]] = own.get(key[0], 0.0) + ms
    m = {k: sum(v) / 2 for k, v in runs.items()}
    flagged = bool(_hip.split_range_flag(reset=True, device=dev))
    r = dict(case="step", x=[B, C, IMGSZ, IMGSZ], conf=0.25, augment_off_ms=m["augment_off"],
             augment_on_ms=m["augment_on"], on_over_off=m["augment_on"] / m["augment_off"],
             img_per_s_off=B / (m["augment_off"] * 1e-3), img_per_s_on=B / (m["augment_on"] * 1e-3),
             tta_kernels_in_step_ms=own, split_range_flagged=flagged, runs_ms=runs)
    print(json.dumps(r), flush=True)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta: needs a GPU")
    dev = torch.device("cuda", 0)
    plan = TTAPlan((IMGSZ, IMGSZ), stride=STRIDE, nl=NL)
    assert [b.n for b in plan.branches] == [33600, 24565, 4116] and plan.A_tot == 62281
    with torch.inference_mode():
        res = bench_views(dev, a.iters, plan) + bench_merge(dev, a.iters, plan)
    if not a.skip_step:
        res += bench_step(dev, max(2, a.iters // 4))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": a.iters, "results": res},
                                          indent=1) + "\n")


if __name__ == "__main__":
    main()
