"""Times sliced inference with test-time augmentation (engine/predictor.py SlicedPredictor(augment=True),
csrc/tile_merge_tta.hip) at scripts/bench_sliced.py's shape: 4 frames of 2160 x 3840, slice 640, overlap 0.2 and the
whole-frame slot: 33 slots per frame, 132 tiles, five model calls of at most 32 tiles, three views per call with
34000 / 24565 / 16660 anchors of which 33600 / 24565 / 4116 are kept, A_tot = 62281, merged [4, 14, 33 * 62281]
(460 MB). GPU only.

  merge  the fused launches (three per call, each branch straight into merged) against the two-pass composition on the
         same GPU in the same process: per call _hip.tta_merge of the three branches into a concatenated
         cat [n, 14, 62281] (112 MB at 32 tiles), then _hip.tile_merge of cat. "kernel" = the C-ABI launches on prebuilt
         descriptors, "wrapper" = _hip.tile_merge_tta (descriptor built and copied per launch). The two results are
         first asserted equal. Bytes for the share of the HBM roof: the kept anchors read once, merged written once
         (larger than the 256 MiB Infinity Cache, so no rotation of buffers is needed).
  step   SlicedPredictor.predict_padded on GPU frames with augment off and on (seed-0 paper model, conf 0.25: random
         weights leave NMS empty, as in bench.py) with the stages timed apart and the peak allocated memory of a step,
         and the augmented step against the same composition: model(x, augment=True) per call, then _hip.tile_merge.

Times are HIP events on the stream over windows of at least 0.3 s after a warm-up, each taken twice, alternating.

  python scripts/bench_sliced_tta.py [--iters 20] [--out FILE.json] [--skip-step]"""
import argparse
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("MIOPEN_USER_DB_PATH", str(ROOT / "yolo-sod_amd" / "miopen_db"))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402
from yolosod_amd.data.tta import TTAPlan  # noqa: E402
from yolosod_amd.engine.predictor import SlicedPredictor  # noqa: E402

HBM_ROOF = 6.3e12  # achievable bytes / s
SHAPE, FRAMES, SLICE, OVERLAP, IMGSZ, BATCH, NC = (2160, 3840), 4, 640, 0.2, 640, 32, 10
STRIDES = (4, 8, 16, 32)


def timeit(fn, iters, warmup=3, min_ms=300.0):
    """ms per call: events on the stream around a window of at least ``iters`` calls and ``min_ms`` of GPU time."""
    for _ in range(warmup):
        fn()
    while True:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(iters):
            fn()
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
        for k, (fn, div) in fns.items():
            runs[k].append(timeit(fn, max(2, iters // div)))
    return runs


def synthetic_calls(plan, tp, dev, seed=0, n_cand=100):
    """Per model call the tuple of branch outputs, in each view's own pixels; about n_cand anchors per branch and tile
    score above conf 0.25."""
    g = torch.Generator(device=dev).manual_seed(seed)
    calls = []
    for lo, hi in plan.chunks(BATCH):
        n = hi - lo
        call = []
        for b in tp.branches:
            y = torch.empty((n, 4 + NC, b.A), device=dev)
            y[:, 0:2] = torch.rand((n, 2, b.A), generator=g, device=dev) * (IMGSZ * b.scale)
            y[:, 2:4] = (8 + 32 * torch.rand((n, 2, b.A), generator=g, device=dev)) * b.scale
            y[:, 4:] = torch.rand((n, NC, b.A), generator=g, device=dev) * 0.2
            pos = torch.rand((n, b.A), generator=g, device=dev).topk(n_cand, dim=1).indices
            y[:, 4].scatter_(1, pos, 0.25 + 0.75 * torch.rand((n, n_cand), generator=g, device=dev))
            call.append(y)
        calls.append(tuple(call))
    return calls


def bench_merge(dev, iters):
    tp = TTAPlan((IMGSZ, IMGSZ), stride=STRIDES, nl=len(STRIDES))

    class _Plans(torch.nn.Linear):
        def tta_plan(self, shape, scales=None, flips=None):
            return tp

    sp = SlicedPredictor(_Plans(1, 1).to(dev), slice=SLICE, overlap=OVERLAP, full_frame=True, batch=BATCH, imgsz=IMGSZ,
                         augment=True)
    plan = sp.plan([SHAPE] * FRAMES)
    A_tot = tp.A_tot
    calls = synthetic_calls(plan, tp, dev)
    n_max = max(c[0].shape[0] for c in calls)
    merged = torch.empty((FRAMES, 4 + NC, plan.S * A_tot), device=dev)
    other = torch.empty_like(merged)
    lib = _hip.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    res = []
    for cm in (None, 2.0):
        sp.cut_margin = cm
        cmf = -1.0 if cm is None else cm
        descs, lo = [], 0
        for c in calls:
            n = c[0].shape[0]
            d = _hip._tile_merge_desc("bench", plan.merge_rows(lo, lo + n), n, FRAMES, plan.S)
            descs.append((torch.from_numpy(d).to(dev), len(d)))
            lo += n

        def kernel():
            for c, (d, nr) in zip(calls, descs):
                for y, b in zip(c, tp.branches):
                    rc = lib.yolosod_tile_merge_tta(y.data_ptr(), y.shape[0], NC, b.A, b.src_lo, b.n, d.data_ptr(), nr,
                                                    merged.data_ptr(), FRAMES, plan.S, A_tot, b.dst, b.scale,
                                                    _hip.TTA_FLIPS[b.flip], float(IMGSZ), float(IMGSZ), cmf, st)
                    assert rc == 0

        def wrapper():
            sp.merge(calls, plan)  # allocates its own merged, as a step does

        def wrapper_into():
            lo = 0
            for c in calls:
                rows = plan.merge_rows(lo, lo + c[0].shape[0])
                for y, b in zip(c, tp.branches):
                    _hip.tile_merge_tta(y, rows, merged, A_tot, b, plan.canvas, cm)
                lo += c[0].shape[0]

        def two_pass():
            lo = 0
            for c in calls:
                n = c[0].shape[0]
                cat = torch.empty((n, 4 + NC, A_tot), device=dev)
                for y, b in zip(c, tp.branches):
                    _hip.tta_merge(y, cat, b.src_lo, b.n, b.dst, b.scale, b.flip, plan.canvas)
                _hip.tile_merge(cat, plan.merge_rows(lo, lo + n), other, A_tot, cm)
                lo += n

        merged.fill_(float("nan"))
        other.fill_(float("nan"))
        kernel()
        a = merged.clone()
        merged.fill_(float("nan"))
        wrapper_into()
        assert torch.equal(a, merged), "prebuilt descriptors differ from the wrapper's"
        assert torch.equal(sp.merge(calls, plan), merged)
        two_pass()
        assert not torch.isnan(other).any()
        assert torch.equal(other, merged), "the fused launches differ from the two-pass composition"
        del a
        runs = twice({"kernel": (kernel, 1), "wrapper": (wrapper_into, 1), "merge_stage": (wrapper, 1),
                      "two_pass": (two_pass, 1)}, iters)
        t = {k: sum(v) / 2 for k, v in runs.items()}
        kept = sum(c[0].shape[0] for c in calls) * (4 + NC) * A_tot * 4
        byt = kept + merged.numel() * 4
        byt2 = 2 * kept + 2 * merged.numel() * 4  # cat written and read on the way
        spread = max(max(v) - min(v) for v in runs.values())
        r = dict(case="merge", cut_margin=cm, frames=FRAMES, shape=list(SHAPE), tiles=len(plan), S=plan.S, A_tot=A_tot,
                 branch_anchors=[b.A for b in tp.branches], kept_anchors=[b.n for b in tp.branches], nc=NC,
                 calls=len(calls), launches=len(calls) * len(tp), merged_bytes=merged.numel() * 4, bytes=byt,
                 two_pass_bytes=byt2, cat_bytes_per_call=n_max * (4 + NC) * A_tot * 4, kernel_ms=t["kernel"],
                 wrapper_ms=t["wrapper"], merge_stage_ms=t["merge_stage"], two_pass_ms=t["two_pass"], runs_ms=runs,
                 spread_between_runs_ms=spread, speedup_vs_two_pass=t["two_pass"] / t["wrapper"],
                 kernel_speedup_vs_two_pass=t["two_pass"] / t["kernel"],
                 hbm_roof_fraction=byt / HBM_ROOF / (t["kernel"] * 1e-3),
                 two_pass_hbm_roof_fraction=byt2 / HBM_ROOF / (t["two_pass"] * 1e-3), fused_equals_two_pass=True)
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


def peak_mb(fn, dev):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 1e6


def bench_step(dev, iters):
    from yolosod_amd.nn.tasks import build_model
    model = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=dev)
    kw = dict(slice=SLICE, overlap=OVERLAP, full_frame=True, batch=BATCH, conf=0.25, iou=0.7, imgsz=IMGSZ)
    off, on = SlicedPredictor(model, **kw), SlicedPredictor(model, augment=True, **kw)
    frames = [torch.randint(0, 256, (*SHAPE, 3), dtype=torch.uint8, device=dev,
                            generator=torch.Generator(device=dev).manual_seed(i)) for i in range(FRAMES)]
    plan = on.plan([SHAPE] * FRAMES)
    tp = on.tta_plan(plan)

    def two_pass_step():
        """The augmented step composed of the pieces that existed before the fused merge."""
        merged = None
        for lo, hi in plan.chunks(BATCH):
            cat = model(on.ingest_tiles(frames, plan, lo, hi), augment=True)[0]
            if merged is None:
                merged = torch.empty((FRAMES, cat.shape[1], plan.S * tp.A_tot), device=dev)
            _hip.tile_merge(cat, plan.merge_rows(lo, hi), merged, tp.A_tot, on.cut_margin)
        return on.postprocess(merged, plan)

    with torch.inference_mode():
        ys_off, ys_on = off.forward_tiles(frames, plan), on.forward_tiles(frames, plan)
        m_off, m_on = off.merge(ys_off, plan), on.merge(ys_on, plan)
        runs = twice({"step_off": (lambda: off.predict_padded(frames), 1),
                      "step_on": (lambda: on.predict_padded(frames), 1),
                      "two_pass_step_on": (two_pass_step, 1),
                      "forward_tiles_off": (lambda: off.forward_tiles(frames, plan), 1),
                      "forward_tiles_on": (lambda: on.forward_tiles(frames, plan), 1),
                      "merge_off": (lambda: off.merge(ys_off, plan), 1),
                      "merge_on": (lambda: on.merge(ys_on, plan), 1),
                      "postprocess_off": (lambda: off.postprocess(m_off, plan), 1),
                      "postprocess_on": (lambda: on.postprocess(m_on, plan), 1)}, iters)
        del ys_off, ys_on, m_off, m_on
        peaks = {k: peak_mb(fn, dev) for k, fn in (("step_off", lambda: off.predict_padded(frames)),
                                                   ("step_on", lambda: on.predict_padded(frames)),
                                                   ("two_pass_step_on", two_pass_step))}
    m = {k: sum(v) / 2 for k, v in runs.items()}
    flagged = bool(_hip.split_range_flag(reset=True, device=dev))
    r = dict(case="step", frames=FRAMES, shape=list(SHAPE), tiles=len(plan), calls=len(plan.chunks(BATCH)),
             A=tp.branches[0].A, A_tot=tp.A_tot, nc=int(model.yaml["nc"]), conf=0.25,
             **{k + "_ms": v for k, v in m.items()}, augment_cost=m["step_on"] / m["step_off"],
             speedup_vs_two_pass_step=m["two_pass_step_on"] / m["step_on"],
             frames_per_s_off=FRAMES / (m["step_off"] * 1e-3), frames_per_s_on=FRAMES / (m["step_on"] * 1e-3),
             peak_allocated_mb=peaks, split_range_flagged=flagged, runs_ms=runs)
    print(json.dumps(r), flush=True)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sliced_tta: needs a GPU")
    dev = torch.device("cuda", 0)
    with torch.inference_mode():
        res = bench_merge(dev, a.iters)
    torch.cuda.empty_cache()
    if not a.skip_step:
        res += bench_step(dev, max(2, a.iters // 4))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": a.iters, "results": res},
                                          indent=1) + "\n")


if __name__ == "__main__":
    main()
