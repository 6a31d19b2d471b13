"""Times sliced inference (engine/predictor.py SlicedPredictor, csrc/tile_merge.hip) on 4 frames of 2160 x 3840 with
slice 640, overlap 0.2 and the whole-frame slot: 33 slots per frame, 132 tiles, five model calls of at most 32 tiles,
A = 34000 anchors per tile, merged [4, 14, 33 * 34000] (251 MB). GPU only.

  merge  the fused merge against the same merge written with torch ops on the same GPU - per tile, arithmetic on the
         box rows of y[i], the cut mask, and a copy into the tile's slot of merged; what a user of the tensors would
         write without the kernel. "kernel" = the C-ABI launches on prebuilt descriptors, "wrapper" = _hip.tile_merge
         (descriptor built and copied per call). cut_margin off and 2. y is synthetic: about 300 anchors per tile score
         above conf 0.25. Bytes for the share of the HBM roof: y read once, merged written once (502 MB; larger than
         the 256 MiB Infinity Cache, so no rotation of buffers is needed).
  nms    NMS on that merged tensor (about 10k candidates per frame).
  step   SlicedPredictor.predict_padded on GPU frames (seed-0 paper model, conf 0.25: random weights leave NMS
         empty, as in bench.py) with its stages timed apart, against the composition on DetectionPredictor's public
         interface: per chunk of 32 tile views predict_padded (ingest + model + per-tile NMS truncated to max_det),
         boxes shifted by the tile offset with torch ops, gathered per frame into a [F, 4+nc, S * max_det] tensor and
         put through a second NMS.

Times are HIP events on the stream over windows of at least 0.3 s after a warm-up, each taken twice, alternating.

  python scripts/bench_sliced.py [--iters 20] [--out FILE.json] [--skip-step]"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("MIOPEN_USER_DB_PATH", str(ROOT / "yolo-sod_amd" / "miopen_db"))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402
from yolosod_amd.engine.predictor import DetectionPredictor, SlicedPredictor  # noqa: E402
from yolosod_amd.utils import ops  # noqa: E402

HBM_ROOF = 6.3e12  # achievable bytes / s
SHAPE, FRAMES, SLICE, OVERLAP, IMGSZ, BATCH, NC = (2160, 3840), 4, 640, 0.2, 640, 32, 10


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


def synthetic_chunks(plan, A, dev, seed=0, n_cand=300):
    g = torch.Generator(device=dev).manual_seed(seed)
    ys = []
    for lo, hi in plan.chunks(BATCH):
        n = hi - lo
        y = torch.empty((n, 4 + NC, A), device=dev)
        y[:, 0:2] = torch.rand((n, 2, A), generator=g, device=dev) * IMGSZ
        y[:, 2:4] = 8 + 32 * torch.rand((n, 2, A), generator=g, device=dev)
        y[:, 4:] = torch.rand((n, NC, A), generator=g, device=dev) * 0.2
        pos = torch.rand((n, A), generator=g, device=dev).topk(n_cand, dim=1).indices
        y[:, 4].scatter_(1, pos, 0.25 + 0.75 * torch.rand((n, n_cand), generator=g, device=dev))
        ys.append(y)
    return ys


def torch_merge(ys, plan, merged, A, cut_margin):
    """The merge with torch ops: per tile a slice of y, the arithmetic, the mask and a copy into merged."""
    lo = 0
    for y in ys:
        for src, f, k, gain, px, py, ox, oy, tw, th, (il, ir, it, ib) in plan.merge_rows(lo, lo + y.shape[0]):
            dst = merged[f, :, k * A:(k + 1) * A]
            if src < 0:
                dst.zero_()
                continue
            t = y[src]
            bx, by, bw, bh = (t[0] - px) / gain, (t[1] - py) / gain, t[2] / gain, t[3] / gain
            dst[0], dst[1], dst[2], dst[3] = bx + ox, by + oy, bw, bh
            cut = None
            if cut_margin is not None and cut_margin >= 0:
                for on, m in ((il, bx - 0.5 * bw <= cut_margin), (ir, bx + 0.5 * bw >= tw - cut_margin),
                              (it, by - 0.5 * bh <= cut_margin), (ib, by + 0.5 * bh >= th - cut_margin)):
                    if on:
                        cut = m if cut is None else cut | m
            if cut is None:
                dst[4:] = t[4:]
            else:
                torch.where(cut[None], t.new_zeros(()), t[4:], out=dst[4:])
        lo += y.shape[0]
    return merged


def bench_merge(dev, iters):
    sp = SlicedPredictor(torch.nn.Linear(1, 1).to(dev), slice=SLICE, overlap=OVERLAP, full_frame=True, batch=BATCH,
                         imgsz=IMGSZ)
    plan = sp.plan([SHAPE] * FRAMES)
    A = sum((IMGSZ // s) ** 2 for s in (4, 8, 16, 32))
    ys = synthetic_chunks(plan, A, dev)
    merged = torch.empty((FRAMES, 4 + NC, plan.S * A), device=dev)
    other = torch.empty_like(merged)
    lib = _hip.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    res = []
    for cm in (None, 2.0):
        sp.cut_margin = cm
        # prebuilt descriptors for the kernel-only timing: the wrapper's own, captured from one call per chunk
        descs, lo = [], 0
        for y in ys:
            rows = plan.merge_rows(lo, lo + y.shape[0])
            d = np.zeros((len(rows), 16), dtype=np.int32)
            fl = d.view(np.float32)
            for i, r in enumerate(rows):
                d[i, :3] = r[:3]
                d[i, 3] = sum(1 << b for b in range(4) if r[10][b])
                fl[i, 4:11] = [float(v) for v in r[3:10]]
            descs.append((torch.from_numpy(d).to(dev), len(rows)))
            lo += y.shape[0]

        def kernel():
            for y, (d, nr) in zip(ys, descs):
                rc = lib.yolosod_tile_merge(y.data_ptr(), y.shape[0], NC, A, d.data_ptr(), nr, merged.data_ptr(), FRAMES,
                                            plan.S, -1.0 if cm is None else cm, st)
                assert rc == 0

        def wrapper():
            lo = 0
            for y in ys:
                _hip.tile_merge(y, plan.merge_rows(lo, lo + y.shape[0]), merged, A, cm)
                lo += y.shape[0]

        kernel()
        a = merged.clone()
        wrapper()
        assert torch.equal(a, merged), "prebuilt descriptors differ from the wrapper's"
        torch_merge(ys, plan, other, A, cm)
        same = bool(torch.equal(other, merged))
        diff = float((other - merged).abs().max())
        runs = twice({"kernel": (kernel, 1), "wrapper": (wrapper, 1),
                      "torch": (lambda: torch_merge(ys, plan, other, A, cm), 4)}, iters)
        t_k, t_w, t_t = (sum(v) / 2 for v in (runs["kernel"], runs["wrapper"], runs["torch"]))
        byt = sum(y.numel() for y in ys) * 4 + merged.numel() * 4
        r = dict(case="merge", cut_margin=cm, frames=FRAMES, shape=list(SHAPE), tiles=len(plan), S=plan.S, A=A, nc=NC,
                 calls=len(ys), merged_bytes=merged.numel() * 4, bytes=byt, kernel_ms=t_k, wrapper_ms=t_w, torch_ms=t_t,
                 runs_ms=runs, speedup_vs_torch=t_t / t_w, hbm_roof_fraction=byt / HBM_ROOF / (t_k * 1e-3),
                 torch_equals_fused=same, max_abs_diff_vs_torch=diff)
        print(json.dumps(r), flush=True)
        res.append(r)
    # NMS on the merged tensor at this load
    nms = lambda: ops.non_max_suppression_padded(merged, 0.25, 0.7, max_det=300, max_wh=7680, in_place=False)  # noqa: E731
    counts = nms()[1]
    cand = int((merged[:, 4:].amax(1) > 0.25).sum()) // FRAMES
    runs = twice({"nms": (nms, 1)}, iters)
    r = dict(case="nms_on_merged", candidates_per_frame=cand, kept=counts.tolist(), nms_ms=sum(runs["nms"]) / 2,
             runs_ms=runs)
    print(json.dumps(r), flush=True)
    res.append(r)
    return res


def composed_step(dp, frames, plan, nc):
    """Sliced inference on DetectionPredictor's public interface and torch ops (no SlicedPredictor, no tile_merge)."""
    F, D, S = len(frames), dp.max_det, plan.S
    pred = torch.zeros((F, 4 + nc, S * D), device=frames[0].device)
    for lo, hi in plan.chunks(BATCH):
        tiles = []
        for f, k in plan.order[lo:hi]:
            y0, x0, y1, x1 = plan.slots[f][k].rect
            tiles.append(frames[f][y0:y1, x0:x1])
        out, counts, _ = dp.predict_padded(tiles)  # boxes in each tile's own pixels, clipped to the tile
        off = torch.tensor([[plan.slots[f][k].rect[1], plan.slots[f][k].rect[0]] for f, k in plan.order[lo:hi]],
                           dtype=torch.float32).pin_memory().to(out.device, non_blocking=True)
        valid = torch.arange(D, device=out.device)[None] < counts[:, None]
        xy = (out[..., 0:2] + out[..., 2:4]) / 2 + off[:, None]
        wh = out[..., 2:4] - out[..., 0:2]
        conf = torch.where(valid, out[..., 4], out.new_zeros(()))
        cls = out[..., 5].long().clamp_(0, nc - 1)
        for i, (f, k) in enumerate(plan.order[lo:hi]):
            dst = pred[f, :, k * D:(k + 1) * D]
            dst[0:2] = xy[i].T
            dst[2:4] = wh[i].T
            dst[4:].scatter_(0, cls[i][None], conf[i][None])
    out, counts, index = ops.non_max_suppression_padded(pred, dp.conf, dp.iou, max_det=D, max_wh=7680, in_place=False)
    geom = torch.tensor([[1.0, 0.0, 0.0, w, h] for h, w in plan.shapes]).pin_memory().to(out.device, non_blocking=True)
    _hip.scale_boxes_padded(out, counts, geom)
    return out, counts, index


def bench_step(dev, iters):
    from yolosod_amd.nn.tasks import build_model
    model = build_model("yolov12-sod-fusion-v5-simple.yaml", seed=0, device=dev)
    nc = int(model.yaml["nc"]) if hasattr(model, "yaml") else NC
    sp = SlicedPredictor(model, slice=SLICE, overlap=OVERLAP, full_frame=True, batch=BATCH, conf=0.25, iou=0.7,
                         imgsz=IMGSZ)
    dp = DetectionPredictor(model, conf=0.25, iou=0.7, imgsz=IMGSZ, rect=False)
    frames = [torch.randint(0, 256, (*SHAPE, 3), dtype=torch.uint8, device=dev,
                            generator=torch.Generator(device=dev).manual_seed(i)) for i in range(FRAMES)]
    plan = sp.plan([SHAPE] * FRAMES)
    with torch.inference_mode():
        ys = sp.forward_tiles(frames, plan)
        merged = sp.merge(ys, plan)
        runs = twice({"sliced_step": (lambda: sp.predict_padded(frames), 1),
                      "composed_step": (lambda: composed_step(dp, frames, plan, nc), 1),
                      "forward_tiles": (lambda: sp.forward_tiles(frames, plan), 1),
                      "merge": (lambda: sp.merge(ys, plan), 1),
                      "postprocess": (lambda: sp.postprocess(merged, plan), 1)}, iters)
    m = {k: sum(v) / 2 for k, v in runs.items()}
    flagged = bool(_hip.split_range_flag(reset=True, device=dev))
    r = dict(case="step", frames=FRAMES, shape=list(SHAPE), tiles=len(plan), calls=len(ys), A=int(ys[0].shape[2]), nc=nc,
             conf=0.25, sliced_step_ms=m["sliced_step"], composed_step_ms=m["composed_step"],
             speedup_vs_composed=m["composed_step"] / m["sliced_step"], forward_tiles_ms=m["forward_tiles"],
             merge_ms=m["merge"], postprocess_ms=m["postprocess"],
             merge_plus_nms_share=(m["merge"] + m["postprocess"]) / m["sliced_step"],
             frames_per_s=FRAMES / (m["sliced_step"] * 1e-3), split_range_flagged=flagged, runs_ms=runs)
    print(json.dumps(r), flush=True)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sliced: needs a GPU")
    dev = torch.device("cuda", 0)
    with torch.inference_mode():
        res = bench_merge(dev, a.iters)
    if not a.skip_step:
        res += bench_step(dev, max(2, a.iters // 4))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": a.iters, "results": res},
                                          indent=1) + "\n")


if __name__ == "__main__":
    main()
