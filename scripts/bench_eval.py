"""Times the evaluator's two ways in (engine/validator.py, csrc/eval_match.hip) on one batch of 32 images x 300
val-mode rows with 20, 200 and 1000 labels per image (synthetic crowds of small objects: every row is a label's box
plus jitter, one class in ten flipped). GPU only.

  host    (a) DetectionEvaluator.update on the per-image slices of the batch's tensors: a .cpu() per image, box_iou on
          the CPU, match_predictions per threshold. Wall clock (it syncs); the slices are cut before the clock starts.
  padded  (b) DetectionEvaluator.update_padded on the padded tensors: labels packed and copied, one matching launch,
          the result queued. "kernel": the C-ABI launch alone on labels already on the device, HIP events on the
          stream. "host": wall clock of issuing the calls (the wrapper's Python). "total": wall clock of the calls
          plus the wait for the stream to drain, per call - what a validation loop pays per batch.
  fetch   (c) the one device-to-host copy in get_stats and the per-image arrays made from it, per queued batch (eight
          batches queued), wall clock.

Each figure is taken twice, alternating. Both paths must give the same metrics before anything is timed.

  python scripts/bench_eval.py [--iters 20] [--out FILE.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402
from yolosod_amd.engine.validator import DetectionEvaluator, pack_labels  # noqa: E402
from yolosod_amd.utils.metrics import IOU_THRESHOLDS  # noqa: E402

B, D, NC, IMG = 32, 300, 3, 640.0
LOADS = (20, 200, 1000)


def batch(n_labels, seed):
    """(out [B, D, 6], counts [B] = D, targets) on the host."""
    rng = np.random.default_rng(seed)
    out = np.empty((B, D, 6), dtype=np.float32)
    targets = []
    for b in range(B):
        cls = rng.integers(0, NC, n_labels).astype(np.float32)
        xy = rng.uniform(0, IMG - 40, (n_labels, 2))
        boxes = np.concatenate([xy, xy + rng.uniform(4, 40, (n_labels, 2))], 1).astype(np.float32)
        src = rng.integers(0, n_labels, D)
        dcls = cls[src].copy()
        flip = rng.uniform(size=D) < 0.1
        dcls[flip] = rng.integers(0, NC, int(flip.sum()))
        out[b, :, :4] = boxes[src] + rng.normal(0, 1.5, (D, 4))
        out[b, :, 4] = np.sort(rng.uniform(0.001, 1.0, D))[::-1]
        out[b, :, 5] = dcls
        targets.append((cls, boxes))
    return out, np.full(B, D, dtype=np.int32), targets


def wall(fn, iters, warmup=1, min_ms=200.0):
    """ms per call by the wall clock, the stream drained before the clock stops."""
    for _ in range(warmup):
        fn()
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if ms >= min_ms:
            return ms / iters
        iters = int(iters * min(20.0, 1.25 * min_ms / max(ms, 1e-3))) + 1


def events(fn, iters, warmup=3, min_ms=100.0):
    """ms per call: HIP events on the stream around the window."""
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


def issue(fn, iters, warmup=3):
    """ms per call of host time spent issuing (nothing waits for the GPU inside the window)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return ms / iters


def bench_load(n_labels, dev, iters):
    out_h, counts_h, targets = batch(n_labels, seed=n_labels)
    out, counts = torch.from_numpy(out_h).to(dev), torch.from_numpy(counts_h).to(dev)
    slices = [out[i, :int(counts_h[i])] for i in range(B)]
    host, padded = DetectionEvaluator(NC), DetectionEvaluator(NC)
    host.update(slices, targets)
    padded.update_padded(out, counts, targets)
    same = host.get_stats() == padded.get_stats() and bool((host.metrics.all_ap == padded.metrics.all_ap).all())
    assert same, "update_padded and update disagree"
    labels, off = pack_labels(targets, dev)
    lib = _hip.load_library()
    thr = np.ascontiguousarray(IOU_THRESHOLDS.numpy(), dtype=np.float32)
    tp = torch.empty((B, D, len(thr)), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def kernel():
        rc = lib.yolosod_match_predictions(out.data_ptr(), counts.data_ptr(), B, D, labels.data_ptr(), off.data_ptr(),
                                           thr.ctypes.data, len(thr), tp.data_ptr(), st)
        assert rc == 0

    sink = [DetectionEvaluator(NC)]

    def padded_call():
        if len(sink[0].stats["tp"]) >= 64:  # keep the queue (and the device memory it holds) bounded
            sink[0] = DetectionEvaluator(NC)
        sink[0].update_padded(out, counts, targets)

    def fetch():
        ev = DetectionEvaluator(NC)
        for _ in range(8):
            ev.update_padded(out, counts, targets)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev._fetch()
        return (time.perf_counter() - t0) * 1e3 / 8

    runs = dict(host_update=[], kernel=[], padded_host=[], padded_total=[], fetch_per_batch=[])
    for _ in range(2):
        runs["host_update"].append(wall(lambda: DetectionEvaluator(NC).update(slices, targets), max(1, iters // 10)))
        runs["kernel"].append(events(kernel, iters))
        runs["padded_host"].append(issue(padded_call, iters))
        runs["padded_total"].append(wall(padded_call, iters, warmup=3))
        fetch()
        runs["fetch_per_batch"].append(min(fetch() for _ in range(3)))
    m = {k: sum(v) / 2 for k, v in runs.items()}
    r = dict(case="eval", images=B, rows=D, labels_per_image=n_labels, thresholds=len(thr), tp_true=int(tp.sum()),
             metrics_equal=bool(same), host_update_ms=m["host_update"], kernel_ms=m["kernel"],
             padded_host_ms=m["padded_host"], padded_total_ms=m["padded_total"],
             fetch_per_batch_ms=m["fetch_per_batch"],
             speedup_vs_host=m["host_update"] / m["padded_total"],
             padded_below_host_in_both_runs=all(p < h for p, h in zip(runs["padded_total"], runs["host_update"])),
             runs_ms=runs)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval: needs a GPU")
    dev = torch.device("cuda", 0)
    res = [bench_load(n, dev, a.iters) for n in LOADS]
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": a.iters, "results": res},
                                          indent=1) + "\n")


if __name__ == "__main__":
    main()
