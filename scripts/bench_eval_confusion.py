"""Times the confusion matrix's two ways in (utils/metrics.ConfusionMatrix on the host, csrc/eval_confusion.hip on the
device) on the batch of scripts/bench_eval.py: 32 images x 300 val-mode rows with 20, 200 and 1000 labels per image
(synthetic crowds of small objects in ten classes: three rows in four are a label's box plus jitter, 30 % of those with
another class, the rest clutter). GPU only.

  host_walk   ConfusionMatrix.process_batch per image on the per-image slices of the batch's tensors, a .cpu() per
              image as DetectionEvaluator.update does it. Wall clock (it syncs); the slices are cut before the clock
              starts.
  kernel      the C-ABI launch alone on labels already on the device, HIP events on the stream.
  padded      DetectionEvaluator.update_padded without and with confusion=True, same process, same tensors: "host" the
              wall clock of issuing the calls, "total" the wall clock of the calls plus the wait for the stream to
              drain, per call - what a validation loop pays per batch. "added" is the difference of the two totals.

Each figure is taken twice, alternating. Both paths must give the same matrix before anything is timed (the crowds hold
no exact IoU tie; asserted with the restatement in tests/confusion_ref.py).

It runs from a checkout: the tie check is the test helper tests/confusion_ref.py (the only definition of the closed form;
a second copy here could drift from what the kernel is tested against) and the three timers are scripts/bench_eval.py's,
so both directories go on sys.path below.

  python scripts/bench_eval_confusion.py [--iters 20] [--out FILE.json]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))
import yolosod_import  # noqa: E402,F401
from bench_eval import events, issue, wall  # noqa: E402
from confusion_ref import confusion_batch_ref  # noqa: E402
from yolosod_amd import _hip  # noqa: E402
from yolosod_amd.engine.validator import DetectionEvaluator, pack_labels  # noqa: E402
from yolosod_amd.utils.metrics import ConfusionMatrix  # noqa: E402

B, D, NC, IMG = 32, 300, 10, 640.0
LOADS = (20, 200, 1000)
CONF, IOU = 0.25, 0.45


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
        xy0 = rng.uniform(0, IMG - 40, (D, 2))
        dbox = np.concatenate([xy0, xy0 + rng.uniform(4, 40, (D, 2))], 1)
        dcls = rng.integers(0, NC, D).astype(np.float32)
        on = rng.uniform(size=D) < 0.75
        dbox[on] = (boxes[src] + rng.normal(0, 1.5, (D, 4)))[on]
        right = on & (rng.uniform(size=D) >= 0.3)
        dcls[right] = cls[src][right]
        out[b, :, :4] = dbox
        out[b, :, 4] = np.sort(rng.uniform(0.001, 1.0, D))[::-1]
        out[b, :, 5] = dcls
        targets.append((cls, boxes))
    return out, np.full(B, D, dtype=np.int32), targets


def bench_load(n_labels, dev, iters):
    out_h, counts_h, targets = batch(n_labels, seed=n_labels)
    out, counts = torch.from_numpy(out_h).to(dev), torch.from_numpy(counts_h).to(dev)
    slices = [out[i, :int(counts_h[i])] for i in range(B)]
    host_t = [(torch.from_numpy(c), torch.from_numpy(b)) for c, b in targets]
    ref, ties = confusion_batch_ref(out_h, counts_h, targets, NC, CONF, IOU)
    assert ties == 0, "the batch holds an exact IoU tie"

    def host_walk():
        cm = ConfusionMatrix(NC, CONF, IOU)
        for s, (cls, bbox) in zip(slices, host_t):
            cm.process_batch(s.float().cpu(), bbox, cls)
        return cm

    ev = DetectionEvaluator(NC, confusion=True)
    ev.update_padded(out, counts, targets)
    ev.get_stats()
    same = bool((host_walk().matrix == ref.sum(0)).all() and (ev.confusion_matrix.matrix == ref.sum(0)).all())
    assert same, "the host walk, update_padded and the restatement disagree"
    labels, off = pack_labels(targets, dev)
    lib = _hip.load_library()
    cm = torch.empty((B, NC + 1, NC + 1), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def kernel():
        rc = lib.yolosod_confusion_matrix(out.data_ptr(), counts.data_ptr(), B, D, labels.data_ptr(), off.data_ptr(),
                                          NC, CONF, IOU, cm.data_ptr(), st)
        assert rc == 0

    def padded(confusion):
        sink = [DetectionEvaluator(NC, confusion=confusion)]

        def call():
            if len(sink[0].stats["tp"]) >= 64:  # keep the queue (and the device memory it holds) bounded
                sink[0] = DetectionEvaluator(NC, confusion=confusion)
            sink[0].update_padded(out, counts, targets)
        return call

    plain, with_cm = padded(False), padded(True)
    runs = dict(host_walk=[], kernel=[], padded_host_plain=[], padded_host_confusion=[], padded_total_plain=[],
                padded_total_confusion=[])
    for _ in range(2):
        runs["host_walk"].append(wall(host_walk, max(1, iters // 10)))
        runs["kernel"].append(events(kernel, iters))
        runs["padded_host_plain"].append(issue(plain, iters))
        runs["padded_host_confusion"].append(issue(with_cm, iters))
        runs["padded_total_plain"].append(wall(plain, iters, warmup=3))
        runs["padded_total_confusion"].append(wall(with_cm, iters, warmup=3))
    m = {k: sum(v) / 2 for k, v in runs.items()}
    added = [c - p for c, p in zip(runs["padded_total_confusion"], runs["padded_total_plain"])]
    r = dict(case="eval_confusion", images=B, rows=D, labels_per_image=n_labels, nc=NC, conf=CONF, iou_thres=IOU,
             matched=int(np.trace(ref.sum(0)[:NC, :NC])), matrices_equal=same, host_walk_ms=m["host_walk"],
             kernel_ms=m["kernel"], padded_host_plain_ms=m["padded_host_plain"],
             padded_host_confusion_ms=m["padded_host_confusion"], padded_total_plain_ms=m["padded_total_plain"],
             padded_total_confusion_ms=m["padded_total_confusion"], added_by_confusion_ms=sum(added) / 2,
             added_below_host_walk_in_both_runs=all(a < h for a, h in zip(added, runs["host_walk"])), runs_ms=runs)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_confusion: needs a GPU")
    dev = torch.device("cuda", 0)
    res = [bench_load(n, dev, a.iters) for n in LOADS]
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": a.iters, "results": res},
                                          indent=1) + "\n")


if __name__ == "__main__":
    main()
