"""Merge-NMS (non_max_suppression_padded(merge=True)) at controlled candidate loads, against plain NMS and against the
torch composition a user would write on top of plain NMS (the reference's commented-out block, ops.py:299-309: the
box_iou matrix of the kept rows against the image's candidates, torch.mm with the scores, divide).

(B = 32, 4+nc = 14, A = 34000) predictions from bench.loaded_predictions with 1 000 / 10 000 / 30 000 candidates per
image in 50 / 1000 clusters; predict mode (conf 0.25, single label) and val mode (conf 0.001, multi-label); max_det
300, in_place=False (the predictors' call: the input is left as it is, so every call sees the same tensor). Events on
the stream around windows of at least 0.3 s; every variant's window is taken twice, the variants alternating. Also the
empty workload (no candidates) and, not asserted, mAP50-95 of engine.validator.validate on recipes.synthetic_eval_set
with and without merging.

usage: python scripts/bench_nms_merge.py [--out profiles/nms_merge_bench_mi355x.json] [--quick]"""
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import yolosod_import  # noqa: E402,F401
from yolosod_amd.utils.ops import non_max_suppression_padded, xywh2xyxy  # noqa: E402
from yolosod_amd.utils.metrics import box_iou  # noqa: E402
from bench import loaded_predictions as make_pred  # noqa: E402

IOU, MAX_DET, MAX_WH = 0.7, 300, 7680
SLICED_STEP_MS = 37.2  # one SlicedPredictor step


def torch_merge(pred, conf, multi_label):
    """Plain NMS, then per image the reference comment's merge in torch (fp32, as it is written there)."""
    out, counts, index = non_max_suppression_padded(pred, conf, IOU, multi_label=multi_label, max_det=MAX_DET,
                                                    in_place=False)
    n = counts.tolist()
    for b in range(pred.shape[0]):
        if not n[b]:
            continue
        sc = pred[b, 4:]
        if multi_label:
            j, a = (sc > conf).nonzero(as_tuple=True)
            s = sc[j, a]
        else:
            s, j = sc.max(0)
            a = (s > conf).nonzero(as_tuple=True)[0]
            s, j = s[a], j[a]
        boxes = xywh2xyxy(pred[b, :4, a].T)
        off = j.to(boxes.dtype)[:, None] * MAX_WH
        rows = out[b, :n[b]]
        iou = box_iou(rows[:, :4] + rows[:, 5:6] * MAX_WH, boxes + off) > IOU
        w = iou * s[None]
        rows[:, :4] = torch.mm(w, boxes) / w.sum(1, keepdim=True)
    return out, counts, index


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(variants, min_window_s):
    """{name: [ms, ms]}: per variant two windows of >= min_window_s, the variants alternating."""
    reps = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(5, math.ceil(min_window_s * 1e3 / window(fn, 3)))
    res = {name: [] for name in variants}
    for _ in range(2):
        for name, fn in variants.items():
            res[name].append(round(window(fn, reps[name]), 4))
    return res


class _NmsOnly:
    """predict_padded for engine.validator.validate on ready-made prediction tensors."""

    def __init__(self, merge):
        self.merge = merge

    def predict_padded(self, pred):
        return non_max_suppression_padded(pred, 0.001, IOU, multi_label=True, max_det=MAX_DET, in_place=False,
                                          merge=self.merge)[:3]


def eval_map(dev, copies):
    """mAP50-95 on recipes.synthetic_eval_set: every synthetic detection as ``copies`` candidates (1: as it is; more:
    jittered by N(0, 0.03 side) per coordinate, scores times U(0.7, 1)), through NMS with and without merging."""
    import recipes
    from yolosod_amd.engine.validator import validate
    nc = 6
    gt, preds = recipes.synthetic_eval_set(21, nc=nc)
    rng = np.random.default_rng(3)
    A = max(1, max(len(p) for p in preds) * copies)
    t = np.zeros((len(preds), 4 + nc, A), np.float32)
    for i, p in enumerate(preds):
        for k, r in enumerate(np.repeat(p, copies, 0)):
            box, s = r[:4].astype(np.float64), float(r[4])
            if copies > 1:
                side = np.array([box[2] - box[0], box[3] - box[1]] * 2)
                box = box + rng.normal(0, 0.03, 4) * side
                s *= rng.uniform(0.7, 1.0)
            t[i, :4, k] = [(box[0] + box[2]) / 2, (box[1] + box[3]) / 2, box[2] - box[0], box[3] - box[1]]
            t[i, 4 + int(r[5]), k] = s
    t = torch.from_numpy(t).to(dev)
    res = {}
    for merge in (False, True):
        r = validate(_NmsOnly(merge), [(t, gt)], nc)
        res["merge" if merge else "plain"] = {k: round(float(v), 5) for k, v in r.items() if "mAP" in k}
    return res


def main():
    args = sys.argv[1:]
    out_path = Path(args[args.index("--out") + 1]) if "--out" in args else None
    quick = "--quick" in args
    dev = torch.device("cuda")
    B, A, nc = 32, 34000, 10
    min_w = 0.05 if quick else 0.3
    rows = []
    print(f"{'mode':8s} {'cand/img':>9s} {'clusters':>8s} {'kept':>6s} {'plain ms':>16s} {'merge ms':>16s} "
          f"{'torch ms':>16s} {'added ms':>9s} {'% of NMS':>8s} {'torch/added':>11s}", flush=True)
    modes = (("predict", 0.25, False), ("val", 0.001, True))
    loads = [(0, 50)] + [(n, c) for n in (1000, 10000, 30000) for c in (50, 1000)]
    for mode, conf, ml in modes:
        for n_cand, clusters in loads:
            if n_cand == 0 and mode == "val":
                continue
            pred = make_pred(B, A, nc, n_cand, clusters, conf, 0, dev)
            kw = dict(conf_thres=conf, iou_thres=IOU, multi_label=ml, max_det=MAX_DET, in_place=False)
            variants = {
                "plain": lambda: non_max_suppression_padded(pred, **kw),
                "merge": lambda: non_max_suppression_padded(pred, merge=True, **kw),
                "torch": lambda: torch_merge(pred, conf, ml),
            }
            got = variants["merge"]()
            ref = variants["torch"]()
            n = got[1].tolist()
            # the two agree to fp32 accuracy wherever the composition's rules coincide (its cluster lacks a zero-area
            # row's own candidate, and it sums in fp32)
            err = max((float((got[0][b, :n[b], :4] - ref[0][b, :n[b], :4]).abs().max()) for b in range(B) if n[b]),
                      default=0.0)
            t = measure(variants, min_w)
            p, m, c = (min(t[k]) for k in ("plain", "merge", "torch"))
            added = m - p
            row = dict(mode=mode, candidates=n_cand, clusters=clusters, kept_per_image=round(sum(n) / B, 1),
                       mean_cluster=round(float(got[3].sum()) / max(1, sum(n)), 1), ms=t, added_ms=round(added, 4),
                       added_share_of_nms=round(added / p, 4), added_share_of_sliced_step=round(added / SLICED_STEP_MS, 5),
                       torch_added_ms=round(c - p, 4), max_abs_diff_vs_torch=err)
            rows.append(row)
            print(f"{mode:8s} {n_cand:9d} {clusters:8d} {sum(n) / B:6.1f} {str(t['plain']):>16s} {str(t['merge']):>16s} "
                  f"{str(t['torch']):>16s} {added:9.4f} {100 * added / p:8.1f} {(c - p) / max(added, 1e-6):11.1f}",
                  flush=True)
    maps = {"as_is": eval_map(dev, 1), "six_jittered_copies": eval_map(dev, 6)}
    print("mAP (synthetic_eval_set, not asserted):", json.dumps(maps), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), B=B, A=A, nc=nc, iou=IOU, max_det=MAX_DET, in_place=False,
                  min_window_s=min_w, sliced_step_ms=SLICED_STEP_MS, loads=rows, map_synthetic_eval_set=maps)
    if out_path:
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
