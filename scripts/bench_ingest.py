"""Times the fused raw-frame ingest (yolosod_letterbox_ingest, csrc/ingest.hip) against the same work written with
torch ops on the same GPU, and yolosod_scale_boxes against a per-image loop over utils.ops.scale_boxes. GPU only.

Cases (batch 32, fp32 and bf16 output):
  a  32 frames of 1080 x 1920 onto the 384 x 640 minimal rectangle
  b  8 each of 1080 x 1920, 765 x 1360, 1500 x 2000 and 640 x 640 onto 640 x 640
Each case keeps enough copies of its batch that a timed iteration never re-reads frames still in the 256 MiB Infinity
Cache (the copies are used in rotation). Times are HIP events on the stream over at least ``--iters`` iterations and
0.3 s after a warm-up, each taken twice. "kernel" = the C-ABI launch on a prebuilt descriptor; "wrapper" =
_hip.letterbox_ingest (descriptor built and copied per call); "torch" = per frame permute / flip / float,
F.interpolate bilinear, F.pad 114, / 255, then stack (and the cast for bf16). Bytes for the share of the HBM roof: the
source rows the resize touches plus the output.

  python scripts/bench_ingest.py [--iters 50] [--out FILE.json]"""
import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402
from yolosod_amd.data.augment import LetterBox  # noqa: E402
from yolosod_amd.utils import ops  # noqa: E402

HBM_ROOF = 6.3e12  # achievable bytes / s
STEP_MS = 9.6      # n640 fp32 step at bs 32 (BENCH_r06.json)


def timeit(fn, iters, warmup=5, min_ms=300.0):
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


def rows_touched(n, m):
    """Source indices the integer bilinear map of extent n -> m reads (csrc/ingest.hip's axis map)."""
    seen = set()
    for d in range(m):
        num, den = (2 * d + 1) * n - m, 2 * m
        s, a = (0, 0) if num < 0 else (num // den, ((num % den) * 2048 + m) // den)
        if s >= n - 1:
            s, a = n - 1, 0
        seen.add(s)
        if a:
            seen.add(min(s + 1, n - 1))
    return len(seen)


def torch_ingest(frames, geoms, dtype):
    xs = []
    for f, (nh, nw, top, left, oh, ow) in zip(frames, geoms):
        x = f.permute(2, 0, 1).flip(0)[None].float()
        if (nh, nw) != tuple(f.shape[:2]):
            x = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False)
        x = F.pad(x, (left, ow - nw - left, top, oh - nh - top), value=114.0)
        xs.append(x[0] / 255)
    return torch.stack(xs).to(dtype)


def bench_case(name, shapes, imgsz, auto, dev, iters):
    lb = LetterBox(imgsz, auto=auto)
    geoms = [lb.geometry(s) for s in shapes]
    canvas = geoms[0][4:]
    B = len(shapes)
    src_bytes = sum(3 * h * w for h, w in shapes)
    touched = sum(rows_touched(h, g[0]) * 3 * w for (h, w), g in zip(shapes, geoms))
    copies = max(2, -(-2 * 256 * 2 ** 20 // touched))  # a rotation reads >= 512 MiB of source rows
    sets = [[torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev) for h, w in shapes] for _ in range(copies)]
    lib = _hip.load_library()
    res = []
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.empty((B, 3, *canvas), dtype=dtype, device=dev)
        descs = [torch.tensor([[t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), *g[:4]] for t, g in zip(fs, geoms)],
                              dtype=torch.int64).to(dev) for fs in sets]
        st = torch.cuda.current_stream(dev).cuda_stream

        def kernel(i):
            rc = lib.yolosod_letterbox_ingest(descs[i % copies].data_ptr(), B, out.data_ptr(), out.stride(0), canvas[0],
                                              canvas[1], int(dtype == torch.bfloat16), 114, st)
            assert rc == 0

        # each timing twice, alternating, to show the spread; the figures reported are the means
        runs = {"kernel": [], "wrapper": [], "torch": []}
        for _ in range(2):
            runs["kernel"].append(timeit(kernel, iters))
            runs["wrapper"].append(timeit(lambda i: _hip.letterbox_ingest(sets[i % copies], canvas, geoms, dtype,
                                                                          out=out), iters))
            runs["torch"].append(timeit(lambda i: torch_ingest(sets[i % copies], geoms, dtype), max(5, iters // 5),
                                        warmup=2))
        t_k, t_w, t_t = (sum(v) / len(v) for v in (runs["kernel"], runs["wrapper"], runs["torch"]))
        err = float((_hip.letterbox_ingest(sets[0], canvas, geoms, torch.float32)
                     - torch_ingest(sets[0], geoms, torch.float32)).abs().max()) * 255
        byt = touched + out.numel() * out.element_size()
        r = dict(case=name, dtype=str(dtype).split(".")[-1], batch=B, canvas=list(canvas), copies=copies,
                 kernel_ms=t_k, wrapper_ms=t_w, torch_ms=t_t, runs_ms=runs, speedup_vs_torch=t_t / t_w, bytes=byt,
                 source_bytes_touched=touched, source_bytes_total=src_bytes, hbm_roof_fraction=byt / HBM_ROOF / (t_k * 1e-3),
                 step_share_fused=t_w / STEP_MS, step_share_torch=t_t / STEP_MS, max_abs_diff_vs_torch_grey_levels=err)
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


def bench_scale_boxes(dev, iters):
    B, D = 32, 300
    g = torch.Generator().manual_seed(0)
    det0 = (torch.rand(B, D, 6, generator=g) * 700 - 30).to(dev)
    counts = torch.randint(0, D + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    shapes = ([(1080, 1920), (765, 1360), (1500, 2000), (640, 640)] * 8)[:B]
    rows = []
    for h0, w0 in shapes:
        gain = min(640 / h0, 640 / w0)
        rows.append([gain, round((640 - w0 * gain) / 2 - 0.1), round((640 - h0 * gain) / 2 - 0.1), w0, h0])
    geom = torch.tensor(rows, dtype=torch.float64).float().to(dev)
    det = det0.clone()

    def loop(i):
        n = counts.tolist()  # the loop needs the counts on the host
        for b in range(B):
            ops.scale_boxes((640, 640), det[b, :n[b], :4], shapes[b])

    t_f = timeit(lambda i: _hip.scale_boxes_padded(det, counts, geom), iters)
    t_l = timeit(loop, max(5, iters // 5), warmup=2)
    r = dict(case="scale_boxes", batch=B, max_det=D, fused_ms=t_f, torch_loop_ms=t_l, speedup=t_l / t_f,
             step_share_fused=t_f / STEP_MS, step_share_torch=t_l / STEP_MS)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest: needs a GPU")
    dev = torch.device("cuda")
    res = []
    with torch.inference_mode():
        res += bench_case("a_1080p_rect", [(1080, 1920)] * 32, (640, 640), True, dev, a.iters)
        res += bench_case("b_mixed_square", [(1080, 1920), (765, 1360), (1500, 2000), (640, 640)] * 8, (640, 640), False,
                          dev, a.iters)
        res.append(bench_scale_boxes(dev, a.iters))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": a.iters, "results": res},
                                          indent=1) + "\n")


if __name__ == "__main__":
    main()
