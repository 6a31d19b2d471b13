"""Times the fused NV12 ingest (yolosod_letterbox_ingest_nv12, csrc/ingest_nv12.hip) against what a user without it
writes, and against the BGR ingest as the yardstick for the kernel itself. GPU only.

Cases (batch 32, fp32 and bf16 output), those of scripts/bench_ingest.py with even sizes:
  a  32 surfaces of 1080 x 1920 onto the 384 x 640 minimal rectangle
  b  8 each of 1080 x 1920, 764 x 1360, 1500 x 2000 and 640 x 640 onto 640 x 640
Three routes on the same surfaces in one process:
  1  the fused NV12 ingest: "nv12_kernel" = the C-ABI launch on a prebuilt descriptor, "nv12_wrapper" =
     _hip.letterbox_ingest_nv12 (descriptor built and copied per call)
  2  "torch_then_bgr": per frame NV12 -> uint8 BGR with torch ops on the GPU (chroma repeat_interleave, the 3 x 3 matrix,
     clamp, to(uint8), stack; written in int32 with the project's coefficients so that the result is bit-equal), then
     _hip.letterbox_ingest on the converted frames
  3  the BGR ingest on frames converted beforehand: "bgr_kernel" and "bgr_wrapper"
The three routes' tensors are compared with torch.equal before anything is timed; a difference ends the run.

Each case keeps enough copies of its batch that a timed iteration never re-reads surfaces still in the 256 MiB Infinity
Cache (the copies are used in rotation). Times are HIP events on the stream over at least ``--iters`` iterations and
0.3 s after a warm-up, each taken twice, alternating. Bytes for the share of the HBM roof: the source rows the resize
touches (Y rows and the chroma rows under them; 3-byte rows for BGR) plus the output.

  python scripts/bench_ingest_nv12.py [--iters 50] [--out FILE.json]"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import yolosod_import  # noqa: E402,F401
from yolosod_amd import _hip  # noqa: E402
from yolosod_amd.data import NV12_COEF, NV12_MATRICES, NV12Frame  # noqa: E402
from yolosod_amd.data.augment import LetterBox  # noqa: E402

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
    """Source indices the integer bilinear map of extent n -> m reads (the kernels' axis map)."""
    seen = set()
    for d in range(m):
        num, den = (2 * d + 1) * n - m, 2 * m
        s, a = (0, 0) if num < 0 else (num // den, ((num % den) * 2048 + m) // den)
        if s >= n - 1:
            s, a = n - 1, 0
        seen.add(s)
        if a:
            seen.add(min(s + 1, n - 1))
    return seen


def torch_nv12_to_bgr(f):
    """uint8 [h, w, 3] BGR of an NV12Frame with torch ops, in int32 with the project's coefficients."""
    yoff, cy, cvr, cug, cvg, cub = NV12_COEF[f.matrix]
    c = f.uv.repeat_interleave(2, 0).repeat_interleave(2, 1).to(torch.int32) - 128
    u, v = c[..., 0], c[..., 1]
    y = (f.y.to(torch.int32) - yoff).clamp_(min=0) * cy + (1 << 19)
    chans = [(y + cub * u) >> 20, (y + cvg * v + cug * u) >> 20, (y + cvr * v) >> 20]
    return torch.stack([t.clamp_(0, 255) for t in chans], -1).to(torch.uint8)


def bench_case(name, shapes, imgsz, auto, dev, iters):
    lb = LetterBox(imgsz, auto=auto)
    geoms = [lb.geometry(s) for s in shapes]
    canvas = geoms[0][4:]
    B = len(shapes)
    touched_nv12 = touched_bgr = 0
    for (h, w), g in zip(shapes, geoms):
        rows = rows_touched(h, g[0])
        touched_nv12 += len(rows) * w + len({r >> 1 for r in rows}) * w
        touched_bgr += len(rows) * 3 * w
    copies = max(2, -(-2 * 256 * 2 ** 20 // touched_nv12))  # a rotation reads >= 512 MiB of source rows
    sets = [[NV12Frame(torch.randint(0, 256, (h, w), dtype=torch.uint8, device=dev),
                       torch.randint(0, 256, (h // 2, w // 2, 2), dtype=torch.uint8, device=dev),
                       NV12_MATRICES[(k + i) % 4]) for i, (h, w) in enumerate(shapes)] for k in range(copies)]
    bgr_sets = [[torch_nv12_to_bgr(f) for f in fs] for fs in sets]
    lib = _hip.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    res = []
    for dtype in (torch.float32, torch.bfloat16):
        bf = int(dtype == torch.bfloat16)
        out = torch.empty((B, 3, *canvas), dtype=dtype, device=dev)
        # the three routes give the same bits (every copy of the batch), before anything is timed
        for fs, bs in zip(sets, bgr_sets):
            x1 = _hip.letterbox_ingest_nv12(fs, canvas, geoms, dtype)
            x2 = _hip.letterbox_ingest([torch_nv12_to_bgr(f) for f in fs], canvas, geoms, dtype)
            x3 = _hip.letterbox_ingest(bs, canvas, geoms, dtype)
            if not (torch.equal(x1, x2) and torch.equal(x1, x3)):
                raise SystemExit(f"bench_ingest_nv12: {name} {dtype}: the routes differ")
        d_nv = [torch.tensor([[f.y.data_ptr(), f.uv.data_ptr(), *f.shape, f.y.stride(0), f.uv.stride(0), *g[:4], 0,
                               NV12_MATRICES.index(f.matrix)] for f, g in zip(fs, geoms)], dtype=torch.int64).to(dev)
                for fs in sets]
        d_bgr = [torch.tensor([[t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), *g[:4]] for t, g in zip(bs, geoms)],
                              dtype=torch.int64).to(dev) for bs in bgr_sets]

        def nv12_kernel(i):
            assert lib.yolosod_letterbox_ingest_nv12(d_nv[i % copies].data_ptr(), B, out.data_ptr(), out.stride(0),
                                                     canvas[0], canvas[1], bf, 114, st) == 0

        def bgr_kernel(i):
            assert lib.yolosod_letterbox_ingest(d_bgr[i % copies].data_ptr(), B, out.data_ptr(), out.stride(0),
                                                canvas[0], canvas[1], bf, 114, st) == 0

        routes = {
            "nv12_kernel": (nv12_kernel, iters),
            "bgr_kernel": (bgr_kernel, iters),
            "nv12_wrapper": (lambda i: _hip.letterbox_ingest_nv12(sets[i % copies], canvas, geoms, dtype, out=out), iters),
            "bgr_wrapper": (lambda i: _hip.letterbox_ingest(bgr_sets[i % copies], canvas, geoms, dtype, out=out), iters),
            "torch_then_bgr": (lambda i: _hip.letterbox_ingest([torch_nv12_to_bgr(f) for f in sets[i % copies]], canvas,
                                                               geoms, dtype, out=out), max(5, iters // 5)),
        }
        # each timing twice, alternating, to show the spread; the figures reported are the means
        runs = {k: [] for k in routes}
        for _ in range(2):
            for k, (fn, n) in routes.items():
                runs[k].append(timeit(fn, n, warmup=2 if k == "torch_then_bgr" else 5))
        ms = {k: sum(v) / len(v) for k, v in runs.items()}
        out_bytes = out.numel() * out.element_size()
        r = dict(case=name, dtype=str(dtype).split(".")[-1], batch=B, canvas=list(canvas), copies=copies,
                 routes_bit_equal=True, **{k + "_ms": v for k, v in ms.items()}, runs_ms=runs,
                 wrapper_speedup_vs_torch_then_bgr=ms["torch_then_bgr"] / ms["nv12_wrapper"],
                 nv12_kernel_over_bgr_kernel=ms["nv12_kernel"] / ms["bgr_kernel"],
                 nv12_bytes=touched_nv12 + out_bytes, bgr_bytes=touched_bgr + out_bytes,
                 nv12_source_bytes_touched=touched_nv12, bgr_source_bytes_touched=touched_bgr,
                 nv12_hbm_roof_fraction=(touched_nv12 + out_bytes) / HBM_ROOF / (ms["nv12_kernel"] * 1e-3),
                 bgr_hbm_roof_fraction=(touched_bgr + out_bytes) / HBM_ROOF / (ms["bgr_kernel"] * 1e-3),
                 step_share_nv12_wrapper=ms["nv12_wrapper"] / STEP_MS,
                 step_share_torch_then_bgr=ms["torch_then_bgr"] / STEP_MS)
        print(json.dumps(r), flush=True)
        res.append(r)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest_nv12: needs a GPU")
    dev = torch.device("cuda")
    res = []
    with torch.inference_mode():
        res += bench_case("a_1080p_rect", [(1080, 1920)] * 32, (640, 640), True, dev, a.iters)
        res += bench_case("b_mixed_square", [(1080, 1920), (764, 1360), (1500, 2000), (640, 640)] * 8, (640, 640), False,
                          dev, a.iters)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": a.iters, "results": res},
                                          indent=1) + "\n")


if __name__ == "__main__":
    main()
