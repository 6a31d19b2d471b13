"""Times a ByteTrack update both ways (engine/tracker.py): ByteTracker, one HIP launch for all streams from
device-resident state (csrc/track.hip), against the host path - fetch ``out`` and ``counts`` (the host sync), then
ByteTrackerHost (utils/bytetrack.py: numpy + scipy) on every stream. GPU only.

The setup: 32 streams, 30 frames, about 100 objects per stream on 1920x1080, seeded (tests/bytetrack_ref.random_scene,
one seed per stream; the detections of every frame are on the device before a clock starts).

  device  HIP events around every update launch, after one warm-up pass over the sequence and a reset; the sequence is
          timed ``--passes`` times and a frame's time is the median over the passes. Reported: the median over the
          frames, and the worst frame separately.
  host    wall clock per frame of out.cpu() + counts.cpu() + ByteTrackerHost.update, one pass. Same two figures.

Nothing is asserted about their ratio. ``ids_equal`` says whether both paths gave the same ids on every frame (the
scenes are not certified: a near-tie may legitimately differ).

``--tracker botsort`` times BotSortTracker / BotSortTrackerHost (the XYWH filter and the camera-motion phase, DESIGN
section 35) on the same workload seen through a moving camera: every stream's scene goes through a seeded camera walk
(tests/botsort_ref.camera_scene: translation up to +-12 px, rotation up to 0.5 degrees, scale 1 +- 0.01 per frame) and
every update is given the 32 frame-to-frame warps, on the device before a clock starts (fp64 [32, 2, 3]; the first
frame's are the identity).

It runs from a checkout: the scenes are the test helpers' (tests/bytetrack_ref.py, tests/botsort_ref.py), so that
directory goes on sys.path.

  python scripts/bench_track.py [--tracker bytetrack|botsort] [--passes 5] [--out profiles/track_bench_mi355x.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import yolosod_import  # noqa: E402,F401
from bytetrack_ref import random_scene  # noqa: E402
from yolosod_amd.engine import tracker as trackers  # noqa: E402

B, FRAMES, OBJECTS, W, H, D, T = 32, 30, 100, 1920, 1080, 300, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tracker", choices=("bytetrack", "botsort"), default="bytetrack")
    a = ap.parse_args()
    bot = a.tracker == "botsort"
    if not torch.cuda.is_available():
        raise SystemExit("bench_track: needs a GPU")
    dev = torch.device("cuda", 0)
    if bot:
        from botsort_ref import IDENTITY, camera_scene
        cams = [camera_scene(seed=100 + s, objects=OBJECTS, frames=FRAMES, width=W, height=H, min_side=16, D=D)
                for s in range(B)]
        scenes = [c[0] for c in cams]
        warps = [torch.from_numpy(np.stack([IDENTITY if c[1][f] is None else c[1][f] for c in cams])).to(dev)
                 for f in range(FRAMES)]
        Dev, Host = trackers.BotSortTracker, trackers.BotSortTrackerHost
    else:
        scenes = [random_scene(seed=100 + s, objects=OBJECTS, frames=FRAMES, width=W, height=H, min_side=16, D=D)
                  for s in range(B)]
        warps = None
        Dev, Host = trackers.ByteTracker, trackers.ByteTrackerHost

    def step(t, f, host=False):
        if not bot:
            return t.update(outs[f].cpu(), counts[f].cpu()) if host else t.update(outs[f], counts[f])
        if host:
            return t.update(outs[f].cpu(), counts[f].cpu(), warps=warps[f].cpu())
        return t.update(outs[f], counts[f], warps=warps[f])
    outs = [torch.from_numpy(np.stack([scenes[s][f][0] for s in range(B)])).to(dev) for f in range(FRAMES)]
    counts = [torch.tensor([scenes[s][f][1] for s in range(B)], dtype=torch.int32, device=dev) for f in range(FRAMES)]
    dets = float(np.mean([c.float().mean().item() for c in counts]))

    trk = Dev(streams=B, capacity=T, device=dev)
    dev_ids = []
    for f in range(FRAMES):  # warm-up pass; its results are the ones compared with the host's
        tr = step(trk, f)
        n = tr.counts.cpu().numpy()
        rows = tr.rows.cpu().numpy()
        dev_ids.append([rows[s, :n[s], 4].astype(int).tolist() for s in range(B)])
    live = float(np.mean([len(x) for x in dev_ids[-1]]))
    per_frame = [[] for _ in range(FRAMES)]
    for _ in range(a.passes):
        trk.reset()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(FRAMES)]
        for f in range(FRAMES):
            ev[f][0].record()
            step(trk, f)
            ev[f][1].record()
        torch.cuda.synchronize()
        for f in range(FRAMES):
            per_frame[f].append(ev[f][0].elapsed_time(ev[f][1]))
    dev_ms = [statistics.median(v) for v in per_frame]

    host = Host(streams=B, capacity=T)
    host_ms, same = [], True
    for f in range(FRAMES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr = step(host, f, host=True)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        n = tr.counts.numpy()
        same &= [tr.rows[s, :n[s], 4].numpy().astype(int).tolist() for s in range(B)] == dev_ids[f]
    r = dict(case="track_update", tracker=a.tracker, warps=bool(bot), streams=B, frames=FRAMES,
             objects_per_stream=OBJECTS, frame=[W, H], capacity=T, rows=D,
             detections_per_frame=dets, live_tracks_last_frame=live, passes=a.passes,
             device_update_median_ms=statistics.median(dev_ms), device_update_worst_frame_ms=max(dev_ms),
             device_worst_frame=int(np.argmax(dev_ms)) + 1, host_update_median_ms=statistics.median(host_ms),
             host_update_worst_frame_ms=max(host_ms), host_worst_frame=int(np.argmax(host_ms)) + 1, ids_equal=bool(same),
             overflow=int(trk.overflow.sum().item()), device_frames_ms=dev_ms, host_frames_ms=host_ms)
    print(json.dumps(r), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": [r]}, indent=1) + "\n")


if __name__ == "__main__":
    main()
