"""Motion regions at b64 1080p (profiles/motion_blobs_b64.json), one process, alternating arms:
  * ops.motion_blobs alone, 64 cameras, on the grids of 1080 x 1920 at cell 16 (68 x 120) and
    cell 8 (135 x 240), max_blobs 16, 8-connectivity, for three masks -- a sparse scene (five
    rectangles per camera), random cells at density 0.5, a one-cell-wide serpentine over half
    the grid -- HIP events around 10 back-to-back launches; in the same rounds ops.frame_watch
    on NV12 noise frames of the same size and cell, and a device-to-device ``copy_`` of the
    labels tensor;
  * the YOLOv8n b64 tracked, watched edge step p50 from 1080p NV12 (engine.measure_latency, one
    hipGraph) with and without regions, same detector object, same conv tiles.
Usage: python tools/motion_blobs_probe.py [out.json] [--kernel-only]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, HS, WS, REPS, ROUNDS = 64, 1080, 1920, 10, 15
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else "bench_outputs/motion_blobs_measure.json"
res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame_hw": [HS, WS],
       "max_blobs": 16, "connectivity": 8, "launches_per_sample": REPS, "rounds": ROUNDS}


def dump():
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


def ev_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def masks(gh, gw):
    g = torch.Generator().manual_seed(0)
    sparse = torch.zeros(B, gh, gw, dtype=torch.uint8)
    for n in range(B):
        for _ in range(5):
            h, w = (int(torch.randint(2, gh // 6, (1,), generator=g)),
                    int(torch.randint(2, gw // 8, (1,), generator=g)))
            y, x = (int(torch.randint(0, gh - h, (1,), generator=g)),
                    int(torch.randint(0, gw - w, (1,), generator=g)))
            sparse[n, y:y + h, x:x + w] = 1
    snake = torch.zeros(B, gh, gw, dtype=torch.uint8)
    snake[:, 0::2] = 1
    snake[:, 1::4, gw - 1] = 1
    snake[:, 3::4, 0] = 1
    rand = (torch.rand(B, gh, gw, generator=g) < 0.5).to(torch.uint8)
    return {"sparse": sparse, "random50": rand, "serpentine": snake}


arms = {}
for cell in (16, 8):
    reg = ops.MotionRegions(B, (HS, WS), cell, device="cuda")
    gh, gw = reg.grid
    a = {"regions": reg, "masks": {k: v.cuda() for k, v in masks(gh, gw).items()},
         "det": torch.empty(B, 16, 6, device="cuda"),
         "count": torch.empty(B, dtype=torch.int32, device="cuda"),
         "labels": torch.empty(B, gh, gw, dtype=torch.int32, device="cuda"),
         "labels2": torch.empty(B, gh, gw, dtype=torch.int32, device="cuda"),
         "frames": [torch.randint(0, 256, (B, HS * 3 // 2, WS), dtype=torch.uint8, device="cuda")
                    for _ in range(3)],
         "state": ops.WatchState(B, (HS, WS), cell=cell, device="cuda"),
         "stats": torch.empty(B, 16, dtype=torch.int32, device="cuda"),
         "mask": torch.empty(B, gh, gw, dtype=torch.uint8, device="cuda")}
    arms[cell] = a


def blobs(cell, name):
    a = arms[cell]
    for _ in range(REPS):
        ops.motion_blobs(a["masks"][name], a["regions"], out_det=a["det"], out_count=a["count"],
                         out_labels=a["labels"])


def watch(cell, _):
    a = arms[cell]
    for i in range(REPS):
        ops.frame_watch(a["frames"][i % 3], a["state"], src_format="nv12", out_stats=a["stats"],
                        out_mask=a["mask"])


def copy(cell, _):
    a = arms[cell]
    for _ in range(REPS):
        a["labels2"].copy_(a["labels"])


runs = [(blobs, c, k) for c in arms for k in ("sparse", "random50", "serpentine")]
runs += [(f, c, f.__name__) for c in arms for f in (watch, copy)]
for f, c, k in runs:  # warm: code objects, primed states
    f(c, k)
torch.cuda.synchronize()
t = {(c, k): [] for _, c, k in runs}
for _ in range(ROUNDS):  # alternating arms
    for f, c, k in runs:
        t[(c, k)].append(ev_ms(lambda: f(c, k)) / REPS)
res["kernel"] = {}
for cell in arms:
    r = {"grid": list(arms[cell]["regions"].grid)}
    for (c, k), v in t.items():
        if c == cell:
            name = {"watch": "frame_watch_nv12", "copy": "labels_copy"}.get(k, k)
            r[name] = {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5),
                       "ms_max": round(max(v), 5)}
    for k in ("sparse", "random50", "serpentine"):  # what the kernel found, for the record
        blobs(cell, k)
        r[k]["regions_mean"] = round(float(arms[cell]["count"].float().mean()), 2)
    r["serpentine_over_sparse"] = round(r["serpentine"]["ms_median"] / r["sparse"]["ms_median"], 2)
    res["kernel"][f"cell{cell}"] = r
    print(cell, r, flush=True)
dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)
arms.clear()
torch.cuda.empty_cache()

from kvedge_amd.models.tracking import KvTracked  # noqa: E402
from kvedge_amd.models.watching import KvWatched  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n  # noqa: E402

# a low threshold, so that random-init weights keep boxes
yolo = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001, max_det=300)
kw = dict(device="cuda", seed=0, frame_hw=(HS, WS), frame_format="nv12")
watched = InferenceEngine(KvWatched(KvTracked(yolo, B), B, frame_hw=(HS, WS), cell=16), B, 640,
                          **kw)
watched.prepare(warmup=2, autotune=True)
regions = InferenceEngine(
    KvWatched(KvTracked(yolo, B), B, frame_hw=(HS, WS), cell=16,
              regions=ops.MotionRegions(B, (HS, WS), 16, device="cuda")), B, 640, **kw)
regions.prepare(warmup=2, autotune=False)
eng = {"watched": watched, "regions": regions}
for e in eng.values():
    for _ in range(20):
        e.run()
p = {k: [] for k in eng}
for _ in range(5):  # alternating arms
    for k, e in eng.items():
        p[k].append(e.measure_latency(100).percentile(50))
torch.cuda.synchronize()
res["step"] = {"source": "synthetic NV12 1080 x 1920 noise, generated inside the step",
               "regions_mean": round(float(regions.outputs[-3].float().mean()), 2)}
for k, v in p.items():
    res["step"][f"p50_ms_{k}_rounds"] = [round(x, 4) for x in v]
    res["step"][f"p50_ms_{k}"] = round(statistics.median(v), 4)
d = res["step"]["p50_ms_regions"] - res["step"]["p50_ms_watched"]
res["step"]["regions_minus_watched_ms"] = round(d, 4)
res["step"]["regions_over_watched_pct"] = round(100.0 * d / res["step"]["p50_ms_watched"], 2)
print("step", res["step"], flush=True)
dump()
print("done", flush=True)
