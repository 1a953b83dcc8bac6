"""Snapshot annotation at b64 (profiles/snapshot_annotate_b64.json): 64 thumbnails of 320 x 180
with boxes in a 1080 x 1920 frame, one process, alternating arms:
  * the kernel (ops.annotate, one launch) with 8 / 50 / 300 rows per camera, privacy off
    (outlines and cls:id labels of the first 32 rows) and on (B = 8, one class of four hidden,
    one polygon), and a device-to-device ``copy_`` of the thumbnails' bytes as the floor this
    project quotes for streaming kernels -- HIP events around 10 back-to-back calls.  The calls
    draw into the same thumbnails again and again: the work depends on the tables, not on the
    pixel values;
  * the YOLOv8n b64 tracked edge step p50 from 1080p NV12 (engine.measure_latency, one hipGraph)
    with bare snapshots and with annotated ones (privacy on), same detector object, same conv
    tiles.
Usage: python tools/annotate_probe.py [out.json] [--kernel-only]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

B, HS, WS, WIDTH, SUB, QUALITY, REPS = 64, 1080, 1920, 320, "420", 75, 10
ROWS = (8, 50, 300)
POLYGON = [(1300, 100), (1900, 100), (1900, 600), (1300, 600)]
args = [a for a in sys.argv[1:] if not a.startswith("--")]

assert torch.cuda.is_available() and ops.load()
OUT = args[0] if args else "bench_outputs/snapshot_annotate_measure.json"
plan = ops.thumbnail_plan((HS, WS), WIDTH)
res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame_hw": [HS, WS],
       "thumbnail_hw": list(plan.dst_hw), "reps_per_event_pair": REPS}


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


def style(privacy: bool) -> "ops.AnnotateStyle":
    s = ops.AnnotateStyle(B, "cuda")
    if privacy:
        s.set_privacy_block(8).set_privacy_classes([0]).set_privacy_polygon(0, POLYGON)
    return s


g = torch.Generator(device="cuda").manual_seed(0)
small = torch.randint(0, 256, (B, *plan.dst_hw, 3), dtype=torch.uint8, device="cuda", generator=g)
small2 = torch.empty_like(small)
# person-sized boxes all over the frame, four classes, ids
c = torch.rand(B, 300, 2, device="cuda", generator=g) * torch.tensor([WS, HS], device="cuda")
sz = (0.03 + 0.12 * torch.rand(B, 300, 2, device="cuda", generator=g)) * torch.tensor(
    [WS, 2.0 * HS], device="cuda")
det300 = torch.zeros(B, 300, 6, device="cuda")
det300[..., 0:2] = c - sz / 2
det300[..., 2:4] = c + sz / 2
det300[..., 5] = (torch.arange(300, device="cuda") % 4).float()
tid300 = torch.arange(B * 300, dtype=torch.int32, device="cuda").view(B, 300)
styles = {"plain": style(False), "privacy": style(True)}
arms = {"copy_thumbnails": lambda: small2.copy_(small)}
for rows in ROWS:
    det, tid = det300[:, :rows].contiguous(), tid300[:, :rows].contiguous()
    count = torch.full((B,), rows, dtype=torch.int32, device="cuda")
    for name, st in styles.items():
        arms[f"annotate_{rows}_{name}"] = (
            lambda det=det, count=count, tid=tid, st=st:
            ops.annotate(small, st, det, count, tid, src_hw=(HS, WS)))


def many(fn):
    for _ in range(REPS):
        fn()


for fn in arms.values():  # warm: code objects
    many(fn)
torch.cuda.synchronize()
t = {k: [] for k in arms}
for _ in range(15):  # alternating arms
    for k, fn in arms.items():
        t[k].append(ev_ms(lambda: many(fn)) / REPS)
res["thumbnail_bytes"] = small.numel()
res["kernel_ms"] = {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5),
                        "max": round(max(v), 5)} for k, v in t.items()}
floor = res["kernel_ms"]["copy_thumbnails"]["median"]
res["over_copy"] = {k: round(v["median"] / floor, 1) for k, v in res["kernel_ms"].items()
                    if k != "copy_thumbnails"}
print(res["kernel_ms"], res["over_copy"], flush=True)
dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)
del small, small2, det300, tid300, arms
torch.cuda.empty_cache()

from kvedge_amd.models.snapshots import KvSnapshots  # noqa: E402
from kvedge_amd.models.tracking import KvTracked  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n  # noqa: E402

# a low threshold, so that random-init weights keep boxes
yolo = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001, max_det=300)
kw = dict(device="cuda", seed=0, frame_hw=(HS, WS), frame_format="nv12")
sk = dict(frame_hw=(HS, WS), width=WIDTH, subsampling=SUB, quality=QUALITY)
bare = InferenceEngine(KvSnapshots(KvTracked(yolo, B), B, **sk), B, 640, **kw)
bare.prepare(warmup=2, autotune=True)
drawn = InferenceEngine(KvSnapshots(KvTracked(yolo, B), B, annotate=styles["privacy"], **sk),
                        B, 640, **kw)
drawn.prepare(warmup=2, autotune=False)
eng = {"snapshots": bare, "annotated": drawn}
for e in eng.values():
    for _ in range(20):
        e.run()
p = {k: [] for k in eng}
for _ in range(5):  # alternating arms
    for k, e in eng.items():
        p[k].append(e.measure_latency(100).percentile(50))
torch.cuda.synchronize()
res["step"] = {"source": "synthetic NV12 1080 x 1920 noise, generated inside the step",
               "rows_per_camera_median": int(drawn.outputs[1].float().median())}
for k, v in p.items():
    res["step"][f"p50_ms_{k}_rounds"] = [round(x, 4) for x in v]
    res["step"][f"p50_ms_{k}"] = round(statistics.median(v), 4)
d = res["step"]["p50_ms_annotated"] - res["step"]["p50_ms_snapshots"]
res["step"]["annotated_minus_snapshots_ms"] = round(d, 4)
res["step"]["annotated_over_snapshots_pct"] = round(100.0 * d / res["step"]["p50_ms_snapshots"], 2)
print("step", res["step"], flush=True)
dump()
print("done", flush=True)
