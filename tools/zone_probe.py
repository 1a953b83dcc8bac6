"""Lines and zones at b64 (profiles/zone_b64.json), one process, alternating arms:
  * ops.zone_update alone, 64 streams, T 64, for count 8 / 50 / 300 with the worst-case table
    (8 lines, 8 zones of 8 vertices), and in the same run ops.track_update on the same inputs --
    HIP events around 20 back-to-back launches on slowly drifting boxes, tracker state in its
    steady regime;
  * the YOLOv8n b64 tracked edge step p50 (engine.measure_latency, one hipGraph) with and
    without zones, same model object, same conv tiles.
Usage: python tools/zone_probe.py [out.json] [--kernel-only]"""
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, MAX_DET, T, REPS = 64, 300, 64, 20
COUNTS = (8, 50, 300)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else "bench_outputs/zone_measure.json"
res = {"device": torch.cuda.get_device_name(0), "batch": B, "max_det": MAX_DET, "max_tracks": T}


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


def worst_table(streams, w=1920.0, h=1080.0):
    """8 lines across the frame and 8 eight-vertex zones (octagons around a 4 x 2 grid of
    centres): every slot and every row is tested against 8 lines and 64 edges."""
    zs = ops.ZoneSet(streams, "cuda")
    for i in range(8):
        x = w * (i + 1) / 9
        zs.set_line(None, i, (x, 0.0), (w - x, h))
    for i in range(8):
        cx, cy = w * (2 * (i % 4) + 1) / 8, h * (2 * (i // 4) + 1) / 4
        zs.set_zone(None, i, [(cx + 300.0 * math.cos(a * math.pi / 4),
                               cy + 300.0 * math.sin(a * math.pi / 4)) for a in range(8)])
    return zs


def boxes(seed):
    """det [B, MAX_DET, 6]: 40 .. 160 px boxes in a 1920 x 1080 frame, with room for the drift."""
    g = torch.Generator().manual_seed(seed)
    wh = 40.0 + 120.0 * torch.rand(B, MAX_DET, 2, generator=g)
    xy = torch.rand(B, MAX_DET, 2, generator=g) * torch.tensor([1560.0, 720.0])
    cls = torch.randint(0, 8, (B, MAX_DET, 1), generator=g).float()
    return torch.cat([xy, xy + wh, torch.rand(B, MAX_DET, 1, generator=g), cls], dim=2)


det = boxes(0).cuda()
drift = torch.zeros(1, 1, 6, device="cuda")
drift[..., :4] = 0.0625  # px per launch: every track is re-found, and the ~3200 launches of a
#                          run move the boxes 200 px, across zone edges and lines, not out of frame
ids = torch.empty(B, MAX_DET, dtype=torch.int32, device="cuda")
mask = torch.empty(B, MAX_DET, dtype=torch.int32, device="cuda")
counts = torch.empty(B, 48, dtype=torch.int32, device="cuda")
table = worst_table(B)
arms = {cnt: (ops.TrackState(B, T, "cuda"), ops.ZoneState(B, T, "cuda"),
              torch.full((B,), cnt, dtype=torch.int32, device="cuda")) for cnt in COUNTS}


def launches(cnt, track, zones):
    ts, zs, count = arms[cnt]
    for _ in range(REPS):
        det.add_(drift)
        if track:
            ops.track_update(det, count, ts, min_hits=3, max_age=30, out=ids)
        if zones:
            ops.zone_update(det, count, ts, zs, table, out_mask=mask, out_counts=counts)


for cnt in COUNTS:  # warm: code objects, steady state
    for _ in range(3):
        launches(cnt, True, True)
torch.cuda.synchronize()
kinds = {"track": (True, False), "zones": (False, True), "both": (True, True)}
t = {(cnt, k): [] for cnt in COUNTS for k in kinds}
add_ms = []
for _ in range(15):  # alternating arms
    add_ms.append(ev_ms(lambda: [det.add_(drift) for _ in range(REPS)]) / REPS)
    for key in t:
        t[key].append(ev_ms(lambda: launches(key[0], *kinds[key[1]])) / REPS)
base = statistics.median(add_ms)  # the box drift's own launch, inside every arm
res["kernel"] = {"drift_launch_ms": round(base, 5)}
for (cnt, k), v in t.items():
    ts, zs, _ = arms[cnt]
    res["kernel"][f"count{cnt}_{k}"] = {
        "ms_median": round(statistics.median(v) - base, 5), "ms_min": round(min(v) - base, 5),
        "ms_max": round(max(v) - base, 5)}
    print(cnt, k, res["kernel"][f"count{cnt}_{k}"], flush=True)
for cnt in COUNTS:
    ts, zs, _ = arms[cnt]
    res["kernel"][f"count{cnt}_state"] = {
        "active_per_stream": ts.active() / B,
        "occupancy_per_stream": float(zs.zone_occ.sum()) / B,
        "crossings_total": int(zs.line_fwd.sum() + zs.line_back.sum())}
dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)

from kvedge_amd.models.tracking import KvTracked, KvZoned  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n  # noqa: E402

# a low threshold, so that random-init weights keep boxes (the cost grows with them)
yolo = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001, max_det=MAX_DET)
tracked = InferenceEngine(KvTracked(yolo, B, max_tracks=T), B, 640, device="cuda", seed=0)
tracked.prepare(warmup=2, autotune=True)
zoned_model = KvZoned(KvTracked(yolo, B, max_tracks=T), worst_table(B, 640.0, 640.0))
zoned = InferenceEngine(zoned_model, B, 640, device="cuda", seed=0)
zoned.prepare(warmup=2, autotune=False)
eng = {"tracked": tracked, "zoned": zoned}
for e in eng.values():
    for _ in range(20):
        e.run()
p = {k: [] for k in eng}
for _ in range(5):  # alternating arms
    for k, e in eng.items():
        p[k].append(e.measure_latency(100).percentile(50))
torch.cuda.synchronize()
res["step"] = {"detections_mean": round(float(tracked.outputs[1].float().mean()), 2)}
for k, v in p.items():
    res["step"][f"p50_ms_{k}_rounds"] = [round(x, 4) for x in v]
    res["step"][f"p50_ms_{k}"] = round(statistics.median(v), 4)
d = res["step"]["p50_ms_zoned"] - res["step"]["p50_ms_tracked"]
res["step"]["zoned_minus_tracked_ms"] = round(d, 4)
res["step"]["zoned_over_tracked_pct"] = round(100.0 * d / res["step"]["p50_ms_tracked"], 2)
print("step", res["step"], flush=True)
dump()
print("done", flush=True)
