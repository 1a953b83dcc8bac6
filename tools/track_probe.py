"""IoU tracker at b64 (profiles/track_b64.json), one process, alternating arms:
  * ops.track_update alone, 64 streams, for count 8 / 50 / 300 and max_tracks 64 / 256, on
    slowly drifting boxes with the state in its steady regime (every slot that can hold a track
    does; the rest of the rows are dropped) -- HIP events around 20 back-to-back launches;
  * the YOLOv8n b64 edge step p50 (engine.measure_latency, one hipGraph) with and without
    tracking, same model object, same conv tiles.
Usage: python tools/track_probe.py [out.json] [--kernel-only]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, MAX_DET, REPS = 64, 300, 20
COUNTS, TRACKS = (8, 50, 300), (64, 256)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else "bench_outputs/track_measure.json"
res = {"device": torch.cuda.get_device_name(0), "batch": B, "max_det": MAX_DET}


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


def boxes(seed):
    """det [B, MAX_DET, 6]: 40 .. 160 px boxes anywhere in a 1920 x 1080 frame."""
    g = torch.Generator().manual_seed(seed)
    wh = 40.0 + 120.0 * torch.rand(B, MAX_DET, 2, generator=g)
    xy = torch.rand(B, MAX_DET, 2, generator=g) * torch.tensor([1760.0, 920.0])
    cls = torch.randint(0, 8, (B, MAX_DET, 1), generator=g).float()
    return torch.cat([xy, xy + wh, torch.rand(B, MAX_DET, 1, generator=g), cls], dim=2)


det = boxes(0).cuda()
drift = torch.zeros(1, 1, 6, device="cuda")
# px per step: every track is re-found and carries a velocity; ~2000 steps in all stay
# inside the 4096 px the tracker's coordinates cover
drift[..., :4] = 0.25
out = torch.empty(B, MAX_DET, dtype=torch.int32, device="cuda")
arms = {}
for T in TRACKS:
    for cnt in COUNTS:
        arms[(T, cnt)] = (ops.TrackState(B, T, "cuda"),
                          torch.full((B,), cnt, dtype=torch.int32, device="cuda"))


def launches(T, cnt):
    st, count = arms[(T, cnt)]
    for _ in range(REPS):
        det.add_(drift)
        ops.track_update(det, count, st, min_hits=3, max_age=30, out=out)


for key in arms:  # warm: code objects, steady state
    launches(*key)
torch.cuda.synchronize()
t = {key: [] for key in arms}
add_ms = []
for _ in range(15):  # alternating arms
    add_ms.append(ev_ms(lambda: [det.add_(drift) for _ in range(REPS)]) / REPS)
    for key in arms:
        t[key].append(ev_ms(lambda: launches(*key)) / REPS)
base = statistics.median(add_ms)  # the box drift's own launch, inside every arm
res["kernel"] = {"drift_launch_ms": round(base, 5)}
for (T, cnt), v in t.items():
    st = arms[(T, cnt)][0]
    res["kernel"][f"T{T}_count{cnt}"] = {
        "ms_median": round(statistics.median(v) - base, 5), "ms_min": round(min(v) - base, 5),
        "ms_max": round(max(v) - base, 5), "active_per_stream": st.active() / B,
        "dropped_total": int(st.dropped.sum())}
    print(T, cnt, res["kernel"][f"T{T}_count{cnt}"], flush=True)
dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)

from kvedge_amd.models.tracking import KvTracked  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n  # noqa: E402

# a low threshold, so that random-init weights keep boxes (the tracker's cost grows with them)
yolo = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001, max_det=MAX_DET)
plain = InferenceEngine(yolo, B, 640, device="cuda", seed=0)
plain.prepare(warmup=2, autotune=True)
eng = {"untracked": plain}
for T in TRACKS:
    e = InferenceEngine(KvTracked(yolo, B, max_tracks=T), B, 640, device="cuda", seed=0)
    eng[f"tracked_T{T}"] = e.prepare(warmup=2, autotune=False)
for e in eng.values():
    for _ in range(20):
        e.run()
p = {k: [] for k in eng}
for _ in range(5):  # alternating arms
    for k, e in eng.items():
        p[k].append(e.measure_latency(100).percentile(50))
torch.cuda.synchronize()
res["step"] = {"detections_mean": round(float(plain.outputs[1].float().mean()), 2)}
for k, v in p.items():
    res["step"][f"p50_ms_{k}_rounds"] = [round(x, 4) for x in v]
    res["step"][f"p50_ms_{k}"] = round(statistics.median(v), 4)
for T in TRACKS:
    d = res["step"][f"p50_ms_tracked_T{T}"] - res["step"]["p50_ms_untracked"]
    res["step"][f"tracked_T{T}_minus_untracked_ms"] = round(d, 4)
    res["step"][f"tracked_T{T}_over_untracked_pct"] = round(
        100.0 * d / res["step"]["p50_ms_untracked"], 2)
print("step", res["step"], flush=True)
dump()
print("done", flush=True)
