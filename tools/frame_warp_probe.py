"""Per-camera views at b64, 1080x1920 -> 640x640 (profiles/frame_warp_b64_1080p.json), RGB
and NV12, HIP events, warmed, alternating arms in one process on one device:
  (a) ops.frame_resize with the letterbox plan: the yardstick;
  (b) ops.frame_warp with the letterbox mesh, (c) a 2x roi mesh, (d) a fisheye mesh;
  then the tracked YOLOv8n edge step p50 with and without views, same conv tiles.
Usage: python tools/frame_warp_probe.py [out.json]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, HS, WS, D = 64, 1080, 1920, 640
ROUNDS = 20
res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame_hw": [HS, WS], "dst": D,
       "rounds": ROUNDS}
OUT = sys.argv[1] if len(sys.argv) > 1 else "bench_outputs/frame_warp_measure.json"


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


MESHES = {
    "letterbox": {},
    "roi_2x": {"roi": (480, 270, 1440, 810)},
    "fisheye": {"lens": {"fisheye": {"f": 600.0, "cx": 959.5, "cy": 539.5, "fov": 120.0}}},
}


def views_of(kwargs):
    v = ops.CameraViews(B, (HS, WS), (D, D), device="cuda")
    mesh = ops.view_mesh((HS, WS), (D, D), **kwargs)
    for s in range(B):
        v.set(s, mesh)
    return v


plan = ops.letterbox_plan((HS, WS), D)
res["kernel"] = {}
for fmt in ("rgb", "nv12"):
    shape = (B, HS * 3 // 2, WS) if fmt == "nv12" else (B, HS, WS, 3)
    src = torch.empty(*shape, dtype=torch.uint8, device="cuda")
    ops.synth_frames(src.view(B, -1, WS, 3) if fmt == "nv12" else src, 1, 0)
    out = torch.empty(B, D, D, 3, dtype=torch.uint8, device="cuda")
    arms = {"resize_letterbox": lambda: ops.frame_resize(src, plan, out=out, src_format=fmt)}
    for name, kwargs in MESHES.items():
        arms[f"warp_{name}"] = lambda v=views_of(kwargs): ops.frame_warp(src, v, out=out,
                                                                          src_format=fmt)
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(ROUNDS):  # alternating arms
        for k, fn in arms.items():
            times[k].append(ev_ms(fn))
    res["kernel"][fmt] = {k: {"ms_median": round(statistics.median(t), 4),
                              "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
                          for k, t in times.items()}
    print(fmt, res["kernel"][fmt], flush=True)
    dump()
    del src, out, arms
    torch.cuda.empty_cache()

# the tracked YOLOv8n step: letterbox resize against the warp through roi views; tiles tuned
# in arm A and kept by arm B (autotune=False)
from kvedge_amd.models.tracking import KvTracked  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n  # noqa: E402

src = torch.empty(B, HS, WS, 3, dtype=torch.uint8, device="cuda")
ops.synth_frames(src, 1, 0)
engines = []
model = KvTracked(KvYoloV8n.build(seed=0, device="cuda"), B)
for views in (None, views_of(MESHES["roi_2x"])):
    e = InferenceEngine(model, B, D, device="cuda", seed=0, synthetic=False, frame_hw=(HS, WS),
                        views=views)
    e.source_frames.copy_(src)
    e.prepare(warmup=2, autotune=not engines)
    engines.append(e)
a, b = engines
for _ in range(20):
    a.run()
    b.run()
pa, pb = [], []
for _ in range(5):  # alternating arms
    pa.append(a.measure_latency(100).percentile(50))
    pb.append(b.measure_latency(100).percentile(50))
res["step_tracked_yolov8n"] = {
    "p50_ms_resize_rounds": [round(x, 4) for x in pa],
    "p50_ms_views_rounds": [round(x, 4) for x in pb],
    "p50_ms_resize": round(statistics.median(pa), 4),
    "p50_ms_views": round(statistics.median(pb), 4)}
print("step", res["step_tracked_yolov8n"], flush=True)
dump()
print("done", flush=True)
