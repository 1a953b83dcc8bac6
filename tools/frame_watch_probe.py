"""The frame watch at b64 1080p (profiles/frame_watch_b64_1080p.json), one process, alternating
arms:
  * ops.frame_watch alone, 64 streams of 1080 x 1920, cell 16, for rgb / nv12 and row_step 1 / 2
    -- HIP events around 10 back-to-back steps, rotating over enough source buffers that no
    step finds its frames in the 256 MiB Infinity Cache -- and in the same rounds a
    device-to-device ``copy_`` of exactly the bytes that step must read (the luma rows of NV12,
    every byte of RGB, the sampled rows only), rotating over the same buffers.  The copy moves
    twice the bytes (it also writes them), so a streaming read of this shape should take no
    longer than the copy;
  * the YOLOv8n b64 tracked edge step p50 from 1080p NV12 (engine.measure_latency, one hipGraph)
    with and without the watch, same detector object, same conv tiles.
Usage: python tools/frame_watch_probe.py [out.json] [--kernel-only]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, HS, WS, CELL, REPS = 64, 1080, 1920, 16, 10
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else "bench_outputs/frame_watch_measure.json"
res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame_hw": [HS, WS], "cell": CELL}


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


def sources(fmt):
    """Source buffers of noise, more than 512 MiB of them together."""
    shape = (B, HS * 3 // 2, WS) if fmt == "nv12" else (B, HS, WS, 3)
    n = 3 if fmt == "nv12" else 2
    return [torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda") for _ in range(n)]


arms = {}
for fmt in ("rgb", "nv12"):
    srcs = sources(fmt)
    for rs in (1, 2):
        rows = -(-HS // rs)
        nbytes = B * rows * WS * (1 if fmt == "nv12" else 3)  # what the step must read
        flat = [s.view(-1)[:nbytes] for s in srcs]
        arms[(fmt, rs)] = {
            "srcs": srcs, "flat": flat, "dst": torch.empty(nbytes, dtype=torch.uint8,
                                                           device="cuda"),
            "state": ops.WatchState(B, (HS, WS), cell=CELL, row_step=rs, device="cuda"),
            "stats": torch.empty(B, 16, dtype=torch.int32, device="cuda"),
            "mask": torch.empty(B, -(-HS // CELL), -(-WS // CELL), dtype=torch.uint8,
                                device="cuda"), "bytes": nbytes}


def watch(key):
    a = arms[key]
    for i in range(REPS):
        ops.frame_watch(a["srcs"][i % len(a["srcs"])], a["state"], src_format=key[0],
                        out_stats=a["stats"], out_mask=a["mask"])


def copy(key):
    a = arms[key]
    for i in range(REPS):
        a["dst"].copy_(a["flat"][i % len(a["flat"])])


for key in arms:  # warm: code objects, primed states
    watch(key)
    copy(key)
torch.cuda.synchronize()
t = {(key, k): [] for key in arms for k in ("watch", "copy")}
for _ in range(15):  # alternating arms
    for key in arms:
        t[(key, "watch")].append(ev_ms(lambda: watch(key)) / REPS)
        t[(key, "copy")].append(ev_ms(lambda: copy(key)) / REPS)
res["kernel"] = {}
for key in arms:
    w, c = t[(key, "watch")], t[(key, "copy")]
    mw, mc = statistics.median(w), statistics.median(c)
    res["kernel"][f"{key[0]}_row_step{key[1]}"] = {
        "bytes_read": arms[key]["bytes"],
        "watch_ms_median": round(mw, 5), "watch_ms_min": round(min(w), 5),
        "watch_ms_max": round(max(w), 5),
        "copy_ms_median": round(mc, 5), "copy_ms_min": round(min(c), 5),
        "copy_ms_max": round(max(c), 5),
        "watch_gb_per_s": round(arms[key]["bytes"] / mw / 1e6, 1),
        "watch_over_copy": round(mw / mc, 3)}
    print(key, res["kernel"][f"{key[0]}_row_step{key[1]}"], flush=True)
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
tracked = InferenceEngine(KvTracked(yolo, B), B, 640, **kw)
tracked.prepare(warmup=2, autotune=True)
watched = InferenceEngine(KvWatched(KvTracked(yolo, B), B, frame_hw=(HS, WS), cell=CELL), B, 640,
                          **kw)
watched.prepare(warmup=2, autotune=False)
eng = {"tracked": tracked, "watched": watched}
for e in eng.values():
    for _ in range(20):
        e.run()
p = {k: [] for k in eng}
for _ in range(5):  # alternating arms
    for k, e in eng.items():
        p[k].append(e.measure_latency(100).percentile(50))
torch.cuda.synchronize()
res["step"] = {"source": "synthetic NV12 1080 x 1920 noise, generated inside the step",
               "detections_mean": round(float(tracked.outputs[1].float().mean()), 2)}
for k, v in p.items():
    res["step"][f"p50_ms_{k}_rounds"] = [round(x, 4) for x in v]
    res["step"][f"p50_ms_{k}"] = round(statistics.median(v), 4)
d = res["step"]["p50_ms_watched"] - res["step"]["p50_ms_tracked"]
res["step"]["watched_minus_tracked_ms"] = round(d, 4)
res["step"]["watched_over_tracked_pct"] = round(100.0 * d / res["step"]["p50_ms_tracked"], 2)
print("step", res["step"], flush=True)
dump()
print("done", flush=True)
