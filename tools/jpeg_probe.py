"""Camera snapshots at b64 from 1080p (profiles/jpeg_snapshots_b64.json): thumbnail width 320,
4:2:0, quality 75, one process, alternating arms:
  * the thumbnail resize (ops.frame_resize with ops.thumbnail_plan) from RGB and from NV12
    1080 x 1920 frames, the encoder (ops.jpeg_encode: its three launches together) on the
    64 thumbnails, and a device-to-device ``copy_`` of the thumbnails' bytes as the floor this
    project quotes for streaming kernels -- HIP events around 10 back-to-back calls;
  * the YOLOv8n b64 tracked edge step p50 from 1080p NV12 (engine.measure_latency, one hipGraph)
    with and without the snapshots, same detector object, same conv tiles.
The encoder's launches one by one come from a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o jt -- python tools/jpeg_probe.py --trace-only
  python tools/jpeg_probe.py --summarize DIR out.json      (no GPU needed; merges into out.json)
Usage: python tools/jpeg_probe.py [out.json] [--kernel-only]"""
import csv
import glob
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402

B, HS, WS, WIDTH, SUB, QUALITY, REPS = 64, 1080, 1920, 320, "420", 75, 10
args = [a for a in sys.argv[1:] if not a.startswith("--")]
KERNELS = ("jpeg_blocks_kernel", "jpeg_entropy_kernel", "jpeg_pack_kernel", "frame_resize")


def summarize(trace_dir, out):
    """Median / min / max device time of the encoder's kernels and the resize in a trace."""
    path = trace_dir
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[-1]
    durs = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                name = k + ("_nv12" if k == "frame_resize" and "nv12" in r["Kernel_Name"] else "")
                durs.setdefault(name, []).append(
                    (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["trace_us"] = {k: {"calls": len(v), "median": round(statistics.median(v), 2),
                           "min": round(min(v), 2), "max": round(max(v), 2)}
                       for k, v in sorted(durs.items())}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["trace_us"], indent=1))


if "--summarize" in sys.argv:
    summarize(args[0], args[1])
    sys.exit(0)

from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
OUT = args[0] if args else "bench_outputs/jpeg_snapshots_measure.json"
plan = ops.thumbnail_plan((HS, WS), WIDTH)
res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame_hw": [HS, WS],
       "thumbnail_hw": list(plan.dst_hw), "subsampling": SUB, "quality": QUALITY}


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


# camera-like frames: a smooth scene with some texture (noise would be the encoder's worst case
# and nothing a camera delivers)
g = torch.Generator(device="cuda").manual_seed(0)
yy = torch.arange(HS, device="cuda").view(1, HS, 1, 1).float()
xx = torch.arange(WS, device="cuda").view(1, 1, WS, 1).float()
ph = torch.rand(B, 1, 1, 3, device="cuda", generator=g) * 6.28
scene = (127 + 90 * torch.sin(xx / 97 + ph) * torch.cos(yy / 61 + ph)
         + 12 * torch.randn(B, HS, WS, 3, device="cuda", generator=g)).clamp(0, 255)
rgb = scene.to(torch.uint8).contiguous()
del scene
nv12 = torch.randint(0, 256, (B, HS * 3 // 2, WS), dtype=torch.uint8, device="cuda", generator=g)
nv12[:, :HS] = rgb[..., 1]          # the green plane as luma: a scene, not noise
nv12[:, HS:] = 128
enc = ops.JpegEncoder(plan.dst_hw, B, SUB, QUALITY, device="cuda")
small = ops.frame_resize(rgb, plan)
small2 = torch.empty_like(small)
buf = torch.empty(B, enc.max_bytes, dtype=torch.uint8, device="cuda")
length = torch.empty(B, dtype=torch.int32, device="cuda")

arms = {
    "resize_rgb": lambda: ops.frame_resize(rgb, plan, out=small2),
    "resize_nv12": lambda: ops.frame_resize(nv12, plan, out=small2, src_format="nv12"),
    "encode": lambda: ops.jpeg_encode(small, enc, out=buf, lengths=length),
    "copy_thumbnails": lambda: small2.copy_(small),
}


def many(fn):
    for _ in range(REPS):
        fn()


for fn in arms.values():  # warm: code objects
    many(fn)
torch.cuda.synchronize()
if "--trace-only" in sys.argv:
    for _ in range(5):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    print("done", flush=True)
    sys.exit(0)

t = {k: [] for k in arms}
for _ in range(15):  # alternating arms
    for k, fn in arms.items():
        t[k].append(ev_ms(lambda: many(fn)) / REPS)
sizes = length.cpu().tolist()
res["files"] = {"bytes_min": min(sizes), "bytes_median": int(statistics.median(sizes)),
                "bytes_max": max(sizes), "row_bytes": enc.max_bytes,
                "thumbnail_bytes": small.numel()}
res["kernel_ms"] = {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5),
                        "max": round(max(v), 5)} for k, v in t.items()}
res["kernel_ms"]["encode_over_copy"] = round(
    res["kernel_ms"]["encode"]["median"] / res["kernel_ms"]["copy_thumbnails"]["median"], 1)
print(res["files"], res["kernel_ms"], flush=True)
dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)
del rgb, nv12, small, small2, buf
torch.cuda.empty_cache()

from kvedge_amd.models.snapshots import KvSnapshots  # noqa: E402
from kvedge_amd.models.tracking import KvTracked  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n  # noqa: E402

# a low threshold, so that random-init weights keep boxes
yolo = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001, max_det=300)
kw = dict(device="cuda", seed=0, frame_hw=(HS, WS), frame_format="nv12")
tracked = InferenceEngine(KvTracked(yolo, B), B, 640, **kw)
tracked.prepare(warmup=2, autotune=True)
snap = InferenceEngine(KvSnapshots(KvTracked(yolo, B), B, frame_hw=(HS, WS), width=WIDTH,
                                   subsampling=SUB, quality=QUALITY), B, 640, **kw)
snap.prepare(warmup=2, autotune=False)
eng = {"tracked": tracked, "snapshots": snap}
for e in eng.values():
    for _ in range(20):
        e.run()
p = {k: [] for k in eng}
for _ in range(5):  # alternating arms
    for k, e in eng.items():
        p[k].append(e.measure_latency(100).percentile(50))
torch.cuda.synchronize()
res["step"] = {"source": "synthetic NV12 1080 x 1920 noise, generated inside the step (the "
                         "encoder's worst case: every file near its largest)",
               "file_bytes_median": int(snap.outputs[-1].float().median())}
for k, v in p.items():
    res["step"][f"p50_ms_{k}_rounds"] = [round(x, 4) for x in v]
    res["step"][f"p50_ms_{k}"] = round(statistics.median(v), 4)
d = res["step"]["p50_ms_snapshots"] - res["step"]["p50_ms_tracked"]
res["step"]["snapshots_minus_tracked_ms"] = round(d, 4)
res["step"]["snapshots_over_tracked_pct"] = round(100.0 * d / res["step"]["p50_ms_tracked"], 2)
print("step", res["step"], flush=True)
dump()
print("done", flush=True)
