"""Detect-then-classify cascade at b64, 1080x1920, K 4, D 224 (profiles/roi_crop_b64_1080p.json):
  * ops.roi_crop for two box mixes, small (~64 px) and large (~600 px) windows, per candidate
    band height (destination rows per workgroup), against its bytes-moved floor (destination
    bytes + the distinct source bytes of the windows), HIP events, warmed, alternating arms;
  * the cascade's edge step p50 (engine.measure_latency) against the sum of a YOLOv8n b64 step
    and a ResNet-50 b256 step on the same box, same conv tiles, alternating arms.
Usage: python tools/roi_crop_probe.py [out.json] [--kernel-only]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402
from kvedge_amd.ops import reference  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, HS, WS, K, D, MAX_DET = 64, 1080, 1920, 4, 224, 300
BANDS = (4, 8, 16, 32)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else "bench_outputs/roi_crop_measure.json"
res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame_hw": [HS, WS],
       "crops_per_image": K, "crop_size": D}


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


def box_mix(side, seed):
    """det [B, MAX_DET, 6]: windows of about ``side`` pixels (0.75 .. 1.25 x) anywhere in the
    frame, fractional corners."""
    g = torch.Generator().manual_seed(seed)
    wh = side * (0.75 + 0.5 * torch.rand(B, MAX_DET, 2, generator=g))
    lim = torch.tensor([WS, HS], dtype=torch.float32)
    xy = torch.rand(B, MAX_DET, 2, generator=g) * (lim - wh).clamp_min(1.0)
    return torch.cat([xy, xy + wh, torch.rand(B, MAX_DET, 2, generator=g)], dim=2)


def floor_bytes(det):
    """Destination bytes + distinct source bytes under the K windows of every image."""
    win = reference.roi_windows(det[:, :K], HS, WS)
    src = 0
    for n in range(B):
        seen = torch.zeros(HS, WS, dtype=torch.bool)
        for x0, y0, w, h in win[n].tolist():
            seen[y0:y0 + h, x0:x0 + w] = True
        src += int(seen.sum()) * 3
    return {"dst_bytes": B * K * D * D * 3, "src_bytes_distinct": src,
            "mean_window_px": round(float((win[..., 2] * win[..., 3]).float().mean()), 1)}


src = torch.empty(B, HS, WS, 3, dtype=torch.uint8, device="cuda")
ops.synth_frames(src, 1, 0)
count = torch.full((B,), K, dtype=torch.int32, device="cuda")
out = torch.empty(B * K, D, D, 3, dtype=torch.uint8, device="cuda")
res["kernel"] = {}
for name, side in (("small_64px", 64.0), ("large_600px", 600.0)):
    det_cpu = box_mix(side, seed=int(side))
    det = det_cpu.cuda()
    for band in BANDS:
        for _ in range(3):
            ops.roi_crop(src, det, count, K, D, out=out, band=band)
    torch.cuda.synchronize()
    t = {band: [] for band in BANDS}
    for _ in range(20):  # alternating arms
        for band in BANDS:
            t[band].append(ev_ms(lambda: ops.roi_crop(src, det, count, K, D, out=out, band=band)))
    fb = floor_bytes(det_cpu)
    total = fb["dst_bytes"] + fb["src_bytes_distinct"]
    res["kernel"][name] = dict(fb, bands={
        str(band): {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                    "ms_max": round(max(v), 4),
                    "GBps_floor_bytes": round(total / statistics.median(v) / 1e6, 1)}
        for band, v in t.items()})
    print(name, res["kernel"][name], flush=True)
    dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)

# cascade step against detector step + classifier step: tiles tuned once, inside the cascade
# (detector at b64, classifier at b256), and kept by the two single-model engines
from kvedge_amd.models.cascade import KvDetectClassify  # noqa: E402
from kvedge_amd.models.resnet import KvResNet50  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n  # noqa: E402

del out
torch.cuda.empty_cache()
# a low threshold, so that the K slots hold real boxes (an empty slot is cheaper to fill)
detector = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001, max_det=MAX_DET)
classifier = KvResNet50.build(seed=0, device="cuda")
cascade = KvDetectClassify(detector, classifier, K, D)
c = InferenceEngine(cascade, B, 640, device="cuda", seed=0, synthetic=False, frame_hw=(HS, WS))
c.source_frames.copy_(src)
c.prepare(warmup=2, autotune=True)
y = InferenceEngine(detector, B, 640, device="cuda", seed=0, synthetic=False, frame_hw=(HS, WS))
y.source_frames.copy_(src)
y.prepare(warmup=2, autotune=False)
r = InferenceEngine(classifier, B * K, D, device="cuda", seed=0, synthetic=False)
ops.synth_frames(r.frames, 0, 0)
r.prepare(warmup=2, autotune=False)
for _ in range(20):
    c.run()
    y.run()
    r.run()
pc, py, pr = [], [], []
for _ in range(5):  # alternating arms
    pc.append(c.measure_latency(100).percentile(50))
    py.append(y.measure_latency(100).percentile(50))
    pr.append(r.measure_latency(100).percentile(50))
torch.cuda.synchronize()
cnt = c.outputs[1]
res["step"] = {
    "p50_ms_cascade_rounds": [round(x, 4) for x in pc],
    "p50_ms_yolov8n_b64_1080p_rounds": [round(x, 4) for x in py],
    "p50_ms_resnet50_b256_rounds": [round(x, 4) for x in pr],
    "p50_ms_cascade": round(statistics.median(pc), 4),
    "p50_ms_yolov8n_b64_1080p": round(statistics.median(py), 4),
    "p50_ms_resnet50_b256": round(statistics.median(pr), 4),
    "cascade_minus_sum_ms": round(statistics.median(pc) - statistics.median(py) -
                                  statistics.median(pr), 4),
    "detections_mean": round(float(cnt.float().mean()), 2),
    "valid_crops": int((c.outputs[2] >= 0).sum())}
print("step", res["step"], flush=True)
dump()
print("done", flush=True)
