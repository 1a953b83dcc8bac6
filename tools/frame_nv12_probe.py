"""NV12 against packed RGB at b64, 1080x1920 (profiles/frame_nv12_b64_1080p.json), alternating
arms in one process:
  * ops.frame_resize from NV12 against from RGB (letterbox into 640, centre-crop into 224),
    HIP events, warmed;
  * ops.roi_crop from NV12 against from RGB (K 4, D 224, ~64 px and ~600 px windows);
  * the pinned host-to-device copy of one batch: 199 MB of NV12 against 398 MB of RGB;
  * the native serve loop fed by a pre-filled pinned ring (DMA + one graph replay per step),
    ``camera`` against ``camera-nv12`` frames, ResNet-50 and YOLOv8n, same conv tiles.
Both sources are random bytes (the kernels are branch-free in the pixel values).
Usage: python tools/frame_nv12_probe.py [out.json] [--kernel-only]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops, runtime  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, HS, WS, K, D, MAX_DET = 64, 1080, 1920, 4, 224, 300
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else "bench_outputs/frame_nv12_measure.json"
res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame_hw": [HS, WS],
       "bytes_rgb": B * HS * WS * 3, "bytes_nv12": B * HS * WS * 3 // 2}


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


def arms(rgb_fn, nv12_fn, rounds=20):
    """Median / min / max ms of the two arms, alternated."""
    for _ in range(3):
        rgb_fn()
        nv12_fn()
    torch.cuda.synchronize()
    tr, tn = [], []
    for _ in range(rounds):
        tr.append(ev_ms(rgb_fn))
        tn.append(ev_ms(nv12_fn))
    out = {}
    for name, t in (("rgb", tr), ("nv12", tn)):
        out[name] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
                     "ms_max": round(max(t), 4)}
    out["nv12_over_rgb"] = round(statistics.median(tn) / statistics.median(tr), 3)
    return out


rgb = torch.empty(B, HS, WS, 3, dtype=torch.uint8, device="cuda")
nv12 = torch.empty(B, HS * 3 // 2, WS, dtype=torch.uint8, device="cuda")
ops.synth_frames(rgb, 1, 0)
ops.synth_frames(nv12.view(B, HS // 2, WS, 3), 2, 0)

res["resize"] = {}
for name, plan in (("letterbox_640", ops.letterbox_plan((HS, WS), 640)),
                   ("center_crop_224", ops.center_crop_plan((HS, WS), 224))):
    out_r = torch.empty(B, *plan.dst_hw, 3, dtype=torch.uint8, device="cuda")
    out_n = torch.empty_like(out_r)
    res["resize"][name] = arms(
        lambda: ops.frame_resize(rgb, plan, out=out_r),
        lambda: ops.frame_resize(nv12, plan, out=out_n, src_format="nv12"))
    print(name, res["resize"][name], flush=True)
    dump()
    del out_r, out_n


def box_mix(side, seed):
    """det [B, MAX_DET, 6]: windows of about ``side`` pixels (0.75 .. 1.25 x) anywhere in the
    frame, fractional corners (tools/roi_crop_probe.py's mixes)."""
    g = torch.Generator().manual_seed(seed)
    wh = side * (0.75 + 0.5 * torch.rand(B, MAX_DET, 2, generator=g))
    lim = torch.tensor([WS, HS], dtype=torch.float32)
    xy = torch.rand(B, MAX_DET, 2, generator=g) * (lim - wh).clamp_min(1.0)
    return torch.cat([xy, xy + wh, torch.rand(B, MAX_DET, 2, generator=g)], dim=2)


count = torch.full((B,), K, dtype=torch.int32, device="cuda")
out_r = torch.empty(B * K, D, D, 3, dtype=torch.uint8, device="cuda")
out_n = torch.empty_like(out_r)
res["roi_crop"] = {}
for name, side in (("small_64px", 64.0), ("large_600px", 600.0)):
    det = box_mix(side, seed=int(side)).cuda()
    res["roi_crop"][name] = arms(
        lambda: ops.roi_crop(rgb, det, count, K, D, out=out_r),
        lambda: ops.roi_crop(nv12, det, count, K, D, out=out_n, src_format="nv12"))
    print(name, res["roi_crop"][name], flush=True)
    dump()
del out_r, out_n
torch.cuda.empty_cache()

# host-to-device copy of one batch from pinned memory
host = {"rgb": torch.empty(rgb.numel(), dtype=torch.uint8).pin_memory(),
        "nv12": torch.empty(nv12.numel(), dtype=torch.uint8).pin_memory()}
host["rgb"].copy_(rgb.view(-1).cpu())
host["nv12"].copy_(nv12.view(-1).cpu())
h2d = arms(lambda: rgb.view(-1).copy_(host["rgb"], non_blocking=True),
           lambda: nv12.view(-1).copy_(host["nv12"], non_blocking=True), rounds=10)
for name in ("rgb", "nv12"):
    h2d[name]["bytes"] = host[name].numel()
    h2d[name]["GBps"] = round(host[name].numel() / h2d[name]["ms_median"] / 1e6, 1)
res["h2d"] = h2d
print("h2d", h2d, flush=True)
dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)


def build(model_name):
    if model_name == "resnet50":
        from kvedge_amd.models.resnet import KvResNet50

        return KvResNet50.build(seed=0, device="cuda"), 224
    from kvedge_amd.models.yolov8 import KvYoloV8n

    return KvYoloV8n.build(seed=0, device="cuda"), 640


res["serve"] = {}
SLOTS = 6
for model_name in ("resnet50", "yolov8n"):
    model, size = build(model_name)
    # tiles tuned by the RGB engine and kept by the NV12 one (autotune=False): same conv tiles
    eng = {"rgb": InferenceEngine(model, B, size, device="cuda", seed=0, synthetic=False,
                                  frame_hw=(HS, WS))}
    eng["rgb"].source_frames.copy_(rgb)
    eng["rgb"].prepare(warmup=2, autotune=True)
    eng["nv12"] = InferenceEngine(model, B, size, device="cuda", seed=0, synthetic=False,
                                  frame_hw=(HS, WS), frame_format="nv12")
    eng["nv12"].source_frames.copy_(nv12)
    eng["nv12"].prepare(warmup=2, autotune=False)
    for _ in range(10):
        eng["rgb"].run()
        eng["nv12"].run()
    torch.cuda.synchronize()
    # serve loop: ring pre-filled (no producer stall inside the timed window), each step =
    # pinned-ring DMA into source_frames + one graph replay
    ring = {f: runtime.FrameRing(SLOTS, e.input_frames.numel()) for f, e in eng.items()}
    rounds = {"rgb": [], "nv12": []}
    for rnd in range(4):  # alternating arms
        for f in ("rgb", "nv12"):
            for i in range(SLOTS):
                assert ring[f].put(host[f], rnd * SLOTS + i, timeout_ms=5000)
            hist = runtime.LatencyHistogram()
            r = eng[f].serve_native(SLOTS, depth=2, hist=hist, ring=ring[f],
                                    ring_timeout_ms=5000)
            rounds[f].append({"steps": r.steps, "frames_in": r.frames_in,
                              "device_ms_per_step": round(r.device_ms / max(1, r.steps), 3),
                              "wall_ms_per_step": round(r.wall_s * 1e3 / max(1, r.steps), 3)})
    entry = {}
    for f in ("rgb", "nv12"):
        wall = statistics.median(x["wall_ms_per_step"] for x in rounds[f])
        entry["camera" if f == "rgb" else "camera-nv12"] = {
            "pinned": ring[f].pinned, "slot_bytes": ring[f].slot_bytes, "rounds": rounds[f],
            "wall_ms_per_step_median": round(wall, 3),
            "frames_per_s": round(B / wall * 1e3, 1)}
    entry["nv12_over_rgb"] = round(entry["camera-nv12"]["wall_ms_per_step_median"] /
                                   entry["camera"]["wall_ms_per_step_median"], 3)
    res["serve"][model_name] = entry
    print(model_name, "serve", entry, flush=True)
    dump()
    for r in ring.values():
        r.close()
    del ring, eng, model
    torch.cuda.empty_cache()
print("done", flush=True)
