"""Camera front end at b64, 1080x1920 (profiles/frame_resize_b64_1080p.json):
  * ops.frame_resize (letterbox into 640, centre-crop into 224) against the bytes-moved floor
    (source lines touched + destination bytes) and against the same resample done with torch
    (uint8 -> float -> F.interpolate -> uint8), HIP events, warmed, alternating arms;
  * edge step p50 (engine.measure_latency) with frame_hw=(1080, 1920) against frames at
    model size, same conv tiles, alternating arms;
  * the pinned host-to-device copy of one batch, and the native serve loop fed by a
    pre-filled pinned ring (DMA + one graph replay per step).
Usage: python tools/frame_resize_probe.py [out.json]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops, runtime  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, HS, WS = 64, 1080, 1920
res = {"device": torch.cuda.get_device_name(0), "batch": B, "frame_hw": [HS, WS]}
OUT = sys.argv[1] if len(sys.argv) > 1 else "bench_outputs/frame_resize_measure.json"


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


def torch_resample(src, plan, out):
    (_, ry, oy, c0y, ny), (_, rx, ox, c0x, nx) = plan.axis_y, plan.axis_x
    x = src.permute(0, 3, 1, 2).float()
    y = F.interpolate(x, size=(ry, rx), mode="bilinear", align_corners=False, antialias=False)
    y = y[:, :, oy:oy + ny, ox:ox + nx].round_().clamp_(0, 255).to(torch.uint8)
    if ny < out.shape[1] or nx < out.shape[2]:
        out.fill_(plan.pad)
    out[:, c0y:c0y + ny, c0x:c0x + nx] = y.permute(0, 2, 3, 1)
    return out


def floor_bytes(plan, n):
    from kvedge_amd.ops.reference import _resize_axis

    cy, y0, y1, wy = _resize_axis(plan.axis_y, plan.dst_hw[0])
    y1 = torch.where(wy > 0, y1, y0)  # a zero-weight tap is not read
    rows = torch.unique(torch.cat([y0[cy], y1[cy]])).numel()
    cx, x0, x1, wx = _resize_axis(plan.axis_x, plan.dst_hw[1])
    x1 = torch.where(wx > 0, x1, x0)
    cols = int(x1[cx].max() - x0[cx].min() + 1)
    dst = plan.dst_hw[0] * plan.dst_hw[1] * 3
    return {"source_rows_touched": rows, "source_cols_span": cols,
            "bytes_full_lines": n * (rows * plan.src_hw[1] * 3 + dst),
            "bytes_touched_span": n * (rows * cols * 3 + dst)}


src = torch.empty(B, HS, WS, 3, dtype=torch.uint8, device="cuda")
ops.synth_frames(src, 1, 0)
res["kernel"] = {}
for name, plan in (("letterbox_640", ops.letterbox_plan((HS, WS), 640)),
                   ("center_crop_224", ops.center_crop_plan((HS, WS), 224))):
    out_k = torch.empty(B, *plan.dst_hw, 3, dtype=torch.uint8, device="cuda")
    out_t = torch.empty_like(out_k)
    for _ in range(3):
        ops.frame_resize(src, plan, out=out_k)
        torch_resample(src, plan, out_t)
    torch.cuda.synchronize()
    tk, tt = [], []
    for _ in range(20):  # alternating arms
        tk.append(ev_ms(lambda: ops.frame_resize(src, plan, out=out_k)))
        tt.append(ev_ms(lambda: torch_resample(src, plan, out_t)))
    diff = (out_k.int() - out_t.int()).abs()
    fb = floor_bytes(plan, B)
    mk = statistics.median(tk)
    res["kernel"][name] = {
        "kernel_ms_median": round(mk, 4), "kernel_ms_min": round(min(tk), 4),
        "kernel_ms_max": round(max(tk), 4),
        "torch_ms_median": round(statistics.median(tt), 4), "torch_ms_min": round(min(tt), 4),
        "max_abs_diff_vs_torch": int(diff.max()), **fb,
        "GBps_full_lines": round(fb["bytes_full_lines"] / mk / 1e6, 1),
        "GBps_touched_span": round(fb["bytes_touched_span"] / mk / 1e6, 1)}
    print(name, res["kernel"][name], flush=True)
    dump()
    del out_k, out_t
torch.cuda.empty_cache()

# host-to-device copy of one batch from pinned memory
host = torch.empty(B * HS * WS * 3, dtype=torch.uint8).pin_memory()
host.copy_(src.view(-1).cpu())
for _ in range(2):
    src.view(-1).copy_(host, non_blocking=True)
torch.cuda.synchronize()
h2d = [ev_ms(lambda: src.view(-1).copy_(host, non_blocking=True)) for _ in range(10)]
res["h2d"] = {"bytes": host.numel(), "ms_median": round(statistics.median(h2d), 3),
              "ms_min": round(min(h2d), 3),
              "GBps": round(host.numel() / statistics.median(h2d) / 1e6, 1)}
print("h2d", res["h2d"], flush=True)
dump()


def build(model_name):
    if model_name == "resnet50":
        from kvedge_amd.models.resnet import KvResNet50

        return KvResNet50.build(seed=0, device="cuda"), 224
    from kvedge_amd.models.yolov8 import KvYoloV8n

    return KvYoloV8n.build(seed=0, device="cuda"), 640


res["step"] = {}
res["serve"] = {}
for model_name in ("resnet50", "yolov8n"):
    model, size = build(model_name)
    # arm A: frames at model size (the path without a frame size); tiles tuned here, kept by
    # arm B (autotune=False), so both arms run the same conv tiles
    a = InferenceEngine(model, B, size, device="cuda", seed=0, synthetic=False)
    ops.synth_frames(a.frames, 0, 0)
    a.prepare(warmup=2, autotune=True)
    b = InferenceEngine(model, B, size, device="cuda", seed=0, synthetic=False,
                        frame_hw=(HS, WS))
    b.source_frames.copy_(src)
    b.prepare(warmup=2, autotune=False)
    for _ in range(20):
        a.run()
        b.run()
    pa, pb = [], []
    for _ in range(5):  # alternating arms
        pa.append(a.measure_latency(100).percentile(50))
        pb.append(b.measure_latency(100).percentile(50))
    res["step"][model_name] = {
        "p50_ms_model_size_rounds": [round(x, 4) for x in pa],
        "p50_ms_1080p_rounds": [round(x, 4) for x in pb],
        "p50_ms_model_size": round(statistics.median(pa), 4),
        "p50_ms_1080p": round(statistics.median(pb), 4),
        "front_end_ms": round(statistics.median(pb) - statistics.median(pa), 4)}
    print(model_name, res["step"][model_name], flush=True)
    dump()
    # serve loop: ring pre-filled (no producer stall inside the timed window), each step =
    # pinned-ring DMA into source_frames + one graph replay
    slots = 6
    ring = runtime.FrameRing(slots, b.input_frames.numel())
    rounds = []
    for rnd in range(3):
        for i in range(slots):
            assert ring.put(host, rnd * slots + i, timeout_ms=5000)
        hist = runtime.LatencyHistogram()
        r = b.serve_native(slots, depth=2, hist=hist, ring=ring, ring_timeout_ms=5000)
        rounds.append({"steps": r.steps, "frames_in": r.frames_in,
                       "device_ms_per_step": round(r.device_ms / max(1, r.steps), 3),
                       "wall_ms_per_step": round(r.wall_s * 1e3 / max(1, r.steps), 3)})
    res["serve"][model_name] = {"pinned": ring.pinned, "slot_bytes": ring.slot_bytes,
                                "rounds": rounds}
    print(model_name, "serve", res["serve"][model_name], flush=True)
    dump()
    ring.close()
    del ring, a, b, model
    torch.cuda.empty_cache()
print("done", flush=True)
