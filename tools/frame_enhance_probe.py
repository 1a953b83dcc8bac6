"""Low-light enhancement at b64, 640x640 (profiles/frame_enhance_b64.json), HIP events, warmed,
alternating arms in one process on one device, for noise in 0..20, a constant frame and
full-range noise:
  (a) ops.frame_enhance with every camera off, in place: the table launch (the apply launch
      leaves at once), for 1 / 2 / 4 / 8 LDS histogram copies per wave;
  (b) ops.frame_enhance on, into a second buffer: both launches; apply = (b) - (a) at the
      same copies;
  (c) a device-to-device copy of the same bytes and ops.frame_watch on them: the yardsticks;
  then the tracked YOLOv8n edge step p50 from 1080p with and without the stage, same conv tiles.
Usage: python tools/frame_enhance_probe.py [out.json]"""
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
COPIES = (1, 2, 4, 8)
res = {"device": torch.cuda.get_device_name(0), "batch": B, "hw": [D, D], "tiles": [8, 8],
       "rounds": ROUNDS, "bytes": B * D * D * 3}
OUT = sys.argv[1] if len(sys.argv) > 1 else "bench_outputs/frame_enhance_measure.json"


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


def enhancer(mode, copies):
    e = ops.FrameEnhance(B, (D, D), device="cuda").set_mode(mode)
    e.hist_copies = copies
    return e


g = torch.Generator("cuda").manual_seed(0)
CONTENT = {"dark_0_20": lambda t: t.random_(0, 21, generator=g),
           "constant": lambda t: t.fill_(37),
           "full_range": lambda t: t.random_(0, 256, generator=g)}
res["kernel"] = {}
for name, fill in CONTENT.items():
    pristine = fill(torch.empty(B, D, D, 3, dtype=torch.uint8, device="cuda"))
    work, other = pristine.clone(), torch.empty_like(pristine)
    watch = ops.WatchState(B, (D, D), device="cuda")
    arms = {"copy_d2d": lambda: other.copy_(pristine),
            "frame_watch": lambda: ops.frame_watch(pristine, watch)}
    for c in COPIES:
        # the off arm reads ``pristine`` and writes nothing; the on arm enhances it into
        # ``work``, so every round sees the same input
        arms[f"tables_copies{c}"] = lambda e=enhancer("off", c): ops.frame_enhance(pristine, e)
        arms[f"both_copies{c}"] = lambda e=enhancer("on", c): ops.frame_enhance(pristine, e,
                                                                               out=work)
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(ROUNDS):  # alternating arms
        for k, fn in arms.items():
            times[k].append(ev_ms(fn))
    r = {k: {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
             "ms_max": round(max(t), 4)} for k, t in times.items()}
    for c in COPIES:
        r[f"apply_copies{c}"] = {"ms_median": round(r[f"both_copies{c}"]["ms_median"]
                                                    - r[f"tables_copies{c}"]["ms_median"], 4)}
    res["kernel"][name] = r
    print(name, r, flush=True)
    dump()
    del arms, pristine, work, other
    torch.cuda.empty_cache()

# the tracked YOLOv8n step from 1080p with and without the stage; tiles tuned in arm A and kept
# by arm B (autotune=False); dark frames, so that auto enhances every camera
from kvedge_amd.models.tracking import KvTracked  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n  # noqa: E402

src = torch.empty(B, HS, WS, 3, dtype=torch.uint8, device="cuda").random_(0, 21, generator=g)
engines = []
model = KvTracked(KvYoloV8n.build(seed=0, device="cuda"), B)
for enh in (None, ops.FrameEnhance(B, (D, D), device="cuda").set_mode("auto")):
    e = InferenceEngine(model, B, D, device="cuda", seed=0, synthetic=False, frame_hw=(HS, WS),
                        enhance=enh)
    e.source_frames.copy_(src)
    e.prepare(warmup=2, autotune=not engines)
    engines.append(e)
a, b = engines
for _ in range(20):
    a.run()
    b.run()
torch.cuda.synchronize()
pa, pb = [], []
for _ in range(5):  # alternating arms
    pa.append(a.measure_latency(100).percentile(50))
    pb.append(b.measure_latency(100).percentile(50))
res["step_tracked_yolov8n_1080p"] = {
    "enhanced_cameras": int((b.enhance_stats[:, 1] > 0).sum()),
    "p50_ms_plain_rounds": [round(x, 4) for x in pa],
    "p50_ms_enhance_rounds": [round(x, 4) for x in pb],
    "p50_ms_plain": round(statistics.median(pa), 4),
    "p50_ms_enhance": round(statistics.median(pb), 4)}
print("step", res["step_tracked_yolov8n_1080p"], flush=True)
dump()
print("done", flush=True)
