"""Sliced detection at b64 (profiles/det_merge_b64.json), one process, alternating arms:
  * ops.det_merge alone, 64 cameras, 5 x 300 and 13 x 300 candidate rows, every row live, boxes
    spread over a 1080p frame (sparse: almost all kept until max_det) or drawn around 12 centres
    per camera (clustered: most absorbed) -- HIP events around 20 back-to-back launches; beside
    it ops.nms on the decoded anchors of a b64 YOLOv8n step (conf 0.001);
  * the tracked YOLOv8n b64 step from 1080p NV12 (engine.measure_latency, one hipGraph), plain
    and with a 2x2 slice grid, same model object and conv tiles, and the merge and the NMS timed
    alone on those steps' own inputs: their shares of the steps.
Usage: python tools/det_merge_probe.py [out.json] [--kernel-only]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402
from kvedge_amd.models.slicing import KvSliced  # noqa: E402
from kvedge_amd.models.tracking import KvTracked  # noqa: E402
from kvedge_amd.models.yolov8 import STRIDES, KvYoloV8n, init_yolov8n  # noqa: E402

assert torch.cuda.is_available() and ops.load()
B, R, REPS, HW = 64, 300, 20, (1080, 1920)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else "bench_outputs/det_merge_measure.json"
res = {"device": torch.cuda.get_device_name(0), "batch": B, "R": R}


def dump():
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


def ev_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / REPS


def boxes(groups, clusters, seed):
    g = torch.Generator().manual_seed(seed)
    wh = 40.0 + 80.0 * torch.rand(groups * B, R, 2, generator=g)
    cls = torch.randint(0, 8, (groups * B, R, 1), generator=g).float()
    if clusters:  # one class per centre, as one object seen by several tiles
        c = torch.rand(groups * B, clusters, 2, generator=g) * torch.tensor([1800.0, 960.0])
        pick = torch.randint(0, clusters, (groups * B, R), generator=g)
        xy = c[torch.arange(groups * B).view(-1, 1), pick] + 9.0 * torch.randn(
            groups * B, R, 2, generator=g)
        cls = (pick % 8).float().unsqueeze(-1)
    else:
        xy = torch.rand(groups * B, R, 2, generator=g) * torch.tensor([1800.0, 960.0])
    return torch.cat([xy, xy + wh, torch.rand(groups * B, R, 1, generator=g), cls], dim=2).cuda()


yolo = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001, max_det=R)
frames = torch.empty(B, 640, 640, 3, dtype=torch.uint8, device="cuda")
ops.synth_frames(frames, 0, 0)
anchors = ops.yolo_decode(yolo.heads(yolo.stem_b1(frames), b1_done=True), STRIDES, yolo.nc)
arms = {"nms_b64": lambda: ops.nms(*anchors, yolo.conf, yolo.iou, R)}
kept = {}
for groups in (5, 13):
    for name, clusters in (("sparse", 0), ("clustered", 12)):
        det = boxes(groups, clusters, groups)
        count = torch.full((groups * B,), R, dtype=torch.int32, device="cuda")
        out = ops.det_merge(det, count, groups)
        kept[f"merge_{groups}x{R}_{name}"] = float(out[1].float().mean())
        arms[f"merge_{groups}x{R}_{name}"] = (
            lambda det=det, count=count, groups=groups, out=out: ops.det_merge(
                det, count, groups, out=out[0], out_count=out[1]))
for fn in arms.values():  # warm: code objects
    fn()
torch.cuda.synchronize()
t = {k: [] for k in arms}
for _ in range(15):  # alternating arms
    for k, fn in arms.items():
        t[k].append(ev_ms(fn))
res["kernel"] = {}
for k, v in t.items():
    res["kernel"][k] = {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5),
                        "ms_max": round(max(v), 5)}
    if k in kept:
        res["kernel"][k]["kept_per_camera"] = kept[k]
    print(k, res["kernel"][k], flush=True)
dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)

sliced = KvSliced(yolo, B, grid=(2, 2), overlap=0.2)
kw = dict(device="cuda", seed=0, frame_hw=HW, frame_format="nv12")
eng = {"plain": InferenceEngine(KvTracked(yolo, B), B, 640, **kw).prepare(warmup=2, autotune=True),
       "sliced_2x2": InferenceEngine(KvTracked(sliced, B), B, 640, **kw).prepare(
           warmup=2, autotune=False)}
for e in eng.values():
    for _ in range(10):
        e.run()
p = {k: [] for k in eng}
for _ in range(5):  # alternating arms
    for k, e in eng.items():
        p[k].append(e.measure_latency(50).percentile(50))
torch.cuda.synchronize()
step = res["step"] = {"frame": "1080p NV12", "tracked": True}
for k, v in p.items():
    step[f"p50_ms_{k}_rounds"] = [round(x, 4) for x in v]
    step[f"p50_ms_{k}"] = round(statistics.median(v), 4)
step["sliced_over_plain"] = round(step["p50_ms_sliced_2x2"] / step["p50_ms_plain"], 3)
# the merge and the NMS alone, on what these steps feed them
e = eng["sliced_2x2"]
gdet, gcount = sliced.group_outputs(e.source_frames, e.frames, e.frame_plan, src_format="nv12")
mout = ops.det_merge(gdet, gcount, 5)
step_anchors = ops.yolo_decode(yolo.heads(yolo.stem_b1(e.frames), b1_done=True), STRIDES, yolo.nc)
torch.cuda.synchronize()
alone = {"merge": [], "nms": []}
for _ in range(15):
    alone["merge"].append(ev_ms(lambda: ops.det_merge(gdet, gcount, 5, out=mout[0],
                                                      out_count=mout[1])))
    alone["nms"].append(ev_ms(lambda: ops.nms(*step_anchors, yolo.conf, yolo.iou, R)))
step["candidates_per_camera"] = round(float(gcount.view(5, B).sum(0).float().mean()), 1)
step["merged_per_camera"] = round(float(mout[1].float().mean()), 1)
step["merge_ms"] = round(statistics.median(alone["merge"]), 5)
step["nms_b64_ms"] = round(statistics.median(alone["nms"]), 5)
step["merge_share_of_sliced_step_pct"] = round(100 * step["merge_ms"] / step["p50_ms_sliced_2x2"], 2)
step["nms_share_of_plain_step_pct"] = round(100 * step["nms_b64_ms"] / step["p50_ms_plain"], 2)
print("step", step, flush=True)
dump()
print("done", flush=True)
