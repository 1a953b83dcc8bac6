"""Appearance search at b64 (profiles/gallery_match_b64.json), one process, alternating arms:
  * ops.gallery_match at M = 256, D = 2048, K = 4 for G in 4096, 65536, 1048576 -- HIP events
    around back-to-back launches -- and in the same rounds a device-to-device copy of the
    gallery bytes (the floor of a kernel that reads the gallery once) and the obvious
    alternative without the kernel, torch.matmul of the dequantised bf16 operands + torch.topk;
  * ops.embed_quantize at [256, 7, 7, 2048];
  * the detect-classify b64 step p50 from 1080p (engine.measure_latency, one hipGraph) with and
    without a 65536-row gallery, same detector and classifier objects.
Usage: python tools/gallery_probe.py [out.json] [--kernel-only]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.engine import InferenceEngine  # noqa: E402

assert torch.cuda.is_available() and ops.load()
M, D, K, ROUNDS = 256, 2048, 4, 9
args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = args[0] if args else "bench_outputs/gallery_measure.json"
res = {"device": torch.cuda.get_device_name(0), "queries": M, "dim": D, "top": K,
       "rounds": ROUNDS}


def dump():
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)


def ev_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def device_gallery(g):
    gal = ops.Gallery.__new__(ops.Gallery)  # device tensors only: no host mirror of 2 GiB
    gal.capacity, gal.dim = g, D
    gal.codes = torch.randint(-127, 128, (g, D), dtype=torch.int8, device="cuda")
    gal.scale = torch.full((g,), 1.0 / 3328.0, device="cuda")
    gal.label = torch.zeros(g, dtype=torch.int32, device="cuda")
    gal.count = torch.tensor([g], dtype=torch.int32, device="cuda")
    return gal


q = torch.randint(-127, 128, (M, D), dtype=torch.int8, device="cuda")
score = torch.empty(M, K, device="cuda")
row = torch.empty(M, K, dtype=torch.int32, device="cuda")
res["gallery_match"] = {}
for g in (4096, 65536, 1048576):
    gal = device_gallery(g)
    other = torch.empty_like(gal.codes)
    reps = 20 if g <= 65536 else 3
    qb = q.to(torch.bfloat16)
    gb = gal.codes.to(torch.bfloat16) if g <= 65536 else None  # 4 GiB at 2^20 rows: in slices

    def matmul_topk():
        if gb is not None:
            return torch.topk(qb @ gb.T * gal.scale, K, dim=1)
        best = None
        for lo in range(0, g, 131072):  # dequantise + score a slice, keep the running top K
            s = qb @ gal.codes[lo:lo + 131072].to(torch.bfloat16).T * gal.scale[lo:lo + 131072]
            v, i = torch.topk(s, K, dim=1)
            if best is not None:
                v, i = torch.cat([best[0], v], 1), torch.cat([best[1], i + lo], 1)
                sel = torch.topk(v, K, dim=1).indices
                v, i = v.gather(1, sel), i.gather(1, sel) - lo
            best = (v, i + lo)
        return best

    arms = {"gallery_match": lambda: ops.gallery_match(q, gal, K, score, row),
            "gallery_copy": lambda: other.copy_(gal.codes),
            "matmul_topk_bf16": matmul_topk}
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(ROUNDS):  # alternating arms
        for k, f in arms.items():
            t[k].append(ev_ms(f, reps))
    r = {k: {"ms_median": round(statistics.median(v), 5), "ms_min": round(min(v), 5),
             "ms_max": round(max(v), 5)} for k, v in t.items()}
    r["gallery_bytes"] = g * D
    r["match_over_copy"] = round(r["gallery_match"]["ms_median"] / r["gallery_copy"]["ms_median"], 2)
    r["matmul_topk_over_match"] = round(r["matmul_topk_bf16"]["ms_median"]
                                        / r["gallery_match"]["ms_median"], 2)
    res["gallery_match"][str(g)] = r
    print(g, r, flush=True)
    del gal, other, gb
    torch.cuda.empty_cache()

feat = torch.randn(256, 7, 7, 2048, device="cuda").to(torch.bfloat16)
feat2 = torch.empty_like(feat)
ec = torch.empty(256, 2048, dtype=torch.int8, device="cuda")
en = torch.empty(256, dtype=torch.int32, device="cuda")
arms = {"embed_quantize": lambda: ops.embed_quantize(feat, ec, en),
        "features_copy": lambda: feat2.copy_(feat)}
t = {k: [] for k in arms}
for _ in range(ROUNDS + 1):
    for k, f in arms.items():
        t[k].append(ev_ms(f, 20))
res["embed_quantize"] = {k: {"ms_median": round(statistics.median(v[1:]), 5),
                             "ms_min": round(min(v[1:]), 5)} for k, v in t.items()}
print("embed", res["embed_quantize"], flush=True)
dump()
if "--kernel-only" in sys.argv:
    print("done", flush=True)
    sys.exit(0)
del feat, feat2
torch.cuda.empty_cache()

from kvedge_amd.models.cascade import KvDetectClassify  # noqa: E402
from kvedge_amd.models.resnet import KvResNet50, init_resnet50  # noqa: E402
from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n  # noqa: E402

B, CROPS = 64, 4
yolo = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001, max_det=300)
clf = KvResNet50(init_resnet50(seed=0), "cuda")
gal = device_gallery(65536)
kw = dict(device="cuda", seed=0, frame_hw=(1080, 1920))
plain = InferenceEngine(KvDetectClassify(yolo, clf, CROPS), B, 640, **kw)
plain.prepare(warmup=2, autotune=True)
search = InferenceEngine(KvDetectClassify(yolo, clf, CROPS, gallery=gal, gallery_top=K), B, 640,
                         **kw)
search.prepare(warmup=2, autotune=False)
eng = {"plain": plain, "gallery": search}
for e in eng.values():
    for _ in range(10):
        e.run()
p = {k: [] for k in eng}
for _ in range(5):  # alternating arms
    for k, e in eng.items():
        p[k].append(e.measure_latency(50).percentile(50))
torch.cuda.synchronize()
res["step"] = {"batch": B, "crops_per_image": CROPS, "gallery_rows": 65536,
               "source": "synthetic RGB 1080 x 1920 frames, generated inside the step"}
for k, v in p.items():
    res["step"][f"p50_ms_{k}_rounds"] = [round(x, 4) for x in v]
    res["step"][f"p50_ms_{k}"] = round(statistics.median(v), 4)
d = res["step"]["p50_ms_gallery"] - res["step"]["p50_ms_plain"]
res["step"]["gallery_minus_plain_ms"] = round(d, 4)
res["step"]["gallery_over_plain_pct"] = round(100.0 * d / res["step"]["p50_ms_plain"], 2)
print("step", res["step"], flush=True)
dump()
print("done", flush=True)
