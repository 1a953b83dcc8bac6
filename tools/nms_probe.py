#!/usr/bin/env python3
"""Time the YOLOv8n NMS kernel of the library this process loaded on the model's own decode
output (random-init weights, synthetic frames).

  python tools/nms_probe.py --batch 192

Where the per-image latency goes: the kernel's phases are switched off at compile time
(-DKVEDGE_NMS_DIAG=n, timing only, outputs wrong: 1 = no greedy suppression, 2 = no top-set
sort, 4 = per-phase durations written over each image's first output row), one variant build
per value, each timed in a fresh process:

  for d in 1 2 3; do
    KVEDGE_VARIANT=nms$d KVEDGE_CFLAGS=-DKVEDGE_NMS_DIAG=$d python -m kvedge_amd._build
    KVEDGE_LIB=_C_nms$d.so python tools/nms_probe.py --batch 192
  done
  KVEDGE_VARIANT=nms4 KVEDGE_CFLAGS=-DKVEDGE_NMS_DIAG=4 python -m kvedge_amd._build
  KVEDGE_LIB=_C_nms4.so python tools/nms_probe.py --batch 192 --stamps
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--stamps", action="store_true",
                    help="print the phase-timestamp table; only a library built with "
                         "-DKVEDGE_NMS_DIAG=4 writes the stamps")
    a = ap.parse_args()
    import torch

    from kvedge_amd import ops
    from kvedge_amd.models.yolov8 import STRIDES, KvYoloV8n

    assert ops.load()
    m = KvYoloV8n.build(seed=0, device="cuda")
    fr = torch.randint(0, 256, (a.batch, 640, 640, 3), dtype=torch.uint8,
                       generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        feats = m.heads(m.stem_b1(fr), b1_done=True)
        boxes, scores, cls = ops.yolo_decode(feats, STRIDES, m.nc)
    torch.cuda.synchronize()
    print(f"candidates per image > conf {m.conf}: "
          f"{float((scores > m.conf).sum(1).float().mean()):.0f} of {scores.shape[1]}")
    lib = ops.library_path()
    if a.stamps:
        out, cnt = ops.nms(boxes, scores, cls, m.conf, m.iou, m.max_det)
        torch.cuda.synchronize()
        ph = out[:, 0, :3].float().cpu() / 100.0  # 10-ns ticks -> us
        print("per-image phase us (median over images): compaction+select %.1f, sort %.1f, "
              "suppression %.1f" % tuple(float(ph[:, i].median()) for i in range(3)) + f"  [{lib}]")
        print("per-image phase us (max over images):    compaction+select %.1f, sort %.1f, "
              "suppression %.1f" % tuple(float(ph[:, i].max()) for i in range(3)) + f"  [{lib}]")
    nc = (scores > m.conf).sum(1)
    print(f"candidates per image: max {int(nc.max())}, images over 1024: {int((nc > 1024).sum())}")
    ts = []
    for _ in range(a.iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out, cnt = ops.nms(boxes, scores, cls, m.conf, m.iou, m.max_det)
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    ts.sort()
    print(f"nms b{a.batch}: {ts[len(ts) // 2]:.1f} us  kept/image {float(cnt.float().mean()):.0f}"
          f"  [{lib}]", flush=True)


if __name__ == "__main__":
    main()
