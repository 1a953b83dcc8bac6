#!/usr/bin/env python
"""First measurements of the on-device JPEG decoder (K29) at the camera shape: batch 64,
1080p, 4:2:0, quality 75.  Writes profiles/jpeg_decode_b64_1080p.json.

Arms, alternated inside one process on one device and timed with device events (median and
p90 over --reps rounds, after --warmup rounds):
  decode_dri_row   ops.jpeg_decode, one restart interval per MCU row (68 per frame)
  decode_no_dri    the same pictures without restart markers: one lane decodes a frame
  d2d_copy         a device-to-device copy of the decoded bytes (64 x 1080 x 1920 x 3)
  h2d_rgb / h2d_nv12 / h2d_jpeg   the pinned host-to-device copies a ring slot costs

No threshold: these are reported as measured.
"""
import argparse
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kvedge_amd import ops  # noqa: E402
from kvedge_amd.ops import reference as ref  # noqa: E402


def pictures(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        coarse = torch.randint(0, 256, (-(-h // 16), -(-w // 16), 3), dtype=torch.uint8,
                               generator=g)
        fine = torch.randint(0, 24, (h, w, 3), dtype=torch.uint8, generator=g)
        pic = coarse.repeat_interleave(16, 0).repeat_interleave(16, 1)[:h, :w] // 2 + 52 + fine
        out.append(pic.numpy())
    return out


def encode(pic, dri):
    from PIL import Image

    buf = io.BytesIO()
    kw = {"restart_marker_rows": 1} if dri else {}
    Image.fromarray(pic).save(buf, "JPEG", quality=75, subsampling=2, **kw)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_b64_1080p.json"))
    a = ap.parse_args()
    assert ops.load()
    b, hw = a.batch, (a.height, a.width)
    pics = pictures(4, *hw, seed=0)
    sets = {name: [encode(p, dri) for p in pics] for name, dri in (("dri_row", True),
                                                                  ("no_dri", False))}
    n = ops.jpeg_row_bytes(hw)
    dec = ops.JpegDecoder(b, hw, n, device="cuda", lanes=a.lanes)
    rows = {k: torch.from_numpy(ref.jpeg_rows([f[i % 4] for i in range(b)], n)).cuda()
            for k, f in sets.items()}
    out = torch.empty(b, *hw, 3, dtype=torch.uint8, device="cuda")
    out2 = torch.empty_like(out)
    pin = {"rgb": torch.empty(b * hw[0] * hw[1] * 3, dtype=torch.uint8).pin_memory(),
           "nv12": torch.empty(b * hw[0] * hw[1] * 3 // 2, dtype=torch.uint8).pin_memory(),
           "jpeg": torch.empty(b * n, dtype=torch.uint8).pin_memory()}
    devbuf = torch.empty(b * hw[0] * hw[1] * 3, dtype=torch.uint8, device="cuda")
    arms = {"decode_dri_row": lambda: ops.jpeg_decode(rows["dri_row"], dec, out=out),
            "decode_no_dri": lambda: ops.jpeg_decode(rows["no_dri"], dec, out=out),
            "d2d_copy": lambda: out2.copy_(out)}
    for k, p in pin.items():
        arms["h2d_" + k] = (lambda p=p: devbuf[:p.numel()].copy_(p, non_blocking=True))
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.reps):
        for k, fn in arms.items():  # the arms alternate inside every round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
        if r == 0:
            assert dec.status.tolist() == [0] * b
    res = {"shape": {"batch": b, "hw": list(hw), "subsampling": "420", "quality": 75,
                     "row_bytes": n, "lanes": a.lanes,
                     "file_bytes": {k: [len(f) for f in v] for k, v in sets.items()}},
           "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "ms": {k: {"p50": round(statistics.median(v), 4),
                      "p90": round(float(np.percentile(v, 90)), 4)} for k, v in times.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["ms"]))


if __name__ == "__main__":
    main()
