#!/usr/bin/env python
"""Measurements of the on-device JPEG decoder (K29) at the camera shape: batch 64, 1080p,
4:2:0, quality 75.  Writes profiles/jpeg_decode_parallel_b64_1080p.json; its decode_dri_row,
decode_no_dri, d2d_copy and h2d_* arms are those of profiles/jpeg_decode_b64_1080p.json, which
``--out`` with that name writes again.

Arms, alternated inside one process on one device and timed with device events (median and
p90 over --reps rounds, after --warmup rounds):
  decode_dri_row / decode_dri_row_parallel   ops.jpeg_decode, one restart interval per MCU row
                   (68 per frame), entropy="serial" (the three launches) / "parallel"
  decode_no_dri / decode_no_dri_parallel     the same pictures without restart markers: one
                   lane decodes a frame / one lane per ops.JPEG_DECODE_SPLIT_BYTES
  prefix_1 .. prefix_6   the first 1 .. 6 launches of decode_no_dri_parallel (scan, plan, spec,
                   stitch, write, decode; colour is the 7th); "launch_ms" in the result is the
                   difference of consecutive medians
  sweep_K / sweep_K_parallel   restart intervals of K MCUs (K = 5, 10, 20, 40: about 130 to
                   1000 bytes): where splitting starts to pay, for the "auto" threshold
  d2d_copy         a device-to-device copy of the decoded bytes (64 x 1080 x 1920 x 3)
  h2d_rgb / h2d_nv12 / h2d_jpeg   the pinned host-to-device copies a ring slot costs
The result also holds dec.paths summed over the batch per decode arm and, for
decode_no_dri_parallel, the split headers: lanes per file, seam rounds and passes, and the
histogram of spec workgroups by their sync rounds over the batch.

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
    """dri: 0 none, "row" one MCU row, or MCUs per restart interval."""
    from PIL import Image

    buf = io.BytesIO()
    kw = {"restart_marker_rows": 1} if dri == "row" else \
        {"restart_marker_blocks": dri} if dri else {}
    Image.fromarray(pic).save(buf, "JPEG", quality=75, subsampling=2, **kw)
    return buf.getvalue()


SWEEP = (5, 10, 20, 40)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "jpeg_decode_parallel_b64_1080p.json"))
    a = ap.parse_args()
    assert ops.load()
    b, hw = a.batch, (a.height, a.width)
    pics = pictures(4, *hw, seed=0)
    kinds = {"dri_row": "row", "no_dri": 0, **{f"sweep_{k}": k for k in SWEEP}}
    sets = {name: [encode(p, dri) for p in pics] for name, dri in kinds.items()}
    n = ops.jpeg_row_bytes(hw)
    decs = {m: ops.JpegDecoder(b, hw, n, device="cuda", lanes=a.lanes, entropy=m)
            for m in ("serial", "parallel")}
    rows = {k: torch.from_numpy(ref.jpeg_rows([f[i % 4] for i in range(b)], n)).cuda()
            for k, f in sets.items()}
    out = torch.empty(b, *hw, 3, dtype=torch.uint8, device="cuda")
    out2 = torch.empty_like(out)
    pin = {"rgb": torch.empty(b * hw[0] * hw[1] * 3, dtype=torch.uint8).pin_memory(),
           "nv12": torch.empty(b * hw[0] * hw[1] * 3 // 2, dtype=torch.uint8).pin_memory(),
           "jpeg": torch.empty(b * n, dtype=torch.uint8).pin_memory()}
    devbuf = torch.empty(b * hw[0] * hw[1] * 3, dtype=torch.uint8, device="cuda")
    arms, arm_dec = {}, {}  # arm -> callable, decode arm -> its decoder
    for k in rows:
        for m, suffix in (("serial", ""), ("parallel", "_parallel")):
            name = (k if k.startswith("sweep") else "decode_" + k) + suffix
            arms[name] = (lambda k=k, m=m: ops.jpeg_decode(rows[k], decs[m], out=out))
            arm_dec[name] = decs[m]
    d = decs["parallel"]
    for count in range(1, 7):
        arms[f"prefix_{count}"] = (lambda c=count: torch.ops.kvedge.jpeg_decode_split(
            rows["no_dri"], d.tables, d.mpos, d.planes, out, d.status, d.split, d.done, d.paths,
            d.lanes, 2, c))
    arms["d2d_copy"] = lambda: out2.copy_(out)
    for k, p in pin.items():
        arms["h2d_" + k] = (lambda p=p: devbuf[:p.numel()].copy_(p, non_blocking=True))
    times = {k: [] for k in arms}
    paths, split_hdr = {}, None
    for r in range(a.warmup + a.reps):
        for k, fn in arms.items():  # the arms alternate inside every round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            if r == 0 and k in arm_dec:
                assert arm_dec[k].status.tolist() == [0] * b
                paths[k] = arm_dec[k].paths.sum(0).tolist()
                if k == "decode_no_dri_parallel":
                    split_hdr = d.split[:, :16].cpu()
    ms = {k: {"p50": round(statistics.median(v), 4),
              "p90": round(float(np.percentile(v, 90)), 4)} for k, v in times.items()}
    steps = [ms[f"prefix_{c}"]["p50"] for c in range(1, 7)] + [ms["decode_no_dri_parallel"]["p50"]]
    names = ("scan", "plan", "spec", "stitch", "write", "decode", "colour")
    res = {"shape": {"batch": b, "hw": list(hw), "subsampling": "420", "quality": 75,
                     "row_bytes": n, "lanes": a.lanes, "split_bytes": ops.JPEG_DECODE_SPLIT_BYTES,
                     "file_bytes": {k: [len(f) for f in v] for k, v in sets.items()}},
           "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "paths_completed_handed_back": paths,
           "decode_no_dri_parallel_split": {
               "lanes_per_file": sorted(set(split_hdr[:, 0].tolist())),
               "seam_rounds_max": int(split_hdr[:, 2].max()),
               "seam_passes_per_file": sorted(set(split_hdr[:, 3].tolist())),
               "workgroups_by_sync_rounds_0_to_11plus": split_hdr[:, 4:].sum(0).tolist()},
           "launch_ms": {nm: round(t - (steps[i - 1] if i else 0.0), 4)
                         for i, (nm, t) in enumerate(zip(names, steps))},
           "ms": ms}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["ms"]))


if __name__ == "__main__":
    main()
