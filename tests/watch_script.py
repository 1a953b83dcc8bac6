"""Shared by the frame-watch tests: the five-frame script (random, the same again, a block
shifted in, all dark, constant) built from seeded random bytes, and a runner that steps a
WatchState through it."""
import torch

from kvedge_amd import ops

STEPS = 5
CD = -842150451  # 0xCDCDCDCD as int32
# per-stream thresholds, so the streams do not all behave alike; hold 2 lets alarms rise
PARAMS = [dict(motion_thr16=160, motion_share_q=10, scene_share_q=512, dark16=384, flat16=24,
               hold=2),
          dict(motion_thr16=0, motion_share_q=1024, scene_share_q=0, dark16=4096, flat16=0,
               hold=1),
          dict(motion_thr16=640, motion_share_q=300, scene_share_q=900, dark16=0, flat16=4096,
               hold=3)]


def shape(fmt, n, h, w):
    return (n, h * 3 // 2, w) if fmt == "nv12" else (n, h, w, 3)


def script(fmt, n, h, w, seed=0):
    """Five uint8 batches [n, ...] of h x w frames in ``fmt``."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randint(0, 256, shape(fmt, n, h, w), dtype=torch.uint8, generator=g)
    f2 = f0.clone()
    bh, bw = max(1, h // 3), max(2, w // 3)
    f2[:, h // 4:h // 4 + bh, w // 2:w // 2 + bw] = 255  # a bright block moves in
    return [f0, f0.clone(), f2, torch.zeros_like(f0), torch.full_like(f0, 200)]


def new_state(streams, h, w, device="cpu", **kw):
    st = ops.WatchState(streams, (h, w), device=device, **kw)
    for s in range(streams):
        st.set_params(s, **PARAMS[s % len(PARAMS)])
    return st


def reference_run(frames, fmt, st, slot0=0):
    """Step the CPU state ``st`` through ``frames``; per step (stats, mask, state copy)."""
    out = []
    for f in frames:
        stats, mask = ops.frame_watch(f, st, slot0=slot0, src_format=fmt)
        out.append((stats.clone(), mask.clone(), st.buf.clone()))
    return out
