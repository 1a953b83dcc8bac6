"""Frame watch on top of any deployed model: is anything moving in front of a camera, and is
its picture usable.

``KvWatched`` wraps a model (KvResNet50, KvYoloV8n, KvDetectClassify, KvTracked, KvZoned) and
appends ``(cam_stats, motion_mask)`` to its outputs: int32 [N, 16] and uint8 [N, GH, GW] of
ops.frame_watch (csrc/kernels/frame_watch.hip).  One batch row = one camera, as for the
tracker: row n of every batch is the next frame of stream ``slot0 + n``.  Every other stage
looks at the detector's boxes; this one looks at the frames themselves -- one more streaming
pass over the bytes already in device memory, at native resolution when the engine has a frame
size (``from_source``), two launches per step, state in device memory (ops.WatchState,
allocated here, outside the graph's pool), no host in the loop.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .. import ops


class KvWatched:
    """inner outputs ``(...)`` -> ``(..., cam_stats, motion_mask)``.  ``frame_hw``: the size of
    the frames the engine serves from (InferenceEngine ``frame_hw``); None = model-size frames.
    ``params``: thresholds by name (ops.WATCH_PARAMS), for every camera; ``watch_state``
    (``set_params``) changes them between steps without recapturing."""

    stateful = True  # InferenceEngine passes slot0 = first batch row of the slice

    def __init__(self, inner, streams: int, frame_hw=None, cell: int = 16, row_step: int = 1,
                 bg_shift: int = 4, **params):
        self.inner = inner
        self.device = inner.device
        self.image_size = getattr(inner, "image_size", 224)
        self.streams = int(streams)
        self.cell, self.row_step, self.bg_shift = int(cell), int(row_step), int(bg_shift)
        self.params = ops.check_watch_params(**params)
        hw = (self.image_size, self.image_size) if frame_hw is None else frame_hw
        self.watch_state = self._new_state(hw)
        self._other = {}  # states for frames of another size (the autotuner's model-size run)
        self.watch_resets = 0  # bumped by reset(): host-side totals start over
        self._inner_stateful = bool(getattr(inner, "stateful", False))

    def _new_state(self, hw) -> "ops.WatchState":
        st = ops.WatchState(self.streams, hw, self.cell, self.row_step, self.bg_shift,
                            device=self.device)
        return st.set_params(None, **self.params)

    def __getattr__(self, name):
        # the tracker / zone state and anything else the module reads off the inner model
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    # -- what the engine, the autotuner and the module read off a model
    def convs(self) -> List:
        return self.inner.convs()

    def flops_per_image(self, *a, **kw) -> int:
        return self.inner.flops_per_image(*a, **kw)

    def frame_plan(self, src_hw, image_size: int = 0) -> "ops.ResizePlan":
        return self.inner.frame_plan(src_hw, image_size)

    def reset(self) -> None:
        """Forget the background, the last frame and every counter (the thresholds stay),
        and reset a stateful inner model with them."""
        self.watch_state.reset()
        for st in self._other.values():
            st.reset()
        self.watch_resets += 1
        if self._inner_stateful:
            self.inner.reset()

    def _slot(self, slot0: int) -> dict:
        return {"slot0": slot0} if self._inner_stateful else {}

    def _state_for(self, hw) -> "ops.WatchState":
        if hw == self.watch_state.frame_hw:
            return self.watch_state
        if hw not in self._other:
            self._other[hw] = self._new_state(hw)
        return self._other[hw]

    def _watch(self, out, src: torch.Tensor, slot0: int, src_format: str = "rgb"):
        hw = ((int(src.shape[1]) * 2 // 3, int(src.shape[2])) if src_format == "nv12"
              else (int(src.shape[1]), int(src.shape[2])))
        stats, mask = ops.frame_watch(src, self._state_for(hw), slot0=slot0,
                                      src_format=src_format)
        return (*out, stats, mask)

    def __call__(self, frames_u8: torch.Tensor, slot0: int = 0):
        """Model-size frames: watched as RGB."""
        out = tuple(self.inner(frames_u8, **self._slot(slot0)))
        return self._watch(out, frames_u8, slot0)

    def from_source(self, source_frames: torch.Tensor, frames: torch.Tensor,
                    plan: "ops.ResizePlan", slot0: int = 0, **fmt):
        """Native-resolution serving: the inner model as the engine would call it, then the
        watch on the native ``source_frames`` (``src_format="nv12"``: on their luma plane)."""
        if hasattr(self.inner, "from_source"):
            out = self.inner.from_source(source_frames, frames, plan, **self._slot(slot0), **fmt)
        else:
            out = self.inner(frames, **self._slot(slot0))
            if hasattr(self.inner, "to_source"):
                out = self.inner.to_source(out, plan)
        return self._watch(tuple(out), source_frames, slot0, fmt.get("src_format", "rgb"))


def decode_stats(row) -> dict:
    """One ``cam_stats`` row (16 ints) by name: levels in luma (mean, sharpness), the grid,
    and per condition whether it holds now, its alarm, its run length and its raise count."""
    row = [int(v) for v in row]
    out = {"mean": row[0] / 16.0, "sharpness": row[1] / 16.0, "moving_cells": row[2],
           "cells": row[3]}
    for c, name in enumerate(ops.WATCH_CONDITIONS):
        out[name] = {"now": bool(row[4] >> c & 1), "alarm": bool(row[5] >> c & 1),
                     "run": row[6 + c], "raised": row[11 + c]}
    return out


def watched(model) -> Optional[KvWatched]:
    """``model`` if it is a KvWatched, else None."""
    return model if isinstance(model, KvWatched) else None
