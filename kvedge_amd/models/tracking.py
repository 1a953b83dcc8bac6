"""Multi-object tracking on top of a detector: the same object keeps the same id from frame
to frame.

``KvTracked`` wraps a model whose outputs start with ``(det, count)`` (KvYoloV8n,
KvDetectClassify) and appends ``track_id`` int32 [N, max_det] to them.  One batch row = one
camera: with tracking on, row n of every batch is the next frame of stream ``slot0 + n``, so a
module of batch B serves B cameras, one frame each per step.  The tracker state lives in
device memory (ops.TrackState) and is updated by one kernel launch per step
(ops.track_update, csrc/kernels/track.hip): no host in the loop, so the step stays one
captured graph -- the state tensors are allocated here, outside the graph's pool, and persist
across replays.

``KvZoned`` wraps a ``KvTracked`` and counts its tracks against virtual lines and polygon zones
(ops.zone_update, csrc/kernels/zones.hip): one more launch per step, counters in device memory.
"""
from __future__ import annotations

from typing import List

import torch

from .. import ops


class KvTracked:
    """inner outputs ``(det, count, ...)`` -> ``(det, count, ..., track_id)``; ``track_index``
    is the position of ``track_id`` in them.  Tracking runs
    on the boxes as they are reported: frame pixels when the engine has a frame size
    (``from_source``), model pixels otherwise."""

    stateful = True  # InferenceEngine passes slot0 = first batch row of the slice

    def __init__(self, inner, streams: int, iou: float = 0.3, max_age: int = 30,
                 min_hits: int = 3, max_tracks: int = 64, class_aware: bool = True):
        self.inner = inner
        self.device = inner.device
        self.iou, self.max_age, self.min_hits = float(iou), int(max_age), int(min_hits)
        self.class_aware = bool(class_aware)
        if not 1 <= ops.track_thr_q(self.iou) <= 1024:
            raise ValueError(f"track iou {iou} outside (0, 1]")
        if not 0 <= self.max_age <= 255:
            raise ValueError(f"max_age {max_age} outside 0..255")
        if not 1 <= self.min_hits <= 255:
            raise ValueError(f"min_hits {min_hits} outside 1..255")
        self.state = ops.TrackState(streams, max_tracks, self.device)
        self.image_size = getattr(inner, "image_size", 640)
        self.track_index = None  # position of track_id in the outputs, set by the first step

    # -- what the engine, the autotuner and the module read off a model
    def convs(self) -> List:
        return self.inner.convs()

    def flops_per_image(self, hw: int = 640) -> int:
        return self.inner.flops_per_image(hw)

    def frame_plan(self, src_hw, image_size: int = 0) -> "ops.ResizePlan":
        return self.inner.frame_plan(src_hw, image_size)

    def reset(self) -> None:
        """Forget every track; ids restart at 0."""
        self.state.reset()

    def _track(self, out, slot0: int):
        det, count = out[0], out[1]
        tid = ops.track_update(det, count, self.state, slot0=slot0, iou=self.iou,
                               max_age=self.max_age, min_hits=self.min_hits,
                               class_aware=self.class_aware)
        self.track_index = len(out)
        return (*out, tid)

    def __call__(self, frames_u8: torch.Tensor, slot0: int = 0):
        return self._track(tuple(self.inner(frames_u8)), slot0)

    def from_source(self, source_frames: torch.Tensor, frames: torch.Tensor,
                    plan: "ops.ResizePlan", slot0: int = 0, **fmt):
        """Native-resolution serving: the inner model's boxes in frame pixels, then the
        tracker on those."""
        if hasattr(self.inner, "from_source"):
            out = self.inner.from_source(source_frames, frames, plan, **fmt)
        else:
            out = self.inner.to_source(self.inner(frames), plan)
        return self._track(tuple(out), slot0)


class KvZoned:
    """A ``KvTracked`` model plus virtual lines and polygon zones: outputs
    ``(det, count, ..., track_id)`` -> ``(det, count, ..., track_id, zone_mask, zone_counts)``.
    One more launch per step (ops.zone_update, csrc/kernels/zones.hip) reads the tracker state
    the step just updated and keeps per-camera counters in device memory (ops.ZoneState): line
    crossings by direction, zone entries, exits, occupancy and dwell frames.  ``zones``
    (ops.ZoneSet, one table row per camera) is in the pixel frame the boxes are reported in:
    frame pixels when the engine has a frame size, model pixels otherwise.  The model takes the
    set over: ``anchor`` ("bottom" or "centre") is written into it (``zones.set_anchor``),
    replacing whatever mode the set held, and later ``set_line`` / ``set_zone`` calls on it take
    effect from the next step."""

    stateful = True

    def __init__(self, inner_tracked: KvTracked, zones: "ops.ZoneSet", anchor="bottom"):
        if not isinstance(inner_tracked, KvTracked):
            raise TypeError("KvZoned wraps a KvTracked model")
        self.inner = inner_tracked
        self.device = inner_tracked.device
        self.state = inner_tracked.state  # the tracker's, as the telemetry reads it
        if zones.streams != self.state.streams or zones.device != self.state.device:
            raise ValueError(f"zones cover {zones.streams} streams on {zones.device}, the tracker "
                             f"{self.state.streams} on {self.state.device}")
        self.zones = zones.set_anchor(anchor)
        self.zone_state = ops.ZoneState(self.state.streams, self.state.max_tracks, self.device)
        self.resets = 0  # bumped by reset(): host-side totals start over with the counters
        self.image_size = inner_tracked.image_size

    def convs(self) -> List:
        return self.inner.convs()

    def flops_per_image(self, hw: int = 640) -> int:
        return self.inner.flops_per_image(hw)

    def frame_plan(self, src_hw, image_size: int = 0) -> "ops.ResizePlan":
        return self.inner.frame_plan(src_hw, image_size)

    def reset(self) -> None:
        """Forget every track and zero every counter, together."""
        self.inner.reset()
        self.zone_state.reset()
        self.resets += 1

    def _zones(self, out, slot0: int):
        mask, counts = ops.zone_update(out[0], out[1], self.state, self.zone_state, self.zones,
                                       slot0=slot0)
        return (*out, mask, counts)

    def __call__(self, frames_u8: torch.Tensor, slot0: int = 0):
        return self._zones(self.inner(frames_u8, slot0=slot0), slot0)

    def from_source(self, source_frames: torch.Tensor, frames: torch.Tensor,
                    plan: "ops.ResizePlan", slot0: int = 0, **fmt):
        return self._zones(self.inner.from_source(source_frames, frames, plan, slot0=slot0,
                                                  **fmt), slot0)
