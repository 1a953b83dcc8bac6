"""Sliced detection: small objects in large frames.

A 1080p frame reaches YOLOv8n through one 640 x 640 letterbox, so a person 40 px tall is 13 px
tall to the model and is lost.  ``KvSliced`` wraps a ``KvYoloV8n`` and, when the engine serves
native frames, also detects on a grid of overlapping tiles at their higher scale: the tiles are
cut from the native frame on the device (ops.frame_warp over ops.slice_views), the model runs
once on all of them plus the engine's own full-frame letterbox, every group's boxes go back to
frame pixels (ops.view_to_source / ops.det_to_source) and one launch merges them into a single
detection list per camera (ops.det_merge, csrc/kernels/det_merge.hip).  No host in the loop: the
step stays one captured graph, and what comes out is ``(det, count)`` in frame pixels with the
inner model's ``max_det`` -- KvTracked, KvZoned, KvWatched and KvSnapshots wrap it unchanged.
"""
from __future__ import annotations

from typing import List

import torch

from .. import ops
from .yolov8 import KvYoloV8n


class KvSliced:
    """``inner`` (a KvYoloV8n) over ``grid`` = (cols, rows) tiles of every frame, neighbours
    sharing ``overlap`` of their size (ops.slice_rois), plus the full frame when ``full``;
    ``mode`` / ``metric`` / ``thr`` are ops.det_merge's.  ``streams``: the most cameras one
    call serves.  Called without native frames it is the inner model."""

    def __init__(self, inner: KvYoloV8n, streams: int, grid=(2, 2), overlap: float = 0.2,
                 full: bool = True, mode: str = "nmm", metric: str = "ios", thr: float = 0.5):
        if not isinstance(inner, KvYoloV8n):
            raise ValueError("KvSliced wraps a KvYoloV8n (the detect-classify cascade is not "
                             f"sliced), got {type(inner).__name__}")
        if mode not in ops.MERGE_MODES or metric not in ops.MERGE_METRICS:
            raise ValueError(f"mode / metric must be of {ops.MERGE_MODES} / {ops.MERGE_METRICS}, "
                             f"got {mode!r} / {metric!r}")
        if not 1 <= ops.track_thr_q(thr) <= 1024:
            raise ValueError(f"merge threshold {thr} outside (0, 1]")
        if streams < 1:
            raise ValueError(f"streams must be >= 1, got {streams}")
        self.inner, self.device = inner, inner.device
        self.streams, self.full = int(streams), bool(full)
        cols, rows, self.overlap = ops.check_slice_grid(grid, overlap)
        self.grid = (cols, rows)
        self.tiles = self.grid[0] * self.grid[1]
        self.groups = self.tiles + int(self.full)
        if self.groups * inner.max_det > ops.MERGE_MAX_CANDIDATES:
            raise ValueError(f"{self.groups} groups of max_det {inner.max_det} exceed the merge's "
                             f"{ops.MERGE_MAX_CANDIDATES} candidates")
        self.mode, self.metric, self.thr = mode, metric, float(thr)
        self.image_size = inner.image_size
        self.views = None  # ops.slice_views, made by frame_plan (or by the first call)

    def convs(self) -> List:
        return self.inner.convs()

    def flops_per_image(self, hw: int = 640) -> int:
        return self.inner.flops_per_image(hw)

    def frame_plan(self, src_hw, image_size: int = 0) -> "ops.ResizePlan":
        """The inner model's plan; the tile views of that frame size are made here, when the
        engine is built, so that no step and no stream slice has to."""
        plan = self.inner.frame_plan(src_hw, image_size)
        self._views_for(plan.src_hw, tuple(plan.dst_hw))
        return plan

    def _views_for(self, src_hw, dst_hw) -> "ops.CameraViews":
        if (self.views is None or self.views.src_hw != tuple(src_hw)
                or self.views.dst_hw != tuple(dst_hw)):
            self.views = ops.slice_views(self.streams, src_hw, dst_hw, self.grid, self.overlap,
                                         self.device)
            if self.device.type == "cuda":  # filled on this stream, read on any
                torch.cuda.synchronize(self.device)
        return self.views

    def to_source(self, outputs, plan: "ops.ResizePlan"):
        return self.inner.to_source(outputs, plan)

    def __call__(self, frames_u8: torch.Tensor):
        return self.inner(frames_u8)

    def tile_frames(self, source_frames: torch.Tensor, frames: torch.Tensor,
                    plan: "ops.ResizePlan", **fmt) -> torch.Tensor:
        """Every group's model input [groups * n, S, S, 3], group-major: tile g of the n frames
        in rows [g * n, (g + 1) * n), the full frames last.  A buffer of its own per call
        (ops.empty: the graph's pool under capture), so the engine's stream slices, which run
        side by side, share nothing; the views are read only."""
        if isinstance(plan, ops.ViewSlots):
            raise ValueError("sliced detection cuts its own tile views: engine views are not "
                             "supported with it")
        n, size = int(frames.shape[0]), int(frames.shape[1])
        if n > self.streams:
            raise ValueError(f"{n} frames, KvSliced was built for {self.streams} streams")
        views = self._views_for(plan.src_hw, (size, size))
        buf = ops.empty(self.groups * n, size, size, 3, dtype=torch.uint8, device=self.device)
        for g in range(self.tiles):
            ops.frame_warp(source_frames, views, out=buf[g * n:(g + 1) * n],
                           slot0=g * self.streams, **fmt)
        if self.full:
            buf[self.tiles * n:].copy_(frames)
        return buf

    def group_outputs(self, source_frames: torch.Tensor, frames: torch.Tensor,
                      plan: "ops.ResizePlan", **fmt):
        """Every group's detections in frame pixels, before the merge: (det fp32
        [groups * n, max_det, 6], count int32 [groups * n]), group-major, the full frame last."""
        n = int(frames.shape[0])
        det, count = self.inner(self.tile_frames(source_frames, frames, plan, **fmt))
        for g in range(self.tiles):
            ops.view_to_source(det[g * n:(g + 1) * n], count[g * n:(g + 1) * n], self.views,
                               slot0=g * self.streams)
        if self.full:
            ops.det_to_source(det[self.tiles * n:], count[self.tiles * n:], plan)
        return det, count

    def from_source(self, source_frames: torch.Tensor, frames: torch.Tensor,
                    plan: "ops.ResizePlan", **fmt):
        """Native-resolution serving: ``frames`` is the engine's full-frame model input of
        ``source_frames`` (RGB, or NV12 with ``src_format="nv12"``) under ``plan``."""
        det, count = self.group_outputs(source_frames, frames, plan, **fmt)
        return ops.det_merge(det, count, self.groups, mode=self.mode, metric=self.metric,
                             thr=self.thr, max_det=self.inner.max_det)
