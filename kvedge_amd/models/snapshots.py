"""Camera snapshots on top of any deployed model: a picture of what each camera sees, made on
the device from the frame that is already there.

``KvSnapshots`` wraps a model (KvResNet50, KvYoloV8n, KvDetectClassify, KvTracked, KvZoned) and
appends ``(snap_jpeg, snap_len)`` to its outputs: uint8 [N, cap] and int32 [N], one baseline
JPEG file per batch row -- one batch row = one camera, as for the tracker and the watch.  Every
step the camera's current frame is stretched to a thumbnail (ops.thumbnail_plan through
ops.frame_resize, from the native-resolution frame when the engine has a frame size, RGB or
NV12) and encoded (ops.jpeg_encode, csrc/kernels/jpeg_encode.hip): four more launches per step
inside the captured graph, no host in the loop.  The encoder's tables and workspaces
(ops.JpegEncoder) are allocated here, outside the graph's pool; ``set_quality`` rewrites the
tables in place, so a captured step encodes at the new quality from its next replay.

With ``annotate`` (an ops.AnnotateStyle) one more launch between the two draws what the device
knows into the thumbnail before it is encoded (ops.annotate, csrc/kernels/annotate.hip): the
boxes of a detector with their ``cls:id`` labels, and a mosaic over boxes of privacy classes
and over fixed privacy polygons.  The style's setters take effect from the next replay too.

A ``KvWatched`` goes around this wrapper, not inside it: the watch stays the outermost stage
and its two outputs the last two.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .. import ops
from .tracking import KvTracked


class KvSnapshots:
    """inner outputs ``(...)`` -> ``(..., snap_jpeg, snap_len)``; ``snap_index`` is the
    position of ``snap_jpeg`` in them (``snap_len`` follows it).  ``frame_hw``: the size of the
    frames the engine serves from (InferenceEngine ``frame_hw``); None = model-size frames.
    ``width``: thumbnail width; the height follows the frame's shape (ops.thumbnail_plan).
    ``cap``: bytes per output row (default and upper limit: ops.jpeg_max_bytes of the
    thumbnail, the derived worst case); a file that does not fit gives ``snap_len = -size``.
    ``annotate``: an ops.AnnotateStyle for ``streams`` cameras, in the pixel frame the boxes are
    reported in (frame pixels when the engine has a frame size, model pixels otherwise); None
    = bare pictures, exactly the launches and bytes of a stage without it."""

    stateful = True  # InferenceEngine passes slot0 = first batch row of the slice

    def __init__(self, inner, streams: int, frame_hw=None, width: int = 320,
                 subsampling: str = "420", quality: int = 75, cap: Optional[int] = None,
                 annotate: Optional["ops.AnnotateStyle"] = None):
        self.inner = inner
        self.device = inner.device
        self.image_size = getattr(inner, "image_size", 224)
        self.streams = int(streams)
        self.width, self.subsampling, self.quality = int(width), subsampling, int(quality)
        self.frame_hw = ((self.image_size, self.image_size) if frame_hw is None
                         else (int(frame_hw[0]), int(frame_hw[1])))
        self._by_hw = {}  # source size -> (plan, encoder); the autotuner runs model-size frames
        self.plan, self.encoder = self._for(self.frame_hw)
        if cap is not None and int(cap) < 1:
            raise ValueError(f"cap must be >= 1, got {cap}")
        self.cap = min(int(cap), self.encoder.max_bytes) if cap else self.encoder.max_bytes
        self.snap_index = None  # set by the first step
        self._inner_stateful = bool(getattr(inner, "stateful", False))
        if annotate is not None:
            if not isinstance(annotate, ops.AnnotateStyle):
                raise TypeError("annotate must be an ops.AnnotateStyle, got "
                                f"{type(annotate).__name__}")
            if (annotate.streams != self.streams
                    or annotate.device.type != torch.device(self.device).type):
                raise ValueError(f"the style covers {annotate.streams} cameras on "
                                 f"{annotate.device}, the stage {self.streams} on {self.device}")
        self.annotate = annotate
        self._tracked = None  # the KvTracked stage inside, whose track_index finds track_id
        m = inner
        while m is not None and self._tracked is None:
            if isinstance(m, KvTracked):
                self._tracked = m
            m = getattr(m, "__dict__", {}).get("inner")

    def _for(self, hw):
        if hw not in self._by_hw:
            plan = ops.thumbnail_plan(hw, self.width)
            enc = ops.JpegEncoder(plan.dst_hw, self.streams, self.subsampling, self.quality,
                                  device=self.device)
            self._by_hw[hw] = (plan, enc)
        return self._by_hw[hw]

    @property
    def thumb_hw(self):
        """(height, width) of the pictures."""
        return self.plan.dst_hw

    def set_quality(self, quality: int) -> "KvSnapshots":
        """JPEG quality 1..100 from the next step on, without recapturing."""
        for _, enc in self._by_hw.values():
            enc.set_quality(quality)
        self.quality = int(quality)
        return self

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
        """Nothing of its own to forget: resets a stateful inner model."""
        if self._inner_stateful:
            self.inner.reset()

    def _slot(self, slot0: int) -> dict:
        return {"slot0": slot0} if self._inner_stateful else {}

    def _snap(self, out, src: torch.Tensor, slot0: int, src_format: str = "rgb"):
        hw = ((int(src.shape[1]) * 2 // 3, int(src.shape[2])) if src_format == "nv12"
              else (int(src.shape[1]), int(src.shape[2])))
        plan, enc = self._for(hw)
        n = int(src.shape[0])
        small = ops.frame_resize(src, plan, out=ops.empty(n, *plan.dst_hw, 3, dtype=torch.uint8,
                                                          device=src.device),
                                 src_format=src_format)
        if self.annotate is not None:
            ops.annotate(small, self.annotate, *self._boxes(out, n), src_hw=hw, slot0=slot0)
        buf = ops.empty(n, min(self.cap, enc.max_bytes), dtype=torch.uint8, device=src.device)
        length = ops.empty(n, dtype=torch.int32, device=src.device)
        ops.jpeg_encode(small, enc, out=buf, lengths=length, slot0=slot0)
        self.snap_index = len(out)
        return (*out, buf, length)

    def _boxes(self, out, n: int):
        """(det, count, track_id) among the inner outputs: the first two of a detector, and
        the tracker's ids where it recorded them; (None, None, None) for a classifier."""
        if not (len(out) >= 2 and out[0].dtype == torch.float32 and out[0].dim() == 3
                and out[0].shape[0] == n and out[0].shape[2] == 6
                and out[1].dtype == torch.int32 and tuple(out[1].shape) == (n,)):
            return None, None, None
        tid = None
        if self._tracked is not None and self._tracked.track_index is not None:
            tid = out[self._tracked.track_index]
        return out[0], out[1], tid

    def __call__(self, frames_u8: torch.Tensor, slot0: int = 0):
        """Model-size frames: the picture is the model's own input, resized."""
        out = self.inner(frames_u8, **self._slot(slot0))
        out = (out,) if isinstance(out, torch.Tensor) else tuple(out)
        return self._snap(out, frames_u8, slot0)

    def from_source(self, source_frames: torch.Tensor, frames: torch.Tensor,
                    plan: "ops.ResizePlan", slot0: int = 0, **fmt):
        """Native-resolution serving: the inner model as the engine would call it, then the
        picture from the native ``source_frames`` (RGB, or NV12 with ``src_format="nv12"``)."""
        if hasattr(self.inner, "from_source"):
            out = self.inner.from_source(source_frames, frames, plan, **self._slot(slot0), **fmt)
        else:
            out = self.inner(frames, **self._slot(slot0))
            if hasattr(self.inner, "to_source"):
                out = self.inner.to_source(out, plan)
        out = (out,) if isinstance(out, torch.Tensor) else tuple(out)
        return self._snap(out, source_frames, slot0, fmt.get("src_format", "rgb"))


def snapshots_of(model) -> Optional[KvSnapshots]:
    """The KvSnapshots stage of ``model`` -- the model itself, or the one inside its watch --
    else None."""
    for m in (model, getattr(model, "__dict__", {}).get("inner")):
        if isinstance(m, KvSnapshots):
            return m
    return None
