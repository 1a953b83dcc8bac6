"""Detect-then-classify cascade: YOLOv8n finds the objects, ResNet-50 says what each one is.

One step on the device, no host in the loop: detect -> ops.roi_crop (the top-K kept boxes of
every image cut from the frame and stretched to the classifier's input size, read straight
from the NMS output in device memory) -> classify.  The engine captures it into one hipGraph
like any other model.

Shapes are static, so every image always yields K crops: slots past the image's detection
count hold ``pad`` pixels, still run through the classifier (the cost of a capturable graph:
the classifier always sees N * K images, however few boxes were kept) and are masked in the
outputs -- class -1, probability 0.
"""
from __future__ import annotations

from typing import List

import torch

from .. import ops
from .resnet import KvResNet50
from .yolov8 import KvYoloV8n

CROP_PAD = 0  # fill of the crop slots without a detection (masked in the outputs anyway)


class KvDetectClassify:
    """frames u8 [N,640,640,3] -> (det fp32 [N,max_det,6], count int32 [N],
    crop_cls int64 [N,K], crop_prob fp32 [N,K]).  ``crop_cls[n, k]`` / ``crop_prob[n, k]``
    are the classifier's top-1 class and its probability for detection row k of image n
    (rows are ordered by score); -1 / 0 where k >= count[n]."""

    image_size = 640

    def __init__(self, detector: KvYoloV8n, classifier: KvResNet50, crops_per_image: int,
                 crop_size: int = 224):
        if not 1 <= crops_per_image <= detector.max_det:
            raise ValueError(f"crops_per_image must be 1..max_det = {detector.max_det}, "
                             f"got {crops_per_image}")
        if crop_size < 32 or crop_size % 32:
            raise ValueError(f"crop_size must be a positive multiple of 32, got {crop_size}")
        self.detector, self.classifier = detector, classifier
        self.k, self.crop_size = int(crops_per_image), int(crop_size)
        self.device = detector.device
        self._slots = torch.arange(self.k, device=self.device).view(1, self.k)

    def convs(self) -> List:
        return self.detector.convs() + self.classifier.convs()

    def flops_per_image(self, hw: int = 640) -> int:
        """Detector FLOPs plus K classifier passes (invalid slots are computed too)."""
        return (self.detector.flops_per_image(hw) +
                self.k * self.classifier.flops_per_image(self.crop_size))

    def frame_plan(self, src_hw, image_size: int = 0) -> "ops.ResizePlan":
        """The detector's letterbox; the crops are cut from the native frames."""
        return self.detector.frame_plan(src_hw, image_size)

    def classify(self, src_u8: torch.Tensor, det: torch.Tensor, count: torch.Tensor,
                 src_format: str = "rgb"):
        """Boxes ``det`` / ``count`` in ``src_u8`` pixels -> (crop_cls, crop_prob) [N, K].
        ``src_format="nv12"``: ``src_u8`` is NV12 [N, Hs * 3 // 2, Ws] and the crops are cut
        from it directly.  Device ops only: no host sync, capturable."""
        n = src_u8.shape[0]
        crops = ops.roi_crop(src_u8, det, count, self.k, self.crop_size, pad=CROP_PAD,
                             src_format=src_format)
        probs, top1 = self.classifier(crops)
        top1 = top1.view(n, self.k)
        prob = probs.gather(1, top1.view(-1, 1)).view(n, self.k)
        invalid = self._slots >= count.view(n, 1)
        return top1.masked_fill(invalid, -1), prob.masked_fill(invalid, 0.0)

    def __call__(self, frames_u8: torch.Tensor):
        """Model-size frames: the crops come from the frames the detector saw."""
        det, count = self.detector(frames_u8)
        crop_cls, crop_prob = self.classify(frames_u8, det, count)
        return det, count, crop_cls, crop_prob

    def from_source(self, source_frames: torch.Tensor, frames: torch.Tensor,
                    plan: "ops.ResizePlan", src_format: str = "rgb"):
        """Native-resolution serving (InferenceEngine(frame_hw=...)): detect on the resized
        ``frames``, map the kept boxes to frame pixels, cut the crops from ``source_frames``
        at full resolution (``src_format="nv12"``: from the NV12 frames)."""
        det, count = self.detector.to_source(self.detector(frames), plan)
        crop_cls, crop_prob = self.classify(source_frames, det, count, src_format=src_format)
        return det, count, crop_cls, crop_prob
