"""Host side of the camera snapshots: which pictures leave the module, and as what.

Every step only the ``snap_len`` row (4 bytes per camera) comes to the host; the bytes of a
picture are copied only for a camera that sends one -- when one of its watch alarms was raised
in this step (``alarm:<condition>``, read off module.watch.CameraTotals) or its periodic timer
ran out (``periodic``) -- or when direct method ``snapshot`` asks for it.

With ``snapshot_annotate`` the pictures carry the boxes, labels and the privacy mosaic
(ops.annotate); the twin's style keys become an ops.AnnotateStyle here, and are written into
it again whenever one of them changes."""
from __future__ import annotations

import base64
from typing import Any, Dict, List, Optional, Tuple

from .. import ops
from ..models.snapshots import snapshots_of


def apply_annotate_style(style: "ops.AnnotateStyle", cfg) -> "ops.AnnotateStyle":
    """Write the twin's snapshot_* style keys into ``style`` (device memory: the captured step
    reads it at every replay).  Privacy zone i of the config is polygon i on the cameras it
    names (all by default)."""
    style.set_boxes(cfg.snapshot_boxes).set_labels(cfg.snapshot_labels)
    style.set_thickness(cfg.snapshot_box_thickness).set_label_scale(cfg.snapshot_label_scale)
    style.set_privacy_classes(cfg.snapshot_privacy_classes)
    style.set_privacy_block(cfg.snapshot_privacy_block).clear_privacy_polygons()
    for i, r in enumerate(cfg.snapshot_privacy_zones):
        for cam in (r["cameras"] if r["cameras"] is not None else [None]):
            style.set_privacy_polygon(i, r["polygon"], camera=cam)
    return style


def build_annotate_style(cfg, device) -> "ops.AnnotateStyle":
    return apply_annotate_style(ops.AnnotateStyle(cfg.batch, device), cfg)


class SnapshotSender:
    def __init__(self, model, cameras: int, now: float):
        self.stage = snapshots_of(model)
        if self.stage is None:
            raise ValueError("the model has no KvSnapshots stage")
        self.cameras = int(cameras)
        self.sent = 0
        self.oversize = 0
        self._raised: Optional[List[List[int]]] = None  # CameraTotals.totals as last seen
        self._last_periodic = [now] * self.cameras

    def _picture(self, outputs, camera: int, length: int) -> bytes:
        return bytes(outputs[self.stage.snap_index][camera, :length].to("cpu").tolist())

    def message(self, outputs, camera: int, length: int) -> Dict[str, Any]:
        h, w = self.stage.thumb_hw
        msg = {"camera": camera, "width": w, "height": h, "bytes": length,
               "jpeg_b64": base64.b64encode(self._picture(outputs, camera, length)).decode()}
        if self.stage.annotate is not None:
            msg["annotated"] = True
        return msg

    def due(self, totals, now: float, every_s: float) -> List[Tuple[int, str]]:
        """(camera, reason) of every picture this step owes.  ``totals``: an updated
        CameraTotals, or None with the watch off."""
        out = []
        if totals is not None:
            seen, cur = self._raised, totals.totals
            if seen is None or any(c < s for a, b in zip(cur, seen) for c, s in zip(a, b)):
                seen = [[0] * len(r) for r in cur]  # a new build, or the model was reset
            for cam, (row, old) in enumerate(zip(cur, seen)):
                for c, name in enumerate(ops.WATCH_CONDITIONS):
                    if row[c] > old[c]:
                        out.append((cam, f"alarm:{name}"))
            self._raised = [list(r) for r in cur]
        if every_s > 0:
            for cam in range(self.cameras):
                if now - self._last_periodic[cam] >= every_s:
                    self._last_periodic[cam] = now
                    out.append((cam, "periodic"))
        return out

    def step(self, outputs, totals, now: float, step: int, every_s: float, max_bytes: int,
             send) -> None:
        """After a step: send what is due through ``send(message)``."""
        lengths = outputs[self.stage.snap_index + 1].to("cpu").tolist()  # syncs with the device
        for cam, reason in self.due(totals, now, every_s):
            n = int(lengths[cam])
            if n < 0 or n > max_bytes:  # (negative: it did not even fit the device row)
                self.oversize += 1
                continue
            msg = self.message(outputs, cam, n)
            out = {"camera": cam, "reason": reason, "step": step, "width": msg["width"],
                   "height": msg["height"], "bytes": n, "jpeg_b64": msg["jpeg_b64"]}
            if "annotated" in msg:
                out["annotated"] = True
            send(out)
            self.sent += 1

    def method(self, outputs, payload, max_bytes: int) -> Tuple[int, Dict[str, Any]]:
        """Direct method ``snapshot`` {camera: n}: the camera's picture of the last step."""
        try:
            cam = int((payload or {}).get("camera"))
        except (TypeError, ValueError):
            return 400, {"error": "payload must be {camera: n}"}
        if outputs is None or self.stage.snap_index is None:
            return 400, {"error": "no step has run yet"}
        if not 0 <= cam < self.cameras:
            return 400, {"error": f"camera {cam} outside 0..{self.cameras - 1}"}
        n = int(outputs[self.stage.snap_index + 1][cam])
        if n < 0 or n > max_bytes:
            return 413, {"error": f"picture of {abs(n)} bytes exceeds snapshot_max_bytes",
                         "camera": cam, "bytes": abs(n)}
        return 200, self.message(outputs, cam, n)

    def summary(self) -> Dict[str, int]:
        return {"sent": self.sent, "oversize": self.oversize}
