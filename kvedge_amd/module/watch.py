"""Host side of the frame watch: exact running totals of the raised alarms from the device's
wrapping int32 counters, and the per-camera view of the ``cam_stats`` rows."""
from __future__ import annotations

from typing import Any, Dict, List

import torch

from .. import ops
from ..models.watching import decode_stats

_M32 = (1 << 32) - 1


class CameraTotals:
    """Python-int totals per camera of a KvWatched model's ``raised`` counters, kept the way
    zones.ZoneTotals keeps its totals: every ``update()`` adds the counters' change since the
    last one modulo 2^32.  A ``reset()`` of the model starts the totals over."""

    def __init__(self, model):
        self.model = model
        self.rebase()

    def _read(self) -> List[List[int]]:
        return self.model.watch_state.raised.to("cpu").tolist()  # syncs with the device

    def rebase(self) -> None:
        """Totals to zero, measured from the counters as they are now."""
        self._last = self._read()
        self._epoch = self.model.watch_resets
        self.totals = [[0] * len(ops.WATCH_CONDITIONS) for _ in self._last]

    def update(self) -> "CameraTotals":
        if self.model.watch_resets != self._epoch:
            self._last = [[0] * len(row) for row in self._last]
            self._epoch = self.model.watch_resets
            self.totals = [[0] * len(row) for row in self._last]
        now = self._read()
        for cam, (row, last) in enumerate(zip(now, self._last)):
            for c in range(len(row)):
                self.totals[cam][c] += (row[c] - last[c]) & _M32
        self._last = now
        return self

    def summed(self) -> Dict[str, int]:
        """``{condition: alarms raised}`` over all cameras."""
        return {name: sum(t[c] for t in self.totals)
                for c, name in enumerate(ops.WATCH_CONDITIONS)}

    def per_camera(self, stats) -> List[Dict[str, Any]]:
        """The ``cam_stats`` rows (int32 [N, 16], any device) decoded by name, ``raised``
        replaced by this object's exact totals."""
        out = []
        for cam, row in enumerate(stats.to("cpu").tolist()):
            d = decode_stats(row)
            for c, name in enumerate(ops.WATCH_CONDITIONS):
                d[name]["raised"] = self.totals[cam][c]
            out.append(d)
        return out


def alarm_counts(stats) -> Dict[str, int]:
    """``{condition: cameras whose alarm bit is set now}`` from ``cam_stats`` [N, 16]."""
    alarms = stats[:, 5].to("cpu")
    return {name: int(((alarms >> c) & 1).sum()) for c, name in enumerate(ops.WATCH_CONDITIONS)}


# -- motion regions (ops.motion_blobs behind KvWatched(regions=...))
REGIONS_PER_MESSAGE = 8  # per camera in a telemetry message; `regions_total` has the count


def apply_motion_regions(regions, cfg) -> "ops.MotionRegions":
    """min_cells and the ignore polygons of the config into an ops.MotionRegions: both are read
    on the device at every step, so this needs no rebuild."""
    regions.set_min_cells(min(cfg.watch_region_min_cells, regions.grid[0] * regions.grid[1]))
    polys: List[list] = [[] for _ in range(regions.streams)]
    for r in cfg.watch_ignore:
        for cam in (r["cameras"] if r["cameras"] is not None else range(regions.streams)):
            polys[cam].append(r["polygon"])
    # every camera's cells on the host, then one upload
    return regions.set_ignore(None, torch.stack([regions.rasterise(p) for p in polys]))


def build_motion_regions(cfg, device) -> "ops.MotionRegions":
    size = cfg.resolved_image_size()
    return apply_motion_regions(
        ops.MotionRegions(cfg.batch, cfg.frame_hw() or (size, size), cfg.watch_cell,
                          device=device), cfg)


def camera_regions(model, outputs) -> List[List[List[int]]]:
    """Per camera the reported blobs of the step as [x1, y1, x2, y2, cells], largest first."""
    det = outputs[model.blob_index].to("cpu")  # syncs with the device
    cnt = outputs[model.blob_index + 1].to("cpu").tolist()
    return [[[int(v) for v in row[:5]] for row in det[cam, :n].tolist()]
            for cam, n in enumerate(cnt)]


def regions_summary(model, outputs) -> List[Dict[str, Any]]:
    """The telemetry's ``regions``: one entry per camera with at least one region --
    ``camera``, at most REGIONS_PER_MESSAGE ``regions`` and ``regions_total``."""
    return [{"camera": cam, "regions": rows[:REGIONS_PER_MESSAGE], "regions_total": len(rows)}
            for cam, rows in enumerate(camera_regions(model, outputs)) if rows]
