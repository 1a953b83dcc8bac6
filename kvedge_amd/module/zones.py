"""Host side of the line / zone counters: the twin's ``lines`` / ``zones`` keys -> an
ops.ZoneSet, and exact running totals from the device's wrapping int32 counters."""
from __future__ import annotations

from typing import Any, Dict, List

from .. import ops
from .config import ModuleConfig

_M32 = (1 << 32) - 1
_ADD = ("line_fwd", "line_back", "zone_enter", "zone_exit", "zone_dwell")  # cumulative groups


def build_zone_set(cfg: ModuleConfig, device) -> "ops.ZoneSet":
    """Region i of the config is line / zone index i on the cameras it names (all by default);
    on the others that index stays empty and counts nothing."""
    zs = ops.ZoneSet(cfg.batch, device)
    for i, r in enumerate(cfg.lines):
        for cam in (r["cameras"] if r["cameras"] is not None else [None]):
            zs.set_line(cam, i, r["a"], r["b"], cls=r["class"])
    for i, r in enumerate(cfg.zones):
        for cam in (r["cameras"] if r["cameras"] is not None else [None]):
            zs.set_zone(cam, i, r["polygon"], cls=r["class"])
    return zs.set_anchor(cfg.zone_anchor)


class ZoneTotals:
    """Python-int totals per camera of a KvZoned model's counters.  The device counters are
    int32 and wrap; every ``update()`` adds their change since the last one modulo 2^32, so
    the totals stay exact as long as fewer than 2^32 events fall between two updates.
    Occupancy is not cumulative and is read as is.  A ``reset()`` of the model (new counters
    from zero) starts the totals over."""

    def __init__(self, model, lines, zones):
        self.model = model
        self.line_names = [r["name"] for r in lines]
        self.zone_names = [r["name"] for r in zones]
        self.rebase()

    def _read(self) -> List[List[int]]:
        return self.model.zone_state.counters.to("cpu").tolist()  # syncs with the device

    def rebase(self) -> None:
        """Totals to zero, measured from the counters as they are now."""
        self._last = self._read()
        self._epoch = self.model.resets
        self.totals = [{g: [0] * 8 for g in _ADD} for _ in self._last]
        self.occupancy = [row[32:40] for row in self._last]

    def update(self) -> "ZoneTotals":
        if self.model.resets != self._epoch:
            self._last = [[0] * 48 for _ in self._last]
            self._epoch = self.model.resets
            self.totals = [{g: [0] * 8 for g in _ADD} for _ in self._last]
        now = self._read()
        for cam, (row, last) in enumerate(zip(now, self._last)):
            for g in _ADD:
                o = 8 * ops.ZONE_COUNTERS.index(g)
                for i in range(8):
                    self.totals[cam][g][i] += (row[o + i] - last[o + i]) & _M32
        self.occupancy = [row[32:40] for row in now]
        self._last = now
        return self

    def camera(self, cam: int) -> Dict[str, Any]:
        t, occ = self.totals[cam], self.occupancy[cam]
        return {
            "lines": {n: {"forward": t["line_fwd"][i], "backward": t["line_back"][i]}
                      for i, n in enumerate(self.line_names)},
            "zones": {n: {"occupancy": occ[i], "entered": t["zone_enter"][i],
                          "exited": t["zone_exit"][i], "dwell_frames": t["zone_dwell"][i]}
                      for i, n in enumerate(self.zone_names)},
        }

    def per_camera(self) -> List[Dict[str, Any]]:
        return [self.camera(c) for c in range(len(self.totals))]

    def summed(self) -> Dict[str, Any]:
        """``{"lines": {name: {forward, backward}}, "zones": {name: {occupancy, entered,
        exited, dwell_frames}}}`` over all cameras."""
        out: Dict[str, Any] = {"lines": {}, "zones": {}}
        for cam in self.per_camera():
            for kind in ("lines", "zones"):
                for name, vals in cam[kind].items():
                    acc = out[kind].setdefault(name, dict.fromkeys(vals, 0))
                    for k, v in vals.items():
                        acc[k] += v
        return out

