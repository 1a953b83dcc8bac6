"""Host side of the frame watch: exact running totals of the raised alarms from the device's
wrapping int32 counters, and the per-camera view of the ``cam_stats`` rows."""
from __future__ import annotations

from typing import Any, Dict, List

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
