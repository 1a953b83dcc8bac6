"""Appearance search in the module: the gallery behind KvDetectClassify(gallery=...), the
telemetry's ``matches`` and the direct methods ``gallery_enrol`` / ``gallery_remove``.

The gallery lives in device memory and the captured step reads its rows and its count at every
replay, so enrolling and removing need no rebuild; only the path and ``gallery_top`` do."""
from __future__ import annotations

import os
from typing import Any, Dict, List, Tuple

import torch

from .. import ops

MATCHES_PER_MESSAGE = 16  # rows of (camera, row, label, cos) a telemetry message carries
MIN_CAPACITY = 4096      # room to enrol into a gallery that starts small or empty


def build_gallery(cfg, device, dim: int = 2048) -> "ops.Gallery":
    """The gallery of ``cfg.gallery`` (an .npz of ops.Gallery.save; a path that does not exist
    yet starts empty), with room for at least as many rows again."""
    rows = 0
    if os.path.exists(cfg.gallery):
        import numpy as np

        with np.load(cfg.gallery) as z:
            rows = int(z["codes"].shape[0])
    cap = min(ops.GALLERY_MAX_CAPACITY, max(MIN_CAPACITY, 2 * rows))
    if rows:
        gal = ops.Gallery.load(cfg.gallery, capacity=cap, device=device)
        if gal.dim != dim:
            raise ValueError(f"{cfg.gallery}: rows of width {gal.dim}, the classifier embeds {dim}")
        return gal
    return ops.Gallery(cap, dim, device)


def match_rows(label: torch.Tensor, cos: torch.Tensor) -> List[Tuple[int, int, int, float]]:
    """(camera, row, label, cos) of every crop whose best match has a label, best first."""
    label, cos = label[..., 0].cpu(), cos[..., 0].cpu()
    hit = torch.nonzero(label >= 0)
    rows = [(int(n), int(k), int(label[n, k]), round(float(cos[n, k]), 6)) for n, k in hit]
    return sorted(rows, key=lambda r: (-r[3], r[0], r[1]))


class MatchTotals:
    """Sightings per label over the steps the module looked at (one per report)."""

    def __init__(self):
        self.sightings: Dict[int, int] = {}

    def summary(self, label: torch.Tensor, cos: torch.Tensor) -> Dict[str, Any]:
        rows = match_rows(label, cos)
        for _, _, lab, _ in rows:
            self.sightings[lab] = self.sightings.get(lab, 0) + 1
        return {"matches": {str(k): v for k, v in sorted(self.sightings.items())},
                "match_rows": [list(r) for r in rows[:MATCHES_PER_MESSAGE]]}


def enrol(cascade, batch: int, payload: Dict[str, Any]) -> Tuple[int, Dict[str, Any]]:
    """``gallery_enrol {camera, row, label}``: the embedding crop (camera, row) produced in the
    last step becomes a gallery row of ``label``."""
    try:
        cam, row, label = (int(payload[k]) for k in ("camera", "row", "label"))
    except (KeyError, TypeError, ValueError) as e:
        return 400, {"error": f"gallery_enrol needs camera, row and label: {e}"}
    emb = cascade.embedding
    if emb is None or emb[0].shape[0] != batch * cascade.k:
        return 409, {"error": "no embedding of a whole batch yet (one stream, after a step)"}
    if not (0 <= cam < batch and 0 <= row < cascade.k):
        return 400, {"error": f"camera 0..{batch - 1}, row 0..{cascade.k - 1}"}
    i = cam * cascade.k + row
    try:
        cascade.gallery.enrol(emb[0][i].cpu(), emb[1][i].cpu(), label)
    except ValueError as e:
        return 400, {"error": str(e)}
    return 200, {"rows": len(cascade.gallery), "label": label}


def remove(cascade, payload: Dict[str, Any]) -> Tuple[int, Dict[str, Any]]:
    """``gallery_remove {label}``."""
    try:
        label = int(payload["label"])
    except (KeyError, TypeError, ValueError) as e:
        return 400, {"error": f"gallery_remove needs a label: {e}"}
    return 200, {"removed": cascade.gallery.remove(label), "rows": len(cascade.gallery)}
