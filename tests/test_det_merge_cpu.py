"""Sliced detection without a GPU: ops.reference.det_merge against a float64 / Python-int brute
force on hand-made cases, the tile grid of ops.slice_rois, and the module's slice_* keys."""
import math

import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig


def _brute(groups, thr, metric, class_aware, nmm, max_det):
    """groups: per group a list of (x1, y1, x2, y2, score, cls), quarter-pixel exact."""
    cand = sorted(((-r[4], g, i, r) for g, rows in enumerate(groups) for i, r in enumerate(rows)))
    kept = []  # [row, hull]
    for _, _, _, r in cand:
        if len(kept) == max_det:
            break
        for k, hull in kept:
            inter = max(0.0, min(k[2], r[2]) - max(k[0], r[0])) * max(0.0, min(k[3], r[3]) - max(k[1], r[1]))
            ak, ar = (k[2] - k[0]) * (k[3] - k[1]), (r[2] - r[0]) * (r[3] - r[1])
            denom = ak + ar - inter if metric == "iou" else min(ak, ar)
            if inter > 0 and inter >= thr * denom and (k[5] == r[5] or not class_aware):
                hull[:] = [min(hull[0], r[0]), min(hull[1], r[1]), max(hull[2], r[2]), max(hull[3], r[3])]
                break
        else:
            kept.append((r, list(r[:4])))
    return [(*(h if nmm else k[:4]), k[4], k[5]) for k, h in kept]


WHOLE, HALF = (100, 100, 200, 300), (100, 100, 200, 196)  # HALF: WHOLE cut by a tile border
CASES = {  # name: (groups, metric, max_det)
    "cut_half_scores_lower": ([[(*HALF, 0.6, 0)], [(*WHOLE, 0.9, 0)]], "ios", 4),
    "cut_half_scores_higher": ([[(*HALF, 0.9, 0)], [(*WHOLE, 0.6, 0)]], "ios", 4),
    # a-b and b-c overlap by 60 %, a-c by 20 %: b goes into a, c is kept
    "chain": ([[(0, 0, 100, 50, 0.9, 1)], [(40, 0, 140, 50, 0.8, 1)], [(80, 0, 180, 50, 0.7, 1)]],
              "ios", 4),
    "equal_scores_lower_group_wins": ([[(10, 10, 60, 60, 0.5, 2)], [(12, 10, 62, 64, 0.5, 2)]],
                                      "iou", 4),
    "same_place_other_class": ([[(10, 10, 60, 60, 0.9, 0)], [(10, 10, 60, 60, 0.8, 1)]], "iou", 4),
    "max_det_reached": ([[(0, 0, 10, 10, 0.9, 0), (50, 0, 60, 10, 0.8, 0)],
                         [(100, 0, 110, 10, 0.7, 0), (50, 0, 60, 12, 0.6, 0)]], "ios", 2),
}


@pytest.mark.parametrize("nmm", [True, False])
@pytest.mark.parametrize("class_aware", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_reference_equals_brute_force(name, class_aware, nmm):
    groups, metric, max_det = CASES[name]
    R = max(max_det, *(len(g) for g in groups))  # max_det <= R: unused rows pad the groups
    det = torch.zeros(len(groups), R, 6)
    for g, rows in enumerate(groups):
        det[g, :len(rows)] = torch.tensor(rows, dtype=torch.float32)
    count = torch.tensor([len(g) for g in groups], dtype=torch.int32)
    out, cnt = ops.det_merge(det, count, len(groups), mode="nmm" if nmm else "nms", metric=metric,
                             thr=0.5, class_aware=class_aware, max_det=max_det)
    want = _brute(groups, 0.5, metric, class_aware, nmm, max_det)
    assert int(cnt[0]) == len(want)
    assert torch.equal(out[0, :len(want)], torch.tensor(want, dtype=torch.float32).view(-1, 6))
    assert not out[0, len(want):].any()
    if name.startswith("cut_half") and nmm:  # the whole box, whichever scores higher
        assert len(want) == 1 and want[0][:4] == WHOLE
    if name == "chain":
        assert len(want) == 2 and want[1][4] == pytest.approx(0.7)
    if name == "equal_scores_lower_group_wins":
        assert len(want) == 1 and (nmm or want[0][:4] == (10, 10, 60, 60))
    if name == "same_place_other_class":
        assert len(want) == (2 if class_aware else 1)


def test_det_merge_refuses_what_it_would_truncate():
    det, count = torch.zeros(14, 300, 6), torch.zeros(14, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.det_merge(det, count, 14)  # 14 * 300 > 4096
    with pytest.raises(ValueError):
        ops.det_merge(det[:4], count[:4], 2, max_det=301)
    with pytest.raises(ValueError):
        ops.det_merge(det[:4], count[:4], 3)
    with pytest.raises(ValueError):
        ops.det_merge(det[:4], count[:4], 2, thr=0.0)


@pytest.mark.parametrize("hw", [(1080, 1920), (1078, 1918), (353, 641)])
@pytest.mark.parametrize("grid,overlap", [((2, 2), 0.2), ((4, 3), 0.25), ((1, 4), 0.0),
                                          ((3, 1), 0.5)])
def test_slice_rois_invariants(hw, grid, overlap):
    rois = ops.slice_rois(hw, grid, overlap)
    assert rois == ops.slice_rois(hw, grid, overlap) and len(rois) == grid[0] * grid[1]
    hs, ws = hw[0] & ~1, hw[1] & ~1
    assert len({r[2:] for r in rois}) == 1 and all(v % 2 == 0 for r in rois for v in r)
    w, h = rois[0][2:]
    xs, ys = sorted({r[0] for r in rois}), sorted({r[1] for r in rois})
    assert (len(xs), len(ys)) == grid and rois == [(x, y, w, h) for y in ys for x in xs]
    assert xs[0] == 0 and xs[-1] + w == ws and ys[0] == 0 and ys[-1] + h == hs
    assert all(a + w - b >= math.floor(overlap * w) for a, b in zip(xs, xs[1:]))
    assert all(a + h - b >= math.floor(overlap * h) for a, b in zip(ys, ys[1:]))


def test_slice_views_cut_the_rois():
    """Tile g of camera n, warped, is the resize of that ROI cut out of the frame by hand: 256 px
    tiles of a 448 px frame into 128 px, an exact 2 : 1 (a wrong ROI convention or slot order
    cannot pass; the meshes themselves are ops.view_mesh's, tested with the views)."""
    n, hw = 3, (448, 448)
    src = torch.randint(0, 256, (n, *hw, 3), dtype=torch.uint8,
                        generator=torch.Generator().manual_seed(0))
    views = ops.slice_views(n, hw, (128, 128), (2, 2), 0.25)
    rois = ops.slice_rois(hw, (2, 2), 0.25)
    assert views.streams == 4 * n and rois == [(x, y, 256, 256) for y in (0, 192) for x in (0, 192)]
    for g, (x, y, w, h) in enumerate(rois):
        cut = src[:, y:y + h, x:x + w].contiguous()
        assert torch.equal(ops.frame_warp(src, views, slot0=g * n),
                           ops.frame_resize(cut, ops.letterbox_plan((h, w), 128)))


def test_config_slice_keys():
    base = dict(model="yolov8n", batch=4, frame_height=1080, frame_width=1920)
    assert not set(ModuleConfig.SLICE_KEYS) & set(ModuleConfig().to_dict())
    cfg = ModuleConfig(**base, slice_grid="2x2").validate()
    assert set(ModuleConfig.SLICE_KEYS) <= set(cfg.to_dict())
    assert cfg.slice_dims() == (2, 2) and cfg.slice_tiles() == 4
    assert all(k in ModuleConfig.REBUILD for k in ModuleConfig.SLICE_KEYS)
    assert cfg.needs_rebuild(cfg.apply_patch({"slice_overlap": 0.3}))
    for bad in (dict(slice_grid="5x2"), dict(slice_grid="2"), dict(slice_overlap=0.6),
                dict(slice_mode="soft"), dict(slice_metric="giou"), dict(slice_thr=0.0),
                dict(slice_grid="2x2", model="detect-classify"),
                dict(slice_grid="2x2", model="resnet50"),
                dict(slice_grid="2x2", frame_height=0, frame_width=0),
                dict(slice_grid="2x2", views=[None]), dict(slice_grid="2x2", enhance=True),
                dict(slice_grid="4x4", max_det=300), dict(slice_grid="2x2", batch=1024)):
        with pytest.raises(ValueError):
            ModuleConfig(**{**base, **bad}).validate()
