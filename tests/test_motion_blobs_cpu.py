"""Motion regions on the CPU: the flood-fill reference (ops.reference.motion_blobs) against
results written out by hand on grids of at most 6 x 6, the wrapper's checks, and the wiring up to
KvWatched, the module config and the telemetry."""
import pytest
import torch

import watch_script as ws
from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig

X = -1


def run(rows, hw=None, ignore=None, min_cells=1, **kw):
    m = torch.tensor(rows, dtype=torch.uint8)[None]
    hw = hw or (m.shape[1] * 16, m.shape[2] * 16)
    reg = ops.MotionRegions(1, hw, 16).set_min_cells(min_cells)
    if ignore is not None:
        reg.set_ignore(0, torch.tensor(ignore, dtype=torch.bool))
    det, cnt, lab = ops.motion_blobs(m, reg, **kw)
    return det[0].tolist(), int(cnt[0]), lab[0].tolist()


def row(x1, y1, x2, y2, n, cls=80):
    return [float(v) for v in (x1, y1, x2, y2, n, cls)]


ZERO = [0.0] * 6

CASES = {
    "diagonal_4": ([[1, 0], [0, 1]], dict(connectivity=4, max_blobs=3),
                   [row(0, 0, 16, 16, 1), row(16, 16, 32, 32, 1), ZERO], 2, [[0, X], [X, 1]]),
    "diagonal_8": ([[1, 0], [0, 1]], dict(connectivity=8, max_blobs=2),
                   [row(0, 0, 32, 32, 2), ZERO], 1, [[0, X], [X, 0]]),
    # the arms only meet in the last row
    "u_shape": ([[1, 0, 1], [1, 0, 1], [1, 1, 1]], dict(connectivity=4, max_blobs=2),
                [row(0, 0, 48, 48, 7), ZERO], 1, [[0, X, 0], [0, X, 0], [0, 0, 0]]),
    # equal n: the lower first cell wins; the larger blob comes before both
    "ties_by_first": ([[0, 1, 0, 1, 1], [0, 1, 0, 0, 0], [0, 0, 0, 1, 1], [1, 1, 1, 0, 0]],
                      dict(connectivity=4, max_blobs=4),
                      [row(0, 48, 48, 64, 3), row(16, 0, 32, 32, 2), row(48, 0, 80, 16, 2),
                       row(48, 32, 80, 48, 2)], 4,
                      [[X, 1, X, 2, 2], [X, 1, X, X, X], [X, X, X, 3, 3], [0, 0, 0, X, X]]),
    "min_cells": ([[1, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 0]],
                  dict(connectivity=4, max_blobs=3, min_cells=2),
                  [row(0, 32, 48, 48, 3), row(32, 0, 64, 16, 2), ZERO], 2,
                  [[X, X, 1, 1], [X, X, X, X], [0, 0, 0, X]]),
    # the cells of the blobs past max_blobs are -1
    "truncated": ([[1, 0, 1, 1], [0, 0, 0, 0], [1, 1, 1, 0]], dict(connectivity=4, max_blobs=2),
                  [row(0, 32, 48, 48, 3), row(32, 0, 64, 16, 2)], 2,
                  [[X, X, 1, 1], [X, X, X, X], [0, 0, 0, X]]),
    "ignore_splits": ([[1, 1, 1, 1, 1]],
                      dict(connectivity=8, max_blobs=2, ignore=[[0, 0, 1, 0, 0]]),
                      [row(0, 0, 32, 16, 2), row(48, 0, 80, 16, 2)], 2, [[0, 0, X, 1, 1]]),
    # frame 40 x 56 at cell 16: the last row and column of cells are partial
    "clamped_box": ([[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]],
                    dict(connectivity=8, max_blobs=1, hw=(40, 56)),
                    [row(32, 16, 56, 40, 4)], 1, [[X, X, X, X], [X, X, 0, 0], [X, X, 0, 0]]),
    # bit 0 of the mask byte is what counts
    "bit0_only": ([[2, 3], [254, 0]], dict(connectivity=4, max_blobs=1),
                  [row(16, 0, 32, 16, 1)], 1, [[X, 0], [X, X]]),
}


@pytest.mark.parametrize("name", CASES)
def test_reference_against_results_written_out(name):
    rows, kw, det, count, labels = CASES[name]
    assert run(rows, **kw) == (det, count, labels)


def test_ignore_polygons_rasterise_cell_centres():
    reg = ops.MotionRegions(2, (64, 96), 16)
    # centres lie at 8, 24, 40, 56, ...: the triangle x < 60, y > 17, y < x + 1 holds six
    reg.set_ignore_polygons(1, [[(16, 17), (60, 17), (60, 61)]])
    want = torch.zeros(4, 6, dtype=torch.uint8)
    want[1, 1:4] = want[2, 2:4] = want[3, 3] = 1
    assert torch.equal(reg.ignore[1], want) and not reg.ignore[0].any()
    reg.set_ignore_polygons(0, [[(0, 0), (17, 0), (17, 17), (0, 17)],
                                [(80, 48), (100, 48), (80, 68)]])
    assert reg.ignore[0].nonzero().tolist() == [[0, 0], [3, 5]]
    assert not reg.clear_ignore(0).ignore[0].any() and reg.ignore[1].sum() == 6


def test_wrapper_rejections():
    reg = ops.MotionRegions(2, (48, 64), 16)
    m = torch.zeros(2, 3, 4, dtype=torch.uint8)
    ops.motion_blobs(m, reg)
    with pytest.raises(TypeError):
        ops.motion_blobs(m, reg.params)
    for bad in (dict(mask=m.int()), dict(mask=m[:, :2]), dict(mask=m.transpose(1, 2)),
                dict(mask=torch.zeros(2, 4, 3, dtype=torch.uint8).transpose(1, 2)),
                dict(slot0=1), dict(slot0=-1), dict(max_blobs=0), dict(max_blobs=65),
                dict(connectivity=6), dict(out_det=torch.zeros(2, 16, 6, dtype=torch.float64)),
                dict(out_count=torch.zeros(3, dtype=torch.int32)),
                dict(out_labels=torch.zeros(2, 3, 4, dtype=torch.int64))):
        with pytest.raises(ValueError):
            ops.motion_blobs(**dict(dict(mask=m, regions=reg), **bad))
    with pytest.raises(ValueError, match="32768"):  # 1080p at cell 8 fits, 4K at cell 8 not
        ops.MotionRegions(1, (2160, 3840), 8)
    assert ops.MotionRegions(1, (1080, 1920), 8).grid == (135, 240)
    for bad in (lambda: reg.set_min_cells(0), lambda: reg.set_min_cells(13),
                lambda: reg.set_class(65536), lambda: reg.set_class(1, camera=2),
                lambda: reg.set_ignore(0, torch.zeros(3, 4)),
                lambda: reg.set_ignore_polygons(0, [[(0, 0), (1, 1)]])):
        with pytest.raises(ValueError):
            bad()


def test_kvwatched_regions_output_order_and_blob_index():
    from test_frame_watch_cpu import _StubDetector

    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.watching import KvWatched

    stub, hw = _StubDetector(), (24, 40)
    reg = ops.MotionRegions(2, hw, 8).set_min_cells(2)
    m = KvWatched(stub, 2, frame_hw=hw, cell=8, regions=reg, max_blobs=3, connectivity=4)
    plain = KvWatched(stub, 2, frame_hw=hw, cell=8)
    assert m.blob_index is None and plain.regions is None
    engs = [InferenceEngine(k, 2, 32, device="cpu", seed=3, frame_hw=hw,
                            synthetic=False).prepare(warmup=1) for k in (m, plain)]
    for f in ws.script("rgb", 2, 24, 40, seed=8)[:3]:
        out, base = engs[0].set_frames(f), engs[1].set_frames(f)
        assert len(out) == len(base) + 2 == 6 and m.blob_index == 2 and plain.blob_index is None
        for a, b in zip(out[:2] + out[-2:], base):
            assert torch.equal(a, b)
        det, cnt, _ = ops.motion_blobs(out[-1], reg, max_blobs=3, connectivity=4)
        assert torch.equal(out[2], det) and torch.equal(out[3], cnt)
    assert int(out[3].sum()) > 0  # the block that moved in
    with pytest.raises(ValueError):  # another grid
        KvWatched(stub, 2, frame_hw=hw, cell=8, regions=ops.MotionRegions(2, hw))


def test_config_region_keys():
    base = dict(model="yolov8n", watch=True, watch_regions=True)
    cfg = ModuleConfig(**base, watch_region_max=4, watch_region_min_cells=3, watch_ignore=[
        {"name": "tree", "polygon": [[0, 0], [9, 0], [9, 9]], "cameras": [0]}]).validate()
    assert cfg.to_dict()["watch_ignore"][0]["polygon"][1] == [9.0, 0.0]
    assert not set(ModuleConfig.REGION_KEYS) & set(ModuleConfig(model="yolov8n").to_dict())
    live = cfg.apply_patch({"watch_region_min_cells": 5, "watch_ignore": "[]"})
    assert not live.needs_rebuild(cfg) and live.watch_ignore == ()
    for patch in ({"watch_region_max": 8}, {"watch_region_connectivity": 4},
                  {"watch_regions": False, "watch_region_max": 16, "watch_region_min_cells": 1,
                   "watch_ignore": []}):
        assert cfg.apply_patch(patch).needs_rebuild(cfg)
    for bad in (dict(watch=False), dict(watch_region_max=0), dict(watch_region_max=65),
                dict(watch_region_connectivity=6), dict(watch_region_min_cells=0),
                dict(watch_ignore=[{"name": "a", "polygon": [[0, 0], [1, 1]]}]),
                dict(watch_ignore=[{"name": "a", "polygon": [[0, 0], [1, 1], [2, 0]],
                                    "cameras": [99]}]),
                dict(frame_height=2160, frame_width=3840, watch_cell=8),
                dict(watch_regions=False, watch_region_min_cells=2)):
        with pytest.raises(ValueError):
            ModuleConfig(**dict(base, **bad)).validate()
    ModuleConfig(**dict(base, frame_height=1080, frame_width=1920, watch_cell=8)).validate()


def test_module_cpu_telemetry_carries_regions():
    from test_frame_watch_cpu import _module

    extra = {"watch": True, "watch_cell": 8, "watch_motion_level": 1}
    off = _module(extra)
    on, out, model, cfg, (status, body), app = _module(dict(
        extra, watch_regions=True, watch_region_max=12, watch_ignore=[
            {"name": "left", "polygon": [[0, 0], [32, 0], [32, 64], [0, 64]], "cameras": [1]}]))
    assert set(on) == set(off[0]) | {"regions"} and len(out) == len(off[1]) + 2
    assert cfg["watch_regions"] is True and model.blob_index == len(out) - 4
    assert model.regions.ignore[1, :, :4].all() and not model.regions.ignore[0].any()
    det, cnt, _ = ops.motion_blobs(out[-1], model.regions, max_blobs=12)
    assert torch.equal(out[-4], det) and torch.equal(out[-3], cnt) and int(cnt.min()) > 0
    assert [r["camera"] for r in on["regions"]] == [0, 1]
    for r, d, n in zip(on["regions"], det.tolist(), cnt.tolist()):
        assert r["regions_total"] == n and len(r["regions"]) == min(n, 8)
        assert r["regions"] == [[int(v) for v in b[:5]] for b in d[:min(n, 8)]]
    assert all(b[0] >= 32 for b in on["regions"][1]["regions"])  # nothing under the polygon
    assert status == 200 and body["cameras"][0]["regions"] == on["regions"][0]["regions"]
    status, full = app.on_method("regions", {})
    assert status == 200 and [len(c) for c in full["cameras"]] == cnt.tolist()
    assert off[5].on_method("regions", {})[0] == 400
    # min_cells is live: written into the device table, no rebuild
    rebuilds = app.state["rebuilds"]
    assert app._apply_patch({"watch_region_min_cells": 64})[0] == 200
    assert app.state["rebuilds"] == rebuilds and model.regions.params[:, 0].tolist() == [64, 64]
