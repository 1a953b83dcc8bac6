"""Motion regions on the GPU (csrc/kernels/motion_blobs.hip) against the flood-fill reference,
bitwise: det, count and labels, pre-filled with poison so that "every element written" is part
of the comparison."""
import pytest
import torch

import blob_cases as bc
import watch_script as ws
from kvedge_amd import ops

pytestmark = pytest.mark.gpu

POISON_F, POISON_I = 12345.5, ws.CD
BIG = [(128, 256), (181, 181)]  # the LDS limit; an odd pitch just under it


def poisoned(n, grid, r):
    return (torch.full((n, r, 6), POISON_F, device="cuda"),
            torch.full((n,), POISON_I, dtype=torch.int32, device="cuda"),
            torch.full((n, *grid), POISON_I, dtype=torch.int32, device="cuda"))


def check(mask, reg, **kw):
    """Run ``mask`` on the GPU into poisoned outputs and compare with the reference, which is
    returned."""
    assert ops.load()
    out = poisoned(mask.shape[0], reg.grid, kw.get("max_blobs", 16))
    got = ops.motion_blobs(mask.cuda(), reg, out_det=out[0], out_count=out[1], out_labels=out[2],
                           **kw)
    want = bc.reference(mask, reg, **kw)
    for g, w, name in zip(got, want, ("det", "count", "labels")):
        assert torch.equal(g.cpu(), w), (name, kw)
    return want


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("grid", [(3, 4), (3, 66), (68, 120)])
def test_small_grids(grid, connectivity):
    for name in ("rand50", "checker", "serpentine"):
        m = torch.stack([bc.PATTERNS[name](*grid), bc.PATTERNS["rand10"](*grid)])
        check(m, bc.regions_for(grid, 2, "cuda"), connectivity=connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("pattern", list(bc.PATTERNS))
@pytest.mark.parametrize("grid", BIG)
def test_large_grids(grid, pattern, connectivity):
    _, cnt, _ = check(bc.PATTERNS[pattern](*grid)[None], bc.regions_for(grid, 1, "cuda"),
                      connectivity=connectivity)
    if pattern in ("serpentine", "comb", "one", "checker"):  # one blob, or singletons
        assert int(cnt) == (16 if (pattern, connectivity) == ("checker", 4) else 1)


def test_truncation_and_ties():
    grid = (68, 120)
    reg = bc.regions_for(grid, 1, "cuda").set_min_cells(3)
    m = bc.random(0.25, seed=3)(*grid)[None]
    det, cnt, _ = check(m, reg, max_blobs=4, connectivity=4)
    full, kept, _ = bc.reference(m, reg, max_blobs=64, connectivity=4)
    n = full[0, :int(kept), 4].tolist()
    assert int(cnt) == 4 < int(kept) and len(set(n)) < len(n)  # truncated, and two share n


def test_three_cameras_at_slot0_2_of_six_streams():
    grid = (68, 120)
    reg = bc.regions_for(grid, 6, "cuda")
    for cam, (mc, cls) in enumerate([(1, 80), (9, 3), (2, 81), (5, 82), (1, 83), (7, 4)]):
        reg.set_min_cells(mc, cam).set_class(cls, cam)
        reg.set_ignore(cam, bc.random(0.05 * cam, seed=cam)(*grid).bool())
    before = (reg.params.clone(), reg.ignore.clone())
    m = torch.stack([bc.PATTERNS[p](*grid) for p in ("rand50", "comb", "rand10")])
    det, cnt, _ = check(m, reg, slot0=2, max_blobs=8)
    assert det[:, 0, 5].tolist() == [81.0, 82.0, 83.0] and int(cnt.min()) > 0
    assert torch.equal(reg.params, before[0]) and torch.equal(reg.ignore, before[1])


@pytest.mark.parametrize("min_cells,cls", [(-5, -1), (1 << 30, 1 << 20)])
def test_hostile_parameter_row_is_clamped(min_cells, cls):
    grid = (3, 66)
    reg = bc.regions_for(grid, 1, "cuda")
    reg.params[0] = torch.tensor([min_cells, cls, -1, 1 << 31 - 1], dtype=torch.int32)
    det, cnt, _ = check(bc.PATTERNS["one"](*grid)[None], reg)
    assert int(cnt) == 1 and det[0, 0, 4:].tolist() == [198.0, 0.0 if cls < 0 else 65535.0]


def test_launcher_rejections_leave_the_outputs_untouched():
    assert ops.load()
    k = torch.ops.kvedge.motion_blobs
    grid = (3, 4)
    reg = bc.regions_for(grid, 2, "cuda")
    m = torch.ones(2, *grid, dtype=torch.uint8, device="cuda")
    det, cnt, lab = poisoned(2, grid, 4)
    big = torch.ones(1, 129, 256, dtype=torch.uint8, device="cuda")  # 33024 cells
    big_lab = torch.full((1, 129, 256), POISON_I, dtype=torch.int32, device="cuda")
    calls = [
        lambda: k(big, reg.params, big, det[:1], cnt[:1], big_lab, 0, 16, 129 * 16, 4096, 8),
        lambda: k(m.int(), reg.params, reg.ignore, det, cnt, lab, 0, 16, 45, 59, 8),
        lambda: k(m, reg.params.float(), reg.ignore, det, cnt, lab, 0, 16, 45, 59, 8),
        lambda: k(m, reg.params, reg.ignore, det, cnt, lab.float(), 0, 16, 45, 59, 8),
        lambda: k(m, reg.params, reg.ignore, det, cnt, lab, 1, 16, 45, 59, 8),
        lambda: k(m, reg.params, reg.ignore, det, cnt, lab, 0, 16, 45, 59, 6),
        lambda: k(m, reg.params, reg.ignore, det, cnt, lab, 0, 12, 45, 59, 8),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="kvedge: motion_blobs"):
            call()
    with pytest.raises(ValueError):
        ops.motion_blobs(m, reg, slot0=1, out_det=det, out_count=cnt, out_labels=lab)
    torch.cuda.synchronize()
    assert (det == POISON_F).all() and (cnt == POISON_I).all() and (lab == POISON_I).all()
    assert (big_lab == POISON_I).all()


def test_captured_step_replayed_three_times():
    assert ops.load()
    grid = (68, 120)
    reg = bc.regions_for(grid, 2, "cuda")
    masks = [torch.stack([bc.random(d, seed=s)(*grid), bc.comb(*grid)])
             for d, s in ((0.3, 1), (0.5, 2), (0.4, 3))]
    m = masks[0].cuda()
    out = poisoned(2, grid, 16)
    kw = dict(out_det=out[0], out_count=out[1], out_labels=out[2])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.motion_blobs(m, reg, **kw)  # warm
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.motion_blobs(m, reg, **kw)
    torch.cuda.synchronize()
    for step, mask in enumerate(masks):
        if step == 1:  # both tables change without recapturing
            reg.set_min_cells(4)
        if step == 2:
            reg.set_ignore(1, bc.checkerboard(*grid).bool())
        m.copy_(mask)
        for o, p in zip(out, (POISON_F, POISON_I, POISON_I)):
            o.fill_(p)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, bc.reference(mask, reg)):
            assert torch.equal(got.cpu(), want), step


def test_engine_watched_with_regions():
    # the blob outputs equal the CPU's, everything else equals a run without regions
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.watching import KvWatched
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    yolo = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.0, max_det=16)
    batch, hw = 4, (120, 160)
    reg = ops.MotionRegions(batch, hw, 8, device="cuda").set_min_cells(2)
    kw = dict(device="cuda", seed=5, frame_hw=hw, frame_format="nv12", synthetic=False)
    m = KvWatched(yolo, batch, frame_hw=hw, cell=8, regions=reg, max_blobs=6)
    plain = KvWatched(yolo, batch, frame_hw=hw, cell=8)
    eng = InferenceEngine(m, batch, 640, **kw).prepare(warmup=1, autotune=False)
    ref_eng = InferenceEngine(plain, batch, 640, **kw).prepare(warmup=1, autotune=False)
    assert eng.graph is not None
    graph_out = eng.outputs
    for f in ws.script("nv12", batch, *hw, seed=11):
        out, base = eng.set_frames(f.cuda()), ref_eng.set_frames(f.cuda())
        torch.cuda.synchronize()
        assert m.blob_index == len(base) - 2 and len(out) == len(base) + 2
        for a, b in zip(out[:m.blob_index] + out[-2:], base):
            assert torch.equal(a, b)
        det, cnt, _ = bc.reference(out[-1], reg, max_blobs=6)
        assert torch.equal(out[m.blob_index].cpu(), det)
        assert torch.equal(out[m.blob_index + 1].cpu(), cnt)
    eng.input_frames.copy_(ws.script("nv12", batch, *hw, seed=11)[2].cuda())
    eng.graph.replay()  # the captured step: the block moves in against the constant frame
    torch.cuda.synchronize()
    det, cnt, _ = bc.reference(graph_out[-1], reg, max_blobs=6)
    assert torch.equal(graph_out[m.blob_index].cpu(), det) and int(cnt.max()) > 0
    assert torch.equal(graph_out[m.blob_index + 1].cpu(), cnt)


def test_module_native_serving_with_regions():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "yolov8n", "batch": 2, "watch": True, "watch_regions": True,
                        "watch_motion_level": 1, "watch_region_max": 12, "source": "camera-nv12",
                        "frame_height": 120, "frame_width": 160, "report_interval_s": 0.01,
                        "steps_per_poll": 2, "conf": 0.0, "max_det": 8})
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None and app.model.blob_index == 2
        app.run(max_steps=2)
        app.report()
        t = tr.outputs("telemetry")[-1]
        torch.cuda.synchronize()
        out = app.engine.outputs
        det, cnt, _ = bc.reference(out[-1], app.model.regions, max_blobs=12)
        assert torch.equal(out[2].cpu(), det) and torch.equal(out[3].cpu(), cnt)
        assert [r["regions_total"] for r in t["regions"]] == [n for n in cnt.tolist() if n]
        for r in t["regions"]:
            want = det[r["camera"], :min(r["regions_total"], 8), :5].int().tolist()
            assert r["regions"] == want
        assert app.on_method("regions", {})[0] == 200
