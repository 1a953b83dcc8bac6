"""Sliced detection on the MI355X: the det_merge kernel against ops.reference.det_merge, bit
for bit, at the chunk edges, the empty and the full list, every mode, and hostile input; then
KvSliced end to end (RGB and NV12, eager and one hipGraph replay; the engine's step with one and
two stream slices) against the same step recomposed from the GPU's per-group detections with
the CPU reference ops."""
import pytest
import torch

from kvedge_amd import ops

pytestmark = pytest.mark.gpu

N = 3
NAN, INF = float("nan"), float("inf")


def _clustered(groups, R, totals, seed, clusters=12):
    """det [groups * N, R, 6] / count: boxes jittered around a few centres per camera (so a good
    share overlap), three classes, scores in 1/64 (so many tie), every row filled; camera n has
    totals[n] candidates, the groups filled in order."""
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand(N, clusters, 2, generator=g) * 1500.0
    pick = torch.randint(0, clusters, (groups, N, R), generator=g)
    c = centre[torch.arange(N).view(1, N, 1), pick]
    xy = c + torch.randn(groups, N, R, 2, generator=g) * 9.0
    wh = 40.0 + torch.rand(groups, N, R, 2, generator=g) * 60.0
    score = torch.randint(0, 65, (groups, N, R, 1), generator=g) / 64.0
    cls = (pick % 3).float().unsqueeze(-1)
    det = torch.cat([xy, xy + wh, score, cls], -1).view(groups * N, R, 6).contiguous()
    count = torch.tensor([min(max(totals[n] - k * R, 0), R) for k in range(groups)
                          for n in range(N)], dtype=torch.int32)
    return det, count


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _check(det, count, groups, **kw):
    assert ops.load()
    want, want_n = ops.det_merge(det, count, groups, **kw)
    got, got_n = ops.det_merge(det.cuda(), count.cuda(), groups, **kw)
    assert torch.equal(got_n.cpu(), want_n)
    assert torch.equal(_bits(got), _bits(want))
    return want, want_n


@pytest.mark.parametrize("class_aware", [True, False])
@pytest.mark.parametrize("metric", ops.MERGE_METRICS)
@pytest.mark.parametrize("mode", ops.MERGE_MODES)
def test_modes_equal_reference(mode, metric, class_aware):
    totals = (700, 450, 129)
    det, count = _clustered(5, 300, totals, seed=1)
    want, want_n = _check(det, count, 5, mode=mode, metric=metric, class_aware=class_aware)
    assert 0 < int(want_n.sum()) < sum(totals)  # some absorbed
    if mode == "nmm":  # and some hull larger than its kept box: the cases are not vacuous
        own, _ = ops.det_merge(det, count, 5, mode="nms", metric=metric, class_aware=class_aware)
        assert (want[..., :4] != ops.reference.track_quantize(own[..., :4]) / 4.0).any()


@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 129])
def test_chunk_edges_equal_reference(total):
    det, count = _clustered(5, 300, (total, (total * 2) // 3, total + 2), seed=total + 2,
                            clusters=40)
    _check(det, count, 5)


@pytest.mark.parametrize("groups,R", [(1, 300), (5, 300), (13, 300), (17, 240), (16, 256)])
def test_full_lists_equal_reference(groups, R):
    full = groups * R  # (16, 256): the 4096 candidates one workgroup holds
    det, count = _clustered(groups, R, (full, full // 3, 65), seed=groups)
    _, want_n = _check(det, count, groups)
    assert int(want_n[0]) < full


@pytest.mark.parametrize("max_det,clusters", [(7, 12), (15, 12), (90, 200)])
def test_stop_inside_a_chunk(max_det, clusters):
    det, count = _clustered(5, 300, (700, 450, 129), seed=3, clusters=clusters)
    _, full_n = ops.det_merge(det, count, 5)
    assert int(full_n.min()) > max_det  # the kept set is larger: the sweep stops early
    _, want_n = _check(det, count, 5, max_det=max_det)
    assert want_n.tolist() == [max_det] * N


@pytest.mark.parametrize("mode", ops.MERGE_MODES)
def test_hostile_input_equals_reference(mode):
    det, _ = _clustered(4, 40, (160, 160, 160), seed=4)
    odd = torch.tensor([(NAN, NAN, NAN, NAN, NAN, NAN), (NAN, 4.0, 20.0, NAN, 0.5, 1.0),
                        (-INF, -INF, INF, INF, INF, 0.0), (INF, INF, -INF, -INF, 0.9, INF),
                        (300.0, 200.0, 100.0, 50.0, 0.7, -3.0), (12.0, 8.0, 12.0, 8.0, 0.6, 0.0),
                        (5000.0, 5000.0, 6000.0, 6000.0, -0.5, 70000.0),
                        (10.0, 10.0, 90.0, 90.0, -0.0, 1.0), (10.0, 10.0, 90.0, 90.0, -INF, 1.0)])
    det[:, 3:3 + len(odd)] = odd
    count = torch.tensor([-1, 47, 40, 12, 0, 40, 40, 40, -7, 40, 33, 1 << 30], dtype=torch.int32)
    _check(det, count, 4, mode=mode, thr=0.3)


HW = (352, 640)


@pytest.fixture(scope="module")
def sliced():
    from kvedge_amd.models.slicing import KvSliced
    from kvedge_amd.models.yolov8 import KvYoloV8n

    assert ops.load()
    inner = KvYoloV8n.build(seed=0, device="cuda")
    inner.conf, inner.max_det = 0.0, 16  # random weights: keep boxes, a short list
    return KvSliced(inner, 4, grid=(2, 2), overlap=0.2)


def _recomposed(model, src, frames, plan, **kw):
    """The step from the GPU's own per-group detections (the model on the same tile batch),
    mapped to the frame and merged by the CPU reference ops."""
    n = int(frames.shape[0])
    gdet, gcount = (t.cpu() for t in model.inner(model.tile_frames(src, frames, plan, **kw)))
    views = ops.slice_views(n, HW, (640, 640), (2, 2), 0.2)
    for k in range(4):
        ops.view_to_source(gdet[k * n:(k + 1) * n], gcount[k * n:(k + 1) * n], views, slot0=k * n)
    ops.det_to_source(gdet[4 * n:], gcount[4 * n:], plan)
    want, want_n = ops.det_merge(gdet, gcount, 5, max_det=16)
    assert 0 < int(want_n.sum()) < int(gcount.sum())
    return want, want_n


@pytest.mark.parametrize("fmt", ops.SRC_FORMATS)
def test_sliced_yolo_end_to_end(sliced, fmt):
    n = 2
    g = torch.Generator().manual_seed(5)
    shape = (n, HW[0] * 3 // 2, HW[1]) if fmt == "nv12" else (n, *HW, 3)
    src = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).cuda()
    kw = {"src_format": fmt} if fmt == "nv12" else {}
    plan = sliced.frame_plan(HW)
    frames = ops.frame_resize(src, plan, **kw)
    det, count = sliced.from_source(src, frames, plan, **kw)
    want, want_n = _recomposed(sliced, src, frames, plan, **kw)
    assert torch.equal(count.cpu(), want_n) and torch.equal(_bits(det), _bits(want))

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gd, gc = sliced.from_source(src, frames, plan, **kw)
    gd.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gc.cpu(), want_n) and torch.equal(_bits(gd), _bits(want))


@pytest.mark.parametrize("streams", [1, 2])
def test_sliced_engine_stream_slices(sliced, streams):
    """The engine's captured step, one slice or two side by side on their own HIP streams:
    every slice against its own recomposition (slices share no buffer)."""
    from kvedge_amd.engine import InferenceEngine

    eng = InferenceEngine(sliced, 4, 640, device="cuda", seed=3, streams=streams, frame_hw=HW,
                          frame_format="nv12").prepare(warmup=1, autotune=False)
    for _ in range(2):
        det, count = eng.run()
    torch.cuda.synchronize()
    per = 4 // streams
    for lo in range(0, 4, per):
        want, want_n = _recomposed(sliced, eng.source_frames[lo:lo + per], eng.frames[lo:lo + per],
                                   eng.frame_plan, src_format="nv12")
        assert torch.equal(count[lo:lo + per].cpu(), want_n)
        assert torch.equal(_bits(det[lo:lo + per]), _bits(want))
