"""Detect-then-classify cascade on the MI355X: the roi_crop kernel against the CPU reference
(bit-identical), its launcher's rejections, the cascade captured into the engine's hipGraph,
and the module serving it through the native loop."""
import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.ops import reference

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes kept 0xCD on either side of the destination
NAN, INF = float("nan"), float("inf")
# hand-written boxes (x1, y1, x2, y2), written for a 36 x 64 frame (tests/test_roi_crop_cpu.py
# pins their windows there); in the other frames they clamp differently, which is the point
TABLE = [
    (10.3, 5.7, 20.2, 15.1),      # fractional
    (12.0, 8.0, 12.0, 8.0),       # zero area
    (30.0, 20.0, 10.0, 5.0),      # inverted
    (-5.5, -3.0, 7.5, 4.0),       # negative corner
    (50.0, 30.0, 100.0, 90.0),    # reaches beyond the frame
    (70.0, 40.0, 80.0, 50.0),     # wholly beyond the frame
    (NAN, NAN, NAN, NAN),
    (NAN, 4.0, 20.0, NAN),
    (-INF, -INF, INF, INF),
    (INF, INF, -INF, -INF),
    (60.0, 32.0, 64.0, 36.0),     # touches the right and bottom edge of 36 x 64
]


def _frames(n, h, w, seed=0):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed))


def _boxes(n, max_det, hs, ws, seed, shift):
    """det [n, max_det, 6]: the table, then seeded random boxes (some reaching past the frame,
    a few touching its right / bottom edge), rotated by ``shift`` rows so that every table row
    lands in a kept slot in one of the runs."""
    g = torch.Generator().manual_seed(seed)
    rows = n * max_det
    lo = torch.rand(rows, 2, generator=g) * torch.tensor([ws, hs]) * 1.1 - 0.05 * ws
    ext = torch.rand(rows, 2, generator=g) * torch.tensor([ws, hs]) * 0.8
    rnd = torch.cat([lo, lo + ext], dim=1)
    rnd[::5, 2], rnd[::5, 3] = float(ws), float(hs)
    tab = torch.tensor(TABLE, dtype=torch.float32)
    box = torch.cat([tab, rnd])[:max(rows, len(TABLE))].roll(shift, 0)[:rows]
    det = torch.cat([box, torch.rand(rows, 2, generator=g)], dim=1)
    return det.view(n, max_det, 6).contiguous()


def _run_guarded(src, det, count, k, d, pad, band=0):
    nbytes = src.shape[0] * k * d * d * 3
    buf = torch.full((GUARD + nbytes + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + nbytes].view(src.shape[0] * k, d, d, 3)
    got = ops.roi_crop(src, det, count, k, d, pad=pad, out=out, band=band)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert (buf[:GUARD] == 0xCD).all() and (buf[GUARD + nbytes:] == 0xCD).all()
    return out.cpu()


CASES = [
    # kept slots are rows 8, 9 and 16..19 of the 24: these four rotations put every table
    # row into one of them
    (3, (36, 64), 32, [0, 2, 8], (8, 13, 6, 9)),
    (3, (17, 23), 32, [0, 2, 8], (8, 13, 6, 9)),
    (3, (7, 5), 32, [0, 2, 8], (8, 13, 6, 9)),   # upscaling, clamps
    (1, (1080, 1920), 224, [3], (0,)),
]


@pytest.mark.parametrize("n,src_hw,d,counts,shifts", CASES)
def test_roi_crop_equals_cpu_reference(n, src_hw, d, counts, shifts):
    assert ops.load()
    k, max_det, pad = 4, 8, 114
    hs, ws = src_hw
    big = _frames(n + 2, hs, ws, seed=d + hs)
    src_cpu = big[1:1 + n]
    # source: a slice of a larger batch (non-zero storage offset, as the stream slices are)
    src = big.cuda()[1:1 + n]
    assert src.storage_offset() > 0 and src.is_contiguous()
    count = torch.tensor(counts, dtype=torch.int32)
    for shift in shifts:
        det = _boxes(n, max_det, hs, ws, seed=hs + shift, shift=shift)
        if hs == 1080:  # two windows of several hundred pixels in the kept slots
            det[0, 1, :4] = torch.tensor([200.5, 100.25, 1500.0, 1079.5])
            det[0, 2, :4] = torch.tensor([0.0, 0.0, 1920.0, 1080.0])
        want = torch.empty(n * k, d, d, 3, dtype=torch.uint8)
        reference.roi_crop(src_cpu, det, count, k, d, pad, want)
        got = _run_guarded(src, det.cuda(), count.cuda(), k, d, pad)
        assert torch.equal(got, want), (src_hw, shift)
        # slots at or past count: all pad, no 0xCD left anywhere
        got = got.view(n, k, d, d, 3)
        for i, c in enumerate(counts):
            assert (got[i, min(c, k):] == pad).all()
    # every instantiated band height computes the same crops
    for band in (4, 16, 32):
        assert torch.equal(_run_guarded(src, det.cuda(), count.cuda(), k, d, pad, band=band),
                           want), band


def test_roi_crop_full_frame_box_equals_frame_resize():
    assert ops.load()
    hs, ws, d = 36, 64, 32
    src = _frames(2, hs, ws, seed=7).cuda()
    det = torch.zeros(2, 3, 6)
    det[..., 2], det[..., 3] = ws, hs
    count = torch.tensor([3, 1], dtype=torch.int32)
    out = ops.roi_crop(src, det.cuda(), count.cuda(), 2, d, pad=9)
    plan = ops.ResizePlan((hs, d, 0, 0, d), (ws, d, 0, 0, d), 9, (hs, ws), (d, d))
    want = ops.frame_resize(src, plan)
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[0])
    assert torch.equal(out[2], want[1]) and (out[3] == 9).all()
    # a D x D source with the full-frame box: the identity
    sq = _frames(1, d, d, seed=8).cuda()
    det = torch.tensor([[[0.0, 0.0, d, d, 0.5, 0.0]]]).cuda()
    one = ops.roi_crop(sq, det, torch.tensor([1], dtype=torch.int32).cuda(), 1, d)
    assert torch.equal(one, sq)


def test_roi_crop_launcher_rejections_leave_dst_untouched():
    assert ops.load()
    k = torch.ops.kvedge.roi_crop
    src = _frames(2, 36, 64).cuda()
    det = _boxes(2, 8, 36, 64, seed=1, shift=0).cuda()
    count = torch.tensor([8, 8], dtype=torch.int32).cuda()

    def dst(n, d):
        return torch.full((n, d, d, 3), 0xCD, dtype=torch.uint8, device="cuda")

    ok = dst(8, 32)
    k(src, det, count, ok, 0)
    torch.cuda.synchronize()
    assert not (ok == 0xCD).all()
    odd = torch.full((8 * 32 * 32 * 3 + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    wide = torch.cat([det, det], dim=2)[:, :, :6]  # [2, 8, 6] view of [2, 8, 12]: strided
    assert not wide.is_contiguous()
    bad = [
        (src, det, count, dst(8, 30), 0),                                    # D % 4 != 0
        (src, det, count, odd[1:1 + 8 * 32 * 32 * 3].view(8, 32, 32, 3), 0),  # misaligned dst
        (src, det, count, dst(2 * 9, 32), 0),                                # K = 9 > max_det
        (src, det.double(), count, dst(8, 32), 0),                           # wrong dtypes
        (src, det, count.long(), dst(8, 32), 0),
        (src.float(), det, count, dst(8, 32), 0),
        (src, wide, count, dst(8, 32), 0),                                   # strided det
        (src, det, count, dst(8, 32), 256),                                  # pad out of range
        (src, det, count, dst(7, 32), 0),                                    # not N * K crops
        (src, det[:1], count, dst(8, 32), 0),                                # det of another N
        (src, det.cpu(), count, dst(8, 32), 0),
    ]
    for i, args in enumerate(bad):
        with pytest.raises(RuntimeError):
            k(*args)
        torch.cuda.synchronize()
        assert (args[3] == 0xCD).all(), i
    assert (odd == 0xCD).all()
    with pytest.raises(RuntimeError):  # a band height that is not instantiated
        torch.ops.kvedge.roi_crop_band(src, det, count, ok, 0, 5)
    # N == 0 is a no-op
    k(src[:0], det[:0], count[:0], dst(8, 32)[:0], 0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def cascade():
    from kvedge_amd.models.cascade import KvDetectClassify
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    det = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.0, max_det=8)
    clf = KvResNet50(init_resnet50(seed=0), "cuda")
    return KvDetectClassify(det, clf, 2)


@pytest.mark.parametrize("batch,streams", [(2, 1), (4, 2)])
def test_engine_graph_cascade(cascade, batch, streams):
    from kvedge_amd.engine import InferenceEngine

    m, K = cascade, 2
    eng = InferenceEngine(m, batch, 640, device="cuda", seed=5, streams=streams,
                          frame_hw=(120, 160)).prepare(warmup=1, autotune=False)
    assert eng.graph is not None and eng.frame_plan == ops.letterbox_plan((120, 160), 640)
    for _ in range(2):  # the generator advances inside the graph
        det, count, crop_cls, crop_prob = eng.run()
    torch.cuda.synchronize()
    print(f"cascade counts b{batch} x{streams}: {count.tolist()}")
    assert det.shape == (batch, 8, 6) and crop_cls.shape == (batch, K)
    assert crop_cls.dtype == torch.int64 and crop_prob.dtype == torch.float32
    assert int(count.min()) >= K  # every slot holds a real detection: nothing vacuous below
    # eager recomposition from the frames the graph saw, slice by slice
    src = eng.source_frames.clone()
    per = batch // streams
    parts = []
    for i in range(streams):
        s = src[i * per:(i + 1) * per]
        d, c = m.detector.to_source(m.detector(ops.frame_resize(s, eng.frame_plan)),
                                    eng.frame_plan)
        crops = ops.roi_crop(s, d, c, K, 224)
        probs, top1 = m.classifier(crops)
        parts.append((d, c, top1.view(per, K),
                      probs.gather(1, top1.view(-1, 1)).view(per, K)))
    torch.cuda.synchronize()
    want = [torch.cat(x) for x in zip(*parts)]
    assert torch.equal(count, want[1])
    assert torch.equal(det, want[0])
    assert torch.equal(crop_cls, want[2]) and (crop_cls >= 0).all()
    assert torch.equal(crop_prob, want[3]) and (crop_prob > 0).all()
    # the crops are cut from the native frames: the kernel against the CPU reference
    crops_ref = torch.empty(batch * K, 224, 224, 3, dtype=torch.uint8)
    reference.roi_crop(src.cpu(), det.cpu(), count.cpu(), K, 224, 0, crops_ref)
    assert torch.equal(ops.roi_crop(src, det, count, K, 224).cpu(), crops_ref)


# ---------------------------------------------------------------- module
def test_module_native_serving_detect_classify():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "detect-classify", "batch": 2, "crops_per_image": 2,
                        "report_interval_s": 0.01, "source": "camera", "steps_per_poll": 2,
                        "conf": 0.0, "max_det": 8})
    # a failed assertion must still stop the camera thread: context manager
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None and app.model.k == 2
        assert tr.reported["config"]["crops_per_image"] == 2
        assert tr.reported["config"]["model"] == "detect-classify"
        app.run(max_steps=2)
        app.report()
        t = tr.outputs("telemetry")[-1]
        assert t["source"] == "camera" and t["images_per_s"] > 0
        assert app.state["total_images"] == 2 * 2 * 2
        torch.cuda.synchronize()
        count, crop_cls = app.engine.outputs[1].cpu(), app.engine.outputs[2].cpu()
        assert t["detections"]["total"] == int(count.sum())
        assert "crop_top1" in t and t["crops"] == int((crop_cls >= 0).sum())
        assert sum(t["crop_top1"].values()) == t["crops"]
        invalid = torch.arange(2).view(1, 2) >= count.view(2, 1)
        assert torch.equal(crop_cls == -1, invalid)
