"""Camera front end on the MI355X: the frame_resize / det_to_source kernels against the CPU
reference (bit-identical resample), the engine resampling native-resolution frames inside its
hipGraph, and the module serving them from the pinned ring through the native loop."""
import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.ops import reference

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes kept 0xCD on either side of the destination


def _frames(n, h, w, seed=0):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed))


CASES = [
    (3, (36, 64), 32, "letterbox"),
    (3, (64, 36), 32, "letterbox"),
    (3, (17, 23), 32, "letterbox"),   # upscale, odd
    (3, (7, 5), 32, "letterbox"),     # clamps
    (3, (1, 1), 32, "letterbox"),
    (3, (32, 32), 32, "letterbox"),   # identity
    (3, (50, 40), 32, "crop"),
    (3, (36, 64), 32, "crop"),
    (1, (1080, 1920), 640, "letterbox"),
    (1, (720, 1280), 224, "crop"),
]


@pytest.mark.parametrize("n,src_hw,dst,form", CASES)
def test_frame_resize_equals_cpu_reference(n, src_hw, dst, form):
    assert ops.load()
    plan = (ops.letterbox_plan if form == "letterbox" else ops.center_crop_plan)(src_hw, dst)
    big = _frames(n + 2, *src_hw, seed=dst + src_hw[0])
    src_cpu = big[1:1 + n]
    want = torch.empty(n, dst, dst, 3, dtype=torch.uint8)
    reference.frame_resize(src_cpu, plan, want)
    # source: a slice of a larger batch (non-zero storage offset, as the stream slices are);
    # destination: carved out of a larger 0xCD-filled allocation
    src = big.cuda()[1:1 + n]
    assert src.storage_offset() > 0 and src.is_contiguous()
    nbytes = n * dst * dst * 3
    buf = torch.full((GUARD + nbytes + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + nbytes].view(n, dst, dst, 3)
    got = ops.frame_resize(src, plan, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), want)
    assert (buf[:GUARD] == 0xCD).all() and (buf[GUARD + nbytes:] == 0xCD).all()
    if form == "letterbox" and src_hw == (32, 32):
        assert torch.equal(out.cpu(), src_cpu)


def test_frame_resize_launcher_rejects_bad_geometry():
    assert ops.load()
    src = _frames(1, 36, 64).cuda()
    k = torch.ops.kvedge.frame_resize
    ok_y, ok_x = [36, 18, 0, 7, 18], [64, 32, 0, 0, 32]
    dst = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device="cuda")
    k(src, dst, ok_y, ok_x, 114)
    for ay, ax in (([36, 18, 0, 20, 18], ok_x),      # content past the destination
                   ([36, 18, 4, 7, 18], ok_x),       # content past the virtual image
                   ([35, 18, 0, 7, 18], ok_x),       # S is not the source extent
                   ([36, 0, 0, 7, 0], ok_x)):        # empty virtual image
        with pytest.raises(RuntimeError):
            k(src, dst, ay, ax, 114)
    with pytest.raises(RuntimeError):                # Wd % 4 != 0
        k(src, torch.zeros(1, 32, 30, 3, dtype=torch.uint8, device="cuda"), ok_y,
          [64, 30, 0, 0, 30], 114)
    with pytest.raises(RuntimeError):                # extent past 8192
        k(torch.zeros(1, 1, 8200, 3, dtype=torch.uint8, device="cuda"), dst, [1, 32, 0, 0, 32],
          [8200, 32, 0, 0, 32], 114)
    with pytest.raises(RuntimeError):
        k(src.cpu(), dst, ok_y, ok_x, 114)
    torch.cuda.synchronize()


def test_det_to_source_equals_reference():
    assert ops.load()
    plan = ops.letterbox_plan((36, 64), 64)  # content rows 14..50 of 64
    g = torch.Generator().manual_seed(11)
    det = torch.rand(3, 8, 6, generator=g) * 64.0
    det[..., :4] -= 4.0  # some boxes reach past the frame: clamped
    count = torch.tensor([0, 3, 8], dtype=torch.int32)
    want = det.clone()
    reference.det_to_source(want, count, plan.box_map(), 36, 64)
    d = det.cuda()
    out = ops.det_to_source(d, count.cuda(), plan)
    torch.cuda.synchronize()
    assert out.data_ptr() == d.data_ptr()
    got = d.cpu()
    diff = (got - want).abs().max()
    print(f"det_to_source max |gpu - reference| = {float(diff):.3e}")
    assert diff <= 1e-3
    assert not torch.equal(got[2, :, :4], det[2, :, :4])
    live = torch.arange(8).view(1, 8) < count.view(3, 1)
    assert torch.equal(got[~live], det[~live])             # rows at or past count: bit-equal
    assert torch.equal(got[..., 4:], det[..., 4:])         # score and class: bit-equal


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def resnet():
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50

    assert ops.load()
    return KvResNet50(init_resnet50(seed=0), "cuda")


@pytest.mark.parametrize("batch,streams", [(2, 1), (4, 2)])
def test_engine_graph_resnet_native_frames(resnet, batch, streams):
    from kvedge_amd.engine import InferenceEngine

    eng = InferenceEngine(resnet, batch, 224, device="cuda", seed=5, streams=streams,
                          frame_hw=(96, 128)).prepare(warmup=1, autotune=False)
    assert eng.graph is not None and eng.source_frames.shape == (batch, 96, 128, 3)
    assert eng.input_frames is eng.source_frames
    for _ in range(2):  # the generator advances inside the graph
        probs, top1 = eng.run()
    torch.cuda.synchronize()
    src = eng.source_frames.clone()
    want = torch.empty(batch, 224, 224, 3, dtype=torch.uint8)
    reference.frame_resize(src.cpu(), eng.frame_plan, want)
    assert torch.equal(eng.frames.cpu(), want)  # every slice resized
    per = batch // streams
    parts = [resnet(ops.frame_resize(src[i * per:(i + 1) * per], eng.frame_plan))
             for i in range(streams)]
    torch.cuda.synchronize()
    assert torch.equal(probs, torch.cat([p[0] for p in parts]))
    assert torch.equal(top1, torch.cat([p[1] for p in parts]))


def test_engine_graph_yolo_boxes_in_frame_pixels():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    y = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001)
    eng = InferenceEngine(y, 2, 640, device="cuda", seed=2, frame_hw=(120, 160)).prepare(
        warmup=1, autotune=False)
    assert eng.graph is not None
    assert eng.frame_plan == ops.letterbox_plan((120, 160), 640)
    det, count = eng.run()
    torch.cuda.synchronize()
    src = eng.source_frames.clone()
    want = torch.empty(2, 640, 640, 3, dtype=torch.uint8)
    reference.frame_resize(src.cpu(), eng.frame_plan, want)
    assert torch.equal(eng.frames.cpu(), want)
    ref_det, ref_count = y(ops.frame_resize(src, eng.frame_plan))  # model coordinates
    model_det = ref_det.clone()
    y.to_source((ref_det, ref_count), eng.frame_plan)
    torch.cuda.synchronize()
    print(f"yolo native-frame counts: {count.tolist()}")
    assert torch.equal(count, ref_count)
    assert torch.equal(det, ref_det)
    n = int(count[0])
    if n:  # kept boxes moved into the 160 x 120 frame
        assert not torch.equal(det[0, :n, :4], model_det[0, :n, :4])
        assert float(det[0, :n, 2].max()) <= 160 and float(det[0, :n, 3].max()) <= 120


# ---------------------------------------------------------------- module
def test_module_native_serving_native_frames():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "resnet50", "batch": 8, "report_interval_s": 0.01,
                        "source": "camera", "steps_per_poll": 4, "frame_height": 120,
                        "frame_width": 160})
    # a failed assertion must still stop the camera thread: context manager
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None
        assert app.engine.source_frames.shape == (8, 120, 160, 3)
        assert app.ring.pinned and app.ring.slot_bytes == 8 * 120 * 160 * 3
        app.run(max_steps=3)
        app.report()
        t = tr.outputs("telemetry")[-1]
        assert t["source"] == "camera" and t["images_per_s"] > 0
        assert app.state["total_images"] == 3 * 4 * 8
        assert app.camera.seq >= 12
        torch.cuda.synchronize()
        # the graph resampled a camera batch that the ring DMA put into source_frames
        src = app.engine.source_frames.cpu()
        assert any(torch.equal(src, f) for f in app.camera.frames)
        want = torch.empty(8, 224, 224, 3, dtype=torch.uint8)
        reference.frame_resize(src, app.engine.frame_plan, want)
        assert torch.equal(app.engine.frames.cpu(), want)
        assert tr.reported["config"]["frame_height"] == 120
