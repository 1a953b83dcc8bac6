"""Detect-then-classify cascade on the CPU tier: the ROI-crop reference against an independent
anchor (frame_resize), the integer window of hand-written boxes, the twin key, and the engine /
module running the composite model through the reference path."""
import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference

NAN, INF = float("nan"), float("inf")

# boxes (x1, y1, x2, y2) in a 36 x 64 (Hs x Ws) frame -> the window (x0, y0, w, h), worked out
# by hand from: f = min(max(v, 0), S) (NaN -> 0); x0 = min(floor(fx1), Ws - 1);
# xe = min(max(ceil(fx2), x0 + 1), Ws); w = xe - x0
HS, WS = 36, 64
BOX_TABLE = [
    ((10.3, 5.7, 20.2, 15.1), (10, 5, 11, 11)),      # fractional: floor / ceil
    ((12.0, 8.0, 12.0, 8.0), (12, 8, 1, 1)),         # zero area
    ((30.0, 20.0, 10.0, 5.0), (30, 20, 1, 1)),       # inverted
    ((-5.5, -3.0, 7.5, 4.0), (0, 0, 8, 4)),          # negative corner
    ((50.0, 30.0, 100.0, 90.0), (50, 30, 14, 6)),    # reaches beyond the frame
    ((70.0, 40.0, 80.0, 50.0), (63, 35, 1, 1)),      # wholly beyond the frame
    ((NAN, NAN, NAN, NAN), (0, 0, 1, 1)),            # NaN
    ((NAN, 4.0, 20.0, NAN), (0, 4, 20, 1)),          # NaN in two corners
    ((-INF, -INF, INF, INF), (0, 0, 64, 36)),        # -inf / +inf: the whole frame
    ((INF, INF, -INF, -INF), (63, 35, 1, 1)),        # +inf / -inf
    ((60.0, 32.0, 64.0, 36.0), (60, 32, 4, 4)),      # touches the right and bottom edge
    ((0.0, 0.0, 64.0, 36.0), (0, 0, 64, 36)),        # the full frame
]


def _frames(n, h, w, seed=0):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed))


def _det(boxes):
    """[N, max_det, 6] from a nested list of (x1, y1, x2, y2)."""
    b = torch.tensor(boxes, dtype=torch.float32)
    return torch.cat([b, torch.zeros(*b.shape[:2], 2)], dim=2)


def _stretch_plan(h, w, d, pad):
    return ops.ResizePlan((h, d, 0, 0, d), (w, d, 0, 0, d), pad, (h, w), (d, d))


# ---------------------------------------------------------------- reference vs anchor
@pytest.mark.parametrize("src_hw,d", [((36, 64), 32), ((17, 23), 32), ((7, 5), 32),
                                      ((50, 40), 16)])
def test_full_frame_box_equals_frame_resize(src_hw, d):
    hs, ws = src_hw
    src = _frames(2, hs, ws, seed=hs)
    det = _det([[(0.0, 0.0, ws, hs)] * 3] * 2)
    count = torch.tensor([3, 1], dtype=torch.int32)
    out = ops.roi_crop(src, det, count, 2, d, pad=7)
    assert out.shape == (4, d, d, 3) and out.dtype == torch.uint8
    want = ops.frame_resize(src, _stretch_plan(hs, ws, d, 7))
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[0])
    assert torch.equal(out[2], want[1])
    assert (out[3] == 7).all()  # slot 1 of image 1: at count


def test_identity_and_slots_past_count_are_pad():
    d = 32
    src = _frames(3, d, d, seed=1)
    det = _det([[(0.0, 0.0, d, d)] * 4] * 3)
    count = torch.tensor([0, 2, 9], dtype=torch.int32)  # 9 > max_det: clamped
    out = torch.full((3 * 4, d, d, 3), 0xCD, dtype=torch.uint8)
    got = ops.roi_crop(src, det, count, 4, d, pad=114, out=out)
    assert got is out
    out = out.view(3, 4, d, d, 3)
    assert (out[0] == 114).all() and (out[1, 2:] == 114).all()
    for n, k in ((1, 0), (1, 1), (2, 0), (2, 3)):
        assert torch.equal(out[n, k], src[n])
    # a negative count keeps nothing
    out = ops.roi_crop(src, det, torch.tensor([-1, -5, 1], dtype=torch.int32), 1, d, pad=9)
    assert (out[:2] == 9).all() and torch.equal(out[2], src[2])


def test_crop_is_the_resized_window():
    src = _frames(1, HS, WS, seed=2)
    det = _det([[(10.3, 5.7, 20.2, 15.1), (50.0, 30.0, 100.0, 90.0)]])
    out = ops.roi_crop(src, det, torch.tensor([2], dtype=torch.int32), 2, 16)
    assert torch.equal(out[0:1], ops.frame_resize(src[:, 5:16, 10:21].contiguous(),
                                                  _stretch_plan(11, 11, 16, 0)))
    assert torch.equal(out[1:2], ops.frame_resize(src[:, 30:36, 50:64].contiguous(),
                                                  _stretch_plan(6, 14, 16, 0)))


def test_roi_crop_rejects_bad_arguments():
    src = _frames(1, HS, WS)
    det = _det([[(0.0, 0.0, 8.0, 8.0)] * 3])
    count = torch.tensor([1], dtype=torch.int32)
    for k, size, pad in ((1, 30, 0), (0, 32, 0), (4, 32, 0), (1, 32, 256), (1, 32, -1)):
        with pytest.raises(ValueError):
            ops.roi_crop(src, det, count, k, size, pad=pad)
    with pytest.raises(ValueError):
        ops.roi_crop(src, det[:, :, :5], count, 1, 32)


# ---------------------------------------------------------------- geometry
def test_window_table():
    boxes = torch.tensor([b for b, _ in BOX_TABLE], dtype=torch.float32)
    want = torch.tensor([w for _, w in BOX_TABLE])
    got = reference.roi_windows(boxes, HS, WS)
    assert got.tolist() == want.tolist()
    # whatever the box: at least 1 x 1 and inside the frame
    g = torch.Generator().manual_seed(3)
    rnd = (torch.rand(4096, 4, generator=g) - 0.25) * 160.0
    x0, y0, w, h = reference.roi_windows(rnd, HS, WS).unbind(-1)
    assert (w >= 1).all() and (h >= 1).all() and (x0 >= 0).all() and (y0 >= 0).all()
    assert (x0 + w <= WS).all() and (y0 + h <= HS).all()


def test_table_boxes_crop_without_leaving_the_frame():
    src = _frames(1, HS, WS, seed=4)
    det = _det([[b for b, _ in BOX_TABLE]])
    k = len(BOX_TABLE)
    out = ops.roi_crop(src, det, torch.tensor([k], dtype=torch.int32), k, 8, pad=3)
    for i, (_, (x0, y0, w, h)) in enumerate(BOX_TABLE):
        want = ops.frame_resize(src[:, y0:y0 + h, x0:x0 + w].contiguous(),
                                _stretch_plan(h, w, 8, 3))
        assert torch.equal(out[i:i + 1], want), BOX_TABLE[i]


# ---------------------------------------------------------------- twin key
def test_config_detect_classify():
    d = ModuleConfig().validate()
    assert d.crops_per_image == 4 and "detect-classify" != d.model
    c = d.apply_patch({"model": "detect-classify", "crops_per_image": 2})
    assert c.model == "detect-classify" and c.crops_per_image == 2
    assert c.resolved_image_size() == 640 and c.to_dict()["crops_per_image"] == 2
    assert c.needs_rebuild(c.apply_patch({"crops_per_image": 3}))
    assert not c.needs_rebuild(c.apply_patch({"report_interval_s": 3.0}))
    for bad in ({"crops_per_image": 0}, {"crops_per_image": 17}, {"crops_per_image": -1},
                {"max_det": 1}, {"crops_per_image": 16, "max_det": 15},
                {"batch": 2049}, {"batch": 1024, "crops_per_image": 5}):
        with pytest.raises(ValueError):
            c.apply_patch(bad)
    assert c.apply_patch({"batch": 2048}).batch == 2048  # 2048 * 2 = 4096: the limit itself
    assert c.apply_patch({"crops_per_image": 16, "max_det": 16}).crops_per_image == 16


def test_config_defaults_of_other_keys_unchanged():
    d = ModuleConfig().to_dict()
    d.pop("crops_per_image")
    assert d == {"model": "resnet50", "batch": 64, "dtype": "bf16", "seed": 0,
                 "report_interval_s": 10.0, "world_size": 1, "image_size": 0, "conf": 0.25,
                 "iou": 0.7, "max_det": 300, "fps": 0.0, "use_graph": True,
                 "source": "synthetic", "frame_height": 0, "frame_width": 0,
                 "native_loop": True, "steps_per_poll": 1, "refine_s": 0.0, "sync_every": 0,
                 "send_interval_s": 5.0, "max_messages": 500}
    # the cross-key limits bind the cascade only: these configs validated before
    assert ModuleConfig(model="resnet50", batch=4096).validate().batch == 4096
    assert ModuleConfig(model="yolov8n", max_det=2).validate().max_det == 2
    assert ModuleConfig(model="yolov8n").resolved_image_size() == 640
    assert ModuleConfig(model="resnet50").resolved_image_size() == 224


def test_module_cli_has_crops_flag():
    import inspect

    from kvedge_amd.module import __main__ as cli

    assert '"--crops-per-image"' in inspect.getsource(cli.main)


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def cascade():
    from kvedge_amd.models.cascade import KvDetectClassify
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    det = KvYoloV8n(init_yolov8n(seed=0, calibrate=False), "cpu", conf=0.0, max_det=8)
    clf = KvResNet50(init_resnet50(seed=0, calibrate=False), "cpu")
    return KvDetectClassify(det, clf, 2, crop_size=64)


def _hand_composed(m, crop_src, frames, plan=None):
    """The cascade spelled out with the reference functions."""
    det, count = m.detector(frames)
    if plan is not None:
        reference.det_to_source(det, count, plan.box_map(), *plan.src_hw)
    n, k, d = frames.shape[0], m.k, m.crop_size
    crops = torch.empty(n * k, d, d, 3, dtype=torch.uint8)
    reference.roi_crop(crop_src, det, count, k, d, 0, crops)
    probs, top1 = m.classifier(crops)
    top1, prob = top1.view(n, k), probs.max(dim=1).values.view(n, k)
    valid = torch.arange(k).view(1, k) < count.view(n, 1)
    return (det, count, torch.where(valid, top1, torch.full_like(top1, -1)),
            torch.where(valid, prob, torch.zeros_like(prob)))


@pytest.mark.parametrize("frame_hw", [None, (48, 64)])
def test_engine_cpu_cascade(cascade, frame_hw):
    from kvedge_amd.engine import InferenceEngine

    m = cascade
    assert m.image_size == 640 and len(m.convs()) == len(m.detector.convs()) + len(
        m.classifier.convs())
    assert m.flops_per_image(64) == (m.detector.flops_per_image(64) +
                                     2 * m.classifier.flops_per_image(64))
    eng = InferenceEngine(m, 2, 64, device="cpu", seed=3, frame_hw=frame_hw).prepare(warmup=1)
    det, count, crop_cls, crop_prob = eng.run()
    assert det.shape == (2, 8, 6) and count.dtype == torch.int32
    assert crop_cls.shape == (2, 2) and crop_cls.dtype == torch.int64
    assert crop_prob.shape == (2, 2) and crop_prob.dtype == torch.float32
    if frame_hw is None:
        assert eng.frame_plan is None
        want = _hand_composed(m, eng.frames, eng.frames)
    else:
        assert eng.frame_plan == ops.letterbox_plan(frame_hw, 64)
        frames = ops.frame_resize(eng.source_frames, eng.frame_plan)
        assert torch.equal(eng.frames, frames)
        want = _hand_composed(m, eng.source_frames, frames, eng.frame_plan)
        n = int(count[0])
        assert det[0, :n, 2].max() <= 64 and det[0, :n, 3].max() <= 48  # frame pixels
    for got, ref in zip((det, count, crop_cls, crop_prob), want):
        assert torch.equal(got, ref)
    invalid = torch.arange(2).view(1, 2) >= count.view(2, 1)
    assert torch.equal(crop_cls == -1, invalid)
    assert int(count.min()) >= 1 and (crop_prob[~invalid] > 0).all()


def test_cascade_masks_slots_past_count(cascade):
    src = _frames(2, 64, 64, seed=8)
    det = _det([[(4.0, 4.0, 40.0, 40.0)] * 8] * 2)
    count = torch.tensor([1, 0], dtype=torch.int32)
    crop_cls, crop_prob = cascade.classify(src, det, count)
    assert crop_cls[0, 0] >= 0 and crop_prob[0, 0] > 0
    assert crop_cls.flatten()[1:].tolist() == [-1, -1, -1]
    assert crop_prob.flatten()[1:].tolist() == [0.0, 0.0, 0.0]


def test_cascade_rejects_bad_crops_per_image(cascade):
    from kvedge_amd.models.cascade import KvDetectClassify

    for k in (0, 9):  # the detector keeps max_det = 8 rows
        with pytest.raises(ValueError):
            KvDetectClassify(cascade.detector, cascade.classifier, k)
    with pytest.raises(ValueError):
        KvDetectClassify(cascade.detector, cascade.classifier, 2, crop_size=30)


# ---------------------------------------------------------------- module
class Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def test_module_cpu_detect_classify():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "detect-classify", "batch": 2, "report_interval_s": 1.0,
                        "image_size": 64, "conf": 0.0, "max_det": 8, "crops_per_image": 2})
    with ModuleApp(tr, device="cpu", clock=Clock()).start() as app:
        assert tr.reported["config"]["crops_per_image"] == 2
        assert app.model.k == 2 and app.model.crop_size == 224
        app.run(max_steps=2)
        app.report()  # summarises the outputs of the last step
        t = tr.outputs("telemetry")[-1]
        assert t["model"] == "detect-classify"
        count, crop_cls = app.engine.outputs[1], app.engine.outputs[2]
        assert t["detections"] == {"total": int(count.sum()), "max_per_image": int(count.max())}
        assert t["crops"] == int((crop_cls >= 0).sum()) and t["crops"] > 0
        assert sum(t["crop_top1"].values()) == t["crops"] and len(t["crop_top1"]) <= 5
        first = app.engine
        tr.push_twin_patch({"crops_per_image": 3})
        app.run(max_steps=2)
        assert app.state["rebuilds"] == 1 and app.engine is not first
        assert app.model.k == 3 and app.engine.outputs[2].shape == (2, 3)
        assert tr.reported["config"]["crops_per_image"] == 3
        tr.push_twin_patch({"crops_per_image": 9})  # > max_det: rejected, nothing rebuilt
        app.run(max_steps=1)
        assert app.state["rejected_patches"] == 1 and app.model.k == 3
