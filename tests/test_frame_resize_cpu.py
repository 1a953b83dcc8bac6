"""Camera front end on the CPU tier: resize plans, the fixed-point reference resample against
torch's float bilinear, boxes back to the frame, the twin keys, and the engine / module
serving native-resolution frames through the reference path."""
import pytest
import torch
import torch.nn.functional as F

from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference


def _frames(n, h, w, seed=0):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- plans
def test_letterbox_plan_pinned_numbers():
    p = ops.letterbox_plan((1080, 1920), 640)
    assert p.axis_y == (1080, 360, 0, 140, 360) and p.axis_x == (1920, 640, 0, 0, 640)
    assert p.pad == 114 and p.src_hw == (1080, 1920) and p.dst_hw == (640, 640)
    p = ops.letterbox_plan((480, 640), 640)
    assert p.axis_y == (480, 480, 0, 80, 480) and p.axis_x == (640, 640, 0, 0, 640)
    # upscaling is allowed
    p = ops.letterbox_plan((17, 23), 32)
    assert p.axis_x == (23, 32, 0, 0, 32) and p.axis_y[1] == 24 and p.axis_y[3] == 4


def test_center_crop_plan_pinned_numbers():
    p = ops.center_crop_plan((1080, 1920), 224)
    assert p.axis_y == (1080, 256, 16, 0, 224) and p.axis_x == (1920, 455, 116, 0, 224)
    assert p.dst_hw == (224, 224)
    p = ops.center_crop_plan((64, 36), 32)  # portrait: the width is the shorter side
    assert p.axis_x[1] == 36 and p.axis_y[1] == 64


def test_plans_are_frozen_and_checked():
    p = ops.letterbox_plan((36, 64), 32)
    with pytest.raises(Exception):
        p.pad = 0
    for bad in ((0, 64), (64, 8193)):
        with pytest.raises(ValueError):
            ops.letterbox_plan(bad, 32)
        with pytest.raises(ValueError):
            ops.center_crop_plan(bad, 32)


# ---------------------------------------------------------------- reference vs torch
def _float_bilinear(src, out_hw):
    x = src.permute(0, 3, 1, 2).double()
    y = F.interpolate(x, size=out_hw, mode="bilinear", align_corners=False, antialias=False)
    return y.permute(0, 2, 3, 1)


def _expected_content(src, plan):
    """round(float64 bilinear) of the content rectangle of ``plan``."""
    (_, ry, oy, _, ny), (_, rx, ox, _, nx) = plan.axis_y, plan.axis_x
    y = _float_bilinear(src, (ry, rx))[:, oy:oy + ny, ox:ox + nx]
    return torch.floor(y + 0.5).long()


LETTERBOX = [((36, 64), 32), ((64, 36), 32), ((17, 23), 32), ((7, 5), 32),
             ((1080, 1920), 640), ((720, 1280), 224)]
CROP = [((36, 64), 32), ((64, 36), 32), ((17, 23), 32), ((7, 5), 32), ((50, 40), 32),
        ((720, 1280), 224)]


@pytest.mark.parametrize("src_hw,dst", LETTERBOX)
def test_reference_letterbox_matches_float_bilinear(src_hw, dst):
    src = _frames(1, *src_hw, seed=src_hw[0])
    plan = ops.letterbox_plan(src_hw, dst)
    out = ops.frame_resize(src, plan)
    assert out.shape == (1, dst, dst, 3) and out.dtype == torch.uint8
    (_, _, _, top, nh), (_, _, _, left, nw) = plan.axis_y, plan.axis_x
    content = out[:, top:top + nh, left:left + nw].long()
    diff = (content - _expected_content(src, plan)).abs().max()
    print(f"letterbox {src_hw} -> {dst}: max |reference - round(float)| = {int(diff)}")
    assert diff <= 1
    mask = torch.ones(dst, dst, dtype=torch.bool)
    mask[top:top + nh, left:left + nw] = False
    assert (out[0][mask] == 114).all()


@pytest.mark.parametrize("src_hw,dst", CROP)
def test_reference_center_crop_matches_float_bilinear(src_hw, dst):
    src = _frames(1, *src_hw, seed=src_hw[1])
    plan = ops.center_crop_plan(src_hw, dst)
    out = ops.frame_resize(src, plan)
    assert out.shape == (1, dst, dst, 3)
    diff = (out.long() - _expected_content(src, plan)).abs().max()
    print(f"crop {src_hw} -> {dst}: max |reference - round(float)| = {int(diff)}")
    assert diff <= 1


def test_reference_identity_is_exact_and_3to1_hits_pixel_centres():
    src = _frames(2, 32, 32, seed=5)
    assert torch.equal(ops.frame_resize(src, ops.letterbox_plan((32, 32), 32)), src)
    # 1080x1920 -> 360x640 is an exact 3:1 ratio: every sample is a source pixel centre
    src = _frames(1, 1080, 1920, seed=6)
    out = ops.frame_resize(src, ops.letterbox_plan((1080, 1920), 640))
    assert torch.equal(out[:, 140:500], src[:, 1::3, 1::3])


@pytest.mark.parametrize("plan_fn", [ops.letterbox_plan, ops.center_crop_plan])
@pytest.mark.parametrize("src_hw", [(36, 64), (17, 23), (7, 5), (1, 1)])
def test_reference_constant_source_stays_constant(plan_fn, src_hw):
    src = torch.empty(1, *src_hw, 3, dtype=torch.uint8)
    src[..., 0], src[..., 1], src[..., 2] = 10, 130, 255
    plan = plan_fn(src_hw, 32)
    out = ops.frame_resize(src, plan)
    (_, _, _, c0y, ny), (_, _, _, c0x, nx) = plan.axis_y, plan.axis_x
    content = out[0, c0y:c0y + ny, c0x:c0x + nx].reshape(-1, 3)
    assert (content == torch.tensor([10, 130, 255], dtype=torch.uint8)).all()


def test_frame_resize_rejects_bad_shapes():
    plan = ops.letterbox_plan((36, 64), 32)
    with pytest.raises(AssertionError):
        ops.frame_resize(_frames(1, 64, 36), plan)
    with pytest.raises(ValueError):
        ops.frame_resize(_frames(1, 36, 64), ops.letterbox_plan((36, 64), 30))


# ---------------------------------------------------------------- boxes back to the frame
@pytest.mark.parametrize("src_hw,dst", [((1080, 1920), 640), ((480, 640), 640), ((17, 23), 32),
                                        ((64, 36), 32)])
def test_det_to_source_round_trip(src_hw, dst):
    hs, ws = src_hw
    plan = ops.letterbox_plan(src_hw, dst)
    (_, _, _, top, nh), (_, _, _, left, nw) = plan.axis_y, plan.axis_x
    det = torch.zeros(2, 4, 6)
    # row 0: the content rectangle; row 1: the whole model image (reaches into the padding)
    det[:, 0] = torch.tensor([left, top, left + nw, top + nh, 0.9, 3.0])
    det[:, 1] = torch.tensor([-5.0, -5.0, dst + 5.0, dst + 5.0, 0.8, 1.0])
    det[:, 2] = torch.tensor([1.0, 2.0, 3.0, 4.0, 0.7, 2.0])
    det[:, 3] = torch.tensor([5.0, 6.0, 7.0, 8.0, 0.6, 5.0])
    before = det.clone()
    count = torch.tensor([2, 0], dtype=torch.int32)
    out = ops.det_to_source(det, count, plan)
    assert out is det
    want = torch.tensor([0.0, 0.0, ws, hs])
    assert (det[0, 0, :4] - want).abs().max() <= 1e-3
    assert torch.equal(det[0, 1, :4], want)              # clamped to the frame
    assert torch.equal(det[0, 2:], before[0, 2:])        # rows at or past count
    assert torch.equal(det[1], before[1])                # count 0: nothing moves
    assert torch.equal(det[..., 4:], before[..., 4:])    # score and class


def test_det_to_source_crop_offset():
    plan = ops.center_crop_plan((1080, 1920), 224)
    cy, sy, cx, sx = plan.box_map()
    assert (cy, cx) == (-16.0, -116.0) and sy == 1080 / 256 and sx == 1920 / 455
    det = torch.tensor([[[0.0, 0.0, 224.0, 224.0, 0.5, 0.0]]])
    ops.det_to_source(det, torch.tensor([1], dtype=torch.int32), plan)
    want = torch.tensor([116 * 1920 / 455, 16 * 1080 / 256, 340 * 1920 / 455, 240 * 1080 / 256])
    assert (det[0, 0, :4] - want).abs().max() <= 1e-3


# ---------------------------------------------------------------- twin keys
def test_config_frame_keys():
    c = ModuleConfig().validate()
    assert (c.frame_height, c.frame_width) == (0, 0) and c.frame_hw() is None
    c2 = c.apply_patch({"frame_height": 1080, "frame_width": 1920})
    assert c2.frame_hw() == (1080, 1920) and c2.to_dict()["frame_width"] == 1920
    assert c2.needs_rebuild(c)
    assert c.apply_patch({"frame_height": 1080, "frame_width": 1920}).needs_rebuild(
        c.apply_patch({"frame_height": 720, "frame_width": 1920}))
    assert c2.needs_rebuild(c2.apply_patch({"frame_width": 1280}))
    for bad in ({"frame_height": 1080}, {"frame_width": 1920},
                {"frame_height": 8, "frame_width": 64}, {"frame_height": 64, "frame_width": 8},
                {"frame_height": 4104, "frame_width": 64}, {"frame_height": 64, "frame_width": 4104},
                {"frame_height": 1080, "frame_width": 1924},
                {"frame_height": -16, "frame_width": -16}):
        with pytest.raises(ValueError):
            c.apply_patch(bad)


def test_module_cli_has_frame_flags():
    import inspect

    from kvedge_amd.module import __main__ as cli

    src = inspect.getsource(cli.main)
    assert '"--frame-height"' in src and '"--frame-width"' in src


# ---------------------------------------------------------------- engine
def test_engine_cpu_resnet_native_frames():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50

    kv = KvResNet50(init_resnet50(seed=0, calibrate=False), "cpu")
    assert not hasattr(kv, "to_source")
    eng = InferenceEngine(kv, 2, 64, device="cpu", seed=3, frame_hw=(48, 64)).prepare(warmup=1)
    assert eng.source_frames.shape == (2, 48, 64, 3) and eng.frames.shape == (2, 64, 64, 3)
    assert eng.input_frames is eng.source_frames
    assert eng.frame_plan == ops.center_crop_plan((48, 64), 64)
    probs, top1 = eng.run()
    want = torch.empty_like(eng.frames)
    reference.frame_resize(eng.source_frames, eng.frame_plan, want)
    assert torch.equal(eng.frames, want)
    ref_p, ref_t = kv(want)
    assert torch.equal(probs, ref_p) and torch.equal(top1, ref_t)
    # real frames instead of the generator
    fr = _frames(2, 48, 64, seed=9)
    probs, _ = eng.set_frames(fr)
    assert torch.equal(eng.source_frames, fr)
    assert torch.equal(probs, kv(ops.frame_resize(fr, eng.frame_plan))[0])


def test_engine_without_frame_size_is_unchanged():
    from kvedge_amd.engine import InferenceEngine

    class Tiny:
        def __call__(self, frames):
            return frames.float().mean(dim=(1, 2))

    eng = InferenceEngine(Tiny(), 2, 16, device="cpu", seed=1).prepare(warmup=1)
    assert eng.source_frames is None and eng.frame_plan is None
    assert eng.input_frames is eng.frames
    assert eng.run().shape == (2, 3)


def test_engine_synthetic_byte_count_is_checked():
    from kvedge_amd.engine import InferenceEngine

    class Tiny:
        def frame_plan(self, src_hw, image_size=0):
            return ops.letterbox_plan(src_hw, image_size)

        def __call__(self, frames):
            return frames.float().mean(dim=(1, 2))

    with pytest.raises(ValueError):
        InferenceEngine(Tiny(), 1, 16, device="cpu", frame_hw=(7, 5))
    # fed frames (no generator) of any size are fine
    eng = InferenceEngine(Tiny(), 1, 16, device="cpu", synthetic=False, frame_hw=(7, 5))
    out = eng.set_frames(_frames(1, 7, 5))
    assert out.shape == (1, 3)


def test_engine_cpu_yolo_boxes_in_frame_pixels():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    kv = KvYoloV8n(init_yolov8n(seed=0, calibrate=False), "cpu", conf=0.0, max_det=20)
    eng = InferenceEngine(kv, 1, 64, device="cpu", seed=4, frame_hw=(48, 64)).prepare(warmup=1)
    plan = eng.frame_plan
    assert plan == ops.letterbox_plan((48, 64), 64) and plan.axis_y[3] == 8
    det, count = eng.run()
    assert int(count[0]) > 0
    ref_det, ref_count = kv(ops.frame_resize(eng.source_frames, plan))
    assert torch.equal(count, ref_count)
    model_boxes = ref_det.clone()
    reference.det_to_source(ref_det, ref_count, plan.box_map(), 48, 64)
    assert torch.equal(det, ref_det)
    n = int(count[0])
    assert not torch.equal(det[0, :n, :4], model_boxes[0, :n, :4])
    assert det[0, :n, 0].min() >= 0 and det[0, :n, 2].max() <= 64
    assert det[0, :n, 1].min() >= 0 and det[0, :n, 3].max() <= 48


# ---------------------------------------------------------------- module
class Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def test_module_cpu_camera_native_frames():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    if not ops.load():
        pytest.skip("native runtime not built")
    tr = FakeTransport({"model": "resnet50", "batch": 2, "report_interval_s": 1.0,
                        "image_size": 64, "source": "camera", "frame_height": 48,
                        "frame_width": 64})
    with ModuleApp(tr, device="cpu", clock=Clock()).start() as app:
        assert app.engine.source_frames.shape == (2, 48, 64, 3)
        assert app.ring.slot_bytes == 2 * 48 * 64 * 3
        assert app.camera.frames[0].shape == (2, 48, 64, 3)
        assert tr.reported["config"]["frame_height"] == 48
        app.run(max_steps=3)
        assert app.state["total_images"] == 3 * 2
        # the engine saw a camera batch, resampled
        src = app.engine.source_frames
        assert any(torch.equal(src, f) for f in app.camera.frames)
        assert torch.equal(app.engine.frames, ops.frame_resize(src, app.engine.frame_plan))
        tr.push_twin_patch({"frame_height": 0, "frame_width": 0})
        app.run(max_steps=2)
        assert app.state["rebuilds"] == 1 and app.engine.source_frames is None
        assert app.engine.input_frames.shape == (2, 64, 64, 3)
        assert app.ring.slot_bytes == 2 * 64 * 64 * 3
        assert app.state["total_images"] == 5 * 2


def test_module_cpu_synthetic_native_frames():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "resnet50", "batch": 1, "report_interval_s": 1.0,
                        "image_size": 64, "frame_height": 48, "frame_width": 64})
    with ModuleApp(tr, device="cpu", clock=Clock()).start() as app:
        assert app.engine.synthetic and app.engine.source_frames.shape == (1, 48, 64, 3)
        app.run(max_steps=2)
        assert app.state["total_images"] == 2
        tr.push_twin_patch({"frame_height": 48})  # a partial patch merges: the width stays 64
        app.run(max_steps=1)
        assert app.state["rejected_patches"] == 0
        tr.push_twin_patch({"frame_width": 0})    # leaves height without width: rejected
        app.run(max_steps=1)
        assert app.state["rejected_patches"] == 1 and app.cfg.frame_hw() == (48, 64)
