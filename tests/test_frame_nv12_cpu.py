"""NV12 camera frames, CPU tier: the integer BT.601 conversion against the float transform over
every (Y, U, V) triple, the plane layout, the wrappers' composition identity and rejections,
the ``camera-nv12`` twin value, and the engine / module plumbing on the reference path."""
import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference


def all_triples_nv12():
    """One 4096 x 4096 NV12 frame holding every (Y, U, V) triple once: (U, V) pair p = U * 256
    + V owns the 64 chroma cells (2 x 2 pixels each, 256 pixels) at cell row p // 32, cell
    columns (p % 32) * 64 .. + 63, whose pixels carry Y = 0 .. 255."""
    p = torch.arange(65536)
    cell_uv = torch.stack([p // 256, p % 256], dim=-1).to(torch.uint8)       # [65536, 2]
    uv = cell_uv.view(2048, 32, 1, 2).expand(2048, 32, 64, 2).reshape(2048, 4096)
    # the 256 pixels of a pair: cell c = 0 .. 63, then (dy, dx) inside it -> Y = c * 4 + dy * 2 + dx
    c, dy, dx = torch.arange(64).view(1, 64, 1), torch.arange(2).view(2, 1, 1), torch.arange(2)
    yy = (c * 4 + dy * 2 + dx).reshape(2, 128).to(torch.uint8)               # [dy, 128 columns]
    y = yy.view(1, 2, 1, 128).expand(2048, 2, 32, 128).reshape(4096, 4096)
    return torch.cat([y, uv], dim=0).unsqueeze(0).contiguous()               # [1, 6144, 4096]


def float_bt601(nv12):
    """Rounded-and-clamped float BT.601 limited-range transform of an NV12 batch."""
    n, rows, ws = nv12.shape
    hs = rows * 2 // 3
    y = nv12[:, :hs].double() - 16.0
    uv = nv12[:, hs:].reshape(n, hs // 2, ws // 2, 2).double() - 128.0
    uv = uv.repeat_interleave(2, 1).repeat_interleave(2, 2)
    u, v = uv[..., 0], uv[..., 1]
    rgb = torch.stack([1.164383 * y + 1.596027 * v,
                       1.164383 * y - 0.391762 * u - 0.812968 * v,
                       1.164383 * y + 2.017232 * u], dim=-1)
    return rgb.round().clamp(0, 255).to(torch.int16)


def _nv12(n, hs, ws, seed=0):
    return torch.randint(0, 256, (n, hs * 3 // 2, ws), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- colour
def test_all_triples_frame_holds_every_triple_once():
    f = all_triples_nv12()
    y = f[0, :4096].long()
    uv = f[0, 4096:].reshape(2048, 2048, 2).long().repeat_interleave(2, 0).repeat_interleave(2, 1)
    key = (y << 16) | (uv[..., 0] << 8) | uv[..., 1]
    assert torch.equal(key.flatten().sort().values, torch.arange(1 << 24))


def test_nv12_to_rgb_within_one_level_of_float_bt601_on_all_triples():
    f = all_triples_nv12()
    got = reference.nv12_to_rgb(f)
    assert got.shape == (1, 4096, 4096, 3) and got.dtype == torch.uint8
    diff = (got.to(torch.int16) - float_bt601(f)).abs()
    print(f"max |integer - float| over 2^24 triples: {int(diff.max())}; "
          f"R clamps low {float((got[..., 0] == 0).float().mean()):.3f} "
          f"high {float((got[..., 0] == 255).float().mean()):.3f}")
    assert int(diff.max()) <= 1


def test_nv12_layout_pinned_on_a_2x4_frame():
    # Y rows, then one UV row: cells (U, V) = (128, 128) grey and (90, 240) red
    f = torch.tensor([[[16, 235, 81, 81],
                       [126, 126, 81, 82],
                       [128, 128, 90, 240]]], dtype=torch.uint8)
    rgb = reference.nv12_to_rgb(f)
    assert rgb.shape == (1, 2, 4, 3)
    assert rgb[0, 0, 0].tolist() == [0, 0, 0] and rgb[0, 0, 1].tolist() == [255, 255, 255]
    assert rgb[0, 1, 0].tolist() == [128, 128, 128] and rgb[0, 1, 1].tolist() == [128, 128, 128]
    # (81, 90, 240): c = 65, d = -38, e = 112 -> R (19370 + 45808 + 128) >> 8 = 255,
    # G (19370 + 3800 - 23296 + 128) >> 8 = 0, B (19370 - 19608 + 128) >> 8 = -1 -> 0
    assert rgb[0, 0, 2].tolist() == [255, 0, 0]
    assert torch.equal(rgb[0, 0, 3], rgb[0, 0, 2]) and torch.equal(rgb[0, 1, 2], rgb[0, 0, 2])
    # (82, 90, 240): G (19668 + 3800 - 23296 + 128) >> 8 = 1, B (19668 - 19608 + 128) >> 8 = 0
    assert rgb[0, 1, 3].tolist() == [255, 1, 0]
    assert torch.equal(ops.nv12_to_rgb(f), rgb)


# ---------------------------------------------------------------- wrappers
@pytest.mark.parametrize("src_hw,dst,form", [((36, 64), 32, "letterbox"), ((18, 22), 32, "letterbox"),
                                             ((50, 40), 32, "crop"), ((2, 2), 32, "letterbox")])
def test_frame_resize_nv12_cpu_is_the_composition(src_hw, dst, form):
    plan = (ops.letterbox_plan if form == "letterbox" else ops.center_crop_plan)(src_hw, dst)
    f = _nv12(2, *src_hw, seed=dst + src_hw[0])
    want = torch.empty(2, dst, dst, 3, dtype=torch.uint8)
    reference.frame_resize(reference.nv12_to_rgb(f), plan, want)
    assert torch.equal(ops.frame_resize(f, plan, src_format="nv12"), want)
    assert torch.equal(ops.frame_resize_nv12(f, plan), want)
    rgb = ops.nv12_to_rgb(f)
    assert torch.equal(ops.frame_resize(rgb, plan), want)                 # default: RGB
    assert torch.equal(ops.frame_resize(rgb, plan, src_format="rgb"), want)


def test_roi_crop_nv12_cpu_is_the_composition():
    f = _nv12(2, 36, 64, seed=3)
    det = torch.zeros(2, 4, 6)
    det[:, 0, :4] = torch.tensor([11.0, 7.0, 12.0, 8.0])     # 1 x 1 at an odd origin
    det[:, 1, :4] = torch.tensor([11.0, 7.0, 20.0, 16.0])    # odd origin, odd extent
    det[:, 2, :4] = torch.tensor([10.0, 6.0, 13.0, 9.0])     # even origin, odd extent
    det[:, 3, :4] = torch.tensor([0.0, 0.0, 64.0, 36.0])
    count = torch.tensor([4, 2], dtype=torch.int32)
    want = torch.empty(8, 16, 16, 3, dtype=torch.uint8)
    reference.roi_crop(reference.nv12_to_rgb(f), det, count, 4, 16, 9, want)
    assert torch.equal(ops.roi_crop(f, det, count, 4, 16, pad=9, src_format="nv12"), want)
    assert torch.equal(ops.roi_crop_nv12(f, det, count, 4, 16, pad=9), want)
    assert (want[6:] == 9).all() and not (want[:6] == 9).all()
    # the 1 x 1 window is the one converted pixel everywhere
    assert (want[0] == reference.nv12_to_rgb(f)[0, 7, 11]).all()


def test_wrappers_reject_bad_nv12():
    plan = ops.letterbox_plan((36, 64), 32)
    det, count = torch.zeros(1, 2, 6), torch.tensor([1], dtype=torch.int32)
    ok = _nv12(1, 36, 64)
    ops.frame_resize(ok, plan, src_format="nv12")
    ops.roi_crop(ok, det, count, 1, 16, src_format="nv12")
    with pytest.raises(ValueError):                              # unknown format
        ops.frame_resize(ok, plan, src_format="yuyv")
    with pytest.raises(ValueError):
        ops.roi_crop(ok, det, count, 1, 16, src_format="nv21")
    with pytest.raises(ValueError):                              # odd Hs (35 * 3 // 2 = 52 rows)
        ops.frame_resize(torch.zeros(1, 52, 64, dtype=torch.uint8),
                         ops.letterbox_plan((35, 64), 32), src_format="nv12")
    with pytest.raises(ValueError):                              # odd Ws
        ops.frame_resize(torch.zeros(1, 54, 63, dtype=torch.uint8),
                         ops.letterbox_plan((36, 63), 32), src_format="nv12")
    with pytest.raises(ValueError):
        ops.roi_crop(torch.zeros(1, 54, 63, dtype=torch.uint8), det, count, 1, 16,
                     src_format="nv12")
    with pytest.raises(ValueError):                              # plane height != Hs * 3 / 2
        ops.frame_resize(torch.zeros(1, 36, 64, dtype=torch.uint8), plan, src_format="nv12")
    with pytest.raises(ValueError):                              # 52 rows: no even Hs fits
        ops.roi_crop(torch.zeros(1, 52, 64, dtype=torch.uint8), det, count, 1, 16,
                     src_format="nv12")
    with pytest.raises(ValueError):
        ops.nv12_to_rgb(torch.zeros(1, 52, 64, dtype=torch.uint8))
    with pytest.raises(ValueError):
        reference.nv12_to_rgb(torch.zeros(1, 54, 63, dtype=torch.uint8))


# ---------------------------------------------------------------- twin keys
def test_config_camera_nv12():
    d = ModuleConfig().validate()
    assert set(d.to_dict()) == {
        "model", "batch", "dtype", "seed", "report_interval_s", "world_size", "image_size",
        "conf", "iou", "max_det", "fps", "use_graph", "source", "frame_height", "frame_width",
        "crops_per_image", "native_loop", "steps_per_poll", "refine_s", "sync_every",
        "send_interval_s", "max_messages"}
    assert d.source == "synthetic" and d.frame_format() == "rgb" and not d.is_camera()
    cam = d.apply_patch({"source": "camera", "frame_height": 48, "frame_width": 64})
    assert cam.is_camera() and cam.frame_format() == "rgb"
    c = cam.apply_patch({"source": "camera-nv12"})
    assert c.source == "camera-nv12" and c.to_dict()["source"] == "camera-nv12"
    assert c.is_camera() and c.frame_format() == "nv12" and c.frame_hw() == (48, 64)
    assert c.needs_rebuild(cam) and cam.needs_rebuild(c)
    for bad in ({"source": "camera-nv12"},                                   # no frame size
                {"source": "camera-nv12", "frame_height": 47, "frame_width": 64},
                {"source": "camera-yuyv", "frame_height": 48, "frame_width": 64}):
        with pytest.raises(ValueError):
            d.apply_patch(bad)
    assert d.apply_patch({"source": "camera", "frame_height": 47, "frame_width": 64}).is_camera()


def test_module_cli_offers_camera_nv12():
    import inspect

    from kvedge_amd.module import __main__ as cli

    assert '"camera-nv12"' in inspect.getsource(cli.main)


# ---------------------------------------------------------------- engine
def test_engine_cpu_resnet_nv12_frames():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50

    kv = KvResNet50(init_resnet50(seed=0, calibrate=False), "cpu")
    with pytest.raises(ValueError, match="frame_hw"):
        InferenceEngine(kv, 2, 64, device="cpu", frame_format="nv12")
    with pytest.raises(ValueError):
        InferenceEngine(kv, 2, 64, device="cpu", frame_hw=(48, 64), frame_format="yuyv")
    with pytest.raises(ValueError):
        InferenceEngine(kv, 2, 64, device="cpu", frame_hw=(47, 64), frame_format="nv12")
    with pytest.raises(ValueError):  # 1 x 2 x 2 x 3 / 2 = 6 bytes: the generator's % 8 rule
        InferenceEngine(kv, 1, 64, device="cpu", frame_hw=(2, 2), frame_format="nv12")
    eng = InferenceEngine(kv, 2, 64, device="cpu", seed=3, frame_hw=(48, 64),
                          frame_format="nv12").prepare(warmup=1)
    assert eng.source_frames.shape == (2, 72, 64) and eng.frames.shape == (2, 64, 64, 3)
    assert eng.input_frames is eng.source_frames
    probs, top1 = eng.run()
    want = torch.empty_like(eng.frames)
    reference.frame_resize(reference.nv12_to_rgb(eng.source_frames), eng.frame_plan, want)
    assert torch.equal(eng.frames, want)
    ref_p, ref_t = kv(want)
    assert torch.equal(probs, ref_p) and torch.equal(top1, ref_t)
    fr = _nv12(2, 48, 64, seed=9)  # real frames instead of the generator
    probs, _ = eng.set_frames(fr)
    assert torch.equal(eng.source_frames, fr)
    assert torch.equal(probs, kv(ops.frame_resize(fr, eng.frame_plan, src_format="nv12"))[0])


def test_engine_passes_the_format_keyword_only_for_nv12():
    from kvedge_amd.engine import InferenceEngine

    class Old:  # a from_source written before the keyword existed
        def frame_plan(self, src_hw, image_size=0):
            return ops.letterbox_plan(src_hw, image_size)

        def from_source(self, source_frames, frames, plan):
            return frames.float().mean(dim=(1, 2))

    class New(Old):
        def from_source(self, source_frames, frames, plan, src_format="rgb"):
            self.seen = (src_format, tuple(source_frames.shape))
            return frames.float().mean(dim=(1, 2))

    assert InferenceEngine(Old(), 2, 16, device="cpu", frame_hw=(8, 8)).prepare(
        warmup=1).run().shape == (2, 3)
    m = New()
    InferenceEngine(m, 2, 16, device="cpu", frame_hw=(8, 8), frame_format="nv12").prepare(
        warmup=1).run()
    assert m.seen == ("nv12", (2, 12, 8))


# ---------------------------------------------------------------- module
class Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def test_module_cpu_camera_nv12():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    if not ops.load():
        pytest.skip("native runtime not built")
    tr = FakeTransport({"model": "resnet50", "batch": 2, "report_interval_s": 1.0,
                        "image_size": 64, "source": "camera-nv12", "frame_height": 48,
                        "frame_width": 64})
    with ModuleApp(tr, device="cpu", clock=Clock()).start() as app:
        assert app.engine.frame_format == "nv12"
        assert app.engine.source_frames.shape == (2, 72, 64)
        assert app.ring.slot_bytes == 2 * 48 * 64 * 3 // 2
        assert app.camera.frames[0].shape == (2, 72, 64)
        assert tr.reported["config"]["source"] == "camera-nv12"
        app.run(max_steps=3)
        app.report()
        assert tr.outputs("telemetry")[-1]["source"] == "camera-nv12"
        assert app.state["total_images"] == 3 * 2
        src = app.engine.source_frames
        assert any(torch.equal(src, f) for f in app.camera.frames)
        want = torch.empty_like(app.engine.frames)
        reference.frame_resize(reference.nv12_to_rgb(src), app.engine.frame_plan, want)
        assert torch.equal(app.engine.frames, want)
        tr.push_twin_patch({"source": "camera"})  # back to RGB: a rebuild, twice the slot
        app.run(max_steps=2)
        assert app.state["rebuilds"] == 1 and app.engine.frame_format == "rgb"
        assert app.engine.source_frames.shape == (2, 48, 64, 3)
        assert app.ring.slot_bytes == 2 * 48 * 64 * 3
