"""Camera snapshots through the module on the CPU path, over FakeTransport: nothing changes
with the key off; with it on the `snapshot` method returns a file Pillow opens, a camera going
dark sends exactly one `alarm:dark` picture in the step its counter rises, the quality patches
without a rebuild, an oversize picture is counted and not sent; and the KvSnapshots wrapper on
a CPU engine, RGB and NV12, native and model-size frames."""
import base64
import io

import pytest
import torch

pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

import jpeg_cases as jc  # noqa: E402
import watch_script as ws  # noqa: E402
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.module.config import ModuleConfig  # noqa: E402
from kvedge_amd.ops import reference as ref  # noqa: E402

BASE = {"model": "yolov8n", "batch": 2, "report_interval_s": 1.0, "image_size": 64, "conf": 0.0,
        "max_det": 8, "track": True, "track_min_hits": 1, "track_max_age": 2}


class Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def _app(extra):
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport(dict(BASE, **extra))
    return tr, ModuleApp(tr, device="cpu", clock=Clock()).start()


def _open(b64):
    im = Image.open(io.BytesIO(base64.b64decode(b64)))
    im.load()
    return im


def test_config_snapshot_keys():
    d = ModuleConfig().validate()
    assert not set(ModuleConfig.SNAPSHOT_KEYS) & set(d.to_dict())   # reports what it reported
    assert (d.snapshots, d.snapshot_width, d.snapshot_subsampling, d.snapshot_quality,
            d.snapshot_every_s, d.snapshot_max_bytes) == (False, 320, "420", 75, 0.0, 131072)
    c = d.apply_patch({"snapshots": True, "snapshot_quality": "60"})
    assert set(ModuleConfig.SNAPSHOT_KEYS) <= set(c.to_dict()) and c.snapshot_quality == 60
    for k, v in (("snapshots", False), ("snapshot_width", 160), ("snapshot_subsampling", "444")):
        assert c.needs_rebuild(c.apply_patch({k: v}))
    for k, v in (("snapshot_quality", 30), ("snapshot_every_s", 5.0), ("snapshot_max_bytes", 9)):
        assert not c.needs_rebuild(c.apply_patch({k: v}))
    for bad in ({"snapshot_width": 15}, {"snapshot_width": 1921}, {"snapshot_subsampling": "422"},
                {"snapshot_quality": 0}, {"snapshot_quality": 101}, {"snapshot_every_s": -1},
                {"snapshot_max_bytes": 0}, {"snapshots": True, "model": "simulated-temperature"}):
        with pytest.raises(ValueError):
            d.apply_patch(bad)
    d.apply_patch({"snapshot_width": 16, "snapshot_quality": 1})
    d.apply_patch({"snapshot_width": 1920, "snapshot_quality": 100})


def test_module_cli_has_snapshot_flags():
    import inspect

    from kvedge_amd.module import __main__ as cli

    src = inspect.getsource(cli.main)
    for key in ModuleConfig.SNAPSHOT_KEYS:
        assert f'"--{key.replace("_", "-")}"' in src and f"{key}=a.{key}" in src


def test_snapshots_off_changes_nothing_and_on_adds_two_outputs():
    runs = {}
    for name, extra in (("off", {}), ("on", {"snapshots": True, "snapshot_width": 32}),
                        ("watch", {"watch": True}),
                        ("both", {"watch": True, "snapshots": True, "snapshot_width": 32})):
        tr, app = _app(extra)
        with app:
            app.run(max_steps=3)
            app.report()
            runs[name] = (tr.outputs("telemetry")[-1], app.engine.outputs,
                          dict(tr.reported["config"]), app.on_method("snapshot", {"camera": 0}),
                          tr.outputs("snapshots"), app.model)
    off, on, watch, both = (runs[k] for k in ("off", "on", "watch", "both"))
    assert not set(ModuleConfig.SNAPSHOT_KEYS) & set(off[2]) and off[3][0] == 400
    assert "snapshots" not in off[0] and off[4] == [] and watch[3][0] == 400
    assert set(on[0]) == set(off[0]) | {"snapshots"} and on[0]["snapshots"] == {"sent": 0,
                                                                               "oversize": 0}
    assert set(both[0]) == set(watch[0]) | {"snapshots"}
    assert len(on[1]) == len(off[1]) + 2 and len(both[1]) == len(watch[1]) + 2
    for a, b in zip(on[1], off[1]):
        assert torch.equal(a, b)
    # the watch stays outermost: its two outputs are the last two, with or without pictures
    assert torch.equal(both[1][-2], watch[1][-2]) and torch.equal(both[1][-1], watch[1][-1])
    from kvedge_amd.models.snapshots import snapshots_of

    for run, n_inner in ((on, len(off[1])), (both, len(off[1]))):
        stage = snapshots_of(run[5])
        assert stage is not None and stage.snap_index == n_inner
        assert run[1][n_inner].dtype == torch.uint8 and run[1][n_inner + 1].dtype == torch.int32
    assert snapshots_of(off[5]) is None and snapshots_of(watch[5]) is None
    assert both[5].snap_index == len(off[1])   # found through the watch, too
    status, body = on[3]
    assert status == 200 and set(body) == {"camera", "width", "height", "bytes", "jpeg_b64"}
    im = _open(body["jpeg_b64"])
    assert im.size == (32, 32) == (body["width"], body["height"])
    assert body["bytes"] == len(base64.b64decode(body["jpeg_b64"])) and body["camera"] == 0
    # the picture is the reference's file of the resized model-size frame
    frame = on[5].plan
    assert frame.src_hw == (64, 64) and frame.dst_hw == (32, 32)


def test_snapshot_method_rejects_bad_cameras():
    tr, app = _app({"snapshots": True, "snapshot_width": 32})
    with app:
        app.run(max_steps=1)
        for bad in ({"camera": 2}, {"camera": -1}, {}, {"camera": "x"}, None):
            assert app.on_method("snapshot", bad)[0] == 400, bad
        assert app.on_method("snapshot", {"camera": 1})[0] == 200
        tr.invoke_method("snapshot", {"camera": 1})
        app.step()
        name, status, body = tr.method_results[-1]
        assert (name, status, body["camera"]) == ("snapshot", 200, 1)


def test_a_camera_going_dark_sends_one_alarm_picture_in_that_step():
    tr, app = _app({"snapshots": True, "snapshot_width": 32, "watch": True, "watch_hold": 1,
                    "watch_cell": 8})
    frames = ws.script("rgb", 2, 64, 64, seed=5)
    frames[3][0] = frames[0][0]            # only camera 1 goes dark in step 4
    with app:
        app.engine.synthetic = False       # the test feeds the frames
        raised = []
        for f in frames:
            app.engine.input_frames.copy_(f)
            app.step()
            raised.append(app.model.watch_state.raised[:, ops.WATCH_CONDITIONS.index("dark")]
                          .tolist())
        app.report()
        assert raised == [[0, 0], [0, 0], [0, 0], [0, 1], [0, 1]]
        msgs = tr.outputs("snapshots")
        dark = [m for m in msgs if m["reason"] == "alarm:dark"]
        assert len(dark) == 1 and dark[0]["camera"] == 1 and dark[0]["step"] == 4
        assert set(dark[0]) == {"camera", "reason", "step", "width", "height", "bytes", "jpeg_b64"}
        im = _open(dark[0]["jpeg_b64"])
        assert im.size == (32, 32) and max(im.getextrema()[0]) < 8      # the black frame itself
        want = ref.jpeg_encode(ops.frame_resize(frames[3][1:2], ops.thumbnail_plan((64, 64), 32)),
                               "420", 75)[0]
        assert base64.b64decode(dark[0]["jpeg_b64"]) == want
        # every message is an alarm of the step it names, none periodic
        assert all(m["reason"].startswith("alarm:") for m in msgs)
        assert {m["reason"] for m in msgs if m["step"] == 2} == {"alarm:frozen"}
        assert tr.outputs("telemetry")[-1]["snapshots"] == {"sent": len(msgs), "oversize": 0}
        assert tr.outputs("telemetry")[-1]["camera_alarms"]["dark"] == 1


def test_quality_patches_without_a_rebuild_and_oversize_is_counted():
    tr, app = _app({"snapshots": True, "snapshot_width": 32, "snapshot_every_s": 0.1})
    with app:
        app.run(max_steps=1)
        first = tr.outputs("snapshots")
        assert [m["reason"] for m in first] == ["periodic", "periodic"]
        rebuilds = app.state["rebuilds"]
        tr.push_twin_patch({"snapshot_quality": 20})
        app.step()                          # the patch is applied at this step's boundary
        app.step()
        assert app.state["rebuilds"] == rebuilds and app.cfg.snapshot_quality == 20
        assert tr.reported["config"]["snapshot_quality"] == 20
        a = base64.b64decode(first[0]["jpeg_b64"])
        b = base64.b64decode(tr.outputs("snapshots")[-1]["jpeg_b64"])
        assert jc.dqt_bytes(a) != jc.dqt_bytes(b)
        assert jc.dqt_bytes(b) == jc.dqt_bytes(ref.jpeg_header((32, 32), "420",
                                                               ref.jpeg_quant_tables(20)))
        _open(tr.outputs("snapshots")[-1]["jpeg_b64"])
        # a limit below the file size: counted, not sent, and the method says so
        sent = len(tr.outputs("snapshots"))
        tr.push_twin_patch({"snapshot_max_bytes": 700})
        app.step()
        before = app.snapshots.summary()
        app.step()
        after = app.snapshots.summary()
        assert app.state["rebuilds"] == rebuilds
        assert after["sent"] == before["sent"] and after["oversize"] == before["oversize"] + 2
        assert len(tr.outputs("snapshots")) == before["sent"] >= sent
        assert app.on_method("snapshot", {"camera": 0})[0] == 413
        # a width change does rebuild
        tr.push_twin_patch({"snapshot_width": 48, "snapshot_max_bytes": 131072})
        app.step()
        app.step()
        assert app.state["rebuilds"] == rebuilds + 1
        assert _open(app.on_method("snapshot", {"camera": 0})[1]["jpeg_b64"]).size == (48, 48)


class _StubDetector:
    """Outputs (det, count) from the frames' first bytes: no convs, any frame size."""
    image_size = 32
    device = torch.device("cpu")

    def convs(self):
        return []

    def flops_per_image(self, hw=32):
        return 7

    def frame_plan(self, src_hw, image_size=0):
        return ops.letterbox_plan(src_hw, image_size or 32)

    def __call__(self, frames):
        n = frames.shape[0]
        det = frames.reshape(n, -1)[:, :12].float().view(n, 2, 6)
        return det, torch.full((n,), 2, dtype=torch.int32)

    def to_source(self, out, plan):
        return out[0] + 1.0, out[1]


def test_kvsnapshots_over_a_stub_detector_on_a_cpu_engine():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.snapshots import KvSnapshots
    from kvedge_amd.models.watching import KvWatched

    stub = _StubDetector()
    m = KvSnapshots(stub, 2, frame_hw=(24, 40), width=20, subsampling="444", quality=60)
    assert m.stateful and m.convs() == [] and m.flops_per_image(32) == 7
    assert m.frame_plan((24, 40), 32) == stub.frame_plan((24, 40), 32) and m.image_size == 32
    assert m.thumb_hw == (12, 20) and m.cap == ops.jpeg_max_bytes((12, 20), "444")
    for fmt in ("rgb", "nv12"):
        eng = InferenceEngine(KvWatched(m, 2, frame_hw=(24, 40), cell=8), 2, 32, device="cpu",
                              frame_hw=(24, 40), frame_format=fmt, synthetic=False)
        eng.prepare(warmup=1)
        f = ws.script(fmt, 2, 24, 40, seed=8)[2]
        out = eng.set_frames(f)
        assert len(out) == 6 and m.snap_index == 2 and out[2].shape == (2, m.cap)
        rgb = ops.nv12_to_rgb(f) if fmt == "nv12" else f
        want = ref.jpeg_encode(ops.frame_resize(rgb, m.plan), "444", 60)
        for cam in range(2):
            assert bytes(out[2][cam, :out[3][cam]].tolist()) == want[cam]
        base = stub.to_source(stub(eng.frames), eng.frame_plan)
        assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1])
    m.set_quality(10)
    out = eng.set_frames(f)
    assert bytes(out[2][1, :out[3][1]].tolist()) == ref.jpeg_encode(
        ops.frame_resize(rgb, m.plan), "444", 10)[1]
    # model-size frames; a small row reports the size it would need
    m2 = KvSnapshots(stub, 2, width=16, cap=700)
    eng = InferenceEngine(m2, 2, 32, device="cpu", synthetic=False).prepare(warmup=1)
    out = eng.set_frames(ws.script("rgb", 2, 32, 32)[0])
    assert m2.thumb_hw == (16, 16) and out[2].shape == (2, 700)
    want = ref.jpeg_encode(ops.frame_resize(eng.frames, m2.plan), "420", 75)
    assert out[3].tolist() == [len(w) if len(w) <= 700 else -len(w) for w in want]
    with pytest.raises(ValueError):
        KvSnapshots(stub, 2, width=0)
    with pytest.raises(ValueError):
        KvSnapshots(stub, 2, subsampling="422")
