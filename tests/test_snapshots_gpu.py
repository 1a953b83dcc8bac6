"""Camera snapshots on the MI355X: the pictures coming out of the captured step -- a tracked,
watched YOLOv8n served from 64 x 96 NV12 frames, in the engine (one and two batch slices) and
in the module's native loop -- equal the CPU reference applied to the resized frame, byte for
byte."""
import base64

import pytest
import torch

import watch_script as ws
from kvedge_amd import ops
from kvedge_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

H, W = 64, 96


def _want(nv12_frames, plan, sub, quality):
    small = ops.frame_resize(ops.nv12_to_rgb(nv12_frames.cpu()), plan)
    return ref.jpeg_encode(small, sub, quality)


def _check(out, idx, want):
    buf, length = out[idx].cpu(), out[idx + 1].cpu()
    assert length.tolist() == [len(f) for f in want]
    for cam, f in enumerate(want):
        assert bytes(buf[cam, :len(f)].tolist()) == f, cam


@pytest.fixture(scope="module")
def yolo():
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    return KvYoloV8n(init_yolov8n(0), "cuda", conf=0.0, max_det=16)


@pytest.mark.parametrize("streams", [1, 2])
def test_engine_snapshots_of_a_tracked_watched_detector(yolo, streams):
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.snapshots import KvSnapshots
    from kvedge_amd.models.tracking import KvTracked
    from kvedge_amd.models.watching import KvWatched

    batch = 2
    kw = dict(device="cuda", seed=5, streams=streams, frame_hw=(H, W), frame_format="nv12",
              synthetic=False)
    tk = dict(iou=0.3, max_age=2, min_hits=1)
    snap = KvSnapshots(KvTracked(yolo, batch, **tk), batch, frame_hw=(H, W), width=48,
                       subsampling="420", quality=75)
    m = KvWatched(snap, batch, frame_hw=(H, W), cell=16, hold=2)
    watched = KvWatched(KvTracked(yolo, batch, **tk), batch, frame_hw=(H, W), cell=16, hold=2)
    eng = InferenceEngine(m, batch, 640, **kw).prepare(warmup=1, autotune=False)
    base_eng = InferenceEngine(watched, batch, 640, **kw).prepare(warmup=1, autotune=False)
    assert eng.graph is not None and eng.n_streams == streams
    assert snap.thumb_hw == (32, 48) and m.snap_index == 3 and m.state is snap.inner.state
    graph_out = eng.outputs
    frames = ws.script("nv12", batch, H, W, seed=11)[:3]
    for f in frames:                       # eagerly: everything else is what it was
        out = eng.set_frames(f.cuda())
        base = base_eng.set_frames(f.cuda())
        torch.cuda.synchronize()
        assert len(out) == len(base) + 2
        for a, b in zip(out[:3] + out[-2:], base):
            assert torch.equal(a, b)
        _check(out, 3, _want(f, snap.plan, "420", 75))
    # the captured step, then again at another quality without recapturing
    for f, quality in ((frames[2], 75), (frames[0], 35)):
        eng.input_frames.copy_(f.cuda())
        snap.set_quality(quality)
        eng.graph.replay()
        torch.cuda.synchronize()
        _check(graph_out, 3, _want(f, snap.plan, "420", quality))


def test_module_native_serving_with_snapshots():
    pytest.importorskip("PIL")
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    import jpeg_cases as jc

    tr = FakeTransport({"model": "yolov8n", "batch": 2, "track": True, "track_min_hits": 1,
                        "watch": True, "watch_hold": 1, "watch_dark_level": 256,
                        "snapshots": True, "snapshot_width": 48, "snapshot_quality": 60,
                        "report_interval_s": 0.01, "steps_per_poll": 2, "conf": 0.0, "max_det": 8,
                        "source": "camera-nv12", "frame_height": H, "frame_width": W})
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None and app.snapshots is not None
        app.run(max_steps=2)
        app.report()
        torch.cuda.synchronize()
        out = app.engine.outputs
        idx = app.model.snap_index
        assert len(out) == 7 and idx == 3 and out[-2].shape == (2, 16)
        stage = app.snapshots.stage
        # the frames the last replay read are still in the input buffer
        want = _want(app.engine.input_frames, stage.plan, "420", 60)
        _check(out, idx, want)
        t = tr.outputs("telemetry")[-1]
        msgs = tr.outputs("snapshots")
        # every frame is below level 256 and hold is 1: both cameras raise `dark` at once
        assert sorted(m["camera"] for m in msgs if m["reason"] == "alarm:dark") == [0, 1]
        assert t["snapshots"] == {"sent": len(msgs), "oversize": 0}
        assert t["camera_alarms"]["dark"] == 2
        for m in msgs:
            assert jc.decode(base64.b64decode(m["jpeg_b64"])).size == (48, 32)
        status, body = app.on_method("snapshot", {"camera": 1})
        assert status == 200 and base64.b64decode(body["jpeg_b64"]) == want[1]
        assert app.on_method("snapshot", {"camera": 2})[0] == 400
