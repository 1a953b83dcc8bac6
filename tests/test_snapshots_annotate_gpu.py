"""Annotated camera snapshots on the MI355X: the pictures coming out of the captured step of a
tracked YOLOv8n served from 64 x 96 NV12 frames -- in the engine (one and two batch slices) and
in the module's native loop -- equal the CPU reference drawing the step's own det / count /
track_id into the resized frame and encoding it, byte for byte; nothing else changes."""
import base64
import io

import pytest
import torch

import watch_script as ws
from kvedge_amd import ops
from kvedge_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

H, W = 64, 96


def _want(nv12_frames, plan, style, out, tid_index, quality):
    small = ops.frame_resize(ops.nv12_to_rgb(nv12_frames.cpu()), plan)
    ref.annotate(small, style.host, style.font_host, out[0].cpu(), out[1].cpu(),
                 out[tid_index].cpu(), (H, W), 0)
    return ref.jpeg_encode(small, "420", quality)


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
def test_engine_annotated_snapshots_of_a_tracked_detector(yolo, streams):
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.snapshots import KvSnapshots
    from kvedge_amd.models.tracking import KvTracked

    batch = 2
    kw = dict(device="cuda", seed=5, streams=streams, frame_hw=(H, W), frame_format="nv12",
              synthetic=False)
    tk = dict(iou=0.3, max_age=2, min_hits=1)
    style = ops.AnnotateStyle(batch, "cuda").set_privacy_block(4)
    style.set_privacy_polygon(0, [(60, 30), (96, 30), (96, 64), (60, 64)], camera=1)
    snap = KvSnapshots(KvTracked(yolo, batch, **tk), batch, frame_hw=(H, W), width=48,
                       subsampling="420", quality=75, annotate=style)
    bare = KvSnapshots(KvTracked(yolo, batch, **tk), batch, frame_hw=(H, W), width=48,
                       subsampling="420", quality=75)
    eng = InferenceEngine(snap, batch, 640, **kw).prepare(warmup=1, autotune=False)
    base_eng = InferenceEngine(bare, batch, 640, **kw).prepare(warmup=1, autotune=False)
    assert eng.graph is not None and eng.n_streams == streams
    assert snap.thumb_hw == (32, 48) and snap.snap_index == 3 and snap.inner.track_index == 2
    graph_out = eng.outputs
    frames = ws.script("nv12", batch, H, W, seed=11)[:3]
    for f in frames:                       # eagerly: every other output is what it was
        out = eng.set_frames(f.cuda())
        base = base_eng.set_frames(f.cuda())
        torch.cuda.synchronize()
        assert len(out) == len(base) == 5 and int(out[1].min()) > 0
        for a, b in zip(out[:3], base[:3]):
            assert torch.equal(a, b)
        want = _want(f, snap.plan, style, out, 2, 75)
        _check(out, 3, want)
        assert bytes(base[3][0, :base[4][0]].tolist()) != want[0]     # the bare picture differs
    # the captured step, then again with a class hidden, without recapturing
    for f, hide in ((frames[2], False), (frames[0], True)):
        eng.input_frames.copy_(f.cuda())
        if hide:
            style.set_privacy_classes([int(graph_out[0][0, 0, 5])]).set_thickness(2)
        eng.graph.replay()
        torch.cuda.synchronize()
        _check(graph_out, 3, _want(f, snap.plan, style, graph_out, 2, 75))


def test_module_native_serving_with_annotated_snapshots():
    Image = pytest.importorskip("PIL.Image")
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "yolov8n", "batch": 2, "track": True, "track_min_hits": 1,
                        "snapshots": True, "snapshot_width": 48, "snapshot_quality": 60,
                        "snapshot_annotate": True, "snapshot_privacy_classes": [0],
                        "snapshot_privacy_block": 4, "snapshot_every_s": 0.001,
                        "report_interval_s": 0.01, "steps_per_poll": 2, "conf": 0.0, "max_det": 8,
                        "source": "camera-nv12", "frame_height": H, "frame_width": W})
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None and app.snapshots is not None
        app.run(max_steps=2)
        torch.cuda.synchronize()
        out = app.engine.outputs
        stage = app.snapshots.stage
        assert len(out) == 5 and stage.snap_index == 3 and stage.annotate is not None
        # the frames the last replay read are still in the input buffer
        want = _want(app.engine.input_frames, stage.plan, stage.annotate, out, 2, 60)
        _check(out, 3, want)
        status, body = app.on_method("snapshot", {"camera": 1})
        assert status == 200 and body["annotated"] is True
        assert base64.b64decode(body["jpeg_b64"]) == want[1]
        im = Image.open(io.BytesIO(want[1]))
        im.load()
        assert im.size == (48, 32)
        msgs = tr.outputs("snapshots")
        assert msgs and all(m["annotated"] is True for m in msgs)
