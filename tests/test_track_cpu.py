"""IoU tracker on the CPU tier: ops.reference.track_update IS the definition the HIP kernel has
to equal bit for bit, so its rules are pinned here by hand-worked traces -- the velocity term,
confirmation, the tie rule, class gating, expiry, slot exhaustion -- along with the wrapper's
rejections, the twin keys and the engine / module running a tracked model through it."""
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference

NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _det(rows, max_det=None):
    """One stream's det [1, max_det, 6] / count [1] from rows (x1, y1, x2, y2[, cls])."""
    max_det = max_det or max(len(rows), 1)
    det = torch.zeros(1, max_det, 6)
    for r, row in enumerate(rows):
        det[0, r, :4] = torch.tensor(row[:4])
        det[0, r, 4] = 0.9
        det[0, r, 5] = float(row[4]) if len(row) > 4 else 0.0
    return det, torch.tensor([len(rows)], dtype=torch.int32)


def _step(state, rows, max_det=None, **kw):
    det, count = _det(rows, max_det)
    return ops.track_update(det, count, state, **kw)[0].tolist()


def _box(x, w=60.0):
    return (x, 10.0, x + w, 50.0)


# ---------------------------------------------------------------- quantisation
def test_quantize_values():
    x = torch.tensor([10.3, -3.0, NAN, INF, 5000.0, -INF, 0.124, 0.125, 4096.0, 4095.9, 0.0,
                      -0.1])
    assert reference.track_quantize(x).tolist() == [41, 0, 0, 16384, 16384, 0, 0, 1, 16384,
                                                    16384, 0, 0]
    assert reference.track_quantize(x).dtype == torch.int64
    c = torch.tensor([3.0, NAN, -2.0, INF, 79.0])
    assert reference.track_class(c).tolist() == [3, 0, 0, 65535, 79]
    assert ops.track_thr_q(0.3) == 307 and ops.track_thr_q(1.0) == 1024
    assert ops.track_thr_q(0.5) == 512 and ops.track_thr_q(0.0004) == 0


# ---------------------------------------------------------------- the three pinned traces
XS = (0.0, 20.0, 40.0, None, 80.0)  # a 60 px box; the fourth frame misses it


def test_trace_velocity_carries_the_track_over_a_missed_frame():
    st = ops.TrackState(1, 64)
    ids = [_step(st, [] if x is None else [_box(x)], max_det=1, iou=0.3, min_hits=1)[0]
           for x in XS]
    assert ids == [0, 0, 0, -1, 0]  # the missed frame has no row; then the same id again
    assert st.vel[0, 0].tolist() == [80, 0, 80, 0]  # quarter pixels per frame
    assert st.box[0, 0].tolist() == [320, 40, 560, 200]
    assert int(st.next_id[0]) == 1 and int(st.hits[0, 0]) == 4 and st.active() == 1


def test_trace_without_velocity_the_track_is_lost():
    st = ops.TrackState(1, 64)
    ids = []
    for x in XS:
        st.vel.zero_()  # the ablation: no motion model
        ids.append(_step(st, [] if x is None else [_box(x)], max_det=1, iou=0.3, min_hits=1)[0])
    # last frame: box at 40 against the detection at 80: IoU 20 / 100 < 0.3 -> a new object
    assert ids == [0, 0, 0, -1, 1]
    assert int(st.next_id[0]) == 2 and st.active() == 2


def test_trace_min_hits_confirms_on_the_third_frame():
    st = ops.TrackState(1, 64)
    ids = [_step(st, [_box(5.0)], iou=0.3, min_hits=3)[0] for _ in range(4)]
    assert ids == [-1, -1, 0, 0]
    assert int(st.next_id[0]) == 1 and st.id[0, 0] == 0 and st.hits[0, 0] == 4


# ---------------------------------------------------------------- rules
def test_tie_lower_slot_wins():
    st = ops.TrackState(1, 64)
    for slot, tid in ((5, 10), (2, 20)):  # two identical live tracks
        st.box[0, slot] = torch.tensor([40, 40, 280, 200], dtype=torch.int32)
        st.hits[0, slot], st.id[0, slot] = 3, tid
    st.next_id[0] = 21
    assert _step(st, [_box(10.0), _box(10.0)], min_hits=1) == [20, 10]  # slot 2 first
    assert st.hits[0, 2] == 4 and st.hits[0, 5] == 4


def test_best_iou_wins_over_slot_order():
    st = ops.TrackState(1, 64)
    st.box[0, 0] = torch.tensor([0, 40, 240, 200], dtype=torch.int32)   # x 0: IoU 40 / 80
    st.box[0, 1] = torch.tensor([80, 40, 320, 200], dtype=torch.int32)  # x 20: IoU 1
    st.hits[0, :2] = 1
    st.id[0, 0], st.id[0, 1] = 0, 1
    st.next_id[0] = 2
    assert _step(st, [_box(20.0)], min_hits=1) == [1]
    assert st.age[0].tolist()[:2] == [1, 0]


def _crossing(class_aware):
    st = ops.TrackState(1, 64)
    kw = dict(iou=0.3, min_hits=1, class_aware=class_aware)
    first = _step(st, [_box(0.0) + (1,), _box(40.0) + (2,)], **kw)
    # the two cross: the class-2 object is now nearer to where the class-1 object was, and
    # its row comes first
    second = _step(st, [_box(15.0) + (2,), _box(25.0) + (1,)], **kw)
    return first, second


def test_class_aware_keeps_ids_of_crossing_boxes():
    assert _crossing(True) == ([0, 1], [1, 0])   # class 2 keeps id 1, class 1 keeps id 0
    assert _crossing(False) == ([0, 1], [0, 1])  # greedy IoU alone swaps them


@pytest.mark.parametrize("max_age", [0, 2])
def test_expiry_after_exactly_max_age_missed_frames(max_age):
    kw = dict(iou=0.3, min_hits=1, max_age=max_age, max_det=1)
    for missed, want in ((max_age, 0), (max_age + 1, 1)):
        st = ops.TrackState(1, 64)
        assert _step(st, [_box(8.0)], **kw) == [0]
        for k in range(missed):
            _step(st, [], **kw)
            assert st.active() == (1 if k + 1 <= max_age else 0)
        assert _step(st, [_box(8.0)], **kw) == [want]


def test_tentative_track_dies_on_its_first_miss():
    st = ops.TrackState(1, 64)
    kw = dict(min_hits=3, max_age=30, max_det=1)
    _step(st, [_box(8.0)], **kw)
    _step(st, [_box(8.0)], **kw)
    assert st.active() == 1 and st.id[0, 0] == -1
    _step(st, [], **kw)
    assert st.active() == 0
    fresh = ops.TrackState(1, 64)
    assert torch.equal(st.buf, fresh.buf)  # all fields zero, id -1


def test_slot_exhaustion_counts_dropped():
    st = ops.TrackState(1, 64)
    rows = [(float(4 * i), 0.0, float(4 * i + 2), 2.0) for i in range(70)]  # disjoint boxes
    ids = _step(st, rows, min_hits=1)
    assert ids == list(range(64)) + [-1] * 6
    assert int(st.dropped[0]) == 6 and int(st.next_id[0]) == 64 and st.active() == 64
    ids = _step(st, rows, min_hits=1)  # the 64 continue, the other six are dropped again
    assert ids == list(range(64)) + [-1] * 6 and int(st.dropped[0]) == 12


def test_count_zero_and_count_past_max_det():
    st = ops.TrackState(2, 64)
    det = torch.zeros(2, 4, 6)
    for r in range(4):
        det[:, r, :4] = torch.tensor([20.0 * r, 0.0, 20.0 * r + 10, 10.0])
    count = torch.tensor([0, 99], dtype=torch.int32)  # clamped to max_det = 4
    out = torch.full((2, 4), 7, dtype=torch.int32)
    got = ops.track_update(det, count, st, min_hits=1, out=out)
    assert got is out and out.tolist() == [[-1] * 4, [0, 1, 2, 3]]
    assert st.next_id.tolist() == [0, 4]
    count = torch.tensor([-5, 2], dtype=torch.int32)
    assert ops.track_update(det, count, st, min_hits=1).tolist() == [[-1] * 4, [0, 1, -1, -1]]


def test_slot0_touches_only_its_streams():
    st = ops.TrackState(5, 64)
    st.buf[0].fill_(77)
    st.buf[4].fill_(-9)
    det, count = _det([_box(3.0)])
    det, count = det.repeat(3, 1, 1), count.repeat(3)
    ops.track_update(det, count, st, slot0=1, min_hits=1)
    assert st.buf[0].eq(77).all() and st.buf[4].eq(-9).all()
    assert st.next_id[1:4].tolist() == [1, 1, 1]


def test_state_views_and_reset():
    st = ops.TrackState(3, 128)
    assert st.buf.shape == (3, 12 * 128 + 4) and st.buf.dtype == torch.int32
    assert st.box.shape == (3, 128, 4) and st.vel.shape == (3, 128, 4)
    for name in ("cls", "id", "age", "hits"):
        assert getattr(st, name).shape == (3, 128)
    assert st.next_id.shape == (3,) and st.dropped.shape == (3,)
    assert st.id.eq(-1).all() and st.hits.eq(0).all() and st.active() == 0
    _step(ops.TrackState(1, 64), [_box(1.0)])
    st.box[1, 5, 2] = 9  # the views write through to the buffer
    assert st.buf[1, 5 * 4 + 2] == 9
    st.hits[2, 0] = 1
    assert st.active() == 1
    st.reset()
    assert st.active() == 0 and st.buf[1, 22] == 0 and st.id.eq(-1).all()
    assert set(ops.TRACK_FIELDS) <= set(vars(st))


def test_wrapper_rejections():
    st = ops.TrackState(2, 64)
    det, count = torch.zeros(2, 4, 6), torch.zeros(2, dtype=torch.int32)
    ops.track_update(det, count, st)  # the base call is fine
    bad = [
        dict(det=det.double()),                                   # dtype
        dict(det=torch.zeros(2, 4, 5)),                           # not 6 columns
        dict(det=torch.zeros(2, 8, 6)[:, ::2]),                   # not contiguous
        dict(count=count.long()),                                 # dtype
        dict(count=torch.zeros(3, dtype=torch.int32)),            # wrong N
        dict(det=torch.zeros(2, 301, 6)),                         # max_det > 300
        dict(slot0=1), dict(slot0=-1),                            # slot0 + N > S, negative
        dict(max_age=-1), dict(max_age=256),
        dict(min_hits=0), dict(min_hits=256),
        dict(iou=0.0), dict(iou=1.01), dict(iou=-0.3),
        dict(out=torch.zeros(2, 4, dtype=torch.int64)),           # out dtype
        dict(out=torch.zeros(2, 5, dtype=torch.int32)),           # out shape
    ]
    for kw in bad:
        args = dict(det=det, count=count)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.track_update(args.pop("det"), args.pop("count"), st, **args)
    with pytest.raises(TypeError):
        ops.track_update(det, count, st.buf)
    for t in (0, 32, 100, 320):
        with pytest.raises(ValueError):
            ops.TrackState(2, t)
    with pytest.raises(ValueError):
        ops.TrackState(0, 64)


# ---------------------------------------------------------------- twin keys
def test_config_track_keys():
    d = ModuleConfig().validate()
    assert (d.track, d.track_iou, d.track_max_age, d.track_min_hits, d.track_max_tracks) == (
        False, 0.3, 30, 3, 64)
    assert "track" not in d.to_dict()  # never asked to track: the config reported before
    c = d.apply_patch({"model": "yolov8n", "track": True, "track_iou": 0.4, "track_max_age": 5,
                       "track_min_hits": 1, "track_max_tracks": 128})
    assert c.track is True and c.to_dict()["track_max_tracks"] == 128
    assert {"track", "track_iou", "track_max_age", "track_min_hits",
            "track_max_tracks"} <= set(c.to_dict())
    for k, v in (("track", False), ("track_iou", 0.5), ("track_max_age", 6),
                 ("track_min_hits", 2), ("track_max_tracks", 64)):
        assert k in ModuleConfig.REBUILD and c.needs_rebuild(c.apply_patch({k: v}))
    assert d.apply_patch({"model": "detect-classify", "track": "true"}).track is True
    for bad in ({"track": True},                                  # resnet50 has no boxes
                {"model": "simulated-temperature", "track": True},
                {"track_iou": 0.0}, {"track_iou": 1.1}, {"track_iou": -1.0},
                {"track_max_age": -1}, {"track_max_age": 256},
                {"track_min_hits": 0}, {"track_min_hits": 256},
                {"track_max_tracks": 0}, {"track_max_tracks": 96}, {"track_max_tracks": 512}):
        with pytest.raises(ValueError):
            d.apply_patch(bad)
    # the cross-key check binds only when track is on
    assert d.apply_patch({"track_max_tracks": 256}).model == "resnet50"
    assert d.apply_patch({"track_iou": 1.0, "track_max_age": 255, "track_min_hits": 255})


def test_module_cli_has_track_flags():
    import inspect

    from kvedge_amd.module import __main__ as cli

    src = inspect.getsource(cli.main)
    for flag in ("--track", "--track-iou", "--track-max-age", "--track-min-hits",
                 "--track-max-tracks"):
        assert f'"{flag}"' in src


# ---------------------------------------------------------------- model / engine
@pytest.fixture(scope="module")
def yolo():
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    return KvYoloV8n(init_yolov8n(seed=0, calibrate=False), "cpu", conf=0.0, max_det=8)


@pytest.mark.parametrize("frame_hw", [None, (48, 64)])
def test_engine_cpu_tracked(yolo, frame_hw):
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.tracking import KvTracked

    m = KvTracked(yolo, 2, iou=0.3, max_age=3, min_hits=1)
    assert m.stateful and m.device == yolo.device and m.convs() == yolo.convs()
    assert m.flops_per_image(64) == yolo.flops_per_image(64)
    assert m.frame_plan((48, 64), 64) == yolo.frame_plan((48, 64), 64)
    eng = InferenceEngine(m, 2, 64, device="cpu", seed=3, frame_hw=frame_hw).prepare(warmup=2)
    # prepare() ran the step, which advanced the state; it leaves it freshly reset
    assert int(m.state.next_id.sum()) == 0 and torch.equal(m.state.buf,
                                                           ops.TrackState(2, 64).buf)
    want = ops.TrackState(2, 64)
    for step in range(3):
        det, count, tid = eng.run()
        assert tid.shape == (2, 8) and tid.dtype == torch.int32
        ref = torch.empty_like(tid)
        reference.track_update(det, count, want, 0, 307, 3, 1, True, ref)
        assert torch.equal(tid, ref) and torch.equal(m.state.buf, want.buf)
        if step == 0:
            n = int(count[0])
            assert n >= 1 and tid[0, :n].tolist() == list(range(n))  # ids start at 0
            if frame_hw is not None:  # tracked where they are reported: frame pixels
                assert int(m.state.box[0, :n, 2].max()) <= 64 * 4
                assert int(m.state.box[0, :n, 3].max()) <= 48 * 4
    assert int(m.state.next_id.sum()) > 0
    eng.reset_tracks()
    assert int(m.state.next_id.sum()) == 0 and m.state.active() == 0
    # an untracked model: reset_tracks is a no-op and the call signatures are untouched
    plain = InferenceEngine(yolo, 2, 64, device="cpu", seed=3, frame_hw=frame_hw).prepare(1)
    plain.reset_tracks()
    det2, count2 = plain.run()
    assert det2.shape == (2, 8, 6) and len(plain.outputs) == 2


def test_tracked_rejects_bad_parameters(yolo):
    from kvedge_amd.models.tracking import KvTracked

    for kw in (dict(iou=0.0), dict(max_age=256), dict(min_hits=0), dict(max_tracks=100)):
        with pytest.raises(ValueError):
            KvTracked(yolo, 2, **kw)


# ---------------------------------------------------------------- module
class Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def _module_telemetry(extra):
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport(dict({"model": "yolov8n", "batch": 2, "report_interval_s": 1.0,
                             "image_size": 64, "conf": 0.0, "max_det": 8}, **extra))
    with ModuleApp(tr, device="cpu", clock=Clock()).start() as app:
        app.run(max_steps=3)
        app.report()
        return tr.outputs("telemetry")[-1], app.engine.outputs, app.model, dict(
            tr.reported["config"])


def test_module_cpu_track_on_and_off():
    off, out_off, model_off, cfg_off = _module_telemetry({})
    on, out_on, model_on, cfg_on = _module_telemetry(
        {"track": True, "track_min_hits": 1, "track_max_age": 2})
    assert "tracks" not in off and len(out_off) == 2 and not hasattr(model_off, "state")
    assert "track" not in cfg_off and cfg_on["track"] is True and cfg_on["track_min_hits"] == 1
    assert set(on) == set(off) | {"tracks"}  # nothing else changes
    assert on["detections"] == off["detections"]
    for a, b in zip(out_on, out_off):
        assert torch.equal(a, b)
    assert len(out_on) == 3 and out_on[2].shape == (2, 8)
    st = model_on.state
    assert st.streams == 2 and st.max_tracks == 64  # one batch row = one camera
    assert on["tracks"] == {"active": st.active(), "unique": int(st.next_id.sum()),
                            "dropped": int(st.dropped.sum())}
    assert on["tracks"]["unique"] >= int(out_on[1].max()) >= 1 and on["tracks"]["active"] >= 1


# ---------------------------------------------------------------- ISA
@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_track_kernel_does_not_spill():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"),
                        os.path.join(ROOT, "csrc", "kernels", "track.hip"), "--no-spill"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    rows = [l for l in r.stdout.splitlines() if l.startswith("| track.hip")]
    assert len(rows) == 4, rows  # T = 64, 128, 192, 256
