"""IoU tracker on the MI355X: the track_update kernel against the CPU reference, state and ids
compared bitwise after every step; its launcher's rejections; a tracked detector captured into
the engine's hipGraph (one and two stream slices, native frames and model-size ones); the
tracked cascade; and the module serving it through the native loop."""
import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.ops import reference

pytestmark = pytest.mark.gpu

GUARD = 64  # int32 words kept 0xCDCDCDCD on either side of track_id
CD = -842150451  # 0xCDCDCDCD as int32
NAN, INF = float("nan"), float("inf")
ODD_ROWS = [  # boxes no tracker should choke on
    (NAN, NAN, NAN, NAN), (NAN, 4.0, 20.0, NAN), (-INF, -INF, INF, INF), (INF, INF, -INF, -INF),
    (300.0, 200.0, 100.0, 50.0),  # inverted
    (12.0, 8.0, 12.0, 8.0),       # zero area
    (5000.0, 5000.0, 6000.0, 6000.0),  # beyond 4096 px
]


def _guarded_ids(n, max_det):
    buf = torch.full((GUARD + n * max_det + GUARD,), CD, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n * max_det].view(n, max_det)


def _walk(streams, objects, steps, seed, span=600.0):
    """[steps, streams, objects, 6]: seeded random-walk boxes (a few px per step, so most are
    re-found, some drift apart or cross), three classes, scores descending by row."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(streams, objects, 2, generator=g) * span
    size = 20.0 + torch.rand(streams, objects, 2, generator=g) * 80.0
    cls = torch.randint(0, 3, (streams, objects), generator=g).float()
    drift = (torch.rand(streams, objects, 2, generator=g) - 0.5) * 16.0
    out = []
    for _ in range(steps):
        pos = pos + drift + torch.randn(streams, objects, 2, generator=g) * 3.0
        box = torch.cat([pos, pos + size], dim=-1)
        score = torch.linspace(0.9, 0.1, objects).expand(streams, objects)
        out.append(torch.cat([box, score.unsqueeze(-1), cls.unsqueeze(-1)], dim=-1))
    return torch.stack(out)


def _pair_of_states(S, T):
    """A GPU and a CPU state with the same content; streams 0 and S - 1 hold a pattern no
    update may touch."""
    gpu, cpu = ops.TrackState(S, T, "cuda"), ops.TrackState(S, T)
    pat = torch.arange(cpu.buf.shape[1], dtype=torch.int32) * 7 - 1000
    for st in (gpu, cpu):
        st.buf[0] = pat.to(st.device)
        st.buf[S - 1] = (-pat).to(st.device)
    return gpu, cpu


COUNTS = [(8, 1, 0), (8, 8, 1), (0, 8, 8), (1, 0, 8), (8, 5, 3), (7, 8, 0)]


@pytest.mark.parametrize("T,min_hits,max_age,class_aware",
                         [(64, 2, 2, True), (64, 1, 1, False), (192, 3, 3, True),
                          (128, 1, 0, True)])
def test_track_update_equals_cpu_reference(T, min_hits, max_age, class_aware):
    assert ops.load()
    S, N, slot0, max_det, steps = 5, 3, 1, 8, 12
    gpu, cpu = _pair_of_states(S, T)
    walk = _walk(N, max_det, steps, seed=T + min_hits)
    kw = dict(slot0=slot0, iou=0.3, max_age=max_age, min_hits=min_hits,
              class_aware=class_aware)
    matched = 0
    for step in range(steps):
        full = torch.zeros(S, max_det, 6)
        full[slot0:slot0 + N] = walk[step]
        if step % 3 == 2:  # rows a detector should never emit, in kept slots
            for i, row in enumerate(ODD_ROWS):
                full[slot0 + i % N, (step + i) % max_det, :4] = torch.tensor(row)
            full[slot0, 0, 5] = NAN
        cnt_full = torch.zeros(S, dtype=torch.int32)
        cnt_full[slot0:slot0 + N] = torch.tensor(COUNTS[step % len(COUNTS)], dtype=torch.int32)
        if step == 7:
            cnt_full[slot0] = 99   # past max_det: clamped
            cnt_full[slot0 + 1] = -3
        # det / count: slices of a larger batch (non-zero storage offset, as the stream
        # slices of the engine are)
        det, count = full.cuda()[slot0:slot0 + N], cnt_full.cuda()[slot0:slot0 + N]
        assert det.storage_offset() > 0 and count.storage_offset() > 0 and det.is_contiguous()
        buf, ids = _guarded_ids(N, max_det)
        got = ops.track_update(det, count, gpu, out=ids, **kw)
        torch.cuda.synchronize()
        assert got.data_ptr() == ids.data_ptr()
        want = torch.full((N, max_det), CD, dtype=torch.int32)
        ops.track_update(full[slot0:slot0 + N], cnt_full[slot0:slot0 + N], cpu, out=want, **kw)
        assert (buf[:GUARD] == CD).all() and (buf[GUARD + N * max_det:] == CD).all()
        assert torch.equal(ids.cpu(), want), step            # every element written
        assert torch.equal(gpu.buf.cpu(), cpu.buf), step     # whole state, streams 0 / 4 too
        matched += int((cpu.hits[slot0:slot0 + N] > 1).sum())
    pat = torch.arange(cpu.buf.shape[1], dtype=torch.int32) * 7 - 1000
    assert torch.equal(gpu.buf[0].cpu(), pat) and torch.equal(gpu.buf[S - 1].cpu(), -pat)
    # nothing vacuous: tracks were continued, ids handed out, slots freed and reused
    assert matched > 20 and int(cpu.next_id[slot0:slot0 + N].sum()) >= 8


def test_track_update_full_loop_t256_300_rows():
    """max_det = count = 300 on T = 256: the whole sequential loop, four slots per lane, and
    more detections than slots."""
    assert ops.load()
    T, max_det, steps = 256, 300, 3
    gpu, cpu = ops.TrackState(1, T, "cuda"), ops.TrackState(1, T)
    walk = _walk(1, max_det, steps, seed=9, span=1800.0)
    count = torch.tensor([max_det], dtype=torch.int32)
    kw = dict(iou=0.3, max_age=1, min_hits=1, class_aware=True)
    for step in range(steps):
        det = walk[step].contiguous()
        buf, ids = _guarded_ids(1, max_det)
        ops.track_update(det.cuda(), count.cuda(), gpu, out=ids, **kw)
        torch.cuda.synchronize()
        want = ops.track_update(det, count, cpu, **kw)
        assert (buf[:GUARD] == CD).all() and (buf[GUARD + max_det:] == CD).all()
        assert torch.equal(ids.cpu(), want), step
        assert torch.equal(gpu.buf.cpu(), cpu.buf), step
    assert cpu.active() == T and int(cpu.dropped[0]) >= steps * (max_det - T)
    assert int((cpu.hits > 1).sum()) > 100  # most tracks were re-found


def test_track_update_launcher_rejections_leave_everything_untouched():
    assert ops.load()
    k = torch.ops.kvedge.track_update
    S, T, N, max_det = 3, 64, 2, 8
    det = _walk(N, max_det, 1, seed=1)[0].contiguous().cuda()
    count = torch.tensor([8, 8], dtype=torch.int32).cuda()

    def state(s=S, t=T):
        return torch.full((s, 12 * t + 4), CD, dtype=torch.int32, device="cuda")

    def ids(n=N, m=max_det):
        return torch.full((n, m), CD, dtype=torch.int32, device="cuda")

    wide = torch.cat([det, det], dim=2)[:, :, :6]  # strided view
    assert not wide.is_contiguous()
    big = torch.zeros(N, 301, 6, device="cuda")
    bad = [
        (det.double(), count, state(), ids(), 0, 307, 30, 3, True),      # wrong dtypes
        (det, count.long(), state(), ids(), 0, 307, 30, 3, True),
        (det, count, state().float(), ids(), 0, 307, 30, 3, True),
        (det, count, state(), ids().long(), 0, 307, 30, 3, True),
        (wide, count, state(), ids(), 0, 307, 30, 3, True),              # not contiguous
        (det, count, state(S, 2 * T)[:, :12 * T + 4], ids(), 0, 307, 30, 3, True),
        (det, count, state(), ids(N, 2 * max_det)[:, :max_det], 0, 307, 30, 3, True),
        (det, count, state(), ids(), 2, 307, 30, 3, True),               # slot0 + N > S
        (det, count, state(), ids(), -1, 307, 30, 3, True),
        (det, count, state(S, 32), ids(), 0, 307, 30, 3, True),          # T not 64..256
        (det, count, state(S, 320), ids(), 0, 307, 30, 3, True),
        (det, count, state(S, 96), ids(), 0, 307, 30, 3, True),
        (det, count, torch.full((S, 12 * T + 5), CD, dtype=torch.int32, device="cuda"), ids(),
         0, 307, 30, 3, True),                                            # not 12 T + 4
        (big, count, state(), ids(N, 301), 0, 307, 30, 3, True),         # max_det > 300
        (det, count, state(), ids(), 0, 307, -1, 3, True),               # max_age
        (det, count, state(), ids(), 0, 307, 256, 3, True),
        (det, count, state(), ids(), 0, 307, 30, 0, True),               # min_hits
        (det, count, state(), ids(), 0, 307, 30, 256, True),
        (det, count, state(), ids(), 0, 0, 30, 3, True),                 # thr_q
        (det, count, state(), ids(), 0, 1025, 30, 3, True),
        (det, count[:1], state(), ids(), 0, 307, 30, 3, True),           # count of another N
        (det, count, state(), ids(N, max_det + 1), 0, 307, 30, 3, True),  # ids of another shape
        (det, count, state().cpu(), ids(), 0, 307, 30, 3, True),
    ]
    for i, args in enumerate(bad):
        with pytest.raises(RuntimeError):
            k(*args)
        torch.cuda.synchronize()
        for t in (args[2], args[3]):
            if t.dtype == torch.int32:
                assert (t == CD).all(), i
    # the ranges' end points are accepted, and N == 0 is a no-op
    st = ops.TrackState(S, T, "cuda")
    for thr_q, max_age, min_hits in ((1, 0, 1), (1024, 255, 255)):
        k(det, count, st.buf, ids(), 1, thr_q, max_age, min_hits, False)
    untouched = state()
    k(det[:0], count[:0], untouched, ids(0), 3, 307, 30, 3, True)
    torch.cuda.synchronize()
    assert (untouched == CD).all()


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def yolo():
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    # conf 0: random-init weights keep boxes
    return KvYoloV8n(init_yolov8n(0), "cuda", conf=0.0, max_det=16)


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("frame_hw", [None, (120, 160)])
def test_engine_graph_tracked(yolo, streams, frame_hw):
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.tracking import KvTracked

    batch = 4
    m = KvTracked(yolo, batch, iou=0.3, max_age=2, min_hits=1)
    eng = InferenceEngine(m, batch, 640, device="cuda", seed=5, streams=streams,
                          frame_hw=frame_hw).prepare(warmup=2, autotune=False)
    assert eng.graph is not None and eng.n_streams == streams
    # warm-up and capture advanced the state; prepare() left it freshly reset
    assert torch.equal(m.state.buf.cpu(), ops.TrackState(batch, 64).buf)
    want = ops.TrackState(batch, 64)
    for step in range(5):
        det, count, tid = eng.run()
        torch.cuda.synchronize()
        assert tid.shape == (batch, 16) and tid.dtype == torch.int32
        det_c, count_c = det.cpu(), count.cpu()
        ref = torch.empty(batch, 16, dtype=torch.int32)
        reference.track_update(det_c, count_c, want, 0, 307, 2, 1, True, ref)
        assert torch.equal(tid.cpu(), ref), step
        assert torch.equal(m.state.buf.cpu(), want.buf), step  # persists across replays
        if step == 0:
            assert int(count_c.min()) >= 1
            for n in range(batch):  # every camera's ids start at 0
                c = int(count_c[n])
                assert ref[n, :c].tolist() == list(range(c))
            if frame_hw is not None:  # tracked in frame pixels
                assert int(want.box[..., 2].max()) <= 160 * 4
                assert int(want.box[..., 3].max()) <= 120 * 4
    print(f"tracked b{batch} x{streams} {frame_hw}: counts {count_c.tolist()} "
          f"unique {want.next_id.tolist()} active {want.active()}")
    eng.reset_tracks()
    assert torch.equal(m.state.buf.cpu(), ops.TrackState(batch, 64).buf)


def test_tracked_cascade_appends_track_id():
    from kvedge_amd.models.cascade import KvDetectClassify
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50
    from kvedge_amd.models.tracking import KvTracked
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    det = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.0, max_det=8)
    plain = KvDetectClassify(det, KvResNet50(init_resnet50(seed=0), "cuda"), 2)
    tracked = KvTracked(plain, 2, min_hits=1)
    frames = torch.randint(0, 256, (2, 640, 640, 3), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(4)).cuda()
    want = plain(frames)
    got = tracked(frames)
    torch.cuda.synchronize()
    assert len(want) == 4 and len(got) == 5
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    tid, count = got[4].cpu(), got[1].cpu()
    assert tid.shape == (2, 8) and tid.dtype == torch.int32
    for n in range(2):
        c = int(count[n])
        assert c >= 1 and tid[n, :c].tolist() == list(range(c)) and (tid[n, c:] == -1).all()
    assert tracked.state.unique() == int(count.sum())


# ---------------------------------------------------------------- module
def test_module_native_serving_tracked():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "yolov8n", "batch": 2, "track": True, "track_min_hits": 1,
                        "track_max_tracks": 128, "report_interval_s": 0.01,
                        "source": "camera", "steps_per_poll": 2, "conf": 0.0, "max_det": 8})
    # a failed assertion must still stop the camera thread: context manager
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None and app.model.stateful
        assert tr.reported["config"]["track"] is True
        assert app.model.state.unique() == 0  # built, tuned, captured: still at zero
        app.run(max_steps=2)
        app.report()
        t = tr.outputs("telemetry")[-1]
        assert t["source"] == "camera" and t["images_per_s"] > 0
        assert app.state["total_images"] == 2 * 2 * 2
        torch.cuda.synchronize()
        st = app.model.state
        assert st.streams == 2 and st.max_tracks == 128
        assert t["tracks"] == {"active": st.active(), "unique": st.unique(),
                               "dropped": int(st.dropped.sum())}
        assert t["tracks"]["unique"] >= 1 and t["tracks"]["active"] >= 1
        assert len(app.engine.outputs) == 3 and app.engine.outputs[2].shape == (2, 8)
        assert t["detections"]["total"] == int(app.engine.outputs[1].sum())
