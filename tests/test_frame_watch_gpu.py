"""The frame watch on the MI355X: the frame_watch kernels against the CPU reference, the whole
state buffer, stats and motion mask compared bitwise after every step of the five-frame script;
poisoned outputs; untouched neighbour streams; a hostile parameter row; the launcher's
rejections; the step inside a captured graph; a watched, tracked detector in the engine; and
the module serving it through the native loop."""
import pytest
import torch

import watch_script as ws
from kvedge_amd import ops

pytestmark = pytest.mark.gpu

POISON_I, POISON_B = ws.CD, 0xCD


def _run_case(fmt, h, w, n, cell=16, row_step=1, bg_shift=4, frames=None, seed=0):
    """The script on the GPU and on the CPU from the same bytes; everything compared bitwise
    after every step.  Returns the reference's per-step results."""
    assert ops.load()
    kw = dict(cell=cell, row_step=row_step, bg_shift=bg_shift)
    frames = frames or ws.script(fmt, n, h, w, seed)
    cpu, gpu = ws.new_state(n, h, w, **kw), ws.new_state(n, h, w, "cuda", **kw)
    assert torch.equal(gpu.buf.cpu(), cpu.buf)
    want = ws.reference_run(frames, fmt, cpu)
    for step, (f, (w_stats, w_mask, w_buf)) in enumerate(zip(frames, want)):
        stats = torch.full((n, 16), POISON_I, dtype=torch.int32, device="cuda")
        mask = torch.full((n, *gpu.grid), POISON_B, dtype=torch.uint8, device="cuda")
        got = ops.frame_watch(f.cuda(), gpu, src_format=fmt, out_stats=stats, out_mask=mask)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == stats.data_ptr() and got[1].data_ptr() == mask.data_ptr()
        assert torch.equal(stats.cpu(), w_stats), (step, stats.cpu(), w_stats)
        assert torch.equal(mask.cpu(), w_mask), step   # every element written: no poison left
        assert torch.equal(gpu.buf.cpu(), w_buf), step
    return want


def _busy(want):
    """Nothing vacuous: the script moved cells, froze, went dark and flat, raised alarms."""
    conds = 0
    for stats, mask, _ in want:
        for c in stats[:, 4].tolist():
            conds |= c
    assert conds == 0b11111, bin(conds)
    assert int(want[-1][0][:, 11:16].sum()) > 0 and int(want[2][1].sum()) > 0


@pytest.mark.parametrize("row_step", [1, 2])
def test_rgb_40x56_partial_cells_both_ways(row_step):
    want = _run_case("rgb", 40, 56, 3, cell=16, row_step=row_step)
    assert want[0][1].shape == (3, 3, 4)
    _busy(want)


@pytest.mark.parametrize("row_step", [1, 4])
def test_nv12_24x528_more_cells_than_lanes(row_step):
    want = _run_case("nv12", 24, 528, 3, cell=8, row_step=row_step, bg_shift=0)
    assert want[0][1].shape == (3, 3, 66)
    _busy(want)


def test_rgb_70x100_cell32_pitch_aligned_to_4():
    want = _run_case("rgb", 70, 100, 3, cell=32, bg_shift=8)
    assert want[0][1].shape == (3, 3, 4)
    _busy(want)


def test_nv12_30x50_pitch_aligned_to_2():
    want = _run_case("nv12", 30, 50, 3)
    assert want[0][1].shape == (3, 2, 4)
    _busy(want)


def test_rgb_256x512_cell8_reduction_over_2048_cells():
    want = _run_case("rgb", 256, 512, 2, cell=8)
    assert want[0][1].shape == (2, 32, 64)
    _busy(want)


@pytest.mark.parametrize("fmt,cell", [("nv12", 32), ("rgb", 16), ("nv12", 16), ("rgb", 8)])
def test_vector_path_sizes(fmt, cell):
    """Pitches % 16 == 0: the wide-load path of every remaining cell size, with a partial last
    cell row (72 = 2 * 32 + 8) and whole columns."""
    _busy(_run_case(fmt, 72, 128, 3, cell=cell, row_step=2))


def test_nv12_4096x4096_all_255_int64_total():
    f = torch.full((1, 4096 * 3 // 2, 4096), 255, dtype=torch.uint8)
    want = _run_case("nv12", 4096, 4096, 1, frames=[f])
    assert 4096 * 4096 * 255 > 2 ** 31
    assert want[0][0][0, :4].tolist() == [4080, 0, 0, 256 * 256]


def test_slot0_leaves_the_other_streams_alone():
    assert ops.load()
    h, w, S, N, slot0 = 40, 56, 4, 2, 1
    cpu, gpu = ws.new_state(S, h, w), ws.new_state(S, h, w, "cuda")
    pat = torch.arange(cpu.buf.shape[1], dtype=torch.int32) * 7 - 300
    for st in (cpu, gpu):
        st.buf[0] = pat.to(st.device)
        st.buf[3] = (-pat).to(st.device)
    for step, f in enumerate(ws.script("rgb", S, h, w, seed=3)):
        part = f.cuda()[slot0:slot0 + N]
        assert part.storage_offset() > 0 and part.is_contiguous()
        stats, mask = ops.frame_watch(part, gpu, slot0=slot0)
        w_stats, w_mask = ops.frame_watch(f[slot0:slot0 + N], cpu, slot0=slot0)
        assert torch.equal(stats.cpu(), w_stats) and torch.equal(mask.cpu(), w_mask), step
        assert torch.equal(gpu.buf.cpu(), cpu.buf), step
    assert torch.equal(gpu.buf[0].cpu(), pat) and torch.equal(gpu.buf[3].cpu(), -pat)


def test_hostile_parameter_row_is_clamped():
    """Thresholds far out of range, hold 0 and 10^6, written straight into the state: the
    kernel behaves as the reference does on the same row, i.e. as on the clamped row."""
    assert ops.load()
    h, w, n = 40, 56, 3
    rows = torch.tensor([[-5, 99999, -7, 10 ** 6, -10 ** 6, 0],
                         [10 ** 6, -3, 2048, -1, 10 ** 7, 10 ** 6],
                         [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 5000, 4097, -9]],
                        dtype=torch.int32)
    clamped = torch.tensor([[0, 1024, 0, 4096, 0, 1], [4080, 0, 1024, 0, 4096, 255],
                            [4080, 0, 1024, 4096, 4096, 1]], dtype=torch.int32)
    hostile_cpu, clamped_cpu = ops.WatchState(n, (h, w)), ops.WatchState(n, (h, w))
    gpu = ops.WatchState(n, (h, w), device="cuda")
    hostile_cpu.params.copy_(rows)
    gpu.params.copy_(rows.cuda())
    clamped_cpu.params.copy_(clamped)
    for step, f in enumerate(ws.script("rgb", n, h, w, seed=5)):
        stats, mask = ops.frame_watch(f.cuda(), gpu)
        a_stats, a_mask = ops.frame_watch(f, hostile_cpu)
        b_stats, b_mask = ops.frame_watch(f, clamped_cpu)
        assert torch.equal(stats.cpu(), a_stats) and torch.equal(a_stats, b_stats), step
        assert torch.equal(mask.cpu(), a_mask) and torch.equal(a_mask, b_mask), step
        assert torch.equal(gpu.buf.cpu(), hostile_cpu.buf), step
        assert torch.equal(gpu.params.cpu(), rows)  # the row itself is only read


def test_launcher_rejections_leave_everything_untouched():
    assert ops.load()
    k = torch.ops.kvedge.frame_watch
    S, N, h, w = 3, 2, 40, 56
    C = 3 * 4
    rgb = torch.zeros(N, h, w, 3, dtype=torch.uint8, device="cuda")
    nv = torch.zeros(N, h * 3 // 2, w, dtype=torch.uint8, device="cuda")

    def state(s=S, width=24 + 3 * C):
        return torch.full((s, width), POISON_I, dtype=torch.int32, device="cuda")

    def stats(n=N, width=16):
        return torch.full((n, width), POISON_I, dtype=torch.int32, device="cuda")

    def mask(n=N, gh=3, gw=4):
        return torch.full((n, gh, gw), POISON_B, dtype=torch.uint8, device="cuda")

    odd = torch.zeros(N, 45, 50, dtype=torch.uint8, device="cuda")       # NV12 of 30 x 50: fine
    bad = [
        (rgb.float(), state(), stats(), mask(), 0, False, 16, 1, 4),      # wrong dtypes
        (rgb, state().float(), stats(), mask(), 0, False, 16, 1, 4),
        (rgb, state(), stats().long(), mask(), 0, False, 16, 1, 4),
        (rgb, state(), stats(), mask().int(), 0, False, 16, 1, 4),
        (rgb[:, :, :, :2], state(), stats(), mask(), 0, False, 16, 1, 4),  # shape, strided
        (rgb[:, :, ::2], state(), stats(), mask(), 0, False, 16, 1, 4),    # not contiguous
        (nv, state(), stats(), mask(), 0, False, 16, 1, 4),                # 3-d as RGB
        (rgb, state(), stats(), mask(), 0, True, 16, 1, 4),                # 4-d as NV12
        (torch.zeros(N, 61, w, dtype=torch.uint8, device="cuda"), state(), stats(), mask(), 0,
         True, 16, 1, 4),                                                  # rows not Hs * 3 / 2
        (torch.zeros(N, 62, w, dtype=torch.uint8, device="cuda"), state(), stats(), mask(), 0,
         True, 16, 1, 4),                                                  # odd NV12 height 41
        (torch.zeros(N, 60, 55, dtype=torch.uint8, device="cuda"), state(), stats(), mask(), 0,
         True, 16, 1, 4),                                                  # odd NV12 width
        (rgb, state(width=24 + 3 * C + 1), stats(), mask(), 0, False, 16, 1, 4),  # state width
        (rgb, state(S, 2 * (24 + 3 * C))[:, :24 + 3 * C], stats(), mask(), 0, False, 16, 1, 4),
        (rgb, state(), stats(N, 15), mask(), 0, False, 16, 1, 4),
        (rgb, state(), stats(N + 1), mask(), 0, False, 16, 1, 4),
        (rgb, state(), stats(N, 32)[:, :16], mask(), 0, False, 16, 1, 4),
        (rgb, state(), stats(), mask(N, 4, 4), 0, False, 16, 1, 4),
        (rgb, state(), stats(), mask(N, 3, 8)[:, :, :4], 0, False, 16, 1, 4),
        (rgb, state(), stats(), mask(N + 1), 0, False, 16, 1, 4),
        (rgb, state(), stats(), mask(), 2, False, 16, 1, 4),               # slot0 + N > S
        (rgb, state(), stats(), mask(), -1, False, 16, 1, 4),
        (rgb, state(), stats(), mask(), 0, False, 12, 1, 4),               # cell
        (rgb, state(), stats(), mask(), 0, False, 16, 3, 4),               # row_step
        (rgb, state(), stats(), mask(), 0, False, 16, 1, 9),               # bg_shift
        (rgb, state(), stats(), mask(), 0, False, 16, 1, -1),
        (rgb, state(), stats(), mask(), 0, False, 8, 1, 4),                # grid of another cell
        (torch.zeros(N, 2, 1, 3, dtype=torch.uint8, device="cuda"), state(width=27), stats(),
         mask(N, 1, 1), 0, False, 16, 1, 4),                               # Ws < 2
        (rgb.cpu(), state(), stats(), mask(), 0, False, 16, 1, 4),         # CPU tensors
        (rgb, state().cpu(), stats(), mask(), 0, False, 16, 1, 4),
        (rgb, state(), stats().cpu(), mask(), 0, False, 16, 1, 4),
        (rgb, state(), stats(), mask().cpu(), 0, False, 16, 1, 4),
    ]
    for i, args in enumerate(bad):
        with pytest.raises(RuntimeError):
            k(*args)
        torch.cuda.synchronize()
        for t, poison in ((args[1], POISON_I), (args[2], POISON_I), (args[3], POISON_B)):
            if t.dtype in (torch.int32, torch.uint8):
                assert (t == poison).all(), i
    # the Python wrapper rejects the same before it reaches the launcher
    st = ops.WatchState(S, (h, w), device="cuda")
    before = st.buf.clone()
    for call in (lambda: ops.frame_watch(rgb, st, slot0=2),
                 lambda: ops.frame_watch(rgb[:, :, ::2], st),
                 lambda: ops.frame_watch(rgb.cpu(), st),
                 lambda: ops.frame_watch(nv, st, src_format="rgb"),
                 lambda: ops.frame_watch(odd, st, src_format="nv12"),
                 lambda: ops.frame_watch(rgb, st, src_format="bgr"),
                 lambda: ops.frame_watch(rgb.int(), st)):
        with pytest.raises((ValueError, TypeError)):
            call()
    assert torch.equal(st.buf, before)
    # the ranges' end points are accepted, and N == 0 is a no-op
    k(rgb, st.buf, stats(), mask(), 1, False, 16, 1, 4)                    # slot0 + N == S
    k(nv, st.buf, stats(), mask(), 0, True, 16, 4, 8)
    tiny = ops.WatchState(1, (1, 2), cell=8, device="cuda")
    k(torch.zeros(1, 1, 2, 3, dtype=torch.uint8, device="cuda"), tiny.buf, stats(1),
      mask(1, 1, 1), 0, False, 8, 1, 0)
    untouched = state()
    k(rgb[:0], untouched, stats(0), mask(0), 3, False, 16, 1, 4)
    torch.cuda.synchronize()
    assert (untouched == POISON_I).all()


def test_captured_step_replayed_three_times():
    assert ops.load()
    h, w, n = 48, 64, 3
    frames = ws.script("nv12", n, h, w, seed=7)
    cpu, gpu = ws.new_state(n, h, w, row_step=2), ws.new_state(n, h, w, "cuda", row_step=2)
    src = frames[0].cuda()
    stats = torch.empty(n, 16, dtype=torch.int32, device="cuda")
    mask = torch.empty(n, *gpu.grid, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.frame_watch(src, gpu, src_format="nv12", out_stats=stats, out_mask=mask)  # warm
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gpu.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.frame_watch(src, gpu, src_format="nv12", out_stats=stats, out_mask=mask)
    torch.cuda.synchronize()
    gpu.reset()  # the capture itself ran nothing, but start from a known state
    want = ws.reference_run(frames[1:4], "nv12", cpu)
    for step, (f, (w_stats, w_mask, w_buf)) in enumerate(zip(frames[1:4], want)):
        src.copy_(f)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(stats.cpu(), w_stats) and torch.equal(mask.cpu(), w_mask), step
        assert torch.equal(gpu.buf.cpu(), w_buf), step
    gpu.set_params(None, hold=1, dark16=4096)  # thresholds change without recapturing
    cpu.set_params(None, hold=1, dark16=4096)
    g.replay()
    torch.cuda.synchronize()
    w_stats, _ = ops.frame_watch(frames[3], cpu, src_format="nv12")
    assert torch.equal(stats.cpu(), w_stats) and bool((w_stats[:, 5] & 4).all())


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def yolo():
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    return KvYoloV8n(init_yolov8n(0), "cuda", conf=0.0, max_det=16)


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("frame_hw,fmt", [(None, "rgb"), ((120, 160), "rgb"),
                                          ((120, 160), "nv12")])
def test_engine_watched_tracked(yolo, streams, frame_hw, fmt):
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.tracking import KvTracked
    from kvedge_amd.models.watching import KvWatched

    batch = 4
    h, w = frame_hw or (640, 640)
    kw = dict(device="cuda", seed=5, streams=streams, frame_hw=frame_hw, frame_format=fmt,
              synthetic=False)
    tk = dict(iou=0.3, max_age=2, min_hits=1)
    m = KvWatched(KvTracked(yolo, batch, **tk), batch, frame_hw=frame_hw, cell=16, row_step=2,
                  hold=2)
    plain = KvTracked(yolo, batch, **tk)
    eng = InferenceEngine(m, batch, 640, **kw).prepare(warmup=1, autotune=False)
    ref_eng = InferenceEngine(plain, batch, 640, **kw).prepare(warmup=1, autotune=False)
    assert eng.graph is not None and eng.n_streams == streams
    graph_out = eng.outputs  # the captured step's outputs (set_frames runs eagerly)
    assert m.state is m.inner.state  # the tracker's state, reached through the wrapper
    want = ops.WatchState(batch, (h, w), cell=16, row_step=2).set_params(None, hold=2)
    assert torch.equal(m.watch_state.buf.cpu(), want.buf)  # prepare() left it freshly reset
    frames = ws.script(fmt, batch, h, w, seed=11)[:3]
    for step, f in enumerate(frames):
        out = eng.set_frames(f.cuda())
        base = ref_eng.set_frames(f.cuda())
        torch.cuda.synchronize()
        assert len(out) == len(base) + 2
        for a, b in zip(out, base):
            assert torch.equal(a, b), step
        w_stats, w_mask = ops.frame_watch(f, want, src_format=fmt)
        assert torch.equal(out[-2].cpu(), w_stats), step
        assert torch.equal(out[-1].cpu(), w_mask), step
        assert torch.equal(m.watch_state.buf.cpu(), want.buf), step
        assert int(want.run[:, 4].min()) == (step == 1)  # the second frame repeats: frozen
    # and the captured step: one replay on the last frame again
    eng.input_frames.copy_(frames[2].cuda())
    eng.graph.replay()
    torch.cuda.synchronize()
    w_stats, w_mask = ops.frame_watch(frames[2], want, src_format=fmt)
    assert len(graph_out) == len(out)
    assert torch.equal(graph_out[-2].cpu(), w_stats) and torch.equal(graph_out[-1].cpu(), w_mask)
    assert torch.equal(m.watch_state.buf.cpu(), want.buf)
    eng.reset_tracks()
    assert int(m.watch_state.primed.sum()) == 0 and int(m.state.hits.sum()) == 0


# ---------------------------------------------------------------- module
@pytest.mark.parametrize("source", [{"source": "camera"},
                                    {"source": "camera-nv12", "frame_height": 120,
                                     "frame_width": 160}])
def test_module_native_serving_watched(source):
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport(dict({"model": "yolov8n", "batch": 2, "track": True, "track_min_hits": 1,
                             "watch": True, "watch_hold": 1, "watch_dark_level": 256,
                             "report_interval_s": 0.01, "steps_per_poll": 2, "conf": 0.0,
                             "max_det": 8}, **source))
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None and app.model.stateful
        assert app.model.watch_state.frame_hw == (source.get("frame_height", 640),
                                                  source.get("frame_width", 640))
        cfg = tr.reported["config"]
        assert cfg["watch"] is True and cfg["watch_hold"] == 1 and cfg["track"] is True
        assert int(app.model.watch_state.primed.sum()) == 0  # built, captured: reset
        app.run(max_steps=2)
        app.report()
        t = tr.outputs("telemetry")[-1]
        torch.cuda.synchronize()
        st = app.model.watch_state
        stats = app.engine.outputs[-2].cpu()
        assert len(app.engine.outputs) == 5 and stats.shape == (2, 16)
        assert torch.equal(stats[:, 6:11], st.run.cpu())
        assert torch.equal(stats[:, 11:16], st.raised.cpu())
        hold = st.params[:, 5].cpu().view(-1, 1)
        on = (st.run.cpu() >= hold).sum(0).tolist()
        assert t["cameras"] == dict(zip(ops.WATCH_CONDITIONS, on))
        assert t["cameras"]["dark"] == 2  # every frame is below level 256
        assert t["camera_alarms"] == dict(zip(ops.WATCH_CONDITIONS, st.raised.cpu().sum(0).tolist()))
        assert t["camera_alarms"]["dark"] == 2 and t["tracks"]["unique"] >= 1
        status, body = app.on_method("cameras", {})
        assert status == 200 and len(body["cameras"]) == 2
        assert body["cameras"][0]["dark"] == {"now": True, "alarm": True,
                                              "run": int(st.run[0, 2]), "raised": 1}
