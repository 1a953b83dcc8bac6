"""Line crossings and zone occupancy on the MI355X: the zone_update kernel against the CPU
reference, zone state, masks and counters compared bitwise after every step; a table no
ZoneSet would build; the launcher's rejections; a zoned detector captured into the engine's
hipGraph; and the module serving it through the native loop."""
import pytest
import torch

import zone_walk as zw
from kvedge_amd import ops
from kvedge_amd.ops import reference

pytestmark = pytest.mark.gpu

GUARD = 64  # int32 words kept 0xCDCDCDCD on either side of both outputs
CD = -842150451  # 0xCDCDCDCD as int32


def _guarded(n, width):
    buf = torch.full((GUARD + n * width + GUARD,), CD, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n * width].view(n, width)


def _guards_intact(buf, n, width):
    return bool((buf[:GUARD] == CD).all() and (buf[GUARD + n * width:] == CD).all())


def _pair_of_zone_states(S, T):
    """A GPU and a CPU zone state with the same content; cameras 0 and S - 1 hold a pattern no
    update may touch."""
    gpu, cpu = ops.ZoneState(S, T, "cuda"), ops.ZoneState(S, T)
    pat = torch.arange(cpu.buf.shape[1], dtype=torch.int32) * 5 - 700
    for st in (gpu, cpu):
        st.buf[0] = pat.to(st.device)
        st.buf[S - 1] = (-pat).to(st.device)
    return gpu, cpu, pat


def _step_both(det, cnt, slot0, n, track, zone, zones, track_kw):
    """One track_update + zone_update on the GPU and on the CPU from the same (CPU) inputs;
    det / count go in as slices of the larger batch.  Asserts everything the two must share."""
    (t_gpu, t_cpu), (z_gpu, z_cpu), (zn_gpu, zn_cpu) = track, zone, zones
    max_det = det.shape[1]
    d_gpu, c_gpu = det.cuda()[slot0:slot0 + n], cnt.cuda()[slot0:slot0 + n]
    ops.track_update(d_gpu, c_gpu, t_gpu, slot0=slot0, **track_kw)
    ops.track_update(det[slot0:slot0 + n], cnt[slot0:slot0 + n], t_cpu, slot0=slot0, **track_kw)
    before = t_gpu.buf.clone()
    mbuf, mask = _guarded(n, max_det)
    cbuf, counts = _guarded(n, 48)
    got = ops.zone_update(d_gpu, c_gpu, t_gpu, z_gpu, zn_gpu, slot0=slot0, out_mask=mask,
                          out_counts=counts)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == mask.data_ptr() and got[1].data_ptr() == counts.data_ptr()
    want_m = torch.full((n, max_det), CD, dtype=torch.int32)
    want_c = torch.full((n, 48), CD, dtype=torch.int32)
    ops.zone_update(det[slot0:slot0 + n], cnt[slot0:slot0 + n], t_cpu, z_cpu, zn_cpu,
                    slot0=slot0, out_mask=want_m, out_counts=want_c)
    assert _guards_intact(mbuf, n, max_det) and _guards_intact(cbuf, n, 48)
    assert torch.equal(t_gpu.buf, before)                 # the tracker state is only read
    assert torch.equal(t_gpu.buf.cpu(), t_cpu.buf)
    assert torch.equal(mask.cpu(), want_m)                # every element written
    assert torch.equal(counts.cpu(), want_c)
    assert torch.equal(z_gpu.buf.cpu(), z_cpu.buf)        # whole state, the other cameras too
    return want_m, want_c


@pytest.mark.parametrize("anchor", ["bottom", "centre"])
@pytest.mark.parametrize("T", [64, 192])
def test_zone_update_equals_cpu_reference(T, anchor):
    assert ops.load()
    S, N, slot0 = zw.S, zw.N, zw.SLOT0
    track = (ops.TrackState(S, T, "cuda"), ops.TrackState(S, T))
    z_gpu, z_cpu, pat = _pair_of_zone_states(S, T)
    zones = (zw.regions("cuda", anchor), zw.regions("cpu", anchor))
    assert torch.equal(zones[0].table.cpu(), zones[1].table)
    assert int(zones[1].n_vertex[slot0, 2]) == 8 and int(zones[1].zone_cls[slot0, 3]) == 2
    seen_bits = 0
    for step in range(zw.STEPS):
        det, cnt = zw.inputs(step)
        d = det.cuda()[slot0:slot0 + N]
        assert d.storage_offset() > 0 and d.is_contiguous()
        mask, _ = _step_both(det, cnt, slot0, N, track, (z_gpu, z_cpu), zones, zw.TRACK_KW)
        for v in mask.flatten().tolist():
            seen_bits |= v
    assert torch.equal(z_gpu.buf[0].cpu(), pat) and torch.equal(z_gpu.buf[S - 1].cpu(), -pat)
    zw.assert_busy(z_cpu)  # nothing vacuous: crossings both ways, entries, exits
    assert seen_bits & 0b100 and seen_bits & 0b1000  # the concave and the class-filtered zone


def test_zone_update_full_size_t256_300_rows():
    """max_det = count = 300 on T = 256: four slots per lane, five row sets, more detections
    than slots."""
    assert ops.load()
    T, max_det, steps = 256, 300, 3
    track = (ops.TrackState(1, T, "cuda"), ops.TrackState(1, T))
    zone = (ops.ZoneState(1, T, "cuda"), ops.ZoneState(1, T))
    zones = []
    for dev in ("cuda", "cpu"):
        one = ops.ZoneSet(1, dev)
        one.table.copy_(zw.regions(dev).table[zw.SLOT0:zw.SLOT0 + 1])
        zones.append(one)
    walk = zw._walk(1, max_det, steps, seed=9, span=700.0)
    cnt = torch.tensor([max_det], dtype=torch.int32)
    rows = 0
    for step in range(steps):
        mask, counts = _step_both(walk[step].contiguous(), cnt, 0, 1, track, zone, zones,
                                  dict(iou=0.3, max_age=1, min_hits=1, class_aware=True))
        rows += int((mask[0, 256:] != 0).sum())
    assert track[1].active() == T and rows >= 30        # rows past the slots carry masks too
    z = zone[1]  # nothing vacuous (the reference alone: 344 entries, 37 exits, 10 + 9 crossings)
    assert int(z.zone_enter.sum()) >= 200 and int(z.zone_exit.sum()) >= 20
    assert int(z.line_fwd.sum()) >= 5 and int(z.line_back.sum()) >= 5


def test_zone_mask_is_zero_past_count_when_a_zone_holds_the_origin():
    """Rows at or past count share a row set with real rows and carry the padding anchor (0, 0),
    class 0.  Zone 3 of the walk has a vertex at the origin and holds it under the rule; with its
    class filter lifted the padding rows would pass it, and must still get mask 0."""
    assert ops.load()
    S, N, slot0, T = zw.S, zw.N, zw.SLOT0, 64
    origin = torch.zeros((), dtype=torch.int64)
    poly = [(int(x * 4), int(y * 4)) for x, y in zw.ZONES[3][1]]
    assert poly[0] == (0, 0) and bool(reference.point_in_polygon(origin, origin, poly))
    track = (ops.TrackState(S, T, "cuda"), ops.TrackState(S, T))
    zone = (ops.ZoneState(S, T, "cuda"), ops.ZoneState(S, T))
    zones = (zw.regions("cuda"), zw.regions("cpu"))
    for zs in zones:
        zs.zone_cls[:, 3] = -1
    partial = hits = 0
    for step in range(6):  # counts 8, 7, 6, 5 among them
        det, cnt = zw.inputs(step)
        mask, _ = _step_both(det, cnt, slot0, N, track, zone, zones, zw.TRACK_KW)
        for n in range(N):
            c = int(cnt[slot0 + n])
            assert (mask[n, c:] == 0).all()  # the reference; the kernel equals it
            hits += int((mask[n, :c] & 0b1000 != 0).sum())
            partial += 0 < c < zw.MAX_DET
    assert partial >= 3 and hits >= 100  # nearly every real row is in zone 3
    # a partly filled second row set: count 70 of max_det 300, one camera
    track = (ops.TrackState(1, T, "cuda"), ops.TrackState(1, T))
    zone = (ops.ZoneState(1, T, "cuda"), ops.ZoneState(1, T))
    ones = []
    for zs in zones:
        one = ops.ZoneSet(1, zs.device)
        one.table.copy_(zs.table[slot0:slot0 + 1])
        ones.append(one)
    walk = zw._walk(1, 300, 1, seed=9, span=500.0)
    mask, _ = _step_both(walk[0].contiguous(), torch.tensor([70], dtype=torch.int32), 0, 1,
                         track, zone, ones, zw.TRACK_KW)
    assert int((mask[0, :70] & 0b1000 != 0).sum()) >= 60 and (mask[0, 70:] == 0).all()


@pytest.mark.parametrize("field,value", [("n_lines", 99), ("n_zones", -1), ("n_zones", 99),
                                         ("n_vertex", 100), ("n_vertex", -5), ("anchor", 7)])
def test_zone_update_clamps_a_hostile_table(field, value):
    """Counts written straight into the table tensor: the kernel clamps them as the reference
    does, so every read stays inside the table."""
    assert ops.load()
    S, N, slot0, T = zw.S, zw.N, zw.SLOT0, 64
    track = (ops.TrackState(S, T, "cuda"), ops.TrackState(S, T))
    zone = (ops.ZoneState(S, T, "cuda"), ops.ZoneState(S, T))
    zones = (zw.regions("cuda"), zw.regions("cpu"))
    for zs in zones:
        view = getattr(zs, field)
        if field == "n_vertex":
            view[:, 0] = value
            view[:, 7] = value
        else:
            view.fill_(value)
    assert torch.equal(zones[0].table.cpu(), zones[1].table)
    for step in range(4):
        det, cnt = zw.inputs(step)
        _step_both(det, cnt, slot0, N, track, zone, zones, zw.TRACK_KW)
    if (field, value) != ("n_zones", -1):
        assert int(zone[1].zone_enter.sum()) > 0


def test_zone_update_launcher_rejections_leave_everything_untouched():
    assert ops.load()
    k = torch.ops.kvedge.zone_update
    S, T, N, max_det = 3, 64, 2, 8
    det = zw.WALK[0, :N].contiguous().cuda()
    count = torch.tensor([8, 8], dtype=torch.int32).cuda()
    table = zw.regions("cuda").table[:S].contiguous()

    def full(*shape):
        return torch.full(shape, CD, dtype=torch.int32, device="cuda")

    def tstate(s=S, t=T):
        return ops.TrackState(s, t, "cuda").buf

    def zstate(s=S, t=T):
        return full(s, 4 * t + 48)

    def mask(n=N, m=max_det):
        return full(n, m)

    def counts(n=N, w=48):
        return full(n, w)

    wide = torch.cat([det, det], dim=2)[:, :, :6]  # strided view
    assert not wide.is_contiguous()
    big = torch.zeros(N, 301, 6, device="cuda")
    bad = [
        (det.double(), count, tstate(), zstate(), table, mask(), counts(), 0),   # wrong dtypes
        (det, count.long(), tstate(), zstate(), table, mask(), counts(), 0),
        (det, count, tstate().float(), zstate(), table, mask(), counts(), 0),
        (det, count, tstate(), zstate().float(), table, mask(), counts(), 0),
        (det, count, tstate(), zstate(), table.long(), mask(), counts(), 0),
        (det, count, tstate(), zstate(), table, mask().long(), counts(), 0),
        (det, count, tstate(), zstate(), table, mask(), counts().long(), 0),
        (wide, count, tstate(), zstate(), table, mask(), counts(), 0),           # not contiguous
        (det, count, tstate(), zstate(S, 2 * T)[:, :4 * T + 48], table, mask(), counts(), 0),
        (det, count, tstate(), zstate(), table, mask(N, 2 * max_det)[:, :max_det], counts(), 0),
        (det, count, tstate(), zstate(), table, mask(), counts(N, 96)[:, :48], 0),
        (det, count, tstate(), zstate(), full(S, 376)[:, :188], mask(), counts(), 0),
        (det, count, tstate(), full(S, 4 * T + 49), table, mask(), counts(), 0),  # state width
        (det, count, tstate(), zstate(S, 128), table, mask(), counts(), 0),       # another T
        (det, count, tstate(), zstate(S + 1), table, mask(), counts(), 0),        # another S
        (det, count, full(S, 12 * 96 + 4), zstate(S, 96), table, mask(), counts(), 0),  # T = 96
        (det, count, tstate(), zstate(), table, mask(), counts(), 2),             # slot0 + N > S
        (det, count, tstate(), zstate(), table, mask(), counts(), -1),
        (big, count, tstate(), zstate(), table, mask(N, 301), counts(), 0),       # max_det > 300
        (det, count, tstate(), zstate(), table[:, :187].contiguous(), mask(), counts(), 0),
        (det, count, tstate(), zstate(), table[:2].contiguous(), mask(), counts(), 0),
        (det, count[:1], tstate(), zstate(), table, mask(), counts(), 0),         # another N
        (det, count, tstate(), zstate(), table, mask(N, max_det + 1), counts(), 0),
        (det, count, tstate(), zstate(), table, mask(N + 1), counts(), 0),        # other shapes
        (det, count, tstate(), zstate(), table, mask(), counts(N, 47), 0),
        (det, count, tstate(), zstate(), table, mask(), counts(N + 1), 0),
        (det.cpu(), count, tstate(), zstate(), table, mask(), counts(), 0),       # CPU tensors
        (det, count, tstate().cpu(), zstate(), table, mask(), counts(), 0),
        (det, count, tstate(), zstate().cpu(), table, mask(), counts(), 0),
        (det, count, tstate(), zstate(), table.cpu(), mask(), counts(), 0),
        (det, count, tstate(), zstate(), table, mask().cpu(), counts(), 0),
    ]
    for i, args in enumerate(bad):
        with pytest.raises(RuntimeError):
            k(*args)
        torch.cuda.synchronize()
        for t in (args[3], args[5], args[6]):
            if t.dtype == torch.int32:
                assert (t == CD).all(), i
    # the ranges' end points are accepted, and N == 0 is a no-op
    zs = ops.ZoneState(S, T, "cuda")
    k(det, count, tstate(), zs.buf, table, mask(), counts(), 1)                    # slot0 + N == S
    k(det[:, :1].contiguous(), count, tstate(), zs.buf, table, mask(N, 1), counts(), 0)
    k(big[:, :300].contiguous(), count, tstate(), zs.buf, table, mask(N, 300), counts(), 0)
    k(det[:1], count[:1], tstate(1, 256), ops.ZoneState(1, 256, "cuda").buf, table[:1],
      mask(1), counts(1), 0)
    untouched, m0, c0 = zstate(), mask(0), counts(0)
    k(det[:0], count[:0], tstate(), untouched, table, m0, c0, 3)
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
def test_engine_graph_zoned(yolo, streams, frame_hw):
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.tracking import KvTracked, KvZoned

    batch = 4
    h, w = frame_hw or (640, 640)
    zones, zones_cpu = ops.ZoneSet(batch, "cuda"), ops.ZoneSet(batch)
    for zs in (zones, zones_cpu):
        zs.set_zone(None, 0, [(0, 0), (w, 0), (w, h), (0, h)])
        zs.set_zone(None, 1, [(0, 0), (w / 2, 0), (w / 2, h), (w / 4, h / 2), (0, h)])
        zs.set_zone(2, 2, [(w / 4, h / 4), (3 * w / 4, h / 4), (w / 2, 3 * h / 4)], cls=0)
        zs.set_line(None, 0, (w / 2, 0), (w / 2, h))
        zs.set_line(1, 1, (0, h / 2), (w, h / 2))
    m = KvZoned(KvTracked(yolo, batch, iou=0.3, max_age=2, min_hits=1), zones, anchor="centre")
    zones_cpu.set_anchor("centre")
    eng = InferenceEngine(m, batch, 640, device="cuda", seed=5, streams=streams,
                          frame_hw=frame_hw).prepare(warmup=2, autotune=False)
    assert eng.graph is not None and eng.n_streams == streams
    # warm-up and capture advanced both states; prepare() left them freshly reset
    assert torch.equal(m.state.buf.cpu(), ops.TrackState(batch, 64).buf)
    assert torch.equal(m.zone_state.buf.cpu(), ops.ZoneState(batch, 64).buf)
    want_t, want_z = ops.TrackState(batch, 64), ops.ZoneState(batch, 64)
    outs = []
    for step in range(5):
        out = eng.run()
        torch.cuda.synchronize()
        assert len(out) == 5
        det, count, tid, mask, counts = (t.cpu() for t in out)
        outs.append(counts)
        assert mask.shape == (batch, 16) and counts.shape == (batch, 48)
        assert mask.dtype == torch.int32 and counts.dtype == torch.int32
        ref = torch.empty(batch, 16, dtype=torch.int32)
        reference.track_update(det, count, want_t, 0, 307, 2, 1, True, ref)
        rm = torch.empty(batch, 16, dtype=torch.int32)
        rc = torch.empty(batch, 48, dtype=torch.int32)
        reference.zone_update(det, count, want_t, want_z, zones_cpu, 0, rm, rc)
        assert torch.equal(tid, ref), step
        assert torch.equal(mask, rm) and torch.equal(counts, rc), step
        assert torch.equal(m.zone_state.buf.cpu(), want_z.buf), step  # persists across replays
        assert torch.equal(m.state.buf.cpu(), want_t.buf), step
    assert len(outs) == 5 and int(want_z.zone_enter[:, 0].min()) >= 1
    assert torch.equal(want_z.zone_dwell[:, 0], sum(o[:, 32] for o in outs))
    print(f"zoned b{batch} x{streams} {frame_hw}: enter {want_z.zone_enter.sum(0).tolist()} "
          f"fwd {want_z.line_fwd.sum(0).tolist()} back {want_z.line_back.sum(0).tolist()}")
    eng.reset_tracks()
    assert torch.equal(m.state.buf.cpu(), ops.TrackState(batch, 64).buf)
    assert torch.equal(m.zone_state.buf.cpu(), ops.ZoneState(batch, 64).buf)


# ---------------------------------------------------------------- module
def test_module_native_serving_zoned():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    frame = [[0, 0], [640, 0], [640, 640], [0, 640]]
    tr = FakeTransport({"model": "yolov8n", "batch": 2, "track": True, "track_min_hits": 1,
                        "report_interval_s": 0.01, "source": "camera", "steps_per_poll": 2,
                        "conf": 0.0, "max_det": 8,
                        "zones": [{"name": "frame", "polygon": frame}],
                        "lines": [{"name": "mid", "a": [320, 0], "b": [320, 640]}]})
    # a failed assertion must still stop the camera thread: context manager
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None and app.model.stateful
        cfg = tr.reported["config"]
        assert cfg["zones"][0]["name"] == "frame" and cfg["lines"][0]["name"] == "mid"
        assert cfg["zone_anchor"] == "bottom" and cfg["track"] is True
        assert int(app.model.zone_state.counters.abs().sum()) == 0  # built, captured: zero
        app.run(max_steps=2)
        app.report()
        t = tr.outputs("telemetry")[-1]
        torch.cuda.synchronize()
        zs = app.model.zone_state
        assert t["zones"]["frame"] == {
            "occupancy": int(zs.zone_occ[:, 0].sum()), "entered": int(zs.zone_enter[:, 0].sum()),
            "exited": int(zs.zone_exit[:, 0].sum()),
            "dwell_frames": int(zs.zone_dwell[:, 0].sum())}
        assert t["zones"]["frame"]["entered"] >= 1
        assert t["lines"] == {"mid": {"forward": int(zs.line_fwd[:, 0].sum()),
                                      "backward": int(zs.line_back[:, 0].sum())}}
        assert len(app.engine.outputs) == 5 and app.engine.outputs[4].shape == (2, 48)
        assert t["tracks"]["unique"] >= 1
        status, body = app.on_method("zones", {})
        assert status == 200 and len(body["cameras"]) == 2
