"""The frame watch without a GPU: the CPU reference on hand-built frames with the answers worked
out here, shapes and layouts against a brute-force per-pixel loop, the twin keys, the KvWatched
wrapper on a CPU engine and the module's telemetry."""
import os
import shutil
import subprocess

import pytest
import torch

import watch_script as ws
from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference

MOTION, SCENE, DARK, FLAT, FROZEN = 1, 2, 4, 8, 16


def _rgb(y):
    """A grey RGB frame batch from luma [N, H, W]: R = G = B = Y gives luma Y exactly
    ((77 + 150 + 29) Y + 128) >> 8 = Y."""
    return torch.as_tensor(y, dtype=torch.uint8).unsqueeze(-1).repeat(1, 1, 1, 3).contiguous()


def _step(st, y, **kw):
    stats, mask = ops.frame_watch(_rgb(y), st, **kw)
    return stats, mask


# ---------------------------------------------------------------- hand-built frames
def test_constant_frame_is_flat_and_primes():
    st = ops.WatchState(1, (32, 48))
    stats, mask = _step(st, torch.full((1, 32, 48), 100))
    assert stats[0, :4].tolist() == [1600, 0, 0, 6]       # mean 100.0, no gradient, 2 x 3 cells
    assert stats[0, 4] == FLAT                            # first frame: no motion, not frozen
    assert mask.shape == (1, 2, 3) and int(mask.sum()) == 0
    assert int(st.primed[0]) == 1 and (st.acc == 1600 << 4).all()
    assert (st.sum == 100 * 256).all() and (st.grad == 0).all()
    stats, _ = _step(st, torch.full((1, 32, 48), 100))
    assert stats[0, 4] == FLAT | FROZEN and stats[0, 2] == 0
    st2 = ops.WatchState(1, (32, 48))
    odd = torch.full((1, 32, 48), 7)
    odd[0, 0, 0] = 8  # 16 * (7 * 1536 + 1) + 768 = 172816; / 1536 = 112 (truncating)
    assert _step(st2, odd)[0][0, 0] == 112


def test_block_moved_by_one_cell_flips_the_cells_it_leaves_and_enters():
    st = ops.WatchState(1, (64, 64), bg_shift=0).set_params(None, motion_thr16=160)
    y = torch.full((1, 64, 64), 50)
    y[0, 16:32, 16:32] = 200
    stats, mask = _step(st, y)
    assert int(mask.sum()) == 0
    y2 = torch.full((1, 64, 64), 50)
    y2[0, 16:32, 32:48] = 200
    stats, mask = _step(st, y2)
    want = torch.zeros(4, 4, dtype=torch.uint8)
    want[1, 1] = want[1, 2] = 1
    assert torch.equal(mask[0], want) and stats[0, 2] == 2
    assert stats[0, 4] & MOTION and not stats[0, 4] & SCENE  # 2 / 16 of the cells
    stats, mask = _step(st, y2)  # k = 0: the background is the last frame
    assert int(mask.sum()) == 0 and stats[0, 4] & FROZEN


@pytest.mark.parametrize("k", [0, 4, 8])
def test_background_recurrence_rising_and_falling(k):
    st = ops.WatchState(1, (8, 8), cell=8, bg_shift=k)
    _step(st, torch.full((1, 8, 8), 100))
    assert int(st.acc[0, 0, 0]) == 1600 << k
    acc = 1600 << k
    for level in [200] * 6 + [10] * 40:
        _step(st, torch.full((1, 8, 8), level))
        acc += 16 * level - (acc >> k)
        assert int(st.acc[0, 0, 0]) == acc
        if level == 10:
            assert (acc >> k) >= 160  # a falling step converges from above, never undershoots
    if k == 0:
        assert acc == 160
    # floor semantics of >> on the scaled accumulator: acc = 2^k * 160 + 1 keeps bg = 160
    st.acc[0, 0, 0] = (160 << k) + (1 if k else 0)
    stats, mask = _step(st.set_params(None, motion_thr16=0), torch.full((1, 8, 8), 10))
    assert int(mask.sum()) == 0 and int(st.acc[0, 0, 0]) == (160 << k) + (1 if k else 0)


def test_five_frame_script_run_counters_hold_and_raised():
    st = ops.WatchState(1, (32, 32)).set_params(
        None, motion_thr16=160, motion_share_q=10, scene_share_q=512, dark16=384, flat16=24,
        hold=2)
    g = torch.Generator().manual_seed(0)
    rnd = torch.randint(0, 256, (1, 32, 32), generator=g)
    shifted = rnd.clone()
    shifted[0, :16, :16] = 255
    seq = [rnd, rnd, shifted, torch.zeros(1, 32, 32), torch.full((1, 32, 32), 200),
           torch.full((1, 32, 32), 200)]
    rows = [_step(st, y)[0][0].tolist() for y in seq]
    conds = [r[4] for r in rows]
    assert conds[0] == 0                                   # primes: nothing
    assert conds[1] == FROZEN
    assert conds[2] == MOTION                              # one of four cells moved
    assert conds[3] == MOTION | SCENE | DARK | FLAT        # everything fell to black
    assert conds[4] == MOTION | SCENE | FLAT
    assert conds[5] & (FLAT | FROZEN) == FLAT | FROZEN
    runs = [r[6:11] for r in rows]
    assert [r[0] for r in runs] == [0, 0, 1, 2, 3, runs[5][0]]      # motion
    assert [r[3] for r in runs] == [0, 0, 0, 1, 2, 3]               # flat
    assert [r[4] for r in runs] == [0, 1, 0, 0, 0, 1]               # frozen
    alarms = [r[5] for r in rows]
    assert alarms[2] == 0 and alarms[3] == MOTION and alarms[4] == MOTION | SCENE | FLAT
    raised = [r[11:16] for r in rows]
    assert raised[3] == [1, 0, 0, 0, 0] and raised[4] == [1, 1, 0, 1, 0]
    assert raised[5][3] == 1                               # raised once, in the frame run == hold
    assert rows[5][6:11] == st.run[0].tolist() and rows[5][11:16] == st.raised[0].tolist()


def test_run_saturates_at_65535_and_raised_wraps():
    st = ops.WatchState(1, (8, 8), cell=8).set_params(None, hold=255, flat16=4096)
    st.run[0, 3] = 65534
    st.raised[0, 3] = 2 ** 31 - 1
    st.run[0, 2] = 254
    st.raised[0, 2] = 2 ** 31 - 1
    st.set_params(None, dark16=4096)
    for want in (65535, 65535):
        stats, _ = _step(st, torch.full((1, 8, 8), 9))
        assert stats[0, 9] == want and stats[0, 5] & FLAT
    assert int(st.raised[0, 3]) == 2 ** 31 - 1             # run passed hold long ago
    assert int(st.raised[0, 2]) == -2 ** 31                # run == hold = 255 once: wrapped


# ---------------------------------------------------------------- shapes and layouts
def _brute(y, cell, row_step):
    """Per-pixel loop over one luma plane [H, W] -> lists [GH][GW] of (n, sum, grad, pairs)."""
    H, W = y.shape
    GH, GW = -(-H // cell), -(-W // cell)
    out = [[[0, 0, 0, 0] for _ in range(GW)] for _ in range(GH)]
    rows = y.tolist()
    for yy in range(0, H, row_step):
        for xx in range(W):
            c = out[yy // cell][xx // cell]
            c[0] += 1
            c[1] += rows[yy][xx]
            if xx + 1 < W and (xx + 1) // cell == xx // cell:
                c[2] += abs(rows[yy][xx + 1] - rows[yy][xx])
                c[3] += 1
    return out


@pytest.mark.parametrize("h,w,cell", [(40, 56, 16), (70, 100, 32), (9, 17, 8)])
@pytest.mark.parametrize("row_step", [1, 2, 4])
def test_cells_against_a_per_pixel_loop(h, w, cell, row_step):
    g = torch.Generator().manual_seed(h + row_step)
    y = torch.randint(0, 256, (1, h, w), generator=g)
    n, s, gr, pr = reference.watch_cells(y.to(torch.int32), cell, row_step)
    want = _brute(y[0], cell, row_step)
    GH, GW = len(want), len(want[0])
    assert s.shape == (1, GH, GW)
    if (h, w, cell) == (40, 56, 16):
        assert (GH, GW) == (3, 4)  # an 8-row and an 8-column remainder
    for i in range(GH):
        for j in range(GW):
            assert [int(n[0, i, j]), int(s[0, i, j]), int(gr[0, i, j]),
                    int(pr[0, i, j])] == want[i][j]
    st = ops.WatchState(1, (h, w), cell=cell, row_step=row_step)
    stats, _ = ops.frame_watch(_rgb(y), st)
    P = sum(c[0] for r in want for c in r)
    Q = sum(c[3] for r in want for c in r)
    assert stats[0, 0] == (16 * sum(c[1] for r in want for c in r) + P // 2) // P
    assert stats[0, 1] == (16 * sum(c[2] for r in want for c in r) + Q // 2) // Q
    assert Q == -(-h // row_step) * (w - GW)
    assert torch.equal(st.sum[0], s[0].to(torch.int32))
    assert torch.equal(st.grad[0], gr[0].to(torch.int32))


def test_nv12_reads_luma_only():
    g = torch.Generator().manual_seed(1)
    f = torch.randint(0, 256, (2, 36, 40), dtype=torch.uint8, generator=g)  # 24 x 40
    a, b = ops.WatchState(2, (24, 40), cell=8), ops.WatchState(2, (24, 40), cell=8)
    f2 = f.clone()
    f2[:, 24:] = 255 - f2[:, 24:]  # every chroma byte changes
    for _ in range(2):
        sa, ma = ops.frame_watch(f, a, src_format="nv12")
        sb, mb = ops.frame_watch(f2, b, src_format="nv12")
        assert torch.equal(sa, sb) and torch.equal(ma, mb) and torch.equal(a.buf, b.buf)
    grey = ops.WatchState(2, (24, 40), cell=8)
    sg, _ = ops.frame_watch(_rgb(f[:, :24]), grey)  # the Y byte as it is
    assert torch.equal(sg[:, :2], ops.frame_watch(f, ops.WatchState(2, (24, 40), cell=8),
                                                  src_format="nv12")[0][:, :2])


def test_rgb_luma_at_the_corners_of_the_colour_cube():
    corners = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    want = {(0, 0, 0): 0, (0, 0, 255): 29, (0, 255, 0): 149, (0, 255, 255): 178,
            (255, 0, 0): 77, (255, 0, 255): 106, (255, 255, 0): 226, (255, 255, 255): 255}
    px = torch.tensor(corners, dtype=torch.uint8).view(1, 1, 8, 3)
    assert reference.watch_luma(px)[0, 0].tolist() == [want[c] for c in corners]
    for c in corners:  # (77 R + 150 G + 29 B + 128) >> 8, worked out by hand above
        assert want[c] == (77 * c[0] + 150 * c[1] + 29 * c[2] + 128) >> 8
    f = px.expand(1, 8, 8, 3).contiguous()
    stats, _ = ops.frame_watch(f, ops.WatchState(1, (8, 8), cell=8))
    assert stats[0, 0] == (16 * sum(want.values()) * 8 + 32) // 64


def test_slot0_leaves_the_other_streams_bit_for_bit_alone():
    st = ws.new_state(4, 40, 56)
    pat = torch.arange(st.buf.shape[1], dtype=torch.int32) * 3 - 99
    st.buf[0], st.buf[3] = pat, -pat
    for f in ws.script("rgb", 2, 40, 56, seed=2):
        ops.frame_watch(f, st, slot0=1)
    assert torch.equal(st.buf[0], pat) and torch.equal(st.buf[3], -pat)
    assert int(st.primed[1]) == 1 and int(st.primed[2]) == 1


def test_nv12_4096x4096_all_255_total_exceeds_int32():
    f = torch.full((1, 4096 * 3 // 2, 4096), 255, dtype=torch.uint8)
    stats, mask = ops.frame_watch(f, ops.WatchState(1, (4096, 4096)), src_format="nv12")
    assert 255 * 4096 * 4096 > 2 ** 31
    assert stats[0, :4].tolist() == [4080, 0, 0, 65536] and mask.shape == (1, 256, 256)


def test_script_is_busy_and_hostile_rows_clamp():
    want = ws.reference_run(ws.script("rgb", 3, 40, 56), "rgb", ws.new_state(3, 40, 56))
    conds = 0
    for stats, _, _ in want:
        for c in stats[:, 4].tolist():
            conds |= c
    assert conds == 0b11111 and int(want[-1][0][:, 11:16].sum()) > 0
    a, b = ops.WatchState(1, (16, 16)), ops.WatchState(1, (16, 16))
    a.params[0] = torch.tensor([-5, 99999, -7, 10 ** 6, -10 ** 6, 0], dtype=torch.int32)
    b.params[0] = torch.tensor([0, 1024, 0, 4096, 0, 1], dtype=torch.int32)
    for f in ws.script("rgb", 1, 16, 16, seed=4):
        assert torch.equal(ops.frame_watch(f, a)[0], ops.frame_watch(f, b)[0])


# ---------------------------------------------------------------- state, wrapper, config
def test_state_views_reset_and_rejections():
    st = ops.WatchState(2, (40, 56), cell=16, row_step=2, bg_shift=3)
    assert st.grid == (3, 4) and st.buf.shape == (2, 24 + 36) and st.acc.shape == (2, 3, 4)
    assert st.params[0].tolist() == [ops.WATCH_DEFAULTS[k] for k in ops.WATCH_PARAMS]
    st.set_params(1, hold=9)
    assert st.params[:, 5].tolist() == [8, 9]
    ops.frame_watch(torch.zeros(2, 40, 56, 3, dtype=torch.uint8), st)
    st.reset()
    assert int(st.buf[:, :16].abs().sum()) == 0 and int(st.buf[:, 24:].abs().sum()) == 0
    assert st.params[:, 5].tolist() == [8, 9]  # the thresholds stay
    for kw in (dict(cell=12), dict(row_step=3), dict(bg_shift=9), dict(bg_shift=-1)):
        with pytest.raises(ValueError):
            ops.WatchState(1, (40, 56), **kw)
    for hw in ((0, 8), (8, 1), (4097, 8), (8, 4097)):
        with pytest.raises(ValueError):
            ops.WatchState(1, hw)
    with pytest.raises(ValueError):
        ops.WatchState(0, (8, 8))
    for bad in (dict(hold=0), dict(hold=256), dict(motion_thr16=4081), dict(dark16=-1),
                dict(motion_share_q=1025), dict(flat16=4097), dict(hold=1.5), dict(nope=1)):
        with pytest.raises(ValueError):
            st.set_params(None, **bad)
    with pytest.raises(ValueError):
        st.set_params(2, hold=1)
    before = st.buf.clone()
    rgb = torch.zeros(2, 40, 56, 3, dtype=torch.uint8)
    for call in (lambda: ops.frame_watch(rgb, st, slot0=1),
                 lambda: ops.frame_watch(rgb[:, :, ::2], st),
                 lambda: ops.frame_watch(rgb.float(), st),
                 lambda: ops.frame_watch(rgb[:, :32], st),
                 lambda: ops.frame_watch(torch.zeros(2, 45, 50, dtype=torch.uint8), st,
                                         src_format="nv12"),
                 lambda: ops.frame_watch(torch.zeros(2, 62, 56, dtype=torch.uint8), st,
                                         src_format="nv12"),
                 lambda: ops.frame_watch(rgb, st, out_stats=torch.zeros(2, 16)),
                 lambda: ops.frame_watch(rgb, st, out_mask=torch.zeros(2, 3, 5,
                                                                       dtype=torch.uint8)),
                 lambda: ops.frame_watch(rgb, st, src_format="bgr")):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        ops.frame_watch(rgb, ops.TrackState(2))
    assert torch.equal(st.buf, before)


def test_config_watch_keys():
    d = ModuleConfig().validate()
    assert not set(ModuleConfig.WATCH_KEYS) & set(d.to_dict())  # reports what it reported
    tracked = d.apply_patch({"model": "yolov8n", "track": True})
    assert not set(ModuleConfig.WATCH_KEYS) & set(tracked.to_dict())
    c = d.apply_patch({"watch": True, "watch_hold": 3, "watch_motion_level": 12.5})
    rep = c.to_dict()
    assert set(ModuleConfig.WATCH_KEYS) <= set(rep) and rep["watch_cell"] == 16
    assert c.watch_params() == {"motion_thr16": 200, "motion_share_q": 10, "scene_share_q": 512,
                                "dark16": 384, "flat16": 24, "hold": 3}
    assert d.watch_params() == ops.WATCH_DEFAULTS
    ops.check_watch_params(**c.watch_params())
    import json

    assert d.apply_patch(json.loads(json.dumps(rep))) == c
    for k, v in (("watch", False), ("watch_cell", 8), ("watch_row_step", 2),
                 ("watch_bg_shift", 0)):
        assert c.needs_rebuild(c.apply_patch({k: v}))
    for k, v in (("watch_hold", 9), ("watch_dark_level", 40.0), ("watch_scene_share", 0.25)):
        assert not c.needs_rebuild(c.apply_patch({k: v}))  # thresholds: no recapture
    assert "watch_hold" in d.apply_patch({"watch_hold": 9}).to_dict()
    for bad in ({"watch_cell": 12}, {"watch_row_step": 3}, {"watch_bg_shift": 9},
                {"watch_bg_shift": -1}, {"watch_motion_level": 256}, {"watch_motion_level": -1},
                {"watch_motion_share": 1.5}, {"watch_scene_share": -0.1},
                {"watch_dark_level": 257}, {"watch_flat_level": -1}, {"watch_hold": 0},
                {"watch_hold": 256}, {"watch": True, "model": "simulated-temperature"}):
        with pytest.raises(ValueError):
            d.apply_patch(bad)
    ends = d.apply_patch({"watch_motion_level": 255, "watch_dark_level": 256,
                          "watch_flat_level": 256, "watch_motion_share": 1.0, "watch_hold": 255})
    ops.check_watch_params(**ends.watch_params())  # the launcher's ranges, end points included


def test_module_cli_has_watch_flags():
    import inspect

    from kvedge_amd.module import __main__ as cli

    src = inspect.getsource(cli.main)
    for key in ModuleConfig.WATCH_KEYS:
        assert f'"--{key.replace("_", "-")}"' in src and f"{key}=a.{key}" in src


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


def test_kvwatched_over_a_stub_detector_on_a_cpu_engine():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.watching import KvWatched, decode_stats

    stub = _StubDetector()
    m = KvWatched(stub, 2, frame_hw=(24, 40), cell=8, hold=1)
    assert m.stateful and m.convs() == [] and m.flops_per_image(32) == 7
    assert m.frame_plan((24, 40), 32) == stub.frame_plan((24, 40), 32) and m.image_size == 32
    assert not hasattr(m, "state") and not hasattr(m, "zone_state")
    for fmt in ("rgb", "nv12"):
        eng = InferenceEngine(m, 2, 32, device="cpu", seed=3, frame_hw=(24, 40),
                              frame_format=fmt, synthetic=False).prepare(warmup=1)
        want = ops.WatchState(2, (24, 40), cell=8).set_params(None, hold=1)
        assert torch.equal(m.watch_state.buf, want.buf)  # prepare() left it freshly reset
        for f in ws.script(fmt, 2, 24, 40, seed=8)[:3]:
            out = eng.set_frames(f)
            assert len(out) == 4
            w_stats, w_mask = ops.frame_watch(f, want, src_format=fmt)
            assert torch.equal(out[2], w_stats) and torch.equal(out[3], w_mask)
            base = stub.to_source(stub(eng.frames), eng.frame_plan)
            assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1])
        assert decode_stats(out[2][0])["motion"]["now"] is True
    # model-size frames are watched as RGB
    m2 = KvWatched(stub, 2, cell=8)
    eng = InferenceEngine(m2, 2, 32, device="cpu", synthetic=False).prepare(warmup=1)
    f = ws.script("rgb", 2, 32, 32)[0]
    out = eng.set_frames(f)
    want = ops.WatchState(2, (32, 32), cell=8)
    assert torch.equal(out[-2], ops.frame_watch(f, want)[0]) and out[-1].shape == (2, 4, 4)
    with pytest.raises(ValueError):
        KvWatched(stub, 2, hold=0)


class Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def _module(extra, steps=3):
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport(dict({"model": "yolov8n", "batch": 2, "report_interval_s": 1.0,
                             "image_size": 64, "conf": 0.0, "max_det": 8, "track": True,
                             "track_min_hits": 1, "track_max_age": 2}, **extra))
    with ModuleApp(tr, device="cpu", clock=Clock()).start() as app:
        app.run(max_steps=steps)
        app.report()
        return (tr.outputs("telemetry")[-1], app.engine.outputs, app.model,
                dict(tr.reported["config"]), app.on_method("cameras", {}), app)


def test_module_cpu_watch_on_and_off():
    off, out_off, model_off, cfg_off, method_off, _ = _module({})
    on, out_on, model_on, cfg_on, method_on, app = _module(
        {"watch": True, "watch_hold": 2, "watch_cell": 8, "watch_dark_level": 256,
         "watch_motion_level": 1})
    assert not set(ModuleConfig.WATCH_KEYS) & set(cfg_off) and method_off[0] == 400
    assert set(on) == set(off) | {"cameras", "camera_alarms"}  # nothing else changes
    assert on["tracks"] == off["tracks"] and on["detections"] == off["detections"]
    assert len(out_on) == len(out_off) + 2
    for a, b in zip(out_on, out_off):
        assert torch.equal(a, b)
    assert model_on.state is model_on.inner.state and cfg_on["watch_hold"] == 2
    st = model_on.watch_state
    assert out_on[-2].shape == (2, 16) and out_on[-1].shape == (2, 8, 8)
    assert torch.equal(out_on[-2][:, 11:16], st.raised)
    # synthetic frames are new noise every step: with a motion level below the noise of a
    # cell's mean, motion and scene are simply always on
    assert on["cameras"] == {"motion": 2, "scene": 2, "dark": 2, "flat": 0, "frozen": 0}
    assert on["camera_alarms"] == {"motion": 2, "scene": 2, "dark": 2, "flat": 0, "frozen": 0}
    status, body = method_on
    assert status == 200 and len(body["cameras"]) == 2
    assert body["cameras"][1]["dark"] == {"now": True, "alarm": True, "run": 3, "raised": 1}
    assert body["cameras"][0]["cells"] == 64 and body["cameras"][0]["mean"] > 100


def test_host_totals_stay_exact_over_a_wrapping_counter():
    from kvedge_amd.module.watch import CameraTotals, alarm_counts

    class Model:
        watch_resets = 0

    m = Model()
    m.watch_state = ops.WatchState(2, (8, 8), cell=8).set_params(None, hold=1, dark16=4096)
    m.watch_state.raised[:, 2] = 2 ** 31 - 1  # counters that have been running for a long time
    tot = CameraTotals(m)
    dark = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    stats, _ = ops.frame_watch(dark, m.watch_state)
    tot.update()
    assert m.watch_state.raised[:, 2].tolist() == [-2 ** 31] * 2  # wrapped on the device
    assert tot.summed() == {"motion": 0, "scene": 0, "dark": 2, "flat": 2, "frozen": 0}
    assert alarm_counts(stats)["dark"] == 2
    assert tot.per_camera(stats)[1]["dark"]["raised"] == 1
    m.watch_state.reset()  # a model reset starts the totals over
    m.watch_resets += 1
    assert tot.update().summed()["dark"] == 0


# ---------------------------------------------------------------- build
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_frame_watch_kernel_cross_compiles_without_warnings(tmp_path):
    from kvedge_amd import _build

    src = os.path.join(ROOT, "csrc", "kernels", "frame_watch.hip")
    assert src in _build.glob.glob(os.path.join(_build.CSRC, "kernels", "*.hip"))
    for extra in ([], ["-DKVEDGE_CHECKS=1"]):  # the bounds-check build covers it too
        r = subprocess.run([_build.hipcc(), *_build.COMMON, *extra, "-Wall", "-Wextra", "-Werror",
                            f"-I{_build.CSRC}/kernels", "-c", src, "-o", str(tmp_path / "fw.o")],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and not (r.stdout + r.stderr).strip(), r.stderr[-2000:]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_frame_watch_kernel_does_not_spill():
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"),
                        os.path.join(ROOT, "csrc", "kernels", "frame_watch.hip"), "--no-spill"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    rows = [l for l in r.stdout.splitlines() if l.startswith("| frame_watch.hip")]
    assert len(rows) == 7, rows  # six cell kernels (rgb / nv12 x cell 8 / 16 / 32) + totals
