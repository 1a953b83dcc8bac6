"""Line crossings and zone occupancy on the CPU: ops.reference.zone_update, the definition the
HIP kernel equals, against hand-computed scenarios, an independent Fraction point-in-polygon
and its own invariants; the host totals over a wrapping counter; the twin keys; the module."""
import os
import random
import shutil
import subprocess
from fractions import Fraction

import pytest
import torch

import zone_walk as zw
from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Scene:
    """One camera: tracker (min_hits 1) + zones, stepped with pixel boxes (x1, y1, x2, y2, cls)."""

    def __init__(self, max_age=2, anchor="bottom", max_det=4):
        self.ts, self.zs, self.zones = ops.TrackState(1, 64), ops.ZoneState(1, 64), ops.ZoneSet(1)
        self.zones.set_anchor(anchor)
        self.max_age, self.max_det = max_age, max_det

    def step(self, *boxes):
        det = torch.zeros(1, self.max_det, 6)
        for r, (x1, y1, x2, y2, cls) in enumerate(boxes):
            det[0, r] = torch.tensor([x1, y1, x2, y2, 0.9 - 0.1 * r, cls])
        cnt = torch.tensor([len(boxes)], dtype=torch.int32)
        ops.track_update(det, cnt, self.ts, min_hits=1, max_age=self.max_age)
        self.mask, counts = ops.zone_update(det, cnt, self.ts, self.zs, self.zones)
        assert torch.equal(counts, self.zs.counters)
        z = self.zs
        assert torch.equal(z.zone_enter - z.zone_exit, z.zone_occ)
        return self

    def line(self, i):
        return int(self.zs.line_fwd[0, i]), int(self.zs.line_back[0, i])

    def zone(self, i):
        z = self.zs
        return {"enter": int(z.zone_enter[0, i]), "exit": int(z.zone_exit[0, i]),
                "occ": int(z.zone_occ[0, i]), "dwell": int(z.zone_dwell[0, i])}


def _box(cx, y2, cls=0.0, w=20.0, h=40.0):
    return (cx - w / 2, y2 - h, cx + w / 2, y2, cls)


# ---------------------------------------------------------------- lines
def test_walk_over_a_vertical_line_and_back():
    # A = (100, 0) -> B = (100, 200): side(P) = (px <= 100); left to right is forward
    sc = Scene()
    sc.zones.set_line(0, 0, (100, 0), (100, 200))
    for cx in (90, 95, 100, 105, 110):
        sc.step(_box(cx, 80))
    assert sc.line(0) == (1, 0)
    for cx in (105, 100, 95, 90):
        sc.step(_box(cx, 80))
    assert sc.line(0) == (1, 1)
    assert sc.ts.unique() == 1  # one track all along


def test_walk_past_the_end_of_the_segment_counts_nothing():
    sc = Scene()
    sc.zones.set_line(0, 0, (100, 0), (100, 200))
    for cx in (90, 95, 100, 105, 110, 105, 100, 95, 90):
        sc.step(_box(cx, 300))  # the anchor passes below B
    assert sc.line(0) == (0, 0) and sc.ts.unique() == 1


def test_move_that_ends_on_the_line_follows_the_half_open_rule():
    # the line's own points are on the side(P) = true side (px <= 100)
    left = Scene()
    left.zones.set_line(0, 0, (100, 0), (100, 200))
    for cx in (96, 100, 96):  # true -> true -> true: never left its side
        left.step(_box(cx, 80))
    assert left.line(0) == (0, 0) and left.ts.unique() == 1
    right = Scene()
    right.zones.set_line(0, 0, (100, 0), (100, 200))
    right.step(_box(104, 80)).step(_box(100, 80))  # false -> true: backward, on arrival
    assert right.line(0) == (0, 1)
    right.step(_box(104, 80))                      # true -> false: forward, on leaving
    assert right.line(0) == (1, 1) and right.ts.unique() == 1


def test_path_through_a_shared_vertex_counts_on_exactly_one_line():
    # (0, 100) -> (100, 100) -> (200, 100); the anchor moves down x = 100 through the vertex.
    # side(P) = (py >= 100) on both; sp(X) = (Xx <= 100): line 0 has sp(A) == sp(B) (both
    # true), line 1 has sp(A) true, sp(B) false.  side goes false -> true: backward on line 1
    for ys in ((90, 110), (90, 100, 110), (95, 100), (100, 105)):
        sc = Scene()
        sc.zones.set_line(0, 0, (0, 100), (100, 100)).set_line(0, 1, (100, 100), (200, 100))
        for y2 in ys:
            sc.step(_box(100, y2, w=40.0))
        want = (0, 1) if ys[0] < 100 else (0, 0)  # starting on the line: already on its side
        assert sc.line(0) == (0, 0) and sc.line(1) == want, ys
        assert sc.ts.unique() == 1


def test_degenerate_line_never_counts():
    sc = Scene()
    sc.zones.set_line(0, 0, (100, 80), (100, 80))
    for cx in (90, 95, 100, 105, 110, 105, 100, 95, 90):
        sc.step(_box(cx, 80))  # straight through the point, stopping on it
    assert sc.line(0) == (0, 0)
    assert int(sc.zones.n_lines[0]) == 1


def test_class_filtered_line_ignores_the_other_class():
    sc = Scene()
    sc.zones.set_line(0, 0, (100, 0), (100, 400), cls=1).set_line(0, 1, (100, 0), (100, 400))
    for cx in (90, 100, 110):
        sc.step(_box(cx, 80, cls=0.0), _box(cx, 300, cls=1.0))
    assert sc.line(0) == (1, 0)  # the class-1 box only
    assert sc.line(1) == (2, 0)


# ---------------------------------------------------------------- zones
L_SHAPE = [(0, 0), (200, 0), (200, 100), (100, 100), (100, 200), (0, 200)]


def test_concave_zone_anchor_in_the_notch_is_outside():
    sc = Scene()
    sc.zones.set_zone(0, 0, L_SHAPE)
    sc.step(_box(150, 150), _box(50, 150), _box(150, 50))
    assert sc.mask[0].tolist() == [0, 1, 1, 0]
    assert sc.zone(0) == {"enter": 2, "exit": 0, "occ": 2, "dwell": 2}


def test_bottom_and_centre_anchors_disagree_for_a_tall_box():
    tall = (40.0, 50.0, 60.0, 150.0, 0.0)  # centre (50, 100), bottom-centre (50, 150)
    got = {}
    for anchor in ("bottom", "centre"):
        sc = Scene(anchor=anchor)
        sc.zones.set_zone(0, 0, [(0, 0), (100, 0), (100, 120), (0, 120)])
        sc.step(tall)
        got[anchor] = (sc.mask[0, 0].item(), sc.zone(0)["occ"], sc.zs.anchor[0, 0].tolist())
    assert got == {"bottom": (0, 0, [200, 600]), "centre": (1, 1, [200, 400])}


def test_track_lost_inside_a_zone_occupies_it_until_max_age_passes():
    sc = Scene(max_age=2)
    sc.zones.set_zone(0, 0, [(0, 0), (200, 0), (200, 200), (0, 200)])
    sc.step(_box(100, 100))
    assert sc.zone(0) == {"enter": 1, "exit": 0, "occ": 1, "dwell": 1}
    sc.step().step()  # coasting: age 1, 2
    assert sc.zone(0) == {"enter": 1, "exit": 0, "occ": 1, "dwell": 3}
    sc.step()         # age 3 > max_age: the track is dropped
    assert sc.zone(0) == {"enter": 1, "exit": 1, "occ": 0, "dwell": 3}
    assert int(sc.zs.seen_id[0, 0]) == -1 and sc.zs.entry[0, 0].tolist() == [-1, 0, 0, 0]


def test_slot_reused_in_the_same_step_exits_the_old_track_and_enters_the_new():
    sc = Scene(max_age=0)
    sc.zones.set_zone(0, 0, [(0, 0), (200, 0), (200, 200), (0, 200)])
    sc.zones.set_zone(0, 1, [(400, 0), (600, 0), (600, 200), (400, 200)])
    sc.zones.set_line(0, 0, (300, 0), (300, 400))  # between the two: not a move of one track
    sc.step(_box(100, 100))
    assert int(sc.ts.id[0, 0]) == 0 and sc.zone(0)["occ"] == 1
    sc.step(_box(500, 100))  # id 0 is dropped at once, id 1 is born into slot 0
    assert int(sc.ts.id[0, 0]) == 1 and int(sc.zs.seen_id[0, 0]) == 1
    assert sc.zone(0) == {"enter": 1, "exit": 1, "occ": 0, "dwell": 1}
    assert sc.zone(1) == {"enter": 1, "exit": 0, "occ": 1, "dwell": 1}
    assert sc.line(0) == (0, 0)


def test_class_filtered_zone_and_unconfirmed_rows():
    # zone_mask is per row, track or not; the counters follow confirmed tracks only
    ts, zs, zones = ops.TrackState(1, 64), ops.ZoneState(1, 64), ops.ZoneSet(1)
    zones.set_zone(None, 0, [(0, 0), (200, 0), (200, 200), (0, 200)], cls=1)
    zones.set_zone(None, 3, [(0, 0), (200, 0), (200, 200), (0, 200)])
    assert int(zones.n_zones[0]) == 4  # zones 1 and 2 are empty
    det = torch.zeros(1, 3, 6)
    det[0, 0] = torch.tensor([40.0, 40.0, 60.0, 80.0, 0.9, 1.0])
    det[0, 1] = torch.tensor([140.0, 40.0, 160.0, 80.0, 0.8, 0.0])
    cnt = torch.tensor([2], dtype=torch.int32)
    ops.track_update(det, cnt, ts, min_hits=3)  # no track is confirmed yet
    mask, counts = ops.zone_update(det, cnt, ts, zs, zones)
    assert mask[0].tolist() == [0b1001, 0b1000, 0] and int(counts.abs().sum()) == 0


# ---------------------------------------------------------------- point in polygon
def _pip_rule(px, py, poly):
    """The written rule, literally, on Python ints."""
    inside = False
    for i in range(len(poly)):
        (xi, yi), (xj, yj) = poly[i], poly[i - 1]
        if (yi > py) != (yj > py):
            t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi)
            if (t > 0) if yj - yi > 0 else (t < 0):
                inside = not inside
    return inside


def _pip_fraction(px, py, poly):
    """Independent: (on_edge, inside) with exact rationals -- a ray to +x crosses an edge that
    straddles py where the edge's x at py lies beyond px."""
    on_edge, inside = False, False
    for i in range(len(poly)):
        (xi, yi), (xj, yj) = poly[i], poly[i - 1]
        if ((xj - xi) * (py - yi) == (yj - yi) * (px - xi) and min(xi, xj) <= px <= max(xi, xj)
                and min(yi, yj) <= py <= max(yi, yj)):
            on_edge = True
        if (yi > py) != (yj > py):
            x_at = Fraction(xi) + Fraction(py - yi, yj - yi) * (xj - xi)
            if x_at > px:
                inside = not inside
    return on_edge, inside


def _polygons(rng, n):
    import math

    out = []
    for k in range(n):
        nv = rng.randint(3, 8)
        kind = k % 3
        if kind == 0:    # convex: points of a circle in angular order
            ang = sorted(rng.uniform(0, 2 * math.pi) for _ in range(nv))
            poly = [(int(24 + 20 * math.cos(a)), int(24 + 20 * math.sin(a))) for a in ang]
        elif kind == 1:  # any vertex order: concave or self-crossing, even-odd all the same
            poly = [(rng.randint(0, 48), rng.randint(0, 48)) for _ in range(nv)]
        else:            # rectilinear staircase: axis-aligned edges, concave from 6 vertices
            xs = sorted(rng.sample(range(0, 48, 2), 3))
            ys = sorted(rng.sample(range(0, 48, 2), 3))
            poly = [(xs[0], ys[0]), (xs[2], ys[0]), (xs[2], ys[1]), (xs[1], ys[1]),
                    (xs[1], ys[2]), (xs[0], ys[2])]
        out.append(poly)
    return out


def test_point_in_polygon_against_fractions():
    rng = random.Random(5)
    total = on_edges = differ = 0
    for poly in _polygons(rng, 240):
        pts = [(rng.randint(-2, 50), rng.randint(-2, 50)) for _ in range(16)]
        pts += poly
        for i in range(len(poly)):
            (xi, yi), (xj, yj) = poly[i], poly[i - 1]
            if (xi == xj or yi == yj) and (xi + xj) % 2 == 0 and (yi + yj) % 2 == 0:
                pts.append(((xi + xj) // 2, (yi + yj) // 2))
        px = torch.tensor([p[0] for p in pts], dtype=torch.int64)
        py = torch.tensor([p[1] for p in pts], dtype=torch.int64)
        got = reference.point_in_polygon(px, py, poly).tolist()
        for (x, y), g in zip(pts, got):
            edge, inside = _pip_fraction(x, y, poly)
            assert g == _pip_rule(x, y, poly), (poly, x, y)
            if edge:
                on_edges += 1
                differ += g != inside
            else:
                assert g == inside, (poly, x, y)
            total += 1
    assert total > 4000 and on_edges > 1000
    print(f"{total} points, {on_edges} on an edge")


def test_zone_mask_uses_the_clamped_table():
    # what the kernel does with a table no ZoneSet would build
    ts, zs, zones = ops.TrackState(1, 64), ops.ZoneState(1, 64), zw.regions()
    det, cnt = zw.inputs(0)
    det, cnt = det[zw.SLOT0:zw.SLOT0 + 1].contiguous(), cnt[zw.SLOT0:zw.SLOT0 + 1].contiguous()
    one = ops.ZoneSet(1)
    one.table.copy_(zones.table[zw.SLOT0:zw.SLOT0 + 1])
    ops.track_update(det, cnt, ts, **zw.TRACK_KW)
    want, _ = ops.zone_update(det, cnt, ts, zs, one)
    assert int(want.max()) > 0
    one.n_lines[0], one.n_zones[0] = 99, 99      # clamped to 8: nothing changes
    one.n_vertex[0, 0] = 100                      # clamped to 8: 4 more vertices at (0, 0)
    got, _ = ops.zone_update(det, cnt, ts, ops.ZoneState(1, 64), one)
    assert torch.equal(got & ~1, want & ~1)
    one.n_zones[0] = -1                           # clamped to 0
    got, _ = ops.zone_update(det, cnt, ts, ops.ZoneState(1, 64), one)
    assert int(got.abs().sum()) == 0


# ---------------------------------------------------------------- the walk
@pytest.mark.parametrize("anchor", ["bottom", "centre"])
def test_walk_invariants_and_floors(anchor):
    ts, zs, zones = ops.TrackState(zw.S, 64), ops.ZoneState(zw.S, 64), zw.regions("cpu", anchor)
    rows = slice(zw.SLOT0, zw.SLOT0 + zw.N)
    dwell = torch.zeros(zw.N, 8, dtype=torch.int32)
    for step in range(zw.STEPS):
        det, cnt = zw.inputs(step)
        before = ts.buf.clone()
        ops.track_update(det[rows], cnt[rows], ts, slot0=zw.SLOT0, **zw.TRACK_KW)
        after = ts.buf.clone()
        mask, counts = ops.zone_update(det[rows], cnt[rows], ts, zs, zones, slot0=zw.SLOT0)
        assert torch.equal(ts.buf, after) and not torch.equal(before, after)  # read only
        assert torch.equal(zs.zone_enter - zs.zone_exit, zs.zone_occ), step
        dwell += zs.zone_occ[rows]
        assert torch.equal(zs.zone_dwell[rows], dwell), step
        assert torch.equal(counts, zs.counters[rows])
        c = cnt[rows].clamp(0, zw.MAX_DET)
        for n in range(zw.N):
            assert (mask[n, int(c[n]):] == 0).all()
    # cameras that were not stepped are untouched
    fresh = ops.ZoneState(zw.S, 64)
    assert torch.equal(zs.buf[0], fresh.buf[0]) and torch.equal(zs.buf[-1], fresh.buf[-1])
    assert int(zs.line_fwd[rows, 4].sum() + zs.line_back[rows, 4].sum()) == 0  # A == B
    assert int(zs.zone_enter[rows, 6].sum()) == 0                             # collinear
    print(anchor, zw.assert_busy(zs))


def test_state_views_reset_and_wrapper_rejections():
    zs = ops.ZoneState(2, 128)
    assert zs.buf.shape == (2, 4 * 128 + 48) and zs.entry.shape == (2, 128, 4)
    assert zs.anchor.shape == (2, 128, 2) and zs.counters.shape == (2, 48)
    zs.buf.fill_(7)
    assert int(zs.zone_dwell[1, 7]) == 7 and int(zs.seen_id[0, 0]) == 7
    zs.reset()
    assert (zs.seen_id == -1).all() and int(zs.buf.sum()) == -2 * 128
    zones = ops.ZoneSet(2)
    assert zones.table.shape == (2, ops.ZONE_TABLE_STRIDE)
    zones.set_line(1, 2, (1.0, 2.0), (3.25, 4.5), cls=7)
    assert zones.line[1, 2].tolist() == [4, 8, 13, 18] and zones.line_cls[1, 2] == 7
    assert zones.n_lines.tolist() == [0, 3] and (zones.line_cls[0] == -1).all()
    for bad in (lambda: zones.set_line(0, 8, (0, 0), (1, 1)),
                lambda: zones.set_line(0, -1, (0, 0), (1, 1)),
                lambda: zones.set_line(2, 0, (0, 0), (1, 1)),
                lambda: zones.set_zone(0, 8, [(0, 0), (1, 0), (1, 1)]),
                lambda: zones.set_zone(0, 0, [(0, 0), (1, 0)]),
                lambda: zones.set_zone(0, 0, [(i, i * i) for i in range(9)]),
                lambda: zones.set_anchor("top"),
                lambda: ops.ZoneState(2, 96), lambda: ops.ZoneSet(0)):
        with pytest.raises(ValueError):
            bad()
    zones.set_anchor("centre").clear()
    assert zones.anchor.tolist() == [1, 1] and int(zones.n_lines.sum()) == 0
    ts = ops.TrackState(2, 128)
    det, cnt = torch.zeros(2, 4, 6), torch.zeros(2, dtype=torch.int32)
    ops.zone_update(det, cnt, ts, zs, zones)
    for args in ((det.double(), cnt, ts, zs, zones), (det, cnt.long(), ts, zs, zones),
                 (det, cnt, ts, ops.ZoneState(2, 64), zones),
                 (det, cnt, ts, zs, ops.ZoneSet(3)),
                 (torch.zeros(2, 301, 6), cnt, ts, zs, zones)):
        with pytest.raises(ValueError):
            ops.zone_update(*args)
    with pytest.raises(ValueError):
        ops.zone_update(det, cnt, ts, zs, zones, slot0=1)
    with pytest.raises(ValueError):
        ops.zone_update(det, cnt, ts, zs, zones, out_mask=torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.zone_update(det, cnt, ts.buf, zs, zones)


# ---------------------------------------------------------------- host totals over a wrap
def test_host_totals_stay_exact_over_a_wrapping_counter():
    from kvedge_amd.module.zones import ZoneTotals

    class Model:
        resets = 0

    m = Model()
    m.zone_state = ops.ZoneState(1, 64)
    ts, zones = ops.TrackState(1, 64), ops.ZoneSet(1)
    zones.set_zone(0, 0, [(0, 0), (200, 0), (200, 200), (0, 200)])
    zones.set_line(0, 0, (100, 0), (100, 200))
    top = 2 ** 31 - 1
    for group in (m.zone_state.zone_enter, m.zone_state.zone_dwell, m.zone_state.line_fwd):
        group[0, 0] = top  # counters that have been running for a long time
    m.zone_state.zone_exit[0, 0] = top  # (enter - exit == occ holds)
    tot = ZoneTotals(m, [{"name": "door"}], [{"name": "bay"}])
    det = torch.zeros(1, 4, 6)
    cnt = torch.tensor([1], dtype=torch.int32)
    for cx in (90.0, 96.0, 104.0, 110.0):
        det[0, 0] = torch.tensor([cx - 10, 40.0, cx + 10, 80.0, 0.9, 0.0])
        ops.track_update(det, cnt, ts, min_hits=1)
        ops.zone_update(det, cnt, ts, m.zone_state, zones)
        tot.update()
    assert int(m.zone_state.zone_enter[0, 0]) == -2 ** 31           # wrapped on the device
    assert int(m.zone_state.zone_dwell[0, 0]) == -2 ** 31 + 3
    assert int(m.zone_state.line_fwd[0, 0]) == -2 ** 31
    assert tot.summed() == {"lines": {"door": {"forward": 1, "backward": 0}},
                            "zones": {"bay": {"occupancy": 1, "entered": 1, "exited": 0,
                                              "dwell_frames": 4}}}
    m.zone_state.reset()  # a model reset starts the totals over
    m.resets += 1
    assert tot.update().summed()["zones"]["bay"] == {"occupancy": 0, "entered": 0, "exited": 0,
                                                     "dwell_frames": 0}


# ---------------------------------------------------------------- twin keys
SQUARE = [[0, 0], [64, 0], [64, 64], [0, 64]]


def test_config_zone_keys():
    d = ModuleConfig().validate()
    assert (d.lines, d.zones, d.zone_anchor) == ((), (), "bottom")
    base = {"model": "yolov8n", "track": True}
    tracked = d.apply_patch(base)
    assert not {"lines", "zones", "zone_anchor"} & set(tracked.to_dict())
    assert not {"lines", "zones", "zone_anchor"} & set(d.to_dict())
    line = {"name": "door", "a": [10, 0], "b": [10, 64]}
    c = d.apply_patch(dict(base, lines=[line], zones=[{"name": "bay", "polygon": SQUARE,
                                                       "class": 2, "cameras": [0]}]))
    rep = c.to_dict()
    assert rep["zone_anchor"] == "bottom" and rep["lines"][0]["name"] == "door"
    assert rep["lines"][0]["class"] == -1 and rep["lines"][0]["cameras"] is None
    assert rep["zones"][0]["class"] == 2 and rep["zones"][0]["polygon"][2] == [64.0, 64.0]
    import json

    assert d.apply_patch(json.loads(json.dumps(dict(rep, lines=json.dumps([line]))))) == c
    for k, v in (("lines", []), ("zones", []), ("zone_anchor", "centre")):
        assert k in ModuleConfig.REBUILD and c.needs_rebuild(c.apply_patch({k: v}))
    assert "zone_anchor" in d.apply_patch(dict(base, zone_anchor="centre")).to_dict()
    poly = lambda n: [[i, i * i] for i in range(n)]  # noqa: E731
    for bad in (dict(base, lines=[dict(line, name=f"l{i}") for i in range(9)]),
                dict(base, zones=[{"name": f"z{i}", "polygon": SQUARE} for i in range(9)]),
                dict(base, zones=[{"name": "z", "polygon": poly(2)}]),
                dict(base, zones=[{"name": "z", "polygon": poly(9)}]),
                dict(base, lines=[line, line]),
                dict(base, zones=[{"name": "z", "polygon": SQUARE}] * 2),
                {"model": "yolov8n", "zones": [{"name": "z", "polygon": SQUARE}]},  # no track
                {"model": "yolov8n", "lines": [line]},
                dict(base, zone_anchor="top"),
                dict(base, lines=[{"a": [0, 0], "b": [1, 1]}]),                    # no name
                dict(base, lines=[dict(line, a=[1, 2, 3])]),
                dict(base, lines=[dict(line, cameras=[64])]),
                dict(base, zones=[{"name": "z", "polygon": SQUARE, "colour": "red"}]),
                dict(base, lines="not json")):
        with pytest.raises(ValueError):
            d.apply_patch(bad)
    assert d.apply_patch(dict(base, zones=[{"name": "z", "polygon": poly(3)},
                                           {"name": "y", "polygon": poly(8)}]))


def test_module_cli_has_zone_flags():
    import inspect

    from kvedge_amd.module import __main__ as cli

    src = inspect.getsource(cli.main)
    for flag in ("--lines-json", "--zones-json", "--zone-anchor"):
        assert f'"{flag}"' in src


# ---------------------------------------------------------------- model / engine / module
class Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def test_engine_cpu_zoned():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.tracking import KvTracked, KvZoned
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    yolo = KvYoloV8n(init_yolov8n(seed=0, calibrate=False), "cpu", conf=0.0, max_det=8)
    zones = ops.ZoneSet(2)
    zones.set_zone(None, 0, [(0, 0), (64, 0), (64, 48), (0, 48)])
    zones.set_line(None, 0, (32, 0), (32, 48))
    tracked = KvTracked(yolo, 2, iou=0.3, max_age=3, min_hits=1)
    m = KvZoned(tracked, zones, anchor="centre")
    assert m.stateful and m.convs() == yolo.convs() and m.state is tracked.state
    assert m.flops_per_image(64) == yolo.flops_per_image(64)
    assert m.frame_plan((48, 64), 64) == yolo.frame_plan((48, 64), 64)
    assert zones.anchor.tolist() == [1, 1]
    eng = InferenceEngine(m, 2, 64, device="cpu", seed=3, frame_hw=(48, 64)).prepare(warmup=2)
    assert torch.equal(m.zone_state.buf, ops.ZoneState(2, 64).buf)  # left freshly reset
    assert torch.equal(m.state.buf, ops.TrackState(2, 64).buf)
    want_t, want_z = ops.TrackState(2, 64), ops.ZoneState(2, 64)
    for step in range(3):
        out = eng.run()
        assert len(out) == 5
        det, count, tid, mask, counts = out
        ref = torch.empty_like(tid)
        reference.track_update(det, count, want_t, 0, 307, 3, 1, True, ref)
        rm, rc = torch.empty_like(mask), torch.empty_like(counts)
        reference.zone_update(det, count, want_t, want_z, zones, 0, rm, rc)
        assert torch.equal(tid, ref) and torch.equal(mask, rm) and torch.equal(counts, rc)
        assert torch.equal(m.zone_state.buf, want_z.buf)
    assert int(want_z.zone_enter.sum()) >= 1
    eng.reset_tracks()
    assert torch.equal(m.zone_state.buf, ops.ZoneState(2, 64).buf) and m.state.active() == 0
    with pytest.raises(TypeError):
        KvZoned(yolo, zones)
    with pytest.raises(ValueError):
        KvZoned(tracked, ops.ZoneSet(3))


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
                dict(tr.reported["config"]), app.on_method("zones", {}))


def test_module_cpu_zones_on_and_off():
    off, out_off, model_off, cfg_off, method_off = _module({})
    on, out_on, model_on, cfg_on, method_on = _module(
        {"zones": [{"name": "frame", "polygon": SQUARE},
                   {"name": "cam1", "polygon": SQUARE, "cameras": [1]}],
         "lines": [{"name": "mid", "a": [32, 0], "b": [32, 64]}], "zone_anchor": "centre"})
    assert not {"lines", "zones", "zone_anchor"} & set(cfg_off) and len(out_off) == 3
    assert not hasattr(model_off, "zone_state") and method_off[0] == 400
    assert set(on) == set(off) | {"lines", "zones"}  # nothing else changes
    assert on["tracks"] == off["tracks"] and on["detections"] == off["detections"]
    for a, b in zip(out_on, out_off):
        assert torch.equal(a, b)
    assert cfg_on["zone_anchor"] == "centre" and cfg_on["zones"][1]["cameras"] == [1]
    assert len(out_on) == 5 and out_on[3].shape == (2, 8) and out_on[4].shape == (2, 48)
    zs = model_on.zone_state
    assert torch.equal(out_on[4], zs.counters)
    assert on["lines"] == {"mid": {"forward": int(zs.line_fwd[:, 0].sum()),
                                   "backward": int(zs.line_back[:, 0].sum())}}
    for i, name in enumerate(("frame", "cam1")):
        assert on["zones"][name] == {
            "occupancy": int(zs.zone_occ[:, i].sum()), "entered": int(zs.zone_enter[:, i].sum()),
            "exited": int(zs.zone_exit[:, i].sum()),
            "dwell_frames": int(zs.zone_dwell[:, i].sum())}
    assert on["zones"]["frame"]["entered"] >= 1
    assert int(zs.zone_enter[0, 1]) == 0 and on["zones"]["cam1"]["entered"] >= 1
    status, body = method_on
    assert status == 200 and len(body["cameras"]) == 2
    assert body["cameras"][1]["zones"]["cam1"]["entered"] == int(zs.zone_enter[1, 1])
    assert body["cameras"][0]["zones"]["cam1"]["entered"] == 0


# ---------------------------------------------------------------- build
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_zones_kernel_cross_compiles_without_warnings(tmp_path):
    from kvedge_amd import _build

    src = os.path.join(ROOT, "csrc", "kernels", "zones.hip")
    assert src in _build.glob.glob(os.path.join(_build.CSRC, "kernels", "*.hip"))
    r = subprocess.run([_build.hipcc(), *_build.COMMON, "-Wall", "-Wextra", "-Werror",
                        f"-I{_build.CSRC}/kernels", "-c", src, "-o", str(tmp_path / "zones.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and not (r.stdout + r.stderr).strip(), r.stderr[-2000:]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_zones_kernel_does_not_spill():
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"),
                        os.path.join(ROOT, "csrc", "kernels", "zones.hip"), "--no-spill"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    rows = [l for l in r.stdout.splitlines() if l.startswith("| zones.hip")]
    assert len(rows) == 4, rows  # T = 64, 128, 192, 256
