"""Snapshot annotation on the CPU: ops.reference.annotate judged on its own -- against Pillow
for outlines, against exact box coverage and an independent block mean for privacy, against a
label renderer written out in annotate_cases -- then the argument checks and the module."""
import base64

import numpy as np
import pytest
import torch

import annotate_cases as ac
from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference as ref


def test_everything_off_is_the_identity():
    img = ac.picture(2, 12, 20, seed=1)
    det, count = ac.dets([[(1, 1, 9, 9, 0)], [(2, 2, 15, 10, 1)]])
    tid = torch.tensor([[5], [6]], dtype=torch.int32)
    off = ac.style_of(2)
    out = ops.annotate(img.clone(), off, det, count, tid)
    assert torch.equal(out, img)
    assert torch.equal(ops.annotate(img.clone(), off), img)
    on = ac.style_of(2, boxes=True, labels="both", classes=[0, 1])
    for c in (0, -3):
        cnt = torch.full((2,), c, dtype=torch.int32)
        assert torch.equal(ops.annotate(img.clone(), on, det, cnt, tid), img)
    assert not torch.equal(ops.annotate(img.clone(), on, det, count, tid), img)
    x = img.clone()
    assert ops.annotate(x, on, det, count, tid) is x        # in place


@pytest.mark.parametrize("t", [1, 2, 3])
def test_outlines_equal_pillow(t):
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    from PIL import Image

    h, w = 36, 68
    # integer thumbnail pixels, both sides >= 2 t
    boxes = [(3, 2, 30, 20), (0, 0, w, h), (10, 5, 10 + 2 * t, 5 + 2 * t), (60, 28, 68, 36),
             (5, 30, 40, 30 + 2 * t)]
    style = ac.style_of(len(boxes), boxes=True, thickness=t)
    det, count = ac.dets([[(*b, 3)] for b in boxes])
    out = ops.annotate(torch.zeros(len(boxes), h, w, 3, dtype=torch.uint8), style, det, count)
    rgb = ac.colour(style, 3)
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        im = Image.new("RGB", (w, h))
        ImageDraw.Draw(im).rectangle([x0, y0, x1 - 1, y1 - 1], outline=rgb, width=t)
        assert np.array_equal(out[i].numpy(), np.asarray(im)), (i, t)


@pytest.mark.parametrize("blk", [4, 8, 16])
def test_privacy_hides_every_pixel_a_hidden_box_meets(blk):
    h, w, src = 36, 68, (90, 160)
    img = ac.picture(2, h, w, seed=2)
    det, count, tid = ac.noisy_case(2, h, w, 12, src, seed=3)
    style = ac.style_of(2, classes=[1, 3], block=blk)
    out = ops.annotate(img.clone(), style, det, count, tid, src_hw=src).numpy()
    for n in range(2):
        means = ac.block_means(img[n].numpy(), blk)
        hidden = np.zeros((h, w), bool)
        for r in range(int(count[n])):
            if int(ref.track_class(det[n, r, 5])) in (1, 3):
                hidden |= ac.covered(det[n, r], src, (h, w))
        assert hidden.any() and not hidden.all()
        blocks = np.zeros((h, w), bool)
        for y, x in zip(*np.nonzero(hidden)):
            blocks[y // blk * blk:y // blk * blk + blk, x // blk * blk:x // blk * blk + blk] = True
        assert np.array_equal(out[n][blocks], means[blocks])
        # each output pixel is the block mean or the picture, nothing else
        same = (out[n] == img[n].numpy()).all(-1) | (out[n] == means).all(-1)
        assert same.all()


def test_privacy_is_blind_inside_a_block_and_covers_rows_past_max_draw():
    h, w, blk = 16, 16, 8
    img = ac.picture(1, h, w, seed=4)
    det, count = ac.dets([[(1, 1, 3, 3, 0), (2, 2, 3, 3, 0), (9, 9, 12, 12, 7)]])
    style = ac.style_of(1, classes=[7], block=blk, boxes=True, max_draw=1)
    out = ops.annotate(img.clone(), style, det, count)
    want = ac.block_means(img[0].numpy(), blk)[8:, 8:]
    assert np.array_equal(out[0, 8:, 8:].numpy(), want)           # row 2 >= max_draw: hidden
    assert torch.equal(out[0, 8:, :8], img[0, 8:, :8])
    assert tuple(out[0, 1, 1].tolist()) == ac.colour(style, 0)    # row 0 drawn ...
    assert torch.equal(out[0, 4:8, 4:8], img[0, 4:8, 4:8])        # ... row 1 not (max_draw)
    # permuting the input inside the pixelated block changes nothing
    perm = img.clone()
    cell = perm[0, 8:, 8:].reshape(-1, 3)
    perm[0, 8:, 8:] = cell[torch.randperm(64, generator=torch.Generator().manual_seed(5))].view(
        8, 8, 3)
    assert not torch.equal(perm, img)
    assert torch.equal(ops.annotate(perm, style, det, count)[0, 8:, 8:], out[0, 8:, 8:])


def test_a_polygon_edge_through_pixel_centres_is_half_open():
    h = w = 16
    img = ac.picture(1, h, w, seed=6)
    # centres of pixels 4 and 8 lie on the edges: 4.5 is inside, 8.5 is not
    poly = [(4.5, 4.5), (8.5, 4.5), (8.5, 8.5), (4.5, 8.5)]
    qx, qy = torch.tensor([[18, 34], [18, 34]]), torch.tensor([[18, 18], [34, 34]])
    inside = ref.point_in_polygon(qx, qy, [(18, 18), (34, 18), (34, 34), (18, 34)])
    assert inside.tolist() == [[True, False], [False, False]]
    out = ops.annotate(img.clone(), ac.style_of(1, polygons=[poly], block=4), src_hw=(h, w))
    want = img[0].numpy().copy()
    want[4:8, 4:8] = ac.block_means(img[0].numpy(), 4)[4:8, 4:8]
    assert np.array_equal(out[0].numpy(), want)
    # the same polygon given in a frame twice the size
    big = [(2 * x, 2 * y) for x, y in poly]
    out2 = ops.annotate(img.clone(), ac.style_of(1, polygons=[big], block=4), src_hw=(32, 32))
    assert np.array_equal(out2[0].numpy(), want)


def test_layers_labels_over_outlines_over_mosaic_lowest_row_on_top():
    h, w = 32, 48
    img = ac.picture(1, h, w, seed=7)
    # row 1 starts on row 0's outline; both are hidden classes
    det, count = ac.dets([[(4, 4, 30, 24, 2), (4, 14, 40, 30, 5)]])
    tid = torch.tensor([[7, 12345]], dtype=torch.int32)
    style = ac.style_of(1, boxes=True, labels="both", classes=[2, 5], block=4, thickness=2)
    out = ops.annotate(img.clone(), style, det, count, tid)[0].numpy()
    c0, c1 = ac.colour(style, 2), ac.colour(style, 5)
    assert np.array_equal(out[4:13, 4:4 + 19], ac.render_label("2:7", c0, 1))
    assert np.array_equal(out[14:23, 4:4 + 43], ac.render_label("5:12345", c1, 1))  # over row 0
    assert tuple(out[24, 4]) == c1 and tuple(out[23, 5]) == c0   # outlines: row 0 wins
    assert tuple(out[23, 29]) == c0 and tuple(out[29, 39]) == c1
    assert tuple(out[15, 47]) == tuple(img[0, 15, 47].tolist())   # outside both
    means = ac.block_means(img[0].numpy(), 4)
    assert np.array_equal(out[6:13, 24:28], means[6:13, 24:28])   # inside row 0, under neither
    assert np.array_equal(out[24:28, 8:28], means[24:28, 8:28])


@pytest.mark.parametrize("tid,mode,text", [(7, "both", "9:7"), (12345, "both", "9:12345"),
                                           (100003, "both", "9:3"), (-1, "both", "9"),
                                           (-1, "id", ""), (100003, "id", "3"),
                                           (42, "class", "9"), (2147483647, "id", "83647")])
def test_label_text(tid, mode, text):
    assert ref.annotate_text(ops.ANNOTATE_LABELS[mode], 9, tid) == text
    img = ac.picture(1, 20, 80, seed=8)
    det, count = ac.dets([[(2, 3, 70, 18, 9)]])
    for s in (1, 2):
        style = ac.style_of(1, labels=mode, scale=s)
        out = ops.annotate(img.clone(), style, det, count,
                           torch.tensor([[tid]], dtype=torch.int32))[0].numpy()
        want = img[0].numpy().copy()
        if text:
            lab = ac.render_label(text, ac.colour(style, 9), s)[:20 - 3, :80 - 2]
            want[3:3 + lab.shape[0], 2:2 + lab.shape[1]] = lab
        assert np.array_equal(out, want), (s, text)


def test_a_label_is_clipped_at_the_right_and_bottom_edge():
    img = ac.picture(1, 12, 20, seed=9)
    det, count = ac.dets([[(14, 8, 20, 12, 4)]])
    style = ac.style_of(1, labels="both", scale=2)
    out = ops.annotate(img.clone(), style, det, count, torch.tensor([[88]], dtype=torch.int32))
    lab = ac.render_label("4:88", ac.colour(style, 4), 2)
    want = img[0].numpy().copy()
    want[8:, 14:] = lab[:4, :6]
    assert np.array_equal(out[0].numpy(), want)


def test_glyph_colour_flips_at_luma_128():
    pal = [(127, 127, 127), (128, 128, 128)] + [(0, 0, 0)] * 14
    style = ac.style_of(1, labels="class", palette=pal)
    det, count = ac.dets([[(0, 0, 8, 12, 0), (8, 0, 16, 12, 1)]])
    out = ops.annotate(torch.zeros(1, 12, 16, 3, dtype=torch.uint8), style, det, count)[0].numpy()
    assert np.array_equal(out[0:9, 0:7], ac.render_label("0", pal[0], 1))
    assert np.array_equal(out[0:9, 8:15], ac.render_label("1", pal[1], 1))
    assert {tuple(p) for p in out[0:9, 0:7].reshape(-1, 3)} == {pal[0], (255, 255, 255)}
    assert {tuple(p) for p in out[0:9, 8:15].reshape(-1, 3)} == {pal[1], (0, 0, 0)}


def test_colour_by_track_and_slot0():
    style = ops.AnnotateStyle(3).set_labels("none").set_colour_by("track", camera=2)
    det, count = ac.dets([[(0, 0, 4, 4, 3)], [(0, 0, 4, 4, 3)]])
    tid = torch.tensor([[21], [-1]], dtype=torch.int32)
    zeros = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    a = ops.annotate(zeros.clone(), style, det[:1], count[:1], tid[:1], slot0=2)
    assert tuple(a[0, 0, 0].tolist()) == ac.colour(style, 21)
    b = ops.annotate(zeros.clone(), style, det[1:], count[1:], tid[1:], slot0=2)
    assert tuple(b[0, 0, 0].tolist()) == ac.colour(style, 3)     # no id yet: the class
    c = ops.annotate(zeros.clone(), style, det[:1], count[:1], tid[:1], slot0=1)
    assert tuple(c[0, 0, 0].tolist()) == ac.colour(style, 3)


def test_argument_checks():
    img = ac.picture(2, 8, 12)
    det, count = ac.dets([[(0, 0, 4, 4, 0)], [(0, 0, 4, 4, 0)]])
    tid = torch.zeros(2, 1, dtype=torch.int32)
    style = ops.AnnotateStyle(2)
    ops.annotate(img.clone(), style, det, count, tid)
    with pytest.raises(TypeError):
        ops.annotate(img.clone(), ops.ZoneSet(2), det, count)
    bad = [dict(images=img.float()), dict(images=img[..., :2]), dict(images=img[:, :, :10]),
           dict(images=img.permute(0, 2, 1, 3)), dict(images=ac.picture(2, 8, 10)),
           dict(det=det.double()), dict(det=det[..., :5]), dict(det=det[:1]),
           dict(det=torch.zeros(2, 301, 6)), dict(det=torch.zeros(2, 0, 6)),
           dict(count=count.long()), dict(count=count[:1]), dict(count=None),
           dict(track_id=tid.long()), dict(track_id=torch.zeros(2, 2, dtype=torch.int32)),
           dict(det=None), dict(det=None, track_id=None),
           dict(slot0=-1), dict(slot0=1), dict(src_hw=(0, 4)), dict(src_hw=(4, 4097)),
           dict(images=img.to("meta"))]
    for kw in bad:
        args = dict(images=img.clone(), det=det, count=count, track_id=tid, slot0=0, src_hw=None)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            ops.annotate(args.pop("images"), style, **args)
    for call in (lambda: style.set_privacy_block(5), lambda: style.set_privacy_block(32),
                 lambda: style.set_thickness(0), lambda: style.set_thickness(5),
                 lambda: style.set_label_scale(0), lambda: style.set_label_scale(3),
                 lambda: style.set_privacy_polygon(0, [(0, 0), (1, 1)]),
                 lambda: style.set_privacy_polygon(0, [(i, i * i) for i in range(9)]),
                 lambda: style.set_privacy_polygon(8, [(0, 0), (1, 1), (0, 1)]),
                 lambda: style.set_privacy_classes(range(9)),
                 lambda: style.set_privacy_classes([-1]), lambda: style.set_labels("name"),
                 lambda: style.set_colour_by("size"), lambda: style.set_max_draw(301),
                 lambda: style.set_boxes(True, camera=2), lambda: style.set_palette([(0, 0, 0)]),
                 lambda: ops.AnnotateStyle(0)):
        with pytest.raises(ValueError):
            call()
    assert torch.equal(style.host, ops.AnnotateStyle(2).host)      # a rejected call wrote nothing


def test_the_table_is_clamped_where_it_is_read():
    img = ac.picture(1, 12, 20, seed=10)
    det, count = ac.dets([[(2, 2, 14, 10, 1)]])
    tid = torch.tensor([[3]], dtype=torch.int32)
    wild = ac.style_of(1, boxes=True, labels="both", classes=[1], polygons=[[(0, 0), (9, 0), (0, 9)]])
    tame = ac.style_of(1, boxes=True, labels="both", classes=[1], polygons=[[(0, 0), (9, 0), (0, 9)]],
                       thickness=4, scale=2, block=16, max_draw=300)
    for name, v in (("thickness", 99), ("scale", 99), ("block", 1 << 20), ("max_draw", 1 << 30)):
        getattr(wild, name).fill_(v)
    wild.n_polygons.fill_(77)
    wild.n_vertex[:, 1:].fill_(-5)
    a = ops.annotate(img.clone(), wild, det, count, tid)
    assert torch.equal(a, ops.annotate(img.clone(), tame, det, count, tid))
    wild.block.fill_(-3)
    wild.thickness.fill_(-3)
    tame.set_privacy_block(4).set_thickness(1)
    assert torch.equal(ops.annotate(img.clone(), wild, det, count, tid),
                       ops.annotate(img.clone(), tame, det, count, tid))


# ------------------------------------------------------------------ the module, CPU device
BASE = {"model": "yolov8n", "batch": 2, "report_interval_s": 1.0, "image_size": 64, "conf": 0.0,
        "max_det": 8, "track": True, "track_min_hits": 1, "track_max_age": 2, "snapshots": True,
        "snapshot_width": 32}


def test_config_annotate_keys():
    d = ModuleConfig().validate()
    assert not set(ModuleConfig.ANNOTATE_KEYS) & set(d.to_dict())   # reports what it reported
    c = d.apply_patch(dict(BASE, snapshot_annotate=True, snapshot_privacy_classes="0,2"))
    assert set(ModuleConfig.ANNOTATE_KEYS) <= set(c.to_dict())
    assert c.snapshot_privacy_classes == (0, 2) and c.needs_rebuild(d.apply_patch(BASE))
    zone = {"name": "door", "polygon": [[0, 0], [9, 0], [9, 9]], "cameras": [1]}
    for k, v in (("snapshot_boxes", False), ("snapshot_labels", "id"),
                 ("snapshot_box_thickness", 3), ("snapshot_label_scale", 2),
                 ("snapshot_privacy_classes", [1]), ("snapshot_privacy_block", 16),
                 ("snapshot_privacy_zones", [zone])):
        assert not c.needs_rebuild(c.apply_patch({k: v})), k
    assert c.apply_patch({"snapshot_privacy_zones": [zone]}).snapshot_privacy_zones[0][
        "polygon"] == [[0.0, 0.0], [9.0, 0.0], [9.0, 9.0]]
    for bad in ({"snapshot_labels": "name"}, {"snapshot_box_thickness": 0},
                {"snapshot_box_thickness": 5}, {"snapshot_label_scale": 3},
                {"snapshot_privacy_block": 5}, {"snapshot_privacy_classes": list(range(9))},
                {"snapshot_privacy_classes": [-1]}, {"snapshots": False},
                {"snapshot_privacy_zones": [dict(zone, polygon=[[0, 0], [1, 1]])]},
                {"snapshot_privacy_zones": [dict(zone, cameras=[2])]},
                {"snapshot_privacy_zones": [zone, zone]},
                {"snapshot_privacy_zones": [dict(zone, **{"class": 1})]},
                {"model": "resnet50", "track": False},               # class option, no boxes
                ):
        with pytest.raises(ValueError):
            c.apply_patch(bad)
    r = d.apply_patch({"model": "resnet50", "snapshots": True, "snapshot_annotate": True,
                       "snapshot_privacy_zones": [dict(zone, cameras=None)]})
    assert r.snapshot_annotate
    with pytest.raises(ValueError):
        r.apply_patch({"snapshot_labels": "id"})
    with pytest.raises(ValueError):
        d.apply_patch({"snapshot_annotate": True})                   # without snapshots


def test_module_cli_has_annotate_flags():
    import inspect

    from kvedge_amd.module import __main__ as cli

    src = inspect.getsource(cli.main)
    for flag in ("--snapshot-annotate", "--snapshot-labels", "--privacy-classes",
                 "--privacy-zones-json"):
        assert f'"{flag}"' in src


class _Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def _app(extra):
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport(dict(BASE, **extra))
    return tr, ModuleApp(tr, device="cpu", clock=_Clock()).start()


def _want(app, style_host):
    """The pictures of the last step from the engine's own outputs, through the reference."""
    stage = app.snapshots.stage
    out = app.engine.outputs
    small = ops.frame_resize(app.engine.frames, stage.plan)
    if style_host is not None:
        ref.annotate(small, style_host, torch.from_numpy(ref.annotate_font()), out[0], out[1],
                     out[stage._tracked.track_index], (64, 64), 0)
    return ref.jpeg_encode(small, "420", 75)


def test_module_annotates_and_a_privacy_patch_needs_no_rebuild():
    tr, app = _app({"snapshot_annotate": True, "snapshot_every_s": 0.1})
    with app:
        app.run(max_steps=2)
        stage = app.snapshots.stage
        assert stage.annotate is not None and stage._tracked.track_index == 2
        assert int(app.engine.outputs[1].min()) > 0
        status, body = app.on_method("snapshot", {"camera": 1})
        assert status == 200 and body["annotated"] is True
        want = _want(app, stage.annotate.host)
        assert base64.b64decode(body["jpeg_b64"]) == want[1]
        assert want[1] != _want(app, None)[1]
        assert all(m["annotated"] is True for m in tr.outputs("snapshots"))
        assert tr.reported["config"]["snapshot_annotate"] is True
        # a privacy class and a zone arrive through the twin: same engine, new pictures
        rebuilds, engine = app.state["rebuilds"], app.engine
        classes = sorted({int(c) for c in app.engine.outputs[0][0, :, 5].tolist()})[:1]
        tr.push_twin_patch({"snapshot_privacy_classes": classes, "snapshot_box_thickness": 2,
                            "snapshot_privacy_zones": [
                                {"name": "door", "cameras": [1],
                                 "polygon": [[40, 40], [64, 40], [64, 64], [40, 64]]}]})
        app.step()
        app.step()
        assert app.state["rebuilds"] == rebuilds and app.engine is engine
        host = stage.annotate.host
        assert host[0, ref.ANN_PRIV_CLS].item() == classes[0] and host[1, ref.ANN_N_POLY] == 1
        assert host[0, ref.ANN_N_POLY] == 0 and host[0, ref.ANN_THICKNESS] == 2
        got = base64.b64decode(app.on_method("snapshot", {"camera": 1})[1]["jpeg_b64"])
        assert got == _want(app, host)[1]
        # the zone alone pixelates the corner of camera 1
        bare = ops.frame_resize(app.engine.frames, stage.plan)
        drawn = ref.annotate(bare.clone(), host, stage.annotate.font_host, None, None, None,
                             (64, 64), 0)
        assert np.array_equal(drawn[1, 24:, 24:].numpy(),
                              ac.block_means(bare[1].numpy(), 8)[24:, 24:])
        assert torch.equal(drawn[0], bare[0])


def test_module_snapshots_without_annotate_stay_bare():
    tr, app = _app({"snapshot_every_s": 0.1, "snapshot_privacy_classes": [0]})
    with app:
        app.run(max_steps=2)
        assert app.snapshots.stage.annotate is None
        status, body = app.on_method("snapshot", {"camera": 0})
        assert status == 200 and "annotated" not in body
        assert base64.b64decode(body["jpeg_b64"]) == _want(app, None)[0]
        assert all("annotated" not in m for m in tr.outputs("snapshots"))


# ------------------------------------------------------------------ the kernel's source
def test_the_kernel_cross_compiles_without_warnings_or_spills(tmp_path):
    import os
    import shutil
    import subprocess

    from kvedge_amd import _build

    if not (os.path.exists(_build.hipcc()) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    src = os.path.join(_build.CSRC, "kernels", "annotate.hip")
    assert src in _build.glob.glob(os.path.join(_build.CSRC, "kernels", "*.hip"))
    for extra in ([], ["-DKVEDGE_CHECKS=1"]):  # the bounds-check build covers it too
        r = subprocess.run([_build.hipcc(), *_build.COMMON, *extra, "-Wall", "-Wextra", "-Werror",
                            "-Rpass-analysis=kernel-resource-usage", f"-I{_build.CSRC}/kernels",
                            "-c", src, "-o", str(tmp_path / "an.o")],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-2000:]
        usage = [l.split("remark:")[1].split("[-R")[0].strip() for l in r.stderr.splitlines()
                 if "remark:" in l]
        assert sum("annotate_kernel" in l for l in usage) == 1
        for key in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill"):
            assert [l for l in usage if l.startswith(key)] == [f"{key}: 0"], usage
