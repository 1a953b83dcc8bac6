"""Snapshot annotation on the MI355X: csrc/kernels/annotate.hip against ops.reference.annotate,
byte for byte, at the smallest shapes where the kernel can go wrong -- smaller than a block,
blocks and tiles clipped at both edges, boxes across tile seams, a full rectangle list -- with
canary rows around the images, and inside a captured graph whose style changes between replays."""
import pytest
import torch

import annotate_cases as ac
from kvedge_amd import ops
from kvedge_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
SRC = (90, 160)
# crosses the 64-wide tile seam of a 36 x 68 thumbnail and two 16-high ones; concave
SEAM_POLY = [(100, 10), (158, 12), (150, 80), (130, 40), (105, 85)]


def _both(style_kw, streams=1):
    return ac.style_of(streams, **style_kw), ac.style_of(streams, "cuda", **style_kw)


def _check(img, cpu_style, gpu_style, det=None, count=None, tid=None, src_hw=None, slot0=0):
    """Run both on ``img``; the device copy sits between two canary images."""
    n = img.shape[0]
    want = ref.annotate(img.clone(), cpu_style.host, cpu_style.font_host, det, count, tid,
                        src_hw or tuple(img.shape[1:3]), slot0)
    alloc = torch.full((n + 2, *img.shape[1:]), CANARY, dtype=torch.uint8, device="cuda")
    alloc[1:n + 1].copy_(img)
    dev = [None if t is None else t.cuda() for t in (det, count, tid)]
    out = ops.annotate(alloc[1:n + 1], gpu_style, *dev, src_hw=src_hw, slot0=slot0)
    torch.cuda.synchronize()
    got = alloc.cpu()
    assert out.data_ptr() == alloc[1:n + 1].data_ptr()
    assert bool((got[0] == CANARY).all()) and bool((got[n + 1] == CANARY).all())
    diff = (got[1:n + 1] != want).any(-1)
    assert not bool(diff.any()), diff.nonzero()[:8].tolist()
    return want


@pytest.mark.parametrize("blk", [4, 8, 16])
@pytest.mark.parametrize("hw", [(4, 4), (12, 20), (36, 68), (32, 48)])
def test_sizes_and_blocks(hw, blk):
    h, w = hw
    img = ac.picture(2, h, w, seed=h + blk)
    det, count, tid = ac.noisy_case(2, h, w, 12, SRC, seed=w)
    cpu, gpu = _both(dict(boxes=True, labels="both", classes=[1, 3], block=blk, thickness=2,
                          colour_by="track", polygons=[SEAM_POLY]), 2)
    want = _check(img, cpu, gpu, det, count, tid, SRC)
    assert not torch.equal(want, img)
    # labels at scale 2 and thin outlines, nothing hidden; then the mosaic alone
    _check(img, *_both(dict(boxes=True, labels="id", scale=2), 2), det, count, tid, SRC)
    _check(img, *_both(dict(classes=[0, 2], block=blk), 2), det, count, tid, SRC)


def test_all_300_rows_meet_one_tile_and_count_beyond_max_det():
    h, w = 36, 68
    img = ac.picture(1, h, w, seed=30)
    g = torch.Generator().manual_seed(31)
    det = torch.zeros(1, 300, 6)
    det[0, :, 0:2] = torch.rand(300, 2, generator=g) * torch.tensor([9.0, 4.0])
    det[0, :, 2:4] = torch.tensor([10.0, 5.0]) + torch.rand(300, 2, generator=g) * torch.tensor(
        [56.0, 30.0])
    det[0, :, 5] = (torch.arange(300) % 5).float()
    tid = torch.arange(300, dtype=torch.int32).view(1, 300) * 7 - 1
    count = torch.tensor([1000], dtype=torch.int32)
    rects = ref.annotate_rects(det[0], (h, w), (h, w))
    assert bool(((rects[:, 0] < 64) & (rects[:, 1] < 16)).all())    # every row in tile (0, 0)
    for kw in (dict(boxes=True, labels="both", max_draw=300, classes=[4], block=4),
               dict(boxes=True, labels="class", max_draw=300),
               dict(classes=[0, 1, 2, 3, 4], block=16), dict(boxes=True, labels="both")):
        _check(img, *_both(kw), det, count, tid)


def test_max_det_one():
    img = ac.picture(3, 12, 20, seed=32)
    det, count = ac.dets([[(3.2, 2.7, 15.1, 9.9, 1)]] * 3)
    count[1], count[2] = 0, 7
    tid = torch.tensor([[4], [5], [-1]], dtype=torch.int32)
    _check(img, *_both(dict(boxes=True, labels="both", classes=[1]), 3), det, count, tid)
    _check(img, *_both(dict(boxes=True, labels="both"), 3), det, count, None)


def test_box_edge_cases():
    h, w = 36, 68
    nan, big = float("nan"), 1e9
    rows = [[(0, 0, 160, 90, 1)],                       # the whole image
            [(40, 30, 40, 30, 1)],                      # zero area
            [(159.9, 89.9, 160, 90, 1)],                # on the last pixel
            [(nan, 10, 80, nan, 1)],                    # NaN -> 0
            [(-50, -20, 500, 300, 1), (170, 95, 400, 200, 1), (-big, 20, big, 25, 1)],  # beyond
            [(80, 60, 20, 10, 1)]]                      # x2 < x1
    det, count = ac.dets(rows)
    count[5] = 9                                        # count > max_det
    img = ac.picture(len(rows), h, w, seed=33)
    tid = torch.arange(18, dtype=torch.int32).view(6, 3)
    for kw in (dict(boxes=True, labels="both", thickness=3), dict(classes=[1], block=8),
               dict(boxes=True, labels="both", classes=[1], thickness=4, scale=2, block=16)):
        _check(img, *_both(kw, len(rows)), det, count, tid, SRC)


def test_polygons():
    h, w = 36, 68
    img = ac.picture(2, h, w, seed=34)
    octagon = [(30, 5), (50, 5), (62, 20), (62, 40), (50, 55), (30, 55), (18, 40), (18, 20)]
    polys = [[(x + 12 * i, y + 3 * i) for x, y in octagon] for i in range(6)]
    polys.append([(5, 60), (40, 62), (38, 88), (22, 70), (20, 88), (8, 86), (12, 74), (4, 70)])
    # lies between pixel centres of the thumbnail: hides nothing
    polys.append([(1.25, 1.5), (1.5, 1.25), (2.0, 1.25), (2.25, 1.5), (2.25, 2.0), (2.0, 2.25),
                  (1.5, 2.25), (1.25, 2.0)])
    for blk in (4, 8, 16):
        cpu, gpu = _both(dict(polygons=polys, block=blk), 2)
        assert cpu.n_polygons.tolist() == [8, 8] and cpu.n_vertex.tolist() == [[8] * 8] * 2
        _check(img, cpu, gpu, src_hw=SRC)
    only = _check(img, *_both(dict(polygons=[polys[7]], block=4), 2), src_hw=SRC)
    assert torch.equal(only, img)
    det, count, tid = ac.noisy_case(2, h, w, 6, SRC, seed=35)
    _check(img, *_both(dict(polygons=polys[5:], boxes=True, labels="both", classes=[2]), 2),
           det, count, tid, SRC)


def test_slot0_picks_the_cameras_style():
    img = ac.picture(2, 12, 20, seed=36)
    det, count, tid = ac.noisy_case(2, 12, 20, 5, SRC, seed=37)
    cpu, gpu = _both(dict(boxes=True, labels="both", classes=[1], block=4), 3)
    for s in (cpu, gpu):   # row 0 is another style, and must not be used
        s.set_boxes(False, camera=0).set_labels("none", camera=0).set_privacy_block(16, camera=0)
        s.set_privacy_classes([0, 1, 2, 3], camera=0).set_thickness(3, camera=2)
    a = _check(img, cpu, gpu, det, count, tid, SRC, slot0=1)
    b = _check(img, cpu, gpu, det, count, tid, SRC, slot0=0)
    assert not torch.equal(a, b)
    with pytest.raises((ValueError, RuntimeError)):
        ops.annotate(img.cuda(), gpu, det.cuda(), count.cuda(), tid.cuda(), src_hw=SRC, slot0=2)


def test_a_captured_graph_follows_the_style_without_recapture():
    hs, ws = 64, 96
    plan = ops.thumbnail_plan((hs, ws), 48)
    assert plan.dst_hw == (32, 48)
    frames = ac.picture(2, hs, ws, seed=38)
    det, count, tid = ac.noisy_case(2, 32, 48, 8, (hs, ws), seed=39)
    cpu, gpu = _both(dict(boxes=True, labels="both"), 2)
    enc = ops.JpegEncoder(plan.dst_hw, 2, "420", 75, device="cuda")
    src, d, c, t = frames.cuda(), det.cuda(), count.cuda(), tid.cuda()
    small = torch.empty(2, 32, 48, 3, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, enc.max_bytes, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(2, dtype=torch.int32, device="cuda")

    def step():
        ops.frame_resize(src, plan, out=small)
        ops.annotate(small, gpu, d, c, t, src_hw=(hs, ws))
        ops.jpeg_encode(small, enc, out, lengths)

    step()   # (warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    seen = []
    for change in (lambda s: s, lambda s: s.set_privacy_classes([int(det[0, 0, 5])])
                   .set_thickness(3)):
        change(cpu), change(gpu)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        drawn = ref.annotate(ops.frame_resize(frames, plan), cpu.host, cpu.font_host, det, count,
                             tid, (hs, ws), 0)
        want = ref.jpeg_encode(drawn, "420", 75)
        assert lengths.tolist() == [len(f) for f in want]
        for m, f in enumerate(want):
            assert bytes(out[m, :len(f)].tolist()) == f, m
        seen.append(want)
    assert seen[0] != seen[1]
