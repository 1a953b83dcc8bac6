"""The JPEG encoder on the MI355X: the three kernels' files against the CPU reference, byte for
byte -- every edge size, the images that reach each branch of the entropy coder at three
qualities, a batch with canaries behind every file, a row too small for its file, a captured
graph picking up a new quality, and a resized frame through the encoder into Pillow."""
import numpy as np
import pytest
import torch

import jpeg_cases as jc
from kvedge_amd import ops
from kvedge_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5


def _encode(arrays, sub, quality, rows=None, cap=None):
    """Encode on the GPU into a canary-filled buffer; returns (buf, length) on the CPU."""
    assert ops.load()
    imgs = jc.as_tensor(*arrays).cuda()
    m, (h, w) = imgs.shape[0], imgs.shape[1:3]
    enc = ops.JpegEncoder((h, w), m, sub, quality, device="cuda")
    out = torch.full((rows or m, cap or enc.max_bytes), CANARY, dtype=torch.uint8, device="cuda")
    lengths = torch.full((rows or m,), -7, dtype=torch.int32, device="cuda")
    got = ops.jpeg_encode(imgs, enc, out, lengths)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == lengths.data_ptr()
    return out.cpu(), lengths.cpu()


def _check(name, h, w, sub, quality):
    want, _ = jc.reference_file(name, h, w, sub, quality)
    buf, length = _encode([jc.image(name, h, w)], sub, quality)
    assert int(length[0]) == len(want), (int(length[0]), len(want))
    got = bytes(buf[0, :len(want)].tolist())
    if got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"first differing byte {first} of {len(want)}: "
                             f"{got[first:first + 8].hex()} != {want[first:first + 8].hex()}")
    assert bool((buf[0, len(want):] == CANARY).all())   # nothing written behind the file


@pytest.mark.parametrize("sub", jc.SUBSAMPLINGS)
@pytest.mark.parametrize("hw", [(1, 1), (8, 8), (9, 17), (17, 9), (16, 16), (45, 70)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_sizes(hw, sub):
    _check("noise", hw[0], hw[1], sub, 75)


@pytest.mark.parametrize("h", [72, 88])
def test_restart_markers_cycle_through_all_eight(h):
    """72 rows: 9 intervals, RST0 .. RST7 each once; 88 rows: 11 intervals, so the counter
    wraps and RST0 and RST1 come twice."""
    want, _ = jc.reference_file("noise", h, 24, "444", 75)
    assert all(want.count(bytes([0xff, 0xd0 + n])) == (2 if h == 88 and n < 2 else 1)
               for n in range(8))
    _check("noise", h, 24, "444", 75)


@pytest.mark.parametrize("name", ["noise", "smooth"])
@pytest.mark.parametrize("hw,sub", [((8, 528), "444"), ((16, 352), "420"), ((24, 150), "420")],
                         ids=["8x528-444", "16x352-420", "24x150-420"])
def test_more_than_64_blocks_per_interval_carry_a_partial_byte(hw, sub, name):
    """198 / 132 / 60 blocks per interval: the first two cross chunks of 64 blocks with a bit
    offset that is no multiple of 8 (checked on the reference's coefficients), and span several
    128-column strips of the block kernel, the last one partial; 150 columns take its byte
    path."""
    h, w = hw
    if hw != (24, 150):   # (one interval)
        coef = ref.jpeg_coefficients(jc.image(name, h, w), sub, ref.jpeg_quant_tables(75))
        st = dict(stuffed=0, zrl=0, eob=0, dc_nonzero=0, max_dc_cat=0, max_ac_cat=0, bits=0)
        ref.jpeg_scan(coef[:, :64], sub, st)
        assert coef.shape[0] == 1 and coef.shape[1] > 64 and st["bits"] % 8 != 0
    _check(name, h, w, sub, 75)


@pytest.mark.parametrize("quality", jc.QUALITIES)
@pytest.mark.parametrize("sub", jc.SUBSAMPLINGS)
@pytest.mark.parametrize("name", ["constant", "noise", "bw_blocks", "sparse_zrl"])
def test_content_that_reaches_every_branch(name, sub, quality):
    _check(name, 16, 32, sub, quality)


@pytest.mark.parametrize("sub", jc.SUBSAMPLINGS)
def test_batch_of_five_leaves_the_canaries(sub):
    names = ["constant", "noise", "bw_blocks", "sparse_zrl", "smooth"]
    want = [jc.reference_file(n, 24, 40, sub, 50)[0] for n in names]
    assert len({len(f) for f in want}) == 5
    buf, length = _encode([jc.image(n, 24, 40) for n in names], sub, 50, rows=7)
    assert length.tolist() == [len(f) for f in want] + [-7, -7]
    for m, f in enumerate(want):
        assert bytes(buf[m, :len(f)].tolist()) == f, names[m]
        assert bool((buf[m, len(f):] == CANARY).all()), names[m]
    assert bool((buf[5:] == CANARY).all())


@pytest.mark.parametrize("sub", jc.SUBSAMPLINGS)
def test_row_too_small_for_its_file(sub):
    names = ["constant", "smooth", "noise", "sparse_zrl", "constant"]
    want = [jc.reference_file(n, 24, 40, sub, 100)[0] for n in names]
    cap = len(want[2]) // 2
    assert all(len(f) <= cap for m, f in enumerate(want) if m != 2)
    buf, length = _encode([jc.image(n, 24, 40) for n in names], sub, 100, cap=cap)
    assert int(length[2]) == -len(want[2])
    assert bool((buf[2] == CANARY).all())
    for m, f in enumerate(want):
        if m != 2:
            assert int(length[m]) == len(f) and bytes(buf[m, :len(f)].tolist()) == f
            assert bool((buf[m, len(f):] == CANARY).all())


def test_captured_graph_sees_new_pixels_and_a_new_quality():
    assert ops.load()
    h, w = 24, 40
    first = jc.as_tensor(jc.image("smooth", h, w), jc.image("constant", h, w))
    second = jc.as_tensor(jc.image("noise", h, w), jc.image("bw_blocks", h, w))
    enc = ops.JpegEncoder((h, w), 2, "420", 75, device="cuda")
    imgs = first.cuda()
    out = torch.full((2, enc.max_bytes), CANARY, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.jpeg_encode(imgs, enc, out, lengths)   # (warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.jpeg_encode(imgs, enc, out, lengths)
    for pixels, quality in ((first, 75), (second, 30)):
        imgs.copy_(pixels)
        enc.set_quality(quality)
        out.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        want = ref.jpeg_encode(pixels, "420", quality)
        assert lengths.tolist() == [len(f) for f in want], quality
        for m, f in enumerate(want):
            assert bytes(out[m, :len(f)].tolist()) == f, (quality, m)
    assert jc.dqt_bytes(want[0]) == jc.dqt_bytes(ref.jpeg_header((h, w), "420",
                                                               ref.jpeg_quant_tables(30)))


def test_resized_frame_through_the_encoder_opens_in_pillow():
    pytest.importorskip("PIL")
    assert ops.load()
    src = jc.as_tensor(jc.image("smooth", 96, 64), jc.image("noise", 96, 64)).cuda()
    plan = ops.thumbnail_plan((96, 64), 30)
    small = ops.frame_resize(src, plan)
    enc = ops.JpegEncoder(plan.dst_hw, 2, "420", 75, device="cuda")
    buf, length = ops.jpeg_encode(small, enc)
    torch.cuda.synchronize()
    assert buf.shape == (2, enc.max_bytes)
    want = ref.jpeg_encode(small.cpu(), "420", 75)
    for m in range(2):
        data = bytes(buf[m, :int(length[m])].tolist())
        assert data == want[m]
        im = jc.decode(data)
        assert im.size == (32, 48)
    # the smooth frame survives the trip
    assert jc.psnr(jc.decode(bytes(buf[0, :int(length[0])].tolist())), small[0].cpu().numpy()) > 30


def test_launcher_rejections_leave_the_outputs_alone():
    assert ops.load()
    enc = ops.JpegEncoder((8, 8), 1, device="cuda")
    imgs = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((1, 700), CANARY, dtype=torch.uint8, device="cuda")
    lengths = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    n = torch.ops.kvedge
    with pytest.raises(RuntimeError):   # a workspace of another geometry
        small = ops.JpegEncoder((8, 8), 1, "444", device="cuda")
        n.jpeg_encode(imgs, enc.qtab, enc.huff, enc.header, small.coef, enc.scratch, enc.seglen,
                      out, lengths, True)
    with pytest.raises(RuntimeError):   # a CPU table
        n.jpeg_encode(imgs, enc.qtab.cpu(), enc.huff, enc.header, enc.coef, enc.scratch,
                      enc.seglen, out, lengths, True)
    with pytest.raises(RuntimeError):   # a short header
        n.jpeg_encode(imgs, enc.qtab, enc.huff, enc.header[:600], enc.coef, enc.scratch,
                      enc.seglen, out, lengths, True)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and int(lengths[0]) == -7
