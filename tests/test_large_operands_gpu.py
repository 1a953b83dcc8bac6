"""Camera-side kernels on batches whose operand passes 2^31 and 2^32 bytes.

The conv families have tests past the 2 GiB-per-operand limit (test_chunking_gpu.py); these
are the other kernels -- camera input, stems, pools, pre- and post-processing -- which address
whole batches through hand-written pointer arithmetic.  Every case here:

  * builds the big operand on the device only, from a seeded device generator, with every
    image different, and poisons the outputs (NaN, 0xA5, an int32 sentinel);
  * takes the fewest images that cross the mark (large_cases.count_past, asserted);
  * copies image 0, the images holding byte 2^31 and byte 2^32 of the operand with their two
    neighbours, and the last image to the host, runs the CPU reference (the same ``ops`` call on
    CPU tensors) on that small batch and compares with the kernel's own rule for that op:
    bitwise where its existing GPU test is bitwise, ``kernel_rules.assert_close`` for the bf16
    arithmetic kernels.  An address that wraps by 2^31 or 2^32 bytes lands in another image
    and fails that comparison (test_large_operands_cpu.py shows it does);
  * checks that what the op must not touch keeps its poison.

Launcher caps are loud: at each cap the largest accepted batch runs and is right on its last
image, the first refused one raises ``RuntimeError`` naming the op and leaves a poisoned output
as it was.  A refusal is a host-side check before any launch.

The stem kernels read their input through 32-bit buffer offsets (input < 0x7ffffff0 bytes), so
only their outputs can cross: stem12_pool_frames (ldy 80) passes 2^32 bytes.  stem_pool's output
is 160 bytes for every 128 bytes of input and yolo_stem2's 4 for every 3, so under the cap these
two pass 2^31 (2.68 and 2.86 GB) and cannot reach 2^32; stem_pool_frames shares stem_pool's
launcher, which holds the frames to the bf16 space-to-depth image they stand for (8 bytes a
pixel, not 3), so its output ends at 2.68 GB as well.

upsample2x's item rule caps N*H*W*C/8 at 2^31 - 2^21 - 1 items of 16 bytes: the boundary
needs a 34 GB input and a 137 GB output.  It is run like every other case and skips, as they
all do, only when the card has less free memory than that.

Left out: yolo_decode (705,600 bytes of head maps an image at 640 x 640: 2^32 at N = 6,088,
with 8,400 x 24 bytes of output each, but its index is per (image, anchor) in 64 bits and a
batch of thousands of 640 x 640 images is not a deployment), nms (8,400 x 24 bytes in, 300 x 24
out: 2^32 at N = 21,306), det_to_source (7,200 bytes: N = 596,524, refused from N * max_det =
2^31), track_update and zone_update (state rows of 3 KB: N above 2^20, refused from 2^24),
motion_blobs (masks of at most 4,096 bytes, N <= 65,535: 268 MB).  None reaches a mark within a
batch any deployment runs.

Cases (computed by large_cases.table(); peak = device bytes the test holds at once):

"""
import gc

import pytest
import torch

import large_cases as lc
from kvedge_amd import ops
from large_cases import CASES

__doc__ += lc.table() + "\n"

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load(), "native kvedge library must be loaded on the GPU box"
    yield


@pytest.fixture(autouse=True)
def _free_after():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _need(nbytes):
    """Skip only when the (shared) card has less free memory than the test states, + 2 GiB."""
    free, _ = torch.cuda.mem_get_info()
    need = int(nbytes) + 2 * lc.GIB
    if free < need:
        pytest.skip(f"needs {need / lc.GIB:.1f} GiB of device memory, {free / lc.GIB:.1f} GiB free")


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _bytes(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=_gen(seed))


def _randn(shape, seed):
    return torch.randn(shape, dtype=BF16, device="cuda", generator=_gen(seed))


def _full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _idx(rows):
    return torch.tensor(rows, device="cuda")


def _all(pred, t, step=1 << 28):
    """``pred(chunk).all()`` over the leading dimension in chunks, so that the boolean
    temporary of a 4 GB operand stays small."""
    rows = max(1, step // max(1, t[0].numel()))
    return all(bool(pred(t[i:i + rows]).all()) for i in range(0, t.shape[0], rows))


def _all_nan(t):
    return _all(torch.isnan, t)


def _all_eq(t, v):
    return _all(lambda c: c == v, t)


def _letterbox(src_hw, dst_hw):
    """Ultralytics' letterbox into a destination that need not be square."""
    (hs, ws), (hd, wd) = src_hw, dst_hw
    r = min(hd / hs, wd / ws)
    nh, nw = min(hd, max(1, int(round(hs * r)))), min(wd, max(1, int(round(ws * r))))
    top, left = int(round((hd - nh) / 2 - 0.1)), int(round((wd - nw) / 2 - 0.1))
    return ops.ResizePlan((hs, nh, 0, top, nh), (ws, nw, 0, left, nw), ops.LETTERBOX_PAD,
                          (hs, ws), (hd, wd))


# ---------------------------------------------------------------------------
# frame_resize, frame_resize_nv12
# ---------------------------------------------------------------------------
def _resize(case, src_shape, plan, fmt):
    _need(case.peak)
    n, rows = case.n, case.rows
    assert n * case.image_bytes > lc.MARK32
    src = _bytes((n, *src_shape), 1)
    alloc = _full((n + 1, *plan.dst_hw, 3), lc.POISON_U8, torch.uint8)  # one guard image behind
    ops.frame_resize(src, plan, out=alloc[:n], src_format=fmt)
    torch.cuda.synchronize()
    want = ops.frame_resize(src[_idx(rows)].cpu(), plan, src_format=fmt)
    lc.check_exact(alloc[_idx(rows)].cpu(), want, rows, case.op)
    assert _all_eq(alloc[n:], lc.POISON_U8)


def test_frame_resize_src_past_4gib():
    _resize(CASES["frame_resize:src"], (*lc.HD, 3), _letterbox(lc.HD, lc.SMALL_DST), "rgb")


def test_frame_resize_dst_past_4gib():
    _resize(CASES["frame_resize:dst"], (8, 12, 3), _letterbox((8, 12), lc.HD), "rgb")


def test_frame_resize_nv12_src_past_4gib():
    _resize(CASES["frame_resize_nv12:src"], (lc.HD[0] * 3 // 2, lc.HD[1]),
            _letterbox(lc.HD, lc.SMALL_DST), "nv12")


# ---------------------------------------------------------------------------
# roi_crop, roi_crop_nv12
# ---------------------------------------------------------------------------
def _boxes(n, k, hw, seed):
    """k boxes a row inside an hw frame, x1 y1 x2 y2 score class (host)."""
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    p = torch.rand(n, k, 2, generator=g) * torch.tensor([w * 0.6, h * 0.6])
    s = torch.rand(n, k, 2, generator=g) * torch.tensor([w * 0.35, h * 0.35]) + 2.0
    det = torch.zeros(n, k, 6)
    det[..., 0:2], det[..., 2:4], det[..., 4] = p, p + s, 0.9
    return det


@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_roi_crop_src_past_4gib(fmt):
    """Boxes only in the sampled images (one of them with a single box): their crops equal the
    reference, every other crop is the pad value."""
    case = CASES["roi_crop:src" if fmt == "rgb" else "roi_crop_nv12:src"]
    _need(case.peak)
    n, rows, K, D, pad = case.n, case.rows, lc.ROI_K, lc.ROI_D, 7
    assert n * case.image_bytes > lc.MARK32
    shape = (*lc.HD, 3) if fmt == "rgb" else (lc.HD[0] * 3 // 2, lc.HD[1])
    src = _bytes((n, *shape), 2)
    det_s = _boxes(len(rows), lc.ROI_MAXDET, lc.HD, 3)
    count_s = torch.full((len(rows),), K, dtype=torch.int32)
    count_s[1] = 1
    det = torch.zeros(n, lc.ROI_MAXDET, 6, device="cuda")
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    det[_idx(rows)], count[_idx(rows)] = det_s.cuda(), count_s.cuda()
    out = _full((n * K, D, D, 3), lc.POISON_U8, torch.uint8)
    ops.roi_crop(src, det, count, K, D, pad=pad, out=out, src_format=fmt)
    torch.cuda.synchronize()
    want = ops.roi_crop(src[_idx(rows)].cpu(), det_s, count_s, K, D, pad=pad, src_format=fmt)
    got = out.view(n, K, D, D, 3)
    lc.check_exact(got[_idx(rows)].cpu(), want.view(len(rows), K, D, D, 3), rows, case.op)
    assert not bool((want.view(len(rows), -1) == pad).all(1).any())  # the crops hold pixels
    others = torch.ones(n, dtype=torch.bool, device="cuda")
    others[_idx(rows)] = False
    assert bool((got[others] == pad).all())


@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_roi_crop_dst_past_4gib(fmt):
    case = CASES["roi_crop:dst" if fmt == "rgb" else "roi_crop_nv12:dst"]
    _need(case.peak)
    n, rows, K, D = case.n, case.rows, lc.ROI_BIG_K, lc.ROI_BIG_D
    assert n * K * D * D * 3 > lc.MARK32
    hs, ws = lc.ROI_BIG_SRC
    src = _bytes((n, hs, ws, 3) if fmt == "rgb" else (n, hs * 3 // 2, ws), 4)
    det_s = _boxes(len(rows), K, lc.ROI_BIG_SRC, 5)
    det = _boxes(1, K, lc.ROI_BIG_SRC, 6).cuda().repeat(n, 1, 1)
    det[_idx(rows)] = det_s.cuda()
    count = torch.full((n,), K, dtype=torch.int32, device="cuda")
    alloc = _full(((n + 1) * K, D, D, 3), lc.POISON_U8, torch.uint8)  # one guard image behind
    ops.roi_crop(src, det, count, K, D, out=alloc[:n * K], src_format=fmt)
    torch.cuda.synchronize()
    want = ops.roi_crop(src[_idx(rows)].cpu(), det_s, count[_idx(rows)].cpu(), K, D,
                        src_format=fmt)
    got = alloc.view(n + 1, K, D, D, 3)
    lc.check_exact(got[_idx(rows)].cpu(), want.view(len(rows), K, D, D, 3), rows, case.op)
    assert _all_eq(got[n:], lc.POISON_U8)


# ---------------------------------------------------------------------------
# frame_watch
# ---------------------------------------------------------------------------
def _watch_steps(src, gpu, cpu, rows, what):
    """Two steps, so that the second reads the state the first wrote; state, stats and mask of
    the sampled streams against the reference, which holds exactly those streams."""
    n = src.shape[0]
    for step in range(2):
        stats = _full((n, 16), lc.POISON_I32, torch.int32)
        mask = _full((n, *gpu.grid), lc.POISON_U8, torch.uint8)
        ops.frame_watch(src, gpu, out_stats=stats, out_mask=mask)
        torch.cuda.synchronize()
        w_stats, w_mask = ops.frame_watch(src[_idx(rows)].cpu(), cpu)
        lc.check_exact(stats[_idx(rows)].cpu(), w_stats, rows, (what, "stats", step))
        lc.check_exact(mask[_idx(rows)].cpu(), w_mask, rows, (what, "mask", step))
        lc.check_exact(gpu.buf[_idx(rows)].cpu(), cpu.buf, rows, (what, "state", step))
        assert not bool((stats == lc.POISON_I32).any()) and bool((mask <= 3).all())
        src.bitwise_right_shift_(1)  # the next frame: half as bright, every cell moves
    assert int(w_stats[:, 2].sum()) > 0  # cells moved in the second step


def test_frame_watch_src_past_4gib():
    case = CASES["frame_watch:src"]
    _need(case.peak)
    n, rows = case.n, case.rows
    assert n * case.image_bytes > lc.MARK32 and lc.grid_accepts(n)
    src = _bytes((n, *lc.WATCH_HW, 3), 7)
    gpu = ops.WatchState(n, lc.WATCH_HW, cell=lc.WATCH_CELL, device="cuda")
    cpu = ops.WatchState(len(rows), lc.WATCH_HW, cell=lc.WATCH_CELL)
    _watch_steps(src, gpu, cpu, rows, "frame_watch")


# ---------------------------------------------------------------------------
# annotate
# ---------------------------------------------------------------------------
def test_annotate_images_past_4gib():
    """One box with its label in every sampled image and in two unsampled ones; every other
    image has no row in the tables and must come back byte for byte."""
    case = CASES["annotate:images"]
    _need(case.peak)
    n, rows = case.n, case.rows
    h, w = lc.ANNOTATE_HW
    assert n * case.image_bytes > lc.MARK32 and lc.grid_accepts(n)
    extra = [r for r in (lc.MARK31 // case.image_bytes + 3, lc.MARK32 // case.image_bytes - 3)
             if r not in rows]
    assert len(extra) == 2
    drawn = sorted(rows + extra)
    images = _bytes((n, h, w, 3), 8)
    orig = images.clone()
    det_s = _boxes(len(drawn), 1, (h, w), 9)
    det_s[..., 5] = torch.arange(len(drawn)).view(-1, 1) % 5
    tid_s = (torch.arange(len(drawn), dtype=torch.int32) * 37 + 5).view(-1, 1)
    det = torch.zeros(n, 1, 6, device="cuda")
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    tid = torch.full((n, 1), -1, dtype=torch.int32, device="cuda")
    det[_idx(drawn)], count[_idx(drawn)], tid[_idx(drawn)] = det_s.cuda(), 1, tid_s.cuda()
    ops.annotate(images, ops.AnnotateStyle(n, device="cuda"), det, count, tid)
    torch.cuda.synchronize()
    want = ops.annotate(orig[_idx(drawn)].cpu(), ops.AnnotateStyle(len(drawn)), det_s,
                        torch.ones(len(drawn), dtype=torch.int32), tid_s)
    lc.check_exact(images[_idx(drawn)].cpu(), want, drawn, "annotate")
    changed = torch.cat([(images[i:i + 4096] != orig[i:i + 4096]).flatten(1).any(1)
                         for i in range(0, n, 4096)])
    assert changed.nonzero().flatten().tolist() == drawn


# ---------------------------------------------------------------------------
# jpeg_encode
# ---------------------------------------------------------------------------
def _jpeg_images(n, hw, seed):
    """Random 8 x 8 blocks of one colour under a little noise: every image different, files of
    a few KB."""
    h, w = hw
    img = torch.randint(0, 8, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=_gen(seed))
    base = torch.randint(0, 248, (n, h // 8, 1, w // 8, 1, 3), dtype=torch.uint8, device="cuda",
                         generator=_gen(seed + 1))
    img.view(n, h // 8, 8, w // 8, 8, 3).add_(base)
    return img


def _jpeg_check(images, n, rows, cap, what):
    m = images.shape[0]
    hw = tuple(images.shape[1:3])
    enc = ops.JpegEncoder(hw, m, "420", quality=50, device="cuda")
    out = _full((m + 1, cap), lc.POISON_U8, torch.uint8)
    length = _full((m + 1,), lc.POISON_I32, torch.int32)
    ops.jpeg_encode(images[:n], enc, out=out, lengths=length)
    torch.cuda.synchronize()
    w_out = torch.full((len(rows), cap), lc.POISON_U8, dtype=torch.uint8)
    w_len = torch.zeros(len(rows), dtype=torch.int32)
    ops.jpeg_encode(images[_idx(rows)].cpu(), ops.JpegEncoder(hw, len(rows), "420", quality=50),
                    out=w_out, lengths=w_len)
    assert bool((w_len > 0).all()), w_len  # every sampled file fits: whole files are compared
    assert torch.equal(length[_idx(rows)].cpu(), w_len), what
    lc.check_exact(out[_idx(rows)].cpu(), w_out, rows, what)  # the file, and the poison behind
    assert bool((out[n:] == lc.POISON_U8).all()) and bool((length[n:] == lc.POISON_I32).all())
    return enc, out, length


def test_jpeg_encode_images_past_4gib():
    case = CASES["jpeg_encode:images"]
    _need(case.peak)
    n, rows = case.n, case.rows
    assert n * case.image_bytes > lc.MARK32 and lc.grid_accepts(n)
    _jpeg_check(_jpeg_images(n, lc.JPEG_HW, 10), n, rows, lc.JPEG_CAP, "jpeg_encode")


# ---------------------------------------------------------------------------
# preprocess, synth_frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("operand", ["y", "x"])
@pytest.mark.parametrize("s2d", [False, True])
def test_preprocess_past_4gib(s2d, operand):
    case = CASES[("preprocess_s2d:" if s2d else "preprocess:") + operand]
    _need(case.peak)
    n, rows = case.n, case.rows
    h, w = lc.PRE_HW
    assert n * (h * w * 8 if operand == "y" else h * w * 3) > lc.MARK32
    x = _bytes((n, h, w, 3), 11)
    alloc = _full((n + 1, h // 2, w // 2, 16) if s2d else (n + 1, h, w, 4), NAN, BF16)
    ops.preprocess(x, out=alloc[:n], s2d=s2d)
    torch.cuda.synchronize()
    # the row sample of the operand under test; the other operand's own marks on top
    rows = sorted(set(rows) | set(lc.sample_rows(n, h * w * (3 if operand == "y" else 8))))
    want = ops.preprocess(x[_idx(rows)].cpu(), s2d=s2d)
    lc.check_close(alloc[_idx(rows)].cpu(), want, rows, case.op)
    assert _all_nan(alloc[n:])


def test_synth_frames_past_4gib():
    """The generator hashes the absolute 8-byte word index, so the CPU op cannot produce a
    window of a big buffer; the sampled frames are compared with the reference's own hash of
    their word indices (large_cases.synth_window), which the CPU op is held to on frame 0."""
    case = CASES["synth_frames:out"]
    _need(case.peak)
    n, rows, seed, step = case.n, case.rows, 1234, 5
    h, w = lc.SYNTH_HW
    assert n * case.image_bytes > lc.MARK32
    alloc = _full((n + 1, h, w, 3), lc.POISON_U8, torch.uint8)
    ops.synth_frames(alloc[:n], seed, step)
    torch.cuda.synchronize()
    b = case.image_bytes
    want = torch.stack([lc.synth_window(seed, step, r * b, b).view(h, w, 3) for r in rows])
    assert torch.equal(ops.synth_frames(torch.empty(2, h, w, 3, dtype=torch.uint8), seed, step),
                       torch.stack([lc.synth_window(seed, step, r * b, b).view(h, w, 3)
                                    for r in (0, 1)]))
    lc.check_exact(alloc[_idx(rows)].cpu(), want, rows, "synth_frames")
    assert _all_eq(alloc[n:], lc.POISON_U8)


# ---------------------------------------------------------------------------
# pools, head, batch norm
# ---------------------------------------------------------------------------
def test_maxpool2d_x_past_4gib():
    """Channel slices on both sides (ldx 64 > C 8, x_coff 8, y_coff 8): the pitch is in the
    product that crosses."""
    case = CASES["maxpool2d:x"]
    _need(case.peak)
    n, rows = case.n, case.rows
    assert n * case.image_bytes > lc.MARK32
    x = _randn((n, 4, 4, 64), 12)
    alloc = _full((n + 1, 2, 2, 16), NAN, BF16)
    ops.maxpool2d(x, 2, 2, 0, out=alloc[:n], C=8, x_coff=8, y_coff=8)
    torch.cuda.synchronize()
    want = ops.maxpool2d(x[_idx(rows)].cpu(), 2, 2, 0, C=8, x_coff=8)
    lc.check_exact(alloc[_idx(rows)][..., 8:].cpu(), want, rows, "maxpool2d")
    assert _all_nan(alloc[..., :8]) and _all_nan(alloc[n:])


def test_upsample2x_y_past_4gib():
    """The output pitch (ldy 64 for C 8) takes y past 2^32 bytes with 2^23 work items, far
    under the launcher's item rule."""
    case = CASES["upsample2x:y"]
    _need(case.peak)
    n, rows = case.n, case.rows
    assert n * case.image_bytes > lc.MARK32 and lc.upsample_accepts(n * 2 * 2)
    x = _randn((n, 2, 2, 8), 13)
    alloc = _full((n + 1, 4, 4, 64), NAN, BF16)
    ops.upsample2x(x, alloc[:n], C=8, y_coff=8)
    torch.cuda.synchronize()
    xs = x[_idx(rows)].cpu()
    want = ops.upsample2x(xs, torch.empty(len(rows), 4, 4, 8, dtype=BF16))
    lc.check_exact(alloc[_idx(rows)][..., 8:16].cpu(), want, rows, "upsample2x")
    assert _all_nan(alloc[..., :8]) and _all_nan(alloc[..., 16:]) and _all_nan(alloc[n:])


def test_global_avgpool_x_past_4gib():
    case = CASES["global_avgpool:x"]
    _need(case.peak)
    n, rows = case.n, case.rows
    assert n * case.image_bytes > lc.MARK32
    x = _randn((n, 8, 8, 64), 14)
    alloc = _full((n + 1, 64), NAN, BF16)
    ops.global_avgpool(x, out=alloc[:n])
    torch.cuda.synchronize()
    lc.check_close(alloc[_idx(rows)].cpu(), ops.global_avgpool(x[_idx(rows)].cpu()), rows,
                   "global_avgpool")
    assert not bool(torch.isnan(alloc[:n]).any()) and _all_nan(alloc[n:])


def test_batchnorm_nhwc_x_past_4gib():
    case = CASES["batchnorm_nhwc:x"]
    _need(case.peak)
    n, rows = case.n, case.rows
    assert n * case.image_bytes > lc.MARK32
    x = _randn((n, 8, 8, 8), 15)
    g = torch.Generator().manual_seed(16)
    scale, shift = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    alloc = _full((n + 1, 8, 8, 8), NAN, BF16)
    ops.batchnorm_nhwc(x, scale.cuda(), shift.cuda(), relu=False, out=alloc[:n])
    torch.cuda.synchronize()
    want = ops.batchnorm_nhwc(x[_idx(rows)].cpu(), scale, shift, relu=False)
    lc.check_close(alloc[_idx(rows)].cpu(), want, rows, "batchnorm_nhwc")
    assert _all_nan(alloc[n:])


@pytest.mark.parametrize("cols", [1000, 1001])
def test_softmax_rows_x_past_4gib(cols):
    """1000 columns: the register-resident row; 1001: the strided loop (rows not 16-B aligned)."""
    case = CASES["softmax_rows:x" if cols == 1000 else "softmax_rows_strided:x"]
    _need(case.peak)
    n, rows = case.n, case.rows
    assert n * cols * 2 > lc.MARK32
    rows = sorted(set(rows) | set(lc.sample_rows(n, cols * 4)))  # y's marks and argmax's too
    x = _randn((n, cols), 17)
    y = _full((n + 1, cols), NAN, torch.float32)
    am = _full((n + 1,), -7, torch.int64)
    ops.softmax_rows(x, out=y[:n], argmax=am[:n])
    torch.cuda.synchronize()
    xs = x[_idx(rows)].cpu()
    want, _ = ops.softmax_rows(xs)
    lc.check_close(y[_idx(rows)].cpu(), want, rows, "softmax_rows")
    first = torch.where(xs == xs.max(1, keepdim=True).values, torch.arange(cols), cols).min(1).values
    assert torch.equal(am[_idx(rows)].cpu(), first)
    assert _all_nan(y[n:]) and int(am[n]) == -7


def test_sppf_pool_buf_past_4gib():
    case = CASES["sppf_pool:buf"]
    _need(case.peak)
    n, rows, C = case.n, case.rows, 16
    assert n * case.image_bytes > lc.MARK32
    buf = _randn((n, 8, 8, 4 * C), 18)
    buf[..., C:] = NAN
    x0 = buf[_idx(rows)][..., :C].cpu()
    ops.sppf_pool(buf, C)
    torch.cuda.synchronize()
    want = torch.full((len(rows), 8, 8, 4 * C), NAN, dtype=BF16)
    want[..., :C] = x0
    ops.sppf_pool(want, C)
    lc.check_exact(buf[_idx(rows)].cpu(), want, rows, "sppf_pool")
    assert _all(lambda c: ~torch.isnan(c), buf)  # every slice of every image written


# ---------------------------------------------------------------------------
# the stems: input just under the launcher's 0x7ffffff0 bytes, outputs past the marks
# ---------------------------------------------------------------------------
def _resnet_stem():
    import torch.nn as nn
    from kvedge_amd.models.layers import DeployedConv, fold_bn

    torch.manual_seed(5)
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    bn = nn.BatchNorm2d(64).eval()
    bn.running_mean.uniform_(-0.2, 0.2)
    bn.running_var.uniform_(0.5, 1.5)
    stem = DeployedConv.stem_s2d(conv, bn, ops.ACT_RELU)
    return stem, ops.pack_stem12(fold_bn(conv, bn)[0])


def _stem(case, x_all, out_shape, y_coff, run, op, bpp=3):
    """``x_all`` holds one image more than the launcher takes.  The largest accepted batch runs
    and is right on the sampled images (its last one among them); one image more is refused
    with the launcher's own code and leaves the poison alone."""
    n, rows = case.n, case.rows
    assert x_all.shape[0] == n + 1 and n - 1 in rows
    h, w = x_all.shape[1:3]
    assert lc.stem_accepts(n, h, w, bpp) and not lc.stem_accepts(n + 1, h, w, bpp)
    alloc = _full((n + 1, *out_shape), NAN, BF16)
    run(x_all[:n], alloc[:n])
    torch.cuda.synchronize()
    got = alloc[_idx(rows)].cpu()
    want = run(x_all[_idx(rows)].cpu(), None)
    lc.check_close(got[..., y_coff:y_coff + want.shape[3]], want, rows, op)
    lo, hi = alloc[:n][..., :y_coff], alloc[:n][..., y_coff + want.shape[3]:]
    assert (lo.numel() == 0 or _all_nan(lo)) and (hi.numel() == 0 or _all_nan(hi))
    assert _all_nan(alloc[n:])
    alloc.fill_(NAN)
    with pytest.raises(RuntimeError, match=op + r" failed rc=-(4|9)\b"):
        run(x_all, alloc)
    torch.cuda.synchronize()
    assert _all_nan(alloc)


def test_stem12_pool_frames_cap_and_y_past_4gib():
    case = CASES["stem12_pool_frames:y"]
    _need(case.peak)
    assert case.n == lc.stem_max_n(*lc.STEM12_HW) and case.bytes > lc.MARK32
    stem, w12 = _resnet_stem()

    def run(fr, out):
        dev = fr.device
        return ops.stem12_pool_frames(fr, w12.to(dev), stem.b.to(dev), out=out,
                                      y_coff=8 if out is not None else 0)

    _stem(case, _bytes((case.n + 1, *lc.STEM12_HW, 3), 19), (10, 5, lc.STEM_LDY), 8, run,
          "stem12_pool_frames")


def test_stem_pool_frames_cap_and_y_past_2gib():
    """The launcher counts 8 bytes a pixel (the space-to-depth image the frames stand for): at
    its cap the frames are 0.8 GB and y ends at 2.68 GB."""
    case = CASES["stem_pool_frames:y"]
    _need(case.peak)
    assert case.n == lc.stem_max_n(*lc.STEMF_HW, lc.STEMF_BPP)
    assert lc.MARK31 < case.bytes < lc.MARK32
    stem, _ = _resnet_stem()

    def run(fr, out):
        dev = fr.device
        return ops.stem_pool_frames(fr, stem.spec, stem.w.to(dev), stem.b.to(dev), out=out,
                                    y_coff=8 if out is not None else 0)

    _stem(case, _bytes((case.n + 1, *lc.STEMF_HW, 3), 20), (9, 5, lc.STEM_LDY), 8, run,
          "stem_pool_frames", lc.STEMF_BPP)


def test_stem_pool_cap_and_y_past_2gib():
    """160 output bytes for 128 input bytes: under the input cap y ends at 2.68 GB."""
    case = CASES["stem_pool:y"]
    _need(case.peak)
    assert case.n == lc.stem_max_n(*lc.STEM_S2D_HW, 32) and lc.MARK31 < case.bytes < lc.MARK32
    stem, _ = _resnet_stem()

    def run(x, out):
        dev = x.device
        return ops.stem_pool(x, stem.spec, stem.w.to(dev), stem.b.to(dev), out=out,
                             y_coff=8 if out is not None else 0)

    _stem(case, _randn((case.n + 1, *lc.STEM_S2D_HW, 16), 21), (3, 4, lc.STEM_LDY), 8, run,
          "stem_pool", 32)


def test_yolo_stem2_cap_and_y_past_2gib():
    """4 output bytes for 3 input bytes: under the input cap y ends at 2.86 GB."""
    from kvedge_amd.models.layers import DeployedConv
    from kvedge_amd.models.yolov8 import Conv

    case = CASES["yolo_stem2:y"]
    _need(case.peak)
    assert case.n == lc.stem_max_n(*lc.YOLO_HW) and lc.MARK31 < case.bytes < lc.MARK32
    torch.manual_seed(6)
    m0, m1 = Conv(3, 16, 3, 2).eval(), Conv(16, 32, 3, 2).eval()
    b0 = DeployedConv.stem_s2d(m0.conv, m0.bn, ops.ACT_SILU, "cpu", in_scale=1.0 / 255)
    b1 = DeployedConv.from_modules(m1.conv, m1.bn, ops.ACT_SILU, "cpu")

    def run(fr, out):
        d = fr.device
        return ops.yolo_stem2(fr, b0.spec, b0.w.to(d), b0.b.to(d), b1.spec, b1.w.to(d),
                              b1.b.to(d), out=out)

    _stem(case, _bytes((case.n + 1, *lc.YOLO_HW, 3), 22), (1, 8, 32), 0, run, "yolo_stem2")


# ---------------------------------------------------------------------------
# the image-in-the-grid caps: N <= 65535
# ---------------------------------------------------------------------------
CAP = lc.GRID_YZ_CAP


def test_frame_watch_cap():
    hw, rows = (8, 8), [0, CAP - 1]
    src = _bytes((CAP + 1, *hw, 3), 23)
    gpu = ops.WatchState(CAP + 1, hw, cell=8, device="cuda")
    _watch_steps(src[:CAP], gpu, ops.WatchState(2, hw, cell=8), rows, "frame_watch cap")
    before = gpu.buf.clone()
    stats = _full((CAP + 1, 16), lc.POISON_I32, torch.int32)
    mask = _full((CAP + 1, *gpu.grid), lc.POISON_U8, torch.uint8)
    assert not lc.grid_accepts(CAP + 1)
    with pytest.raises(RuntimeError, match="frame_watch"):
        ops.frame_watch(src, gpu, out_stats=stats, out_mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(gpu.buf, before)
    assert bool((stats == lc.POISON_I32).all()) and bool((mask == lc.POISON_U8).all())


def test_annotate_cap():
    h, w = 12, 20
    images = _bytes((CAP + 1, h, w, 3), 24)
    orig = images.clone()
    det = _boxes(1, 1, (h, w), 25).cuda().repeat(CAP + 1, 1, 1)
    count = torch.ones(CAP + 1, dtype=torch.int32, device="cuda")
    style = ops.AnnotateStyle(CAP + 1, device="cuda")
    ops.annotate(images[:CAP], style, det[:CAP], count[:CAP])
    torch.cuda.synchronize()
    rows = [0, CAP - 1]
    want = ops.annotate(orig[_idx(rows)].cpu(), ops.AnnotateStyle(2), det[:2].cpu(), count[:2].cpu())
    lc.check_exact(images[_idx(rows)].cpu(), want, rows, "annotate cap")
    assert not torch.equal(want, orig[_idx(rows)].cpu()) and torch.equal(images[CAP], orig[CAP])
    images.copy_(orig)
    with pytest.raises(RuntimeError, match="annotate"):
        ops.annotate(images, style, det, count)
    torch.cuda.synchronize()
    assert torch.equal(images, orig)


def test_jpeg_encode_cap():
    images = _jpeg_images(CAP + 1, (16, 16), 26)
    enc, out, length = _jpeg_check(images, CAP, [0, CAP - 1], 2048, "jpeg_encode cap")
    out.fill_(lc.POISON_U8)
    length.fill_(lc.POISON_I32)
    with pytest.raises(RuntimeError, match="jpeg_encode"):
        ops.jpeg_encode(images, enc, out=out, lengths=length)
    torch.cuda.synchronize()
    assert bool((out == lc.POISON_U8).all()) and bool((length == lc.POISON_I32).all())


def test_pooled_fc_cap():
    """The image is grid y of the head's one launch: 65535 run, 65536 are refused by the
    launcher with its own code (not by a failed launch)."""
    g = torch.Generator().manual_seed(27)
    x = _randn((CAP + 1, 2, 2, 64), 28)
    w = (torch.randn(24, 64, generator=g) * 0.1).to(BF16)
    bias = torch.randn(24, generator=g)
    out = _full((CAP + 1, 24), NAN, BF16)
    ops.pooled_fc(x[:CAP], w.cuda(), bias.cuda(), out=out[:CAP])
    torch.cuda.synchronize()
    rows = [0, CAP - 1]
    want = ops.pooled_fc(x[_idx(rows)].cpu(), w, bias)
    lc.check_close(out[_idx(rows)].cpu(), want, rows, "pooled_fc cap")
    assert not bool(torch.isnan(out[:CAP]).any()) and _all_nan(out[CAP:])
    out.fill_(NAN)
    with pytest.raises(RuntimeError, match=r"pooled_fc failed rc=-2\b"):
        ops.pooled_fc(x, w.cuda(), bias.cuda(), out=out)
    torch.cuda.synchronize()
    assert _all_nan(out)


def test_upsample2x_item_cap():
    """The item rule at its boundary: 2^31 - 2^21 - 1 source vectors of 16 bytes (34 GB in,
    137 GB out) run and are right on image 0, on the images around both marks of x and on the
    last one; one more is refused before any launch."""
    case = CASES["upsample2x_cap:x"]
    _need(case.peak)
    m = lc.UPSAMPLE_MAX_WORK
    assert case.n == m + 1 and lc.upsample_accepts(m) and not lc.upsample_accepts(m + 1)
    x = _randn((m + 1, 1, 1, 8), 29)
    y = _full((m + 1, 2, 2, 8), NAN, BF16)
    ops.upsample2x(x[:m], y[:m])
    torch.cuda.synchronize()
    rows = sorted(set(lc.sample_rows(m, 16)) | set(lc.sample_rows(m, 64)))
    xs = x[_idx(rows)].cpu()
    want = ops.upsample2x(xs, torch.empty(len(rows), 2, 2, 8, dtype=BF16))
    lc.check_exact(y[_idx(rows)].cpu(), want, rows, "upsample2x cap")
    assert _all(lambda c: ~torch.isnan(c), y[:m]) and _all_nan(y[m:])
    y.fill_(NAN)
    with pytest.raises(RuntimeError, match=r"upsample2x failed rc=-1\b"):
        ops.upsample2x(x, y)
    torch.cuda.synchronize()
    assert _all_nan(y)
