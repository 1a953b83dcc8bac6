"""NV12 camera frames on the MI355X: the NV12 resize and ROI-crop kernels against the CPU
composition reference(nv12_to_rgb) -> reference resample (byte for byte), every (Y, U, V)
triple through the device conversion, the launchers' rejections, the engine resampling NV12
frames inside its hipGraph, the cascade cutting its crops from them, and the module serving
``camera-nv12`` from the pinned ring through the native loop."""
import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.ops import reference

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes kept 0xCD on either side of the destination
NAN, INF = float("nan"), float("inf")
# the hand-written boxes (x1, y1, x2, y2) of tests/test_roi_crop_gpu.py, written for a 36 x 64
# frame, plus three whose window origin / extent parity decides which chroma cells are read
TABLE = [
    (10.3, 5.7, 20.2, 15.1),      # fractional
    (12.0, 8.0, 12.0, 8.0),       # zero area
    (30.0, 20.0, 10.0, 5.0),      # inverted
    (-5.5, -3.0, 7.5, 4.0),       # negative corner
    (50.0, 30.0, 100.0, 90.0),    # reaches beyond the frame
    (70.0, 40.0, 80.0, 50.0),     # wholly beyond the frame
    (NAN, NAN, NAN, NAN),
    (NAN, 4.0, 20.0, NAN),
    (-INF, -INF, INF, INF),
    (INF, INF, -INF, -INF),
    (60.0, 32.0, 64.0, 36.0),     # touches the right and bottom edge of 36 x 64
    (11.0, 7.0, 12.0, 8.0),       # 1 x 1 at an odd origin
    (11.0, 7.0, 20.0, 16.0),      # odd origin, odd extent
    (10.0, 6.0, 13.0, 9.0),       # even origin, odd extent
]


def _nv12(n, hs, ws, seed=0):
    return torch.randint(0, 256, (n, hs * 3 // 2, ws), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed))


def _guarded(shape):
    nbytes = 1
    for s in shape:
        nbytes *= s
    buf = torch.full((GUARD + nbytes + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes].view(*shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == 0xCD).all()) and bool((buf[-GUARD:] == 0xCD).all())


# ---------------------------------------------------------------- resize
RESIZE_CASES = [
    (3, (36, 64), 32, "letterbox"),
    (3, (64, 36), 32, "letterbox"),
    (3, (18, 22), 32, "letterbox"),   # upscale
    (3, (2, 2), 32, "letterbox"),     # one chroma cell, all clamps
    (3, (32, 32), 32, "letterbox"),   # identity
    (3, (50, 40), 32, "crop"),
    (3, (36, 64), 32, "crop"),
    (1, (1080, 1920), 640, "letterbox"),
    (1, (720, 1280), 224, "crop"),
]


@pytest.mark.parametrize("n,src_hw,dst,form", RESIZE_CASES)
def test_frame_resize_nv12_equals_cpu_reference(n, src_hw, dst, form):
    assert ops.load()
    plan = (ops.letterbox_plan if form == "letterbox" else ops.center_crop_plan)(src_hw, dst)
    big = _nv12(n + 2, *src_hw, seed=dst + src_hw[0])
    src_cpu = big[1:1 + n]
    rgb = reference.nv12_to_rgb(src_cpu)
    want = torch.empty(n, dst, dst, 3, dtype=torch.uint8)
    reference.frame_resize(rgb, plan, want)
    # source: a slice of a larger batch (non-zero storage offset, as the stream slices are);
    # destination: carved out of a larger 0xCD-filled allocation
    src = big.cuda()[1:1 + n]
    assert src.storage_offset() > 0 and src.is_contiguous()
    buf, out = _guarded((n, dst, dst, 3))
    got = ops.frame_resize(src, plan, out=out, src_format="nv12")
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu(), want)
    assert _guards_intact(buf)
    if form == "letterbox" and src_hw == (32, 32):
        assert torch.equal(out.cpu(), rgb)


def all_triples_nv12():
    """One 4096 x 4096 NV12 frame holding every (Y, U, V) triple once (the layout of
    tests/test_frame_nv12_cpu.py, which also checks it): (U, V) pair p = U * 256 + V owns the
    64 chroma cells at cell row p // 32, cell columns (p % 32) * 64 .. + 63, whose 256 pixels
    carry Y = 0 .. 255."""
    p = torch.arange(65536)
    cell_uv = torch.stack([p // 256, p % 256], dim=-1).to(torch.uint8)
    uv = cell_uv.view(2048, 32, 1, 2).expand(2048, 32, 64, 2).reshape(2048, 4096)
    c, dy, dx = torch.arange(64).view(1, 64, 1), torch.arange(2).view(2, 1, 1), torch.arange(2)
    yy = (c * 4 + dy * 2 + dx).reshape(2, 128).to(torch.uint8)
    y = yy.view(1, 2, 1, 128).expand(2048, 2, 32, 128).reshape(4096, 4096)
    return torch.cat([y, uv], dim=0).unsqueeze(0).contiguous()


def test_every_yuv_triple_through_the_device_conversion():
    assert ops.load()
    f = all_triples_nv12()
    want = reference.nv12_to_rgb(f)
    plan = ops.letterbox_plan((4096, 4096), 4096)  # the identity: every weight is 0
    got = ops.frame_resize(f.cuda(), plan, src_format="nv12")
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)


# ---------------------------------------------------------------- ROI crop
def _boxes(n, max_det, hs, ws, seed, shift):
    """det [n, max_det, 6]: the table, then seeded random boxes (some reaching past the frame,
    a few touching its right / bottom edge), rotated by ``shift`` rows so that every table row
    lands in a kept slot in one of the runs."""
    g = torch.Generator().manual_seed(seed)
    rows = n * max_det
    lo = torch.rand(rows, 2, generator=g) * torch.tensor([ws, hs]) * 1.1 - 0.05 * ws
    ext = torch.rand(rows, 2, generator=g) * torch.tensor([ws, hs]) * 0.8
    rnd = torch.cat([lo, lo + ext], dim=1)
    rnd[::5, 2], rnd[::5, 3] = float(ws), float(hs)
    tab = torch.tensor(TABLE, dtype=torch.float32)
    box = torch.cat([tab, rnd])[:max(rows, len(TABLE))].roll(shift, 0)[:rows]
    det = torch.cat([box, torch.rand(rows, 2, generator=g)], dim=1)
    return det.view(n, max_det, 6).contiguous()


def _crop_guarded(src, det, count, k, d, pad, band=0):
    buf, out = _guarded((src.shape[0] * k, d, d, 3))
    got = ops.roi_crop(src, det, count, k, d, pad=pad, out=out, band=band, src_format="nv12")
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert _guards_intact(buf)
    return out.cpu()


# kept slots are rows 8, 9 and 16..19 of the 24: these four rotations put every table row into
# one of them (checked below)
SHIFTS = (16, 12, 8, 4)
ROI_CASES = [
    (3, (36, 64), 32, [0, 2, 8], SHIFTS),
    (3, (18, 22), 32, [0, 2, 8], SHIFTS),    # upscaling
    (3, (2, 2), 32, [0, 2, 8], SHIFTS),      # one chroma cell, every box clamps to it
    (1, (1080, 1920), 224, [3], (0,)),
]


def test_rotations_put_every_table_row_into_a_kept_slot():
    kept = {8, 9, 16, 17, 18, 19}
    assert all(any((t + s) % 24 in kept for s in SHIFTS) for t in range(len(TABLE)))


@pytest.mark.parametrize("n,src_hw,d,counts,shifts", ROI_CASES)
def test_roi_crop_nv12_equals_cpu_reference(n, src_hw, d, counts, shifts):
    assert ops.load()
    k, max_det, pad = 4, 8, 114
    hs, ws = src_hw
    big = _nv12(n + 2, hs, ws, seed=d + hs)
    rgb = reference.nv12_to_rgb(big[1:1 + n])
    src = big.cuda()[1:1 + n]
    assert src.storage_offset() > 0 and src.is_contiguous()
    count = torch.tensor(counts, dtype=torch.int32)
    for shift in shifts:
        det = _boxes(n, max_det, hs, ws, seed=hs + shift, shift=shift)
        if hs == 1080:  # a window of several hundred pixels (odd origin) and the full frame
            det[0, 1, :4] = torch.tensor([201.5, 101.25, 1500.0, 1079.5])
            det[0, 2, :4] = torch.tensor([0.0, 0.0, 1920.0, 1080.0])
        want = torch.empty(n * k, d, d, 3, dtype=torch.uint8)
        reference.roi_crop(rgb, det, count, k, d, pad, want)
        got = _crop_guarded(src, det.cuda(), count.cuda(), k, d, pad)
        assert torch.equal(got, want), (src_hw, shift)
        # slots at or past count: all pad, no 0xCD left anywhere
        got = got.view(n, k, d, d, 3)
        for i, c in enumerate(counts):
            assert (got[i, min(c, k):] == pad).all()
    # every instantiated band height computes the same crops
    for band in (4, 8, 16, 32):
        assert torch.equal(_crop_guarded(src, det.cuda(), count.cuda(), k, d, pad, band=band),
                           want), band


def test_roi_crop_nv12_full_frame_box_equals_frame_resize_nv12():
    assert ops.load()
    hs, ws, d = 36, 64, 32
    src = _nv12(2, hs, ws, seed=7).cuda()
    det = torch.zeros(2, 3, 6)
    det[..., 2], det[..., 3] = ws, hs
    count = torch.tensor([3, 1], dtype=torch.int32)
    out = ops.roi_crop(src, det.cuda(), count.cuda(), 2, d, pad=9, src_format="nv12")
    plan = ops.ResizePlan((hs, d, 0, 0, d), (ws, d, 0, 0, d), 9, (hs, ws), (d, d))
    want = ops.frame_resize(src, plan, src_format="nv12")
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[0])
    assert torch.equal(out[2], want[1]) and (out[3] == 9).all()


# ---------------------------------------------------------------- launchers
def test_nv12_launchers_reject_bad_input():
    assert ops.load()
    fr, rc = torch.ops.kvedge.frame_resize_nv12, torch.ops.kvedge.roi_crop_nv12
    src = _nv12(2, 36, 64).cuda()
    ok_y, ok_x = [36, 18, 0, 7, 18], [64, 32, 0, 0, 32]
    det = _boxes(2, 8, 36, 64, seed=1, shift=0).cuda()
    count = torch.tensor([8, 8], dtype=torch.int32).cuda()

    def dst(n, h, w):
        return torch.full((n, h, w, 3), 0xCD, dtype=torch.uint8, device="cuda")

    def u8(*shape):
        return torch.zeros(*shape, dtype=torch.uint8, device="cuda")

    def valid():
        a, b = dst(2, 32, 32), dst(8, 32, 32)
        fr(src, a, ok_y, ok_x, 114)
        rc(src, det, count, b, 0)
        torch.cuda.synchronize()
        assert not (a == 0xCD).all() and not (b == 0xCD).all()

    valid()
    # an odd source address: a one-byte-offset view of a larger allocation
    odd = u8(2 * 54 * 64 + 2)[1:1 + 2 * 54 * 64].view(2, 54, 64)
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    bad_resize = [
        (u8(2, 52, 64), dst(2, 32, 32), [35, 18, 0, 7, 18], ok_x),           # odd Hs
        (u8(2, 54, 62)[:, :, :61].contiguous(), dst(2, 32, 32), ok_y,
         [61, 32, 0, 0, 32]),                                                # odd Ws
        (src, dst(2, 32, 30), ok_y, [64, 30, 0, 0, 30]),                     # Wd % 4 != 0
        (u8(2, 36, 64), dst(2, 32, 32), ok_y, ok_x),                         # plane != Hs * 3 / 2
        (u8(2, 56, 64), dst(2, 32, 32), ok_y, ok_x),
        (src.cpu(), dst(2, 32, 32), ok_y, ok_x),                             # a CPU tensor
        (odd, dst(2, 32, 32), ok_y, ok_x),                                   # odd source address
    ]
    for i, (s, d, ay, ax) in enumerate(bad_resize):
        with pytest.raises(RuntimeError):
            fr(s, d, ay, ax, 114)
        torch.cuda.synchronize()
        assert (d == 0xCD).all(), i
    bad_crop = [
        (u8(2, 52, 64), dst(8, 32, 32)),                                     # no even Hs: 52 rows
        (u8(2, 54, 62)[:, :, :61].contiguous(), dst(8, 32, 32)),             # odd Ws
        (src, dst(8, 30, 30)),                                               # D % 4 != 0
        (u8(2, 36, 64, 3), dst(8, 32, 32)),                                  # an RGB batch
        (src.cpu(), dst(8, 32, 32)),                                         # a CPU tensor
        (odd, dst(8, 32, 32)),                                               # odd source address
    ]
    for i, (s, d) in enumerate(bad_crop):
        with pytest.raises(RuntimeError):
            rc(s, det, count, d, 0)
        torch.cuda.synchronize()
        assert (d == 0xCD).all(), i
    with pytest.raises(RuntimeError):  # a band height that is not instantiated
        torch.ops.kvedge.roi_crop_nv12_band(src, det, count, dst(8, 32, 32), 0, 5)
    valid()


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def resnet():
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50

    assert ops.load()
    return KvResNet50(init_resnet50(seed=0), "cuda")


@pytest.fixture(scope="module")
def yolo():
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    return KvYoloV8n(init_yolov8n(0), "cuda", conf=0.0, max_det=8)


@pytest.mark.parametrize("batch,streams", [(2, 1), (4, 2)])
def test_engine_graph_resnet_nv12_frames(resnet, batch, streams):
    from kvedge_amd.engine import InferenceEngine

    eng = InferenceEngine(resnet, batch, 224, device="cuda", seed=5, streams=streams,
                          frame_hw=(96, 128), frame_format="nv12").prepare(warmup=1,
                                                                           autotune=False)
    assert eng.graph is not None and eng.source_frames.shape == (batch, 144, 128)
    assert eng.input_frames is eng.source_frames
    for _ in range(2):  # the generator advances inside the graph
        probs, top1 = eng.run()
    torch.cuda.synchronize()
    src = eng.source_frames.clone()
    want = torch.empty(batch, 224, 224, 3, dtype=torch.uint8)
    reference.frame_resize(reference.nv12_to_rgb(src.cpu()), eng.frame_plan, want)
    assert torch.equal(eng.frames.cpu(), want)  # every slice resized
    per = batch // streams
    parts = [resnet(ops.frame_resize(src[i * per:(i + 1) * per], eng.frame_plan,
                                     src_format="nv12")) for i in range(streams)]
    torch.cuda.synchronize()
    assert torch.equal(probs, torch.cat([p[0] for p in parts]))
    assert torch.equal(top1, torch.cat([p[1] for p in parts]))


def test_engine_graph_yolo_nv12_equals_rgb_path(yolo):
    from kvedge_amd.engine import InferenceEngine

    eng = InferenceEngine(yolo, 2, 640, device="cuda", seed=2, frame_hw=(120, 160),
                          frame_format="nv12").prepare(warmup=1, autotune=False)
    assert eng.graph is not None and eng.source_frames.shape == (2, 180, 160)
    det, count = eng.run()
    torch.cuda.synchronize()
    src = eng.source_frames.clone()
    rgb_eng = InferenceEngine(yolo, 2, 640, device="cuda", synthetic=False, use_graph=False,
                              frame_hw=(120, 160))
    ref_det, ref_count = rgb_eng.set_frames(ops.nv12_to_rgb(src))
    torch.cuda.synchronize()
    print(f"yolo NV12 counts: {count.tolist()}")
    assert torch.equal(eng.frames, rgb_eng.frames)
    assert int(count.min()) > 0
    assert torch.equal(count, ref_count) and torch.equal(det, ref_det)


def test_engine_graph_cascade_nv12_equals_rgb_from_source(yolo, resnet):
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.cascade import KvDetectClassify

    m = KvDetectClassify(yolo, resnet, 2)
    eng = InferenceEngine(m, 2, 640, device="cuda", seed=5, frame_hw=(120, 160),
                          frame_format="nv12").prepare(warmup=1, autotune=False)
    assert eng.graph is not None
    got = eng.run()
    torch.cuda.synchronize()
    rgb = ops.nv12_to_rgb(eng.source_frames.clone())
    want = m.from_source(rgb, ops.frame_resize(rgb, eng.frame_plan), eng.frame_plan)
    torch.cuda.synchronize()
    print(f"cascade NV12 counts: {got[1].tolist()}")
    assert int(got[1].min()) >= 2  # every slot holds a real detection
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert (got[2] >= 0).all() and (got[3] > 0).all()


# ---------------------------------------------------------------- module
def test_module_native_serving_camera_nv12():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "resnet50", "batch": 8, "report_interval_s": 0.01,
                        "source": "camera-nv12", "steps_per_poll": 4, "frame_height": 120,
                        "frame_width": 160})
    # a failed assertion must still stop the camera thread: context manager
    with ModuleApp(tr, device="cuda").start() as app:
        assert app.engine.graph is not None
        assert app.engine.source_frames.shape == (8, 180, 160)
        assert app.ring.pinned and app.ring.slot_bytes == 8 * 120 * 160 * 3 // 2
        app.run(max_steps=3)
        app.report()
        t = tr.outputs("telemetry")[-1]
        assert t["source"] == "camera-nv12" and t["images_per_s"] > 0
        assert app.state["total_images"] == 3 * 4 * 8
        torch.cuda.synchronize()
        # the graph resampled a camera batch that the ring DMA put into source_frames
        src = app.engine.source_frames.cpu()
        assert any(torch.equal(src, f) for f in app.camera.frames)
        want = torch.empty(8, 224, 224, 3, dtype=torch.uint8)
        reference.frame_resize(reference.nv12_to_rgb(src), app.engine.frame_plan, want)
        assert torch.equal(app.engine.frames.cpu(), want)
        assert tr.reported["config"]["source"] == "camera-nv12"
