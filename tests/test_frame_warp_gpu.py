"""csrc/kernels/frame_warp.hip against ops.reference.frame_warp / view_to_source, byte for
byte, at the smallest shapes where it can go wrong: a quarter tile, tile tails in both axes,
several tiles; odd RGB sizes; per-camera meshes behind a slot offset; folded and minifying
meshes."""
import numpy as np
import pytest
import torch

from kvedge_amd import ops

pytestmark = pytest.mark.gpu

STREAMS, SLOT0, N = 5, 2, 3
SRC_HW = {"rgb": (37, 53), "nv12": (38, 54)}
DSTS = [(16, 16), (32, 48), (48, 80)]
MESHES = ["rot90", "perspective", "barrel", "random"]
CANARY = 0xA5


def _meshes(name, src_hw, dst_hw):
    """[STREAMS, Gy, Gx, 2]: a different mesh for every camera."""
    hs, ws = src_hw
    rng = np.random.default_rng(11)
    out = []
    for s in range(STREAMS):
        if name == "rot90":  # identity scale, shifted per camera; leaves the frame -> pad
            gy, gx = np.meshgrid(np.arange(dst_hw[0] // 16 + 1), np.arange(dst_hw[1] // 16 + 1),
                                 indexing="ij")
            m = np.stack([64 * ws - 1024 * gy + 37 * s, 1024 * gx - 21 * s], -1)
        elif name == "perspective":
            h = [[1.0, 0.05 * s, -2.0], [0.03, 1.0 + 0.1 * s, 1.0], [4e-4, 6e-4 * s, 1.0]]
            m = ops.view_mesh(src_hw, dst_hw, homography=h, fit="stretch")
        elif name == "barrel":  # the corners leave the frame
            lens = {"fx": ws * 0.6, "fy": ws * 0.6, "cx": ws / 2 + s, "cy": hs / 2 - s,
                    "k1": 0.5 + 0.2 * s, "k2": 0.1, "p1": 0.01, "p2": -0.02, "k3": 0.05}
            m = ops.view_mesh(src_hw, dst_hw, lens=lens)
        else:  # the full clamped range, a band around the frame, in-frame jitter: folded cells
            lo, hi = [(-(1 << 20), 1 << 20), (-600, 64 * ws + 600), (0, 64 * hs)][s % 3]
            m = rng.integers(lo, hi, (dst_hw[0] // 16 + 1, dst_hw[1] // 16 + 1, 2))
        out.append(np.asarray(m, dtype=np.int64))
    return out


def _frames(fmt, n, hw, seed=5):
    rng = np.random.default_rng(seed)
    shape = (n, hw[0] * 3 // 2, hw[1]) if fmt == "nv12" else (n, *hw, 3)
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))


def _both(meshes, src_hw, dst_hw):
    cpu, gpu = (ops.CameraViews(STREAMS, src_hw, dst_hw, device=d) for d in ("cpu", "cuda"))
    for s, m in enumerate(meshes):
        for v in (cpu, gpu):
            v.set(s, m, pad=10 + 40 * s)
    return cpu, gpu


def _warp(src, gpu_views, dst_hw, fmt):
    """The kernel's result, from a canary-backed buffer whose tail is checked."""
    nbytes = src.shape[0] * dst_hw[0] * dst_hw[1] * 3
    flat = torch.full((nbytes + 64,), CANARY, dtype=torch.uint8, device="cuda")
    out = flat[:nbytes].view(src.shape[0], *dst_hw, 3)
    ops.frame_warp(src.cuda(), gpu_views, out=out, slot0=SLOT0, src_format=fmt)
    assert (flat[nbytes:] == CANARY).all()
    return out.cpu()


@pytest.mark.parametrize("name", MESHES)
@pytest.mark.parametrize("dst_hw", DSTS)
@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_frame_warp_equals_reference(fmt, dst_hw, name):
    src_hw = SRC_HW[fmt]
    src = _frames(fmt, N, src_hw)
    cpu, gpu = _both(_meshes(name, src_hw, dst_hw), src_hw, dst_hw)
    want = ops.frame_warp(src, cpu, slot0=SLOT0, src_format=fmt)
    assert torch.equal(_warp(src, gpu, dst_hw, fmt), want)
    if name != "random":  # the views show the frame, not just padding
        assert (want != want[:, :1, :1]).any()


@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_minifying_mesh(fmt):
    """600 x 600 -> 16 x 16: one quarter tile whose taps span the whole frame, turned and
    mirrored per camera."""
    src = _frames(fmt, N, (600, 600), seed=6)
    meshes = [ops.view_mesh((600, 600), (16, 16), rotate=90 * (s % 4), mirror=bool(s & 1))
              for s in range(STREAMS)]
    cpu, gpu = _both(meshes, (600, 600), (16, 16))
    want = ops.frame_warp(src, cpu, slot0=SLOT0, src_format=fmt)
    assert torch.equal(_warp(src, gpu, (16, 16), fmt), want)


def test_view_to_source_equals_reference():
    src_hw, dst_hw = SRC_HW["rgb"], (48, 80)
    cpu, gpu = _both(_meshes("perspective", src_hw, dst_hw), src_hw, dst_hw)
    rng = np.random.default_rng(12)
    det = rng.uniform(-8, 90, (2, 150, 6)).astype(np.float32)  # inverted boxes included
    det[0, 3, 0], det[0, 4, 3], det[1, 5, 2], det[1, 6, 1] = np.nan, np.inf, -np.inf, 1e30
    det = torch.from_numpy(det)
    count = torch.tensor([150, 97], dtype=torch.int32)
    want = ops.view_to_source(det.clone(), count, cpu, slot0=SLOT0)
    got = ops.view_to_source(det.clone().cuda(), count.cuda(), gpu, slot0=SLOT0).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[1, 97:].view(torch.int32), det[1, 97:].view(torch.int32))
    assert not torch.equal(got[1, :97, :4], det[1, :97, :4])


@pytest.mark.parametrize("case,code", [("width", 1), ("extent", 2), ("mesh", 3), ("slots", 4),
                                       ("dst_align", 5), ("nv12_odd", 8)])
def test_launcher_refuses_and_writes_nothing(case, code):
    hd, wd, gy, gx, slot0, nv12 = 32, 32, 3, 3, SLOT0, False
    src = torch.zeros(N, 37, 53, 3, dtype=torch.uint8, device="cuda")
    if case == "width":
        wd = 24
    elif case == "extent":
        hd, gy = 8208, 514
    elif case == "mesh":
        gx = 4
    elif case == "slots":
        slot0 = STREAMS - N + 1
    elif case == "nv12_odd":
        src, nv12 = torch.zeros(N, 57, 53, dtype=torch.uint8, device="cuda"), True
    flat = torch.full((N * hd * wd * 3 + 4,), CANARY, dtype=torch.uint8, device="cuda")
    off = 1 if case == "dst_align" else 0
    dst = flat[off:off + N * hd * wd * 3].view(N, hd, wd, 3)
    mesh = torch.zeros(STREAMS, gy, gx, 2, dtype=torch.int32, device="cuda")
    pad = torch.zeros(STREAMS, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=rf"frame_warp failed rc=-{code}\b"):
        torch.ops.kvedge.frame_warp(src, dst, mesh, pad, slot0, nv12)
    assert (flat == CANARY).all()


def test_empty_batch_is_a_no_op():
    gpu = ops.CameraViews(STREAMS, (37, 53), (32, 32), device="cuda")
    out = ops.frame_warp(torch.zeros(0, 37, 53, 3, dtype=torch.uint8, device="cuda"), gpu)
    assert out.shape == (0, 32, 32, 3)


def test_engine_graph_views_and_live_update():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    src_hw, dst_hw = (96, 128), (640, 640)
    first = ops.view_mesh(src_hw, dst_hw, roi=(16, 8, 112, 88), rotate=180)
    other = ops.view_mesh(src_hw, dst_hw, rotate=90, mirror=True)
    cpu, gpu = (ops.CameraViews(2, src_hw, dst_hw, device=d) for d in ("cpu", "cuda"))
    cpu.set(1, first)
    gpu.set(1, first)
    y = KvYoloV8n(init_yolov8n(0), "cuda", conf=0.001)
    eng = InferenceEngine(y, 2, 640, device="cuda", seed=2, frame_hw=src_hw, views=gpu).prepare(
        warmup=1, autotune=False)
    assert eng.graph is not None
    for mesh in (first, other):  # the second replay of the same graph reads the new mesh
        cpu.set(1, mesh)
        gpu.set(1, mesh)
        det, count = eng.run()
        torch.cuda.synchronize()
        want = ops.frame_warp(eng.source_frames.cpu(), cpu)
        assert torch.equal(eng.frames.cpu(), want)
        live = torch.arange(det.shape[1]).view(1, -1, 1) < count.cpu().view(2, 1, 1)
        boxes = torch.where(live, det.cpu()[..., :4], torch.zeros(()))
        assert (boxes >= 0).all()  # frame pixels, through the mesh
        assert (boxes[..., 0::2] <= 128).all() and (boxes[..., 1::2] <= 96).all()
    assert not torch.equal(ops.frame_warp(eng.source_frames.cpu(), cpu.set(1, first)), want)
