"""Per-camera views on the CPU: the warp's sampling rule (ops.reference.frame_warp) against
things that are not the rule -- numpy rotations, frame_resize, hand-computed boxes."""
import numpy as np
import pytest
import torch

from kvedge_amd import ops

HS, WS = 32, 48


def _grid(hd, wd, step=16):
    """Nodes 64 * step * g: destination pixel (dx, dy) samples source position step * (dx, dy)."""
    gy, gx = np.meshgrid(np.arange(hd // 16 + 1), np.arange(wd // 16 + 1), indexing="ij")
    return np.stack([gx, gy], -1).astype(np.int64) * 64 * step


def _views(mesh, src_hw, pad=114, streams=1):
    hd, wd = (mesh.shape[0] - 1) * 16, (mesh.shape[1] - 1) * 16
    v = ops.CameraViews(streams, src_hw, (hd, wd))
    for s in range(streams):
        v.set(s, mesh, pad)
    return v


@pytest.fixture(scope="module")
def src():
    rng = np.random.default_rng(7)
    return torch.from_numpy(rng.integers(0, 256, (1, HS, WS, 3), dtype=np.uint8))


def test_identity_mesh_is_the_source(src):
    assert torch.equal(ops.frame_warp(src, _views(_grid(HS, WS), (HS, WS))), src)


@pytest.mark.parametrize("name", ["rot90", "rot180", "rot270", "mirror"])
def test_swapped_and_reversed_meshes_are_exact_rotations(src, name):
    s = src[0].numpy()
    g, gv = _grid(HS, WS), _grid(WS, HS)  # nodes of a 32 x 48 view and of a 48 x 32 one
    mesh, want, kwargs = {
        # np.rot90: out[i, j] = src[j, W - 1 - i]: view point (xv, yv) samples (W - yv, xv)
        "rot90": (np.stack([64 * WS - gv[..., 1], gv[..., 0]], -1), np.rot90(s, 1),
                  {"rotate": 90}),
        "rot180": (np.stack([64 * WS - g[..., 0], 64 * HS - g[..., 1]], -1), np.rot90(s, 2),
                   {"rotate": 180}),
        "rot270": (np.stack([gv[..., 1], 64 * HS - gv[..., 0]], -1), np.rot90(s, 3),
                   {"rotate": 270}),
        "mirror": (np.stack([64 * WS - g[..., 0], g[..., 1]], -1), np.flip(s, 1),
                   {"mirror": True}),
    }[name]
    got = ops.frame_warp(src, _views(mesh, (HS, WS)))[0].numpy()
    assert np.array_equal(got, want)
    # and the builder's convention is numpy's
    assert np.array_equal(ops.view_mesh((HS, WS), want.shape[:2], **kwargs), mesh)


def test_double_step_mesh_is_the_2x2_mean_of_frame_resize(src):
    s = src[:, :, :32].contiguous()  # 32 x 32 -> 16 x 16, S = 2 R
    plan = ops.ResizePlan((32, 16, 0, 0, 16), (32, 16, 0, 0, 16), 0, (32, 32), (16, 16))
    got = ops.frame_warp(s, _views(_grid(16, 16, 32), (32, 32)))
    assert torch.equal(got, ops.frame_resize(s, plan))
    mean = (s.long().view(1, 16, 2, 16, 2, 3).sum((2, 4)) + 2) >> 2
    assert torch.equal(got.long(), mean)


def test_mesh_outside_the_frame_is_all_pad(src):
    mesh = _grid(16, 16) + 64 * 1000
    assert torch.equal(ops.frame_warp(src, _views(mesh, (HS, WS), pad=9)),
                       torch.full((1, 16, 16, 3), 9, dtype=torch.uint8))
    assert (ops.frame_warp(src, _views(-mesh - 1, (HS, WS), pad=200)) == 200).all()


def test_nv12_equals_the_rgb_warp_of_the_converted_frame():
    rng = np.random.default_rng(8)
    nv = torch.from_numpy(rng.integers(0, 256, (2, HS * 3 // 2, WS), dtype=np.uint8))
    views = ops.CameraViews(2, (HS, WS), (32, 32))
    views.set(1, ops.view_mesh((HS, WS), (32, 32), roi=(5, 3, 41, 30), rotate=90, mirror=True), 0)
    assert torch.equal(ops.frame_warp(nv, views, src_format="nv12"),
                       ops.frame_warp(ops.nv12_to_rgb(nv), views))


@pytest.mark.parametrize("src_hw,fit", [((96, 48), "letterbox"), ((48, 96), "letterbox"),
                                        ((64, 64), "letterbox"), ((64, 128), "stretch")])
def test_plain_view_mesh_equals_frame_resize(src_hw, fit):
    """Integer scale ratios in both axes (a 96 x 64 frame letterboxes to 32 x 21 content, a
    ratio of 64 / 21 that 1/64-pixel nodes cannot hold), so the affine mesh is exact."""
    rng = np.random.default_rng(9)
    s = torch.from_numpy(rng.integers(0, 256, (1, *src_hw, 3), dtype=np.uint8))
    if fit == "letterbox":
        plan = ops.letterbox_plan(src_hw, 32)
    else:
        plan = ops.ResizePlan((64, 32, 0, 0, 32), (128, 32, 0, 0, 32), 0, src_hw, (32, 32))
    views = ops.CameraViews(1, src_hw, (32, 32), fit=fit)
    assert torch.equal(ops.frame_warp(s, views), ops.frame_resize(s, plan))


def test_crop_fit_follows_center_crop_plan():
    plan = ops.center_crop_plan((512, 1024), 224)  # 256 x 512 resized, crop offsets 16 / 144
    mesh = ops.view_mesh((512, 1024), (224, 224), fit="crop")
    assert mesh[0, 0].tolist() == [64 * 144 * 2, 64 * 16 * 2]
    assert mesh[-1, -1].tolist() == [64 * (144 + 224) * 2, 64 * (16 + 224) * 2]
    assert plan.axis_x[1:3] == (512, 144) and plan.axis_y[1:3] == (256, 16)


def test_view_to_source_roi_rot90_by_hand():
    # roi 40 x 32 at (8, 4) turned counter-clockwise: the view is 32 wide, 40 high and fills
    # 32 x 48 from row 4 at scale 1.  View point (xv, yv) is source (8 + 40 - (yv - 4), 4 + xv).
    views = ops.CameraViews(2, (64, 64), (48, 32))
    views.set_view(1, {"roi": [8, 4, 48, 36], "rotate": 90})
    det = torch.zeros(1, 4, 6)
    det[0, 0] = torch.tensor([2.0, 10.0, 12.0, 30.0, 0.75, 3.0])
    det[0, 1] = torch.tensor([float("nan"), 44.0, 40.0, float("inf"), 0.5, 1.0])
    det[0, 2] = torch.tensor([1.0, 2.0, 3.0, 4.0, 0.25, 7.0])
    before = det.clone()
    ops.view_to_source(det, torch.tensor([2], dtype=torch.int32), views, slot0=1)
    # x: 48 - (30 - 4) .. 48 - (10 - 4); y: 4 + 2 .. 4 + 12
    assert det[0, 0].tolist() == [22.0, 6.0, 42.0, 16.0, 0.75, 3.0]
    # NaN -> 0, 40 -> the view's 32, inf -> the view's 48: x 48 - (48 - 4) .. 48 - (44 - 4),
    # y 4 + 0 .. 4 + 32
    assert det[0, 1].tolist() == [4.0, 4.0, 8.0, 36.0, 0.5, 1.0]
    assert torch.equal(det[0, 2:], before[0, 2:])


@pytest.mark.parametrize("kwargs", [
    {"roi": (10, 4, 10, 20)}, {"roi": (1, 2, 3)}, {"rotate": 45}, {"rotate": True},
    {"homography": [[1, 2, 3], [2, 4, 6], [0, 0, 1]]}, {"homography": [[1, 0], [0, 1]]},
    {"homography": [[1, 0, 0], [0, 1, 0], [0, 0, -1]]}, {"fit": "pad"},
    {"lens": {"fx": 0, "fy": 1}}, {"lens": {"fx": 1, "fy": 1, "k9": 0.1}},
    {"lens": {"fisheye": {"f": 10, "cx": 1, "cy": 1, "fov": 180}}}])
def test_view_mesh_refuses(kwargs):
    with pytest.raises(ValueError):
        ops.view_mesh((HS, WS), (32, 32), **kwargs)


def test_views_refuse():
    with pytest.raises(ValueError):
        ops.view_mesh((HS, WS), (30, 32))
    views = ops.CameraViews(2, (HS, WS), (32, 32))
    for bad in (lambda: views.set(2, _grid(32, 32)), lambda: views.set(0, _grid(16, 32)),
                lambda: views.set(0, _grid(32, 32), pad=256),
                lambda: views.set(0, _grid(32, 32).astype(np.float32)),
                lambda: views.set_view(0, {"zoom": 2}), lambda: views.set_view(0, {"pad": -1}),
                lambda: ops.frame_warp(torch.zeros(3, HS, WS, 3, dtype=torch.uint8), views),
                lambda: ops.frame_warp(torch.zeros(1, HS, WS + 2, 3, dtype=torch.uint8), views)):
        with pytest.raises(ValueError):
            bad()
    views.set(0, np.full((3, 3, 2), 1 << 40))  # clamped, not wrapped
    assert views.mesh[0].max().item() == views.mesh[0].min().item() == (1 << 20) - 1


def test_module_views_are_live():
    """The twin's ``views`` reach the device meshes of the running engine: new frames, boxes
    in frame pixels, no rebuild; a bad entry rejects the patch."""
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "yolov8n", "batch": 2, "image_size": 64, "conf": 0.0,
                        "max_det": 8, "frame_height": 48, "frame_width": 64,
                        "views": [None, {"rotate": 180}]})
    with ModuleApp(tr, device="cpu").start() as app:
        app.step()
        plain = ops.frame_resize(app.engine.source_frames, ops.letterbox_plan((48, 64), 64))
        assert torch.equal(app.engine.frames[0], plain[0])
        assert torch.equal(app.engine.frames[1], plain[1].flip(0, 1))
        rebuilds, engine = app.state["rebuilds"], app.engine
        tr.push_twin_patch({"views": [{"mirror": True}]})
        app.step()
        app.step()
        assert app.state["rebuilds"] == rebuilds and app.engine is engine
        plain = ops.frame_resize(app.engine.source_frames, ops.letterbox_plan((48, 64), 64))
        assert torch.equal(app.engine.frames[0], plain[0].flip(1))
        assert torch.equal(app.engine.frames[1], plain[1])
        det = app.engine.outputs[0][..., :4]
        assert det.min() >= 0 and det[..., 0::2].max() <= 64 and det[..., 1::2].max() <= 48
        tr.push_twin_patch({"views": [{"rotate": 30}]})
        app.step()
        assert app.state["rejected_patches"] == 1 and app.cfg.views == ({"mirror": True},)
