"""Low-light enhancement on the CPU: the reference's own properties, the setters' ranges, the
engine running the reference, and the module's keys."""
import numpy as np
import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference


def _dark(n, h, w, seed=0, hi=21):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, hi, (n, h, w, 3), dtype=torch.uint8, generator=g)


@pytest.mark.parametrize("clip_q8", [256, 512, 16384])
@pytest.mark.parametrize("kind", ["dark", "constant", "full"])
def test_tile_table_is_monotone_ends_at_255_and_keeps_the_total(kind, clip_q8):
    g = np.random.default_rng(1)
    y = {"dark": g.integers(0, 21, 1000), "constant": np.full(777, 9),
         "full": g.integers(0, 256, 1000)}[kind]
    hist = np.bincount(y, minlength=256)
    lut, h = reference.enhance_tile_table(hist, clip_q8)
    assert int(h.sum()) == hist.sum() and h.min() >= 0
    assert (np.diff(lut.astype(int)) >= 0).all() and lut[255] == 255


@pytest.mark.parametrize("size,tiles", [(8, 1), (12, 2), (67, 8), (96, 16), (4096, 16)])
def test_axis_tables(size, tiles):
    t0, t1, w = reference.enhance_axis(size, tiles)
    assert t0.min() == 0 and t1.max() == tiles - 1 and ((t1 - t0) | 1).max() == 1
    assert w.min() >= 0 and w.max() <= 64 and (w[t0 == t1] == 0).all()
    pos = t0 * 64 + w  # the position between the tile centres never steps back
    assert (np.diff(pos) >= 0).all()


def test_alpha_zero_is_the_identity_and_a_dark_ramp_widens():
    ramp = (torch.arange(84) // 4).to(torch.uint8)[None, None, :, None].expand(2, 64, 84, 3)
    ramp = ramp.contiguous()
    enh = ops.FrameEnhance(2, (64, 84), tiles=(2, 2))
    # clip 64: no bin of the 21 is clipped, the tables equalise in full
    enh.set_mode("off", camera=0).set_mode("auto", camera=1).set_levels(24, 64).set_clip(64.0)
    out, stats = ops.frame_enhance(ramp, enh, out=torch.full_like(ramp, 7))
    assert torch.equal(out[0], ramp[0]) and stats[0].tolist() == [160, 0]
    assert stats[1].tolist() == [160, 256]  # mean luma 10 is below the dark level: in full
    y0, y1 = reference.watch_luma(ramp[1:]), reference.watch_luma(out[1:])
    assert int(y0.max() - y0.min()) == 20 and int(y1.max() - y1.min()) > 100
    c = out[1].to(torch.int32)  # R, G and B moved together: the chroma stays
    assert torch.equal(c[..., 0], c[..., 1]) and torch.equal(c[..., 1], c[..., 2])
    # between the levels auto scales the strength; above the bright level it is off
    enh.set_levels(5, 15, camera=1).set_strength(200, camera=1)
    assert ops.frame_enhance(ramp, enh, out=out)[1][1].tolist() == [160, 100]
    enh.set_levels(2, 9, camera=1)
    out2, stats = ops.frame_enhance(ramp.clone(), enh)
    assert stats[1].tolist() == [160, 0] and torch.equal(out2, ramp)


def test_setters_ranges_and_the_empty_tile_refusal():
    enh = ops.FrameEnhance(3, (40, 67))
    assert enh.params[:, :5].tolist() == [[1, 256, 512, 384, 1024]] * 3
    enh.set_mode("auto", camera=1).set_strength(77, 2).set_clip(64.0).set_levels(10, 11, 0)
    assert enh.params[:, :5].tolist() == [[1, 256, 16384, 160, 176], [2, 256, 16384, 384, 1024],
                                          [1, 77, 16384, 384, 1024]]
    for bad in (lambda: enh.set_mode("dim"), lambda: enh.set_mode(3), lambda: enh.set_strength(257),
                lambda: enh.set_strength(0.5), lambda: enh.set_clip(0.99),
                lambda: enh.set_clip(64.5), lambda: enh.set_levels(10, 10.9),
                lambda: enh.set_levels(-1, 20), lambda: enh.set_levels(200, 300),
                lambda: enh.set_mode("on", camera=3)):
        with pytest.raises(ValueError):
            bad()
    assert enh.params[0, :5].tolist() == [1, 256, 16384, 160, 176]  # a refused call stores nothing
    for hw, tiles in (((12, 20), (5, 1)), ((12, 20), (1, 17)), ((12, 20), (0, 1)),
                      ((12, 20), (2, 16)), ((4097, 8), (1, 1))):
        with pytest.raises(ValueError):
            ops.FrameEnhance(1, hw, tiles=tiles)
    with pytest.raises(ValueError):
        ops.frame_enhance(_dark(2, 40, 67), enh, slot0=2)
    # words outside their ranges are clamped, not trusted
    enh.params[0, :5] = torch.tensor([9, 999, 1, 5000, 0], dtype=torch.int32)
    assert reference.enhance_params(enh.params[0].tolist()) == (2, 256, 256, 4080, 4096)


def test_engine_on_cpu_runs_the_reference_and_fills_enhance_stats():
    from kvedge_amd.engine import InferenceEngine

    seen = []

    def model(frames):
        seen.append(frames.clone())
        return (frames.float().mean(dim=(1, 2, 3)),)

    f = _dark(2, 32, 32, seed=3)
    want, want_stats = ops.frame_enhance(f.clone(), ops.FrameEnhance(2, (32, 32)))
    enh = ops.FrameEnhance(2, (32, 32))
    eng = InferenceEngine(model, 2, 32, device="cpu", synthetic=False, enhance=enh)
    eng.set_frames(f)
    eng.set_frames(f)  # fed once, served twice: the fed input is not enhanced again
    assert torch.equal(eng.frames, f) and torch.equal(seen[0], want) and torch.equal(seen[1], want)
    assert torch.equal(eng.enhance_stats, want_stats) and int(want_stats[0, 1]) == 256
    model.frame_plan = ops.letterbox_plan  # served from 24 x 40 frames: in place on the resize
    eng = InferenceEngine(model, 2, 32, device="cpu", synthetic=False, frame_hw=(24, 40),
                          enhance=enh)
    src = _dark(2, 24, 40, seed=4)
    eng.set_frames(src)
    small = ops.frame_resize(src, ops.letterbox_plan((24, 40), 32))
    assert torch.equal(seen[2], ops.frame_enhance(small, enh)[0]) and torch.equal(seen[2], eng.frames)
    for bad in (ops.FrameEnhance(3, (32, 32)), ops.FrameEnhance(2, (32, 64))):
        with pytest.raises(ValueError):
            InferenceEngine(model, 2, 32, device="cpu", enhance=bad)
    with pytest.raises(TypeError):
        InferenceEngine(model, 2, 32, device="cpu", enhance=object())


def test_module_keys_live_words_and_rebuild():
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    d = ModuleConfig()
    assert not set(ModuleConfig.ENHANCE_KEYS) & set(d.to_dict())
    c = d.apply_patch({"enhance": "true", "enhance_mode": "on", "enhance_strength": "0.5"})
    assert c.enhance and c.needs_rebuild(d) and c.to_dict()["enhance_strength"] == 0.5
    for k, v in (("enhance_mode", "auto"), ("enhance_strength", 1.0), ("enhance_clip", 4.0),
                 ("enhance_dark_level", 30.0), ("enhance_bright_level", 90.0)):
        assert not c.needs_rebuild(c.apply_patch({k: v}))
    for bad in ({"enhance_mode": "off"}, {"enhance_strength": 1.5}, {"enhance_clip": 0.5},
                {"enhance_bright_level": 24.5}, {"enhance": True, "model": "simulated-temperature"}):
        with pytest.raises(ValueError):
            d.apply_patch(bad)
    tr = FakeTransport({"model": "yolov8n", "batch": 2, "image_size": 64, "max_det": 8,
                        "report_interval_s": 1.0, "enhance": True, "enhance_mode": "on"})
    with ModuleApp(tr, device="cpu").start() as app:
        app.run(max_steps=1)
        assert app.report()["enhanced"] == 2
        engine = app.engine
        assert app.enhance.params[:, :5].tolist() == [[1, 256, 512, 384, 1024]] * 2
        status, _ = app._apply_patch({"enhance_mode": "auto", "enhance_strength": 0.25,
                                      "enhance_clip": 3.0, "enhance_dark_level": 20,
                                      "enhance_bright_level": 40})
        assert status == 200 and app.engine is engine  # no rebuild: the same captured step
        assert app.enhance.params[:, :5].tolist() == [[2, 64, 768, 320, 640]] * 2
        app.run(max_steps=1)
        assert app.report()["enhanced"] == 0  # synthetic frames are mid-grey noise: not dark
        assert app._apply_patch({"enhance": False})[0] == 200
        assert app.engine is not engine and app.enhance is None
        assert "enhanced" not in app.report()
