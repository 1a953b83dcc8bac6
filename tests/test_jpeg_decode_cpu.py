"""The JPEG decoder, CPU tier: the reference against Pillow's decoder (libjpeg-turbo: slow
integer IDCT, fancy upsampling -- byte equality is the target and, as measured, holds for every
sampling), the ``camera-jpeg`` twin value and the engine / module plumbing on the reference
path."""
import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_decode_cases as dc
from kvedge_amd import ops
from kvedge_amd.module.config import ModuleConfig
from kvedge_amd.ops import reference as ref


def _max_diff(data, hw):
    rgb, status, _ = dc.reference([data], hw)
    assert status.tolist() == [0]
    return int(np.abs(rgb[0].astype(int) - dc.pillow_decode(data).astype(int)).max())


@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimised"])
@pytest.mark.parametrize("dri", ["none", "row", "3"])
@pytest.mark.parametrize("sub", dc.SUBS)
@pytest.mark.parametrize("hw", [(16, 16), (40, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_equals_pillow(hw, sub, dri, optimize):
    d = _max_diff(dc.pillow_file("noise", *hw, sub, dri, 95 if optimize else 75, optimize), hw)
    print(f"max |reference - Pillow| = {d}")
    assert d == 0


@pytest.mark.parametrize("sub", jc.SUBSAMPLINGS)
def test_reference_decodes_the_projects_encoder(sub):
    assert _max_diff(jc.reference_file("smooth", 45, 70, sub, 75)[0], (45, 70)) == 0


def test_malformed_files_have_a_status_and_header_errors_a_zero_image():
    corpus = dc.malformed_corpus()
    rgb, status, _ = dc.reference(list(corpus.values()), dc.MALFORMED_HW)
    got = dict(zip(corpus, status.tolist()))
    E = ref.JPEG_DECODE_ERRORS
    assert got["good"] == 0 and got["progressive"] == -E["unsupported"]
    assert got["size_mismatch"] == -E["size"] and got["no_soi"] == -E["marker"]
    assert got["flip_dht_symbol"] == -E["entropy"] and got["cut_before_eoi"] == -E["no_eoi"]
    assert all(got[k] < 0 for k in corpus if k.startswith("cut_"))
    for i, st in enumerate(status.tolist()):
        assert (rgb[i].max() == 0) == bool(-st & ref.JPEG_DECODE_HEADER_ERRORS)


def test_config_camera_jpeg():
    d = ModuleConfig().validate()
    assert "jpeg_max_bytes" not in d.to_dict() and d.frame_codec() == "raw"
    with pytest.raises(ValueError, match="frame_height"):
        d.apply_patch({"source": "camera-jpeg"})
    c = d.apply_patch({"source": "camera-jpeg", "frame_height": 48, "frame_width": 64})
    assert c.is_camera() and c.frame_format() == "rgb" and c.frame_codec() == "jpeg"
    assert c.to_dict()["jpeg_max_bytes"] == 0 and c.jpeg_row_bytes() == 48 * 64 // 2
    big = c.apply_patch({"jpeg_max_bytes": 4096})
    assert big.jpeg_row_bytes() == 4096 and big.needs_rebuild(c)
    with pytest.raises(ValueError):
        c.apply_patch({"jpeg_max_bytes": 4100})


def test_engine_rejects_what_does_not_combine():
    from kvedge_amd.engine import InferenceEngine

    for kw in ({}, {"frame_hw": (48, 64), "frame_format": "nv12"},
               {"frame_hw": (48, 64), "synthetic": True}):
        with pytest.raises(ValueError):
            InferenceEngine(lambda x: x, 2, 64, device="cpu",
                            **{"synthetic": False, "frame_codec": "jpeg", **kw})


class Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        self.t += 0.3
        return self.t


def test_module_cpu_camera_jpeg_equals_camera_fed_the_decoded_frames():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    if not ops.load():
        pytest.skip("native runtime not built")
    tr = FakeTransport({"model": "resnet50", "batch": 2, "report_interval_s": 1.0,
                        "image_size": 64, "source": "camera-jpeg", "frame_height": 48,
                        "frame_width": 64})
    with ModuleApp(tr, device="cpu", clock=Clock()).start() as app:
        eng = app.engine
        assert eng.frame_codec == "jpeg" and eng.input_frames.shape == (2, 48 * 64 // 2)
        assert app.ring.slot_bytes == 2 * 48 * 64 // 2
        app.run(max_steps=3)
        app.report()
        t = tr.outputs("telemetry")[-1]
        assert t["source"] == "camera-jpeg" and t["decode_errors"] == 0
        assert any(torch.equal(eng.input_frames, f) for f in app.camera.frames)
        rgb, status = ref.jpeg_decode(eng.input_frames, (48, 64))
        assert status.tolist() == [0, 0] and rgb.std() > 10
        assert torch.equal(eng.source_frames, torch.from_numpy(rgb))
        plain = InferenceEngine(app.model, 2, 64, device="cpu", synthetic=False,
                                frame_hw=(48, 64))
        want = plain.set_frames(torch.from_numpy(rgb))
        assert all(torch.equal(a, b) for a, b in zip(eng.outputs, want))
