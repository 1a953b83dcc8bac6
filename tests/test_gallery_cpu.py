"""Appearance search on the CPU: the two references against naive loops, the planted rows of
embed_quantize, ops.Gallery, the module's keys and the cascade with a gallery."""
import math

import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.ops import reference


def planted_features(c=64):
    """bf16 [4, 1, 2, c]: a NaN and +-1e6 (clamped), an all-zero row, a row whose largest sum
    rounds to 128 (255 -> (255 + 1) >> 1, clamped to 127), and a plain row."""
    x = torch.zeros(4, 1, 2, c)
    x[0, 0, 0, 0], x[0, 0, 0, 1], x[0, 0, 1, 1], x[0, 0, 0, 2] = float("nan"), 1e6, 1e6, -1e6
    x[2, 0, 0, 0], x[2, 0, 0, 1] = 255 / 256, -3 / 256
    x[3, 0, :, :] = torch.arange(2 * c).view(2, c) / 64 - 1
    return x.to(torch.bfloat16)


def embed(x):
    m, c = x.shape[0], x.shape[3]
    return reference.embed_quantize(x, torch.empty(m, c, dtype=torch.int8),
                                    torch.empty(m, dtype=torch.int32))


def test_embed_quantize_reference_against_loop():
    x = (torch.randn(2, 2, 3, 64, generator=torch.Generator().manual_seed(1)) * 3).to(torch.bfloat16)
    codes, nrm2 = embed(x)
    for m in range(2):
        s = [sum(int(round(float(x[m, i, j, c]) * 256)) for i in range(2) for j in range(3))
             for c in range(64)]  # bf16 * 256 is exact, round() only sees integers
        e = max(0, max(abs(v) for v in s).bit_length() - 7)
        want = [int(math.copysign(min(127, (abs(v) + (1 << (e - 1) if e else 0)) >> e), v))
                for v in s]
        assert codes[m].tolist() == want and int(nrm2[m]) == sum(v * v for v in want)


def test_embed_quantize_planted_rows():
    codes, nrm2 = embed(planted_features())
    # clamp(+-1e6) = +-16384 -> sums 2^23 and -2^22, e = 17: codes 64 and -32; the NaN is 0
    assert codes[0, :3].tolist() == [0, 64, -32] and int(nrm2[0]) == 64 * 64 + 32 * 32
    assert not codes[1].any() and int(nrm2[1]) == 0
    assert codes[2, :2].tolist() == [127, -2]  # e = 1: (255 + 1) >> 1 = 128 -> 127
    assert int(codes[3].abs().max()) in range(64, 128)


def test_gallery_match_reference_against_loop():
    g = torch.Generator().manual_seed(2)
    q = torch.randint(-127, 128, (3, 64), generator=g, dtype=torch.int8)
    codes = torch.randint(-127, 128, (5, 64), generator=g, dtype=torch.int8)
    codes[3] = codes[1]  # a tie: the lower row first
    scale = torch.tensor([0.5, 0.25, 0.0, 0.25, 1.0])  # row 2 does not count, row 4 is past count
    score, row = reference.gallery_match(q, codes, scale, torch.tensor([4], dtype=torch.int32),
                                         torch.empty(3, 2), torch.empty(3, 2, dtype=torch.int32))
    for m in range(3):
        cand = [(-float(torch.tensor(float(sum(int(a) * int(b) for a, b in zip(q[m], codes[j]))))
                        * scale[j]), j) for j in (0, 1, 3)]
        best = sorted(cand)[:2]
        assert row[m].tolist() == [j for _, j in best]
        assert score[m].tolist() == [-s for s, _ in best]


def test_gallery_enrol_remove_save_load(tmp_path):
    codes, nrm2 = embed(planted_features())
    gal = ops.Gallery(8, 64)
    with pytest.raises(ValueError, match="nrm2 == 0"):
        gal.enrol(codes[1], nrm2[1], 5)
    gal.enrol(codes[[0, 2]], nrm2[[0, 2]], [7, 9]).enrol(codes[3], nrm2[3], 7)
    assert len(gal) == 3 and gal.labels().tolist() == [7, 9, 7]
    assert torch.equal(gal.scale[:3], 1.0 / torch.sqrt(nrm2[[0, 2, 3]].float()))
    score, row = ops.gallery_match(codes[[3]], gal, top=4)
    assert int(row[0, 0]) == 2 and int(row[0, 3]) == -1 and float(score[0, 3]) == 0.0
    assert abs(float(score[0, 0]) / math.sqrt(int(nrm2[3])) - 1.0) < 1e-6
    path = tmp_path / "g.npz"
    gal.save(path)
    back = ops.Gallery.load(path, capacity=8)
    assert len(back) == 3 and torch.equal(back.codes, gal.codes) and torch.equal(back.scale, gal.scale)
    assert gal.remove(7) == 2 and len(gal) == 1 and gal.labels().tolist() == [9]
    assert torch.equal(gal.codes[0], codes[2]) and float(gal.scale[1]) == 0.0
    assert len(gal.clear()) == 0
    with pytest.raises(ValueError):
        ops.Gallery(8, 96)


def test_module_config_gallery_keys():
    from kvedge_amd.module.config import ModuleConfig

    d = ModuleConfig().validate().to_dict()
    assert not {"gallery", "gallery_top", "gallery_threshold"} & set(d)
    cfg = ModuleConfig(model="detect-classify", gallery="g.npz", gallery_top=2).validate()
    assert cfg.to_dict()["gallery"] == "g.npz" and cfg.to_dict()["gallery_top"] == 2
    with pytest.raises(ValueError, match="detect-classify"):
        ModuleConfig(model="yolov8n", gallery="g.npz").validate()
    with pytest.raises(ValueError):
        ModuleConfig(model="detect-classify", gallery="g.npz", gallery_top=9).validate()


def test_cascade_with_and_without_gallery():
    from kvedge_amd.models.cascade import KvDetectClassify
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    det = KvYoloV8n(init_yolov8n(seed=0, calibrate=False), "cpu", conf=0.0, max_det=8)
    clf = KvResNet50(init_resnet50(seed=0, calibrate=False), "cpu")
    frames = torch.randint(0, 256, (2, 64, 64, 3), generator=torch.Generator().manual_seed(3),
                           dtype=torch.uint8)
    plain = KvDetectClassify(det, clf, 2, crop_size=64)(frames)
    assert len(plain) == 4
    gal = ops.Gallery(4, 2048)
    m = KvDetectClassify(det, clf, 2, crop_size=64, gallery=gal, gallery_top=2)
    out = m(frames)
    assert len(out) == 6 and all(torch.equal(a, b) for a, b in zip(out[:4], plain))
    assert out[4].shape == (2, 2, 2) and out[4].dtype == torch.int32 and (out[4] == -1).all()
    assert int(out[1].min()) >= 2
    codes, nrm2 = m.embedding
    gal.enrol(codes[3], nrm2[3], 42)  # image 1, crop 1
    label, cos = m(frames)[4:]
    assert int(label[1, 1, 0]) == 42 and abs(float(cos[1, 1, 0]) - 1.0) < 1e-6
    assert (label[..., 1] == -1).all() and (cos[..., 1] == 0).all()  # one row enrolled
    m.set_gallery_threshold(1.0)
    assert ((m(frames)[4] == 42) == (cos >= 1.0)).all()
