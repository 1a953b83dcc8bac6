"""The JPEG encoder's definition (ops.reference.jpeg_encode) against an independent decoder and
encoder -- Pillow / libjpeg: every file opens at the right size, loses no more quality than
libjpeg's own file of the same settings, and the test images reach every branch of the entropy
coder; then the CPU face of ops.jpeg_encode: quality changes, the capacity contract, the size
bound and the thumbnail geometry."""
import io

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

import jpeg_cases as jc  # noqa: E402
from kvedge_amd import ops  # noqa: E402
from kvedge_amd.ops import reference as ref  # noqa: E402

# (H, W): one pixel, one block, both axes padded (and transposed), one 4:2:0 MCU, the
# prototype's odd size
SIZES = [(1, 1), (8, 8), (9, 17), (17, 9), (16, 16), (45, 70)]
# how far below Pillow's own file (same quality and subsampling) the PSNR may fall, in dB;
# the measured shortfalls are in docs/kernels.md (at most 0.00 for 4:4:4, 0.19 for 4:2:0, whose
# gap is libjpeg's different chroma filter)
MARGIN_DB = {"444": 0.25, "420": 1.5}
PIL_SUB = {"444": 0, "420": 2}


@pytest.mark.parametrize("quality", jc.QUALITIES)
@pytest.mark.parametrize("sub", jc.SUBSAMPLINGS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_file_opens_at_the_true_size(hw, sub, quality):
    h, w = hw
    data, _ = jc.reference_file("noise", h, w, sub, quality)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    im = Image.open(io.BytesIO(data))
    assert im.format == "JPEG" and im.size == (w, h) and im.mode == "RGB"
    im.load()


@pytest.mark.parametrize("quality", [30, 75, 95])
@pytest.mark.parametrize("sub", jc.SUBSAMPLINGS)
@pytest.mark.parametrize("name", ["smooth", "noise"])
def test_no_worse_than_pillow_at_the_same_settings(name, sub, quality):
    src = jc.image(name, 45, 70)
    data, _ = jc.reference_file(name, 45, 70, sub, quality)
    ours = jc.psnr(jc.decode(data), src)
    b = io.BytesIO()
    Image.fromarray(src).save(b, "JPEG", quality=quality, subsampling=PIL_SUB[sub])
    pil = jc.psnr(jc.decode(b.getvalue()), src)
    print(f"{name} {sub} q{quality}: ours {ours:.2f} dB, Pillow {pil:.2f} dB, "
          f"shortfall {pil - ours:.2f} dB, {len(data)} vs {len(b.getvalue())} bytes")
    assert pil - ours <= MARGIN_DB[sub], (ours, pil)


def test_noise_at_95_stuffs_bytes():
    for sub in jc.SUBSAMPLINGS:
        assert jc.reference_file("noise", 45, 70, sub, 95)[1]["stuffed"] >= 1


def test_lone_last_coefficient_needs_zrl_and_no_eob():
    data, st = jc.reference_file("sparse_zrl", 16, 32, "444", 50)
    blocks = 2 * 4
    assert st["zrl"] == 3 * blocks        # 62 zeros in front of coefficient 63 of every Y block
    assert st["eob"] == 2 * blocks        # the chroma blocks only: Y ends on coefficient 63
    assert jc.reference_file("sparse_zrl", 16, 32, "420", 50)[1]["zrl"] >= 1
    jc.decode(data)


def test_black_beside_white_reaches_dc_category_11():
    for sub in jc.SUBSAMPLINGS:
        assert jc.reference_file("bw_blocks", 16, 32, sub, 100)[1]["max_dc_cat"] == 11


def test_noise_at_100_reaches_ac_category_9():
    for sub in jc.SUBSAMPLINGS:
        assert jc.reference_file("noise", 45, 70, sub, 100)[1]["max_ac_cat"] >= 9


def test_constant_image_is_eobs_and_zero_dc_differences():
    for sub, intervals, blocks in (("444", 6, 6 * 9 * 3), ("420", 3, 3 * 5 * 6)):
        _, st = jc.reference_file("constant", 45, 70, sub, 50)
        assert st["eob"] == blocks and st["zrl"] == 0 and st["max_ac_cat"] == 0
        # the prediction restarts in every interval: only each component's first block there
        # carries a difference
        assert st["dc_nonzero"] == 3 * intervals


def test_size_bound_holds_and_is_the_derived_formula():
    for sub in jc.SUBSAMPLINGS:
        data, _ = jc.reference_file("noise", 45, 70, sub, 100)
        assert len(data) <= ops.jpeg_max_bytes((45, 70), sub)
    # 45 x 70: 6 intervals of 9 MCUs of 3 blocks | 3 intervals of 5 MCUs of 6 blocks
    assert ops.jpeg_max_bytes((45, 70), "444") == 611 + 6 * (27 * 416 + 3) + 2
    assert ops.jpeg_max_bytes((45, 70), "420") == 611 + 3 * (30 * 416 + 3) + 2
    assert (22 + 63 * 26 + 7) // 8 * 2 == ops.JPEG_BLOCK_BYTES
    # no code of the four tables is longer than the bound assumes
    huff = ref.jpeg_huff_codes() >> 16
    assert huff[:2].max() <= 11 and huff[2:].max() == 16
    with pytest.raises(ValueError):
        ops.jpeg_max_bytes((0, 8), "420")
    with pytest.raises(ValueError):
        ops.jpeg_max_bytes((8, 8193), "420")
    with pytest.raises(ValueError):
        ops.jpeg_max_bytes((8, 8), "422")


def test_quant_tables_scale_the_libjpeg_way():
    q50, q1, q100 = (ref.jpeg_quant_tables(q) for q in (50, 1, 100))
    assert q50[0, :4].tolist() == [16, 11, 10, 16] and q50[1, :4].tolist() == [17, 18, 24, 47]
    assert q100.min() == 1 and q100.max() == 1 and q1.max() == 255
    assert ref.jpeg_quant_tables(25)[0, 0] == (16 * 200 + 50) // 100
    assert ref.jpeg_quant_tables(75)[0, 0] == (16 * 50 + 50) // 100
    for bad in (0, 101, True):
        with pytest.raises(ValueError):
            ref.jpeg_quant_tables(bad)


def test_cpu_op_equals_the_reference_and_set_quality_rewrites_only_the_dqt_bytes():
    imgs = jc.as_tensor(jc.image("noise", 9, 17), jc.image("smooth", 9, 17))
    enc = ops.JpegEncoder((9, 17), 4, "420", 75)
    head75 = bytes(enc.header.tolist())
    buf, length = ops.jpeg_encode(imgs, enc)
    assert buf.shape == (2, ops.jpeg_max_bytes((9, 17), "420")) and length.dtype == torch.int32
    want = ref.jpeg_encode(imgs, "420", 75)
    for m in range(2):
        assert bytes(buf[m, :length[m]].tolist()) == want[m]
    assert enc.set_quality(30) is enc and enc.quality == 30
    head30 = bytes(enc.header.tolist())
    diff = {i for i in range(len(head75)) if head75[i] != head30[i]}
    dqt = {o + i for o in ref.JPEG_DQT_OFFSETS for i in range(64)}
    assert diff and diff <= dqt
    assert jc.dqt_bytes(head30) != jc.dqt_bytes(head75)
    assert head30 == ref.jpeg_header((9, 17), "420", ref.jpeg_quant_tables(30))
    buf, length = ops.jpeg_encode(imgs, enc)
    assert bytes(buf[1, :length[1]].tolist()) == ref.jpeg_encode(imgs, "420", 30)[1]
    with pytest.raises(ValueError):
        enc.set_quality(0)
    assert enc.quality == 30


def test_a_file_that_does_not_fit_reports_its_size_and_touches_nothing():
    imgs = jc.as_tensor(*(jc.image(n, 16, 16) for n in ("constant", "smooth", "noise")))
    enc = ops.JpegEncoder((16, 16), 3, "444", 100)
    want = ref.jpeg_encode(imgs, "444", 100)
    cap = len(want[2]) // 2
    assert len(want[0]) <= cap < len(want[2])
    out = torch.full((4, cap), 0xA5, dtype=torch.uint8)
    lengths = torch.full((4,), -7, dtype=torch.int32)
    got = ops.jpeg_encode(imgs, enc, out, lengths)
    assert got[0] is out and got[1] is lengths
    assert lengths[2] == -len(want[2]) and lengths[3] == -7
    assert bool((out[2:] == 0xA5).all())
    for m in range(2):
        if len(want[m]) <= cap:
            assert lengths[m] == len(want[m])
            assert bytes(out[m, :lengths[m]].tolist()) == want[m]
            assert bool((out[m, lengths[m]:] == 0xA5).all())
        else:
            assert lengths[m] == -len(want[m]) and bool((out[m] == 0xA5).all())


def test_the_op_rejects_what_the_encoder_was_not_made_for():
    enc = ops.JpegEncoder((8, 8), 2)
    ok = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for bad in (torch.zeros(3, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 9, 3, dtype=torch.uint8),
                torch.zeros(1, 8, 8, 4, dtype=torch.uint8), torch.zeros(1, 8, 8, 3),
                ok.transpose(1, 2)):
        with pytest.raises(ValueError):
            ops.jpeg_encode(bad, enc)
    with pytest.raises(TypeError):
        ops.jpeg_encode(ok, None)
    for slot0 in (1, -1):   # workspace rows [slot0, slot0 + 2) of an encoder for 2 images
        with pytest.raises(ValueError):
            ops.jpeg_encode(ok, enc, slot0=slot0)
    assert int(ops.jpeg_encode(ok[:1], enc, slot0=1)[1][0]) > 611
    with pytest.raises(ValueError):
        ops.jpeg_encode(ok, enc, out=torch.zeros(1, 4000, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.jpeg_encode(ok, enc, lengths=torch.zeros(2, dtype=torch.int64))
    for kw in (dict(hw=(8, 8), max_images=0), dict(hw=(8, 8), max_images=1, subsampling="411"),
               dict(hw=(8, 9000), max_images=1), dict(hw=(8, 8), max_images=1, quality=101)):
        with pytest.raises(ValueError):
            ops.JpegEncoder(**kw)


def test_thumbnail_plan_geometry():
    p = ops.thumbnail_plan((1080, 1920), 320)
    assert p.dst_hw == (180, 320) and p.src_hw == (1080, 1920) and p.pad == 0
    assert p.axis_y == (1080, 180, 0, 0, 180) and p.axis_x == (1920, 320, 0, 0, 320)
    # both rounded up to a multiple of 4: 30 -> 32 wide, round(30 * 96 / 64) = 45 -> 48 high
    assert ops.thumbnail_plan((96, 64), 30).dst_hw == (48, 32)
    assert ops.thumbnail_plan((4000, 16), 16).dst_hw == (4000, 16)
    assert ops.thumbnail_plan((2, 4000), 16).dst_hw == (4, 16)    # never zero rows
    for bad in (0, -4):
        with pytest.raises(ValueError):
            ops.thumbnail_plan((1080, 1920), bad)
    with pytest.raises(ValueError):
        ops.thumbnail_plan((8192, 16), 64)                          # 32768 rows
    # a stretch: every destination pixel has content, and a resized frame encodes at that size
    src = jc.as_tensor(jc.image("smooth", 96, 64))
    small = ops.frame_resize(src, ops.thumbnail_plan((96, 64), 30))
    assert small.shape == (1, 48, 32, 3)
    buf, length = ops.jpeg_encode(small, ops.JpegEncoder((48, 32), 1))
    assert jc.decode(buf[0, :length[0]].tolist()).size == (32, 48)


# ---------------------------------------------------------------- build
import os  # noqa: E402
import shutil  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_jpeg_kernels_cross_compile_without_warnings(tmp_path):
    from kvedge_amd import _build

    src = os.path.join(ROOT, "csrc", "kernels", "jpeg_encode.hip")
    assert src in _build.glob.glob(os.path.join(_build.CSRC, "kernels", "*.hip"))
    for extra in ([], ["-DKVEDGE_CHECKS=1"]):  # the bounds-check build covers it too
        r = subprocess.run([_build.hipcc(), *_build.COMMON, *extra, "-Wall", "-Wextra", "-Werror",
                            f"-I{_build.CSRC}/kernels", "-c", src, "-o", str(tmp_path / "jp.o")],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and not (r.stdout + r.stderr).strip(), r.stderr[-2000:]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_jpeg_kernels_do_not_spill():
    import sys

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"),
                        os.path.join(ROOT, "csrc", "kernels", "jpeg_encode.hip"), "--no-spill"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    rows = [l for l in r.stdout.splitlines()
            if l.startswith("| jpeg_encode.hip") and "_kernel" in l]  # (not the zigzag table)
    assert len(rows) == 5, rows  # blocks and entropy x (4:2:0, 4:4:4) + pack
