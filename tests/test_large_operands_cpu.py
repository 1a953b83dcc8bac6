"""The arithmetic behind test_large_operands_gpu.py, checked without a GPU: the launcher caps
pinned as numbers and against the kernel sources, the choice of images, and -- the point of the
whole module -- that its comparison rejects what a kernel with a 32-bit byte offset would
produce (image k replaced by the image at k's byte offset mod 2^32), built on the CPU side
only."""
import os
import re

import pytest
import torch

import large_cases as lc
import pool_oracles as po
from kvedge_amd import ops
from large_cases import CASES

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc",
                       "kernels")


def _src(name):
    with open(os.path.join(KERNELS, name)) as f:
        return f.read()


def test_stem_cap_boundaries():
    assert lc.STEM_CAP == 0x7ffffff0 == 2147483632
    assert lc.stem_max_n(38, 20) == 941878 and lc.stem_max_n(36, 20, lc.STEMF_BPP) == 372827
    assert lc.stem_max_n(4, 32) == 5592405 and lc.stem_max_n(6, 8, 32) == 1398101
    assert lc.stem_accepts(941878, 38, 20) and not lc.stem_accepts(941879, 38, 20)
    # the launchers hold the same constant, on the same product
    assert "(long long)N * H0 * W0 * 3 >= 0x7ffffff0LL" in _src("stem12.hip")
    assert "(long long)N * H0 * W0 * 3 >= 0x7ffffff0ll" in _src("yolo_stem2.hip")
    assert "(long long)N * H * W * 16 * 2 >= 0x7ffffff0LL" in _src("stem_pool.hip")


def test_grid_caps():
    assert lc.GRID_YZ_CAP == 65535 and lc.grid_accepts(65535) and not lc.grid_accepts(65536)
    assert "if (N > 65535) return -9;" in _src("frame_watch.hip")
    assert re.search(r"N < 0 \|\| N > 65535", _src("annotate.hip"))
    assert "if (M < 0 || M > 65535) return -2;" in _src("jpeg_encode.hip")
    assert "if (N > 65535) return -2;  // grid y" in _src("pool_misc.hip")


def test_upsample_cap_is_the_pool_oracle():
    assert lc.UPSAMPLE_STRIDE == po.UPSAMPLE_STRIDE and lc.UPSAMPLE_MAX_WORK == 2145386495
    for work in (lc.UPSAMPLE_MAX_WORK, lc.UPSAMPLE_MAX_WORK + 1, 2 ** 31 - 1):
        assert lc.upsample_accepts(work) == po.upsample_accepts(work)
    assert lc.upsample_accepts(lc.UPSAMPLE_MAX_WORK) and not lc.upsample_accepts(
        lc.UPSAMPLE_MAX_WORK + 1)
    assert "work + 8192ll * kBlock >= (1ll << 31)" in _src("pool_misc.hip")


def test_counts_and_rows():
    for key, c in CASES.items():
        if key.startswith("upsample2x_cap"):
            continue
        crossing = lc.MARK31 if c.op in ("stem_pool", "stem_pool_frames", "yolo_stem2") else lc.MARK32
        assert c.bytes > crossing, key
        rows = c.rows
        assert rows[0] == 0 and rows[-1] == c.n - 1 and len(rows) <= 8, (key, rows)
        for mark in (lc.MARK31, crossing):
            k = mark // c.image_bytes
            assert k * c.image_bytes <= mark < (k + 1) * c.image_bytes
            assert {k - 1, k, k + 1} <= set(rows), (key, mark)
        if not c.op.startswith(("stem", "yolo")):
            assert (c.n - 2) * c.image_bytes <= lc.MARK32, key  # the fewest images that cross
    assert CASES["frame_resize:src"].n == 692 and CASES["frame_resize_nv12:src"].n == 1382
    for key in ("frame_watch:src", "annotate:images", "jpeg_encode:images"):
        assert lc.grid_accepts(CASES[key].n), key
    assert all(c.op in lc.table() for c in CASES.values())


def test_wrapped_row():
    b = CASES["frame_resize:src"].image_bytes
    assert [lc.wrapped_row(k, b) for k in (0, 345, 690)] == [0, 345, 690]  # below 2^32: itself
    assert lc.wrapped_row(691, b) == (691 * b - 2 ** 32) // b == 0
    assert lc.wrapped_row(346, b, bits=31) == 0 and lc.wrapped_row(345, b, bits=31) == 345


def _rejects(check, got, want, rows):
    with pytest.raises(AssertionError):
        check(got, want, rows, "wrapped")


def test_comparison_rejects_a_32_bit_wrap_uint8():
    """frame_resize with src past 2^32 bytes: the reference of the sampled images against what
    a kernel that keeps the source offset in 32 (or 31) bits computes for them."""
    c = CASES["frame_resize:src"]
    plan = ops.ResizePlan((1080, 27, 0, 2, 27), (1920, 48, 0, 0, 48), 114, lc.HD, lc.SMALL_DST)
    shape = (*lc.HD, 3)
    for bits in (32, 31):
        rows = [r for r in c.rows if lc.wrapped_row(r, c.image_bytes, bits) != r][:2]
        assert rows, bits
        want = ops.frame_resize(torch.stack([lc.image_u8(r, shape) for r in rows]), plan)
        wrapped = ops.frame_resize(torch.stack(
            [lc.image_u8(lc.wrapped_row(r, c.image_bytes, bits), shape) for r in rows]), plan)
        lc.check_exact(want.clone(), want, rows)
        _rejects(lc.check_exact, wrapped, want, rows)
        if len(rows) > 1:  # one wrapped image among right ones is enough
            _rejects(lc.check_exact, torch.cat([want[:1], wrapped[1:]]), want, rows)


def test_comparison_rejects_a_32_bit_wrap_bf16():
    """preprocess with y past 2^32 bytes (a wrapped store leaves the poison in image k and its
    values in another image) and global_avgpool with x past 2^32 (a wrapped load), under
    kernel_rules.assert_close."""
    c = CASES["global_avgpool:x"]
    rows = [r for r in c.rows if lc.wrapped_row(r, c.image_bytes) != r]
    assert rows
    want = ops.global_avgpool(torch.stack([lc.image_bf16(r, (8, 8, 64)) for r in rows]))
    wrapped = ops.global_avgpool(torch.stack(
        [lc.image_bf16(lc.wrapped_row(r, c.image_bytes), (8, 8, 64)) for r in rows]))
    lc.check_close(want.clone(), want, rows)
    _rejects(lc.check_close, wrapped, want, rows)
    c = CASES["preprocess:y"]
    rows = [r for r in c.rows if lc.wrapped_row(r, c.image_bytes) != r][:2]
    want = ops.preprocess(torch.stack([lc.image_u8(r, (*lc.PRE_HW, 3)) for r in rows]))
    poisoned = torch.full_like(want, float("nan"))  # image k never written
    _rejects(lc.check_close, poisoned, want, rows)
    other = ops.preprocess(torch.stack([lc.image_u8(lc.wrapped_row(r, c.image_bytes),
                                                    (*lc.PRE_HW, 3)) for r in rows]))
    _rejects(lc.check_close, other, want, rows)


def test_synth_window_is_the_reference():
    out = ops.synth_frames(torch.empty(3, 8, 8, 3, dtype=torch.uint8), 99, 4)
    assert torch.equal(out.flatten(), lc.synth_window(99, 4, 0, 3 * 192))
    assert torch.equal(out[2].flatten(), lc.synth_window(99, 4, 2 * 192, 192))
