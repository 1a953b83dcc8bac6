"""What the large-operand tests share (test_large_operands_gpu.py, test_large_operands_cpu.py):
the arithmetic that makes an operand cross 2^31 and 2^32 bytes with the fewest images, the
images worth copying to the host, the launcher caps as one-line oracles, the comparison every
case ends in, and the table of cases in the GPU module's docstring.

An address computed in 32 bits wraps by 2^32 bytes (by 2^31 when the offset is signed) and so
lands in another image of the same operand: every image is filled with different random data,
so the comparison of a few well-chosen images with the CPU reference sees it."""
from dataclasses import dataclass

import numpy as np
import torch

import kernel_rules
from kvedge_amd.ops import reference as ref

MARK31, MARK32 = 2 ** 31, 2 ** 32
STEM_CAP = 0x7ffffff0          # the stem kernels' 32-bit buffer range: input bytes below this
GRID_YZ_CAP = 65535            # images per launch of the kernels that put the image in grid y / z
UPSAMPLE_STRIDE = 8192 * 256   # upsample2x: one grid stride past the last item must fit an int
POISON_U8 = 0xA5
POISON_I32 = -0x5A5A5A5B
GIB = 2 ** 30


def count_past(mark, bytes_per_image):
    """The fewest images whose operand ends past ``mark`` with a whole image behind it."""
    n = mark // bytes_per_image + 2
    assert n * bytes_per_image > mark
    return n


def sample_rows(n, bytes_per_image, marks=(MARK31, MARK32)):
    """Image 0, the image holding byte ``mark`` of the operand with its two neighbours for every
    mark the operand reaches, and the last image."""
    rows = {0, n - 1}
    for m in marks:
        k = m // bytes_per_image
        rows.update(r for r in (k - 1, k, k + 1) if 0 <= r < n)
    return sorted(rows)


def wrapped_row(k, bytes_per_image, bits=32):
    """The image a kernel reaches for image ``k`` when its byte offset is kept in ``bits`` bits."""
    return (k * bytes_per_image) % (1 << bits) // bytes_per_image


def stem_accepts(n, h, w, bytes_per_pixel=3):
    """The launcher rule of stem12_pool_frames and yolo_stem2 (uint8 frames, 3 bytes a pixel),
    of stem_pool (bf16 space-to-depth image, 32 bytes a pixel) and of stem_pool_frames, which
    shares stem_pool's launcher and is held to the space-to-depth image its frames stand for
    (32 bytes for 2 x 2 pixels: STEMF_BPP = 8 bytes a pixel)."""
    return n * h * w * bytes_per_pixel < STEM_CAP


def stem_max_n(h, w, bytes_per_pixel=3):
    n = (STEM_CAP - 1) // (h * w * bytes_per_pixel)
    assert stem_accepts(n, h, w, bytes_per_pixel) and not stem_accepts(n + 1, h, w, bytes_per_pixel)
    return n


def upsample_accepts(work):
    return work + UPSAMPLE_STRIDE < 2 ** 31


UPSAMPLE_MAX_WORK = 2 ** 31 - UPSAMPLE_STRIDE - 1


def grid_accepts(n):
    return n <= GRID_YZ_CAP


def jpeg_smallest_hw(mcu=16):
    """The smallest image of whole MCUs (fewest pixels, then the squarest) whose batch passes
    2^32 bytes with no more than GRID_YZ_CAP images."""
    best = None
    for h in range(mcu, 1024 + 1, mcu):
        for w in range(mcu, 1024 + 1, mcu):
            if count_past(MARK32, h * w * 3) <= GRID_YZ_CAP:
                key = (h * w, abs(h - w))
                if best is None or key < best[0]:
                    best = (key, (h, w))
                break  # wider only grows
    return best[1]


def grid_smallest_hw(step_h=4, step_w=4):
    """The same for plain uint8 RGB frames: the smallest H x W (multiples of the steps)."""
    best = None
    for h in range(step_h, 512 + 1, step_h):
        for w in range(step_w, 512 + 1, step_w):
            if count_past(MARK32, h * w * 3) <= GRID_YZ_CAP:
                key = (h * w, abs(h - w))
                if best is None or key < best[0]:
                    best = (key, (h, w))
                break
    return best[1]


@dataclass(frozen=True)
class Case:
    op: str
    operand: str
    image_bytes: int    # bytes of one image of the crossing operand
    n: int
    other_bytes: int    # every other device byte of the test, per image (operands and copies)
    fixed_bytes: int = 0

    @property
    def bytes(self):
        return self.n * self.image_bytes

    @property
    def peak(self):
        return self.n * (self.image_bytes + self.other_bytes) + self.fixed_bytes

    @property
    def rows(self):
        return sample_rows(self.n, self.image_bytes)


def _past32(op, operand, image_bytes, other_bytes, fixed=0):
    return Case(op, operand, image_bytes, count_past(MARK32, image_bytes), other_bytes, fixed)


HD = (1080, 1920)
HD_RGB = HD[0] * HD[1] * 3
HD_NV12 = HD[0] * HD[1] * 3 // 2
SMALL_DST = (32, 48)
ROI_K, ROI_D, ROI_MAXDET = 2, 16, 4
ROI_BIG_K, ROI_BIG_D, ROI_BIG_SRC = 4, 224, (64, 64)
WATCH_HW = grid_smallest_hw(4, 4)
WATCH_CELL = 16
ANNOTATE_HW = WATCH_HW
JPEG_HW = jpeg_smallest_hw()
JPEG_CAP = 16384
PRE_HW = (224, 224)
SYNTH_HW = (64, 64)
STEM12_HW, STEMF_HW, STEM_S2D_HW, YOLO_HW = (38, 20), (36, 20), (6, 8), (4, 32)
STEM_LDY = 80
STEMF_BPP = 8


def _watch_cells(hw=WATCH_HW, cell=WATCH_CELL):
    return -(-hw[0] // cell) * -(-hw[1] // cell)


def _jpeg_workspace(hw=JPEG_HW):
    mh, mw = hw[0] // 16, hw[1] // 16
    blocks = mw * 6
    return mh * (blocks * 128 + blocks * 416 + 16 + 4)


def _pooled(hp, wp, ldy=STEM_LDY):
    return hp * wp * ldy * 2


def _stem_case(op, hw, bpp, out_hw, ldy):
    n = stem_max_n(hw[0], hw[1], bpp)
    # the output is the operand that can cross; one image more is allocated for the refusal
    in_bytes = hw[0] * hw[1] * (3 if op.endswith(("frames", "stem2")) else 32)
    return Case(op, "y", out_hw[0] * out_hw[1] * ldy * 2, n, in_bytes,
                in_bytes + out_hw[0] * out_hw[1] * ldy * 2)


CASES = {c.op + ":" + c.operand: c for c in [
    _past32("frame_resize", "src", HD_RGB, SMALL_DST[0] * SMALL_DST[1] * 3),
    _past32("frame_resize", "dst", HD_RGB, 8 * 12 * 3),
    _past32("frame_resize_nv12", "src", HD_NV12, SMALL_DST[0] * SMALL_DST[1] * 3),
    _past32("roi_crop", "src", HD_RGB, ROI_K * ROI_D * ROI_D * 3 + ROI_MAXDET * 24 + 4),
    _past32("roi_crop_nv12", "src", HD_NV12, ROI_K * ROI_D * ROI_D * 3 + ROI_MAXDET * 24 + 4),
    _past32("roi_crop", "dst", ROI_BIG_K * ROI_BIG_D * ROI_BIG_D * 3,
            ROI_BIG_SRC[0] * ROI_BIG_SRC[1] * 3 + ROI_BIG_K * 24 + 4),
    _past32("roi_crop_nv12", "dst", ROI_BIG_K * ROI_BIG_D * ROI_BIG_D * 3,
            ROI_BIG_SRC[0] * ROI_BIG_SRC[1] * 3 // 2 + ROI_BIG_K * 24 + 4),
    _past32("frame_watch", "src", WATCH_HW[0] * WATCH_HW[1] * 3,
            (24 + 3 * _watch_cells()) * 4 + 64 + _watch_cells()),
    # the clone that proves the untouched rows, and the byte mask of the comparison
    _past32("annotate", "images", ANNOTATE_HW[0] * ANNOTATE_HW[1] * 3,
            2 * ANNOTATE_HW[0] * ANNOTATE_HW[1] * 3 + 168 * 4 + 24 + 8),
    _past32("jpeg_encode", "images", JPEG_HW[0] * JPEG_HW[1] * 3, _jpeg_workspace() + JPEG_CAP + 4),
    _past32("preprocess", "y", PRE_HW[0] * PRE_HW[1] * 8, PRE_HW[0] * PRE_HW[1] * 3),
    _past32("preprocess_s2d", "y", PRE_HW[0] * PRE_HW[1] * 8, PRE_HW[0] * PRE_HW[1] * 3),
    _past32("preprocess", "x", PRE_HW[0] * PRE_HW[1] * 3, PRE_HW[0] * PRE_HW[1] * 8),
    _past32("preprocess_s2d", "x", PRE_HW[0] * PRE_HW[1] * 3, PRE_HW[0] * PRE_HW[1] * 8),
    _past32("synth_frames", "out", SYNTH_HW[0] * SYNTH_HW[1] * 3, 0),
    # maxpool2d: x [N, 4, 4, 64] read through the channel slice [8, 16), 2x2 / 2 into [N, 2, 2, 16]
    _past32("maxpool2d", "x", 4 * 4 * 64 * 2, 2 * 2 * 16 * 2),
    # upsample2x: x [N, 2, 2, 8] into the slice [8, 16) of y [N, 4, 4, 64]
    _past32("upsample2x", "y", 4 * 4 * 64 * 2, 2 * 2 * 8 * 2 + 4 * 4 * 64),
    _past32("global_avgpool", "x", 8 * 8 * 64 * 2, 64 * 2),
    _past32("batchnorm_nhwc", "x", 8 * 8 * 8 * 2, 8 * 8 * 8 * 2),
    # softmax_rows: an "image" is one row; 1000 columns take the register path, 1001 the strided
    _past32("softmax_rows", "x", 1000 * 2, 1000 * 4 + 8),
    _past32("softmax_rows_strided", "x", 1001 * 2, 1001 * 4 + 8),
    # sppf_pool: in place on [N, 8, 8, 64], C = 16
    _past32("sppf_pool", "buf", 8 * 8 * 64 * 2, 0),
    _stem_case("stem12_pool_frames", STEM12_HW, 3, (10, 5), STEM_LDY),
    _stem_case("stem_pool_frames", STEMF_HW, STEMF_BPP, (9, 5), STEM_LDY),
    _stem_case("stem_pool", STEM_S2D_HW, 32, (3, 4), STEM_LDY),
    _stem_case("yolo_stem2", YOLO_HW, 3, (1, 8), 32),
    # x [N, 1, 1, 8] into y [N, 2, 2, 8]: the item count IS the image count
    Case("upsample2x_cap", "x", 16, UPSAMPLE_MAX_WORK + 1, 64, GIB),
]}


def table():
    """The cases as text: op, crossing operand, images, its bytes, peak device memory."""
    lines = ["%-22s %-7s %11s %14s %9s" % ("op", "operand", "N", "bytes", "peak GiB"),
             "-" * 67]
    for c in CASES.values():
        lines.append("%-22s %-7s %11d %14d %9.1f" % (c.op, c.operand, c.n, c.bytes, c.peak / GIB))
    return "\n".join(lines)


# ---------------------------------------------------------------------------
# the comparison of the sampled images
# ---------------------------------------------------------------------------
def check_exact(got, want, rows, what=""):
    """Bitwise: ``got`` and ``want`` hold the sampled images in the order of ``rows``."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    for i, r in enumerate(rows):  # torch.equal: a NaN left of the poison equals nothing
        assert torch.equal(got[i], want[i]), (what, "image", r)


def check_close(got, want, rows, what=""):
    """kernel_rules.assert_close image by image, and no NaN left of the poison."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not torch.isnan(got.float()).any(), (what, "poison left")
    for i, r in enumerate(rows):
        kernel_rules.assert_close(got[i], want[i], (what, "image", r))


def image_u8(k, shape, seed=0):
    """Image ``k`` of a batch no host holds: a pure function of (seed, k)."""
    g = torch.Generator().manual_seed(seed * 1_000_003 + k)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def image_bf16(k, shape, seed=0):
    g = torch.Generator().manual_seed(seed * 1_000_003 + k)
    return torch.randn(shape, generator=g).to(torch.bfloat16)


def synth_window(seed, step, byte0, nbytes):
    """Bytes [byte0, byte0 + nbytes) of ops.synth_frames' buffer, from the reference's own hash
    of the absolute 8-byte word index (byte0 and nbytes multiples of 8)."""
    assert byte0 % 8 == 0 and nbytes % 8 == 0
    i = np.arange(byte0 // 8, (byte0 + nbytes) // 8, dtype=np.uint64)
    with np.errstate(over="ignore"):
        mix = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ (np.uint64(step) * np.uint64(0xD1B54A32D192ED03))
        h = ref._splitmix64(mix ^ i)
    return torch.from_numpy(h.view(np.uint8).copy())
