"""What the JPEG decoder tests share (test_jpeg_decode_cpu.py, test_jpeg_decode_gpu.py) with
tools/jpeg_decode_hostcheck.py: files made by Pillow with each feature the decoder must
read, the malformed corpus, and a cache of the reference's answers."""
import functools
import io

import numpy as np

from kvedge_amd.ops import reference as ref

import jpeg_cases

SUBS = {"444": 0, "422": 1, "420": 2}  # Pillow's subsampling numbers
MCU = {"444": (8, 8), "422": (8, 16), "420": (16, 16)}  # (rows, columns)


@functools.lru_cache(maxsize=None)
def pillow_file(content, h, w, sub, dri="none", quality=75, optimize=False, comment=b""):
    """One file from Pillow.  dri: "none", "row" (one MCU row) or "3" (three MCUs)."""
    from PIL import Image

    kw = {}
    if dri == "row":
        kw["restart_marker_rows"] = 1
    elif dri != "none":
        kw["restart_marker_blocks"] = int(dri)
    if comment:
        kw["comment"] = comment
    buf = io.BytesIO()
    Image.fromarray(jpeg_cases.image(content, h, w)).save(
        buf, "JPEG", quality=quality, subsampling=SUBS[sub], optimize=optimize, **kw)
    return buf.getvalue()


def pillow_decode(data):
    return np.asarray(jpeg_cases.decode(data).convert("RGB"))


def row_bytes(files):
    return -(-max(len(f) for f in files) // 16) * 16 + 16


_cache = {}


def reference(files, hw, n=None):
    """(rgb [N, H, W, 3], status [N], rows [N, n]) of the reference, once per set of files."""
    n = n or row_bytes(files)
    key = (tuple(files), tuple(hw), n)
    if key not in _cache:
        rows = ref.jpeg_rows(files, n)
        rgb, st = ref.jpeg_decode(rows, hw)
        for a in (rows, rgb, st):
            a.setflags(write=False)
        _cache[key] = (rgb, st, rows)
    return _cache[key]


def _segment(data, marker):
    """Offset of the first segment with this marker byte (walks the header)."""
    pos = 2
    while data[pos + 1] != marker:
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return pos


MALFORMED_HW = (40, 67)


@functools.lru_cache(maxsize=None)
def malformed_corpus():
    """{name: file} around one 40 x 67 4:2:0 file with a restart interval of one MCU row."""
    h, w = MALFORMED_HW
    good = pillow_file("noise", h, w, "420", "row", 90)
    sos = _segment(good, 0xda)
    e0 = sos + 2 + ((good[sos + 2] << 8) | good[sos + 3])

    def flip(at, mask=0x40):
        b = bytearray(good)
        b[at] ^= mask
        return bytes(b)

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(jpeg_cases.image("noise", h, w)).save(buf, "JPEG", progressive=True)
    return {
        "good": good,
        "cut_after_header": good[:e0],
        "cut_mid_interval": good[:e0 + (len(good) - e0) // 2],
        "cut_before_eoi": good[:-2],
        "flip_dqt": flip(_segment(good, 0xdb) + 9, 0xff),
        "flip_dht": flip(_segment(good, 0xc4) + 6, 0x0f),
        "flip_dht_symbol": flip(_segment(good, 0xc4) + 4 + 17 + 3),
        "flip_sof": flip(_segment(good, 0xc0) + 11),
        "flip_entropy": flip(e0 + 40),
        "flip_entropy_late": flip(e0 + (len(good) - e0) * 3 // 4, 0x18),
        "progressive": buf.getvalue(),
        "size_mismatch": pillow_file("noise", h + 8, w, "420", "row", 90),
        "no_soi": b"\x00" + good[1:],
    }
