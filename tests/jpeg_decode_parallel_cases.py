"""Files without restart markers that test_jpeg_decode_parallel_{cpu,gpu}.py share with
tools/jpeg_decode_hostcheck.py: the corpus's entropy and truncation damage around a file that
is one long restart interval, and the batch that moves stuffed bytes across the cuts."""
import functools

import jpeg_decode_cases as dc

HW = dc.MALFORMED_HW


@functools.lru_cache(maxsize=None)
def malformed_no_dri():
    good = dc.pillow_file("noise", *HW, "420", "none", 90)
    sos = dc._segment(good, 0xda)
    e0, n = sos + 2 + ((good[sos + 2] << 8) | good[sos + 3]), len(good)

    def flip(at, mask):
        return good[:at] + bytes([good[at] ^ mask]) + good[at + 1:]

    return {"good": good, "cut_after_header": good[:e0], "cut_mid_interval": good[:e0 + (n - e0) // 2],
            "cut_before_eoi": good[:-2], "flip_entropy": flip(e0 + 40, 0x40),
            "flip_entropy_late": flip(e0 + (n - e0) * 3 // 4, 0x18)}


def stuffed_batch():
    """Comments of 0..15 bytes move every FF 00 pair through every phase of a 16-byte word."""
    return [dc.pillow_file("noise", *HW, "444", "none", 95, True, b"x" * k) for k in range(16)]
