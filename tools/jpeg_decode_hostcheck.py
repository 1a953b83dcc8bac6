#!/usr/bin/env python
"""Run the JPEG decoder core (csrc/kernels/jpeg_decode_core.h) on the CPU under
AddressSanitizer + UBSan over the decoder tests' files -- the malformed corpus above all --
and compare pixels and status words with ops.reference.jpeg_decode.

The core is what the device kernels execute per file: header parser, bit reader, Huffman
walk, IDCT, upsampling and colour.  The program is a plain executable built by
``python -m kvedge_amd._build --asan``; nothing is loaded into Python under a sanitizer.
Run this before the malformed cases go to a GPU: ``python tools/jpeg_decode_hostcheck.py``.

Files without restart markers (and the row-interval ones again) also go through
``--parallel G``: the split path's lane steps run lane by lane in groups of G lanes, which
must equal the serial walk inside the program and the reference here.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import jpeg_decode_cases as dc  # noqa: E402
import jpeg_decode_parallel_cases as pc  # noqa: E402

BIN = os.path.join(ROOT, "kvedge_amd", "bin", "kv_jpeg_decode_selftest_asan")


def check(name, files, hw, group=0):
    """group > 0: through the split path in groups of that many lanes."""
    rgb, status, rows = dc.reference(files, hw)
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "corpus.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(np.asarray([len(files), rows.shape[1], hw[0], hw[1]], np.int32).tobytes())
            f.write(rows.tobytes())
        mode = ["--parallel", str(group)] if group else []
        r = subprocess.run([BIN, *mode, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True)
        if r.returncode != 0:
            print(r.stdout)
            raise SystemExit(f"{name}: the sanitizer build exited with {r.returncode}")
        got = np.fromfile(dst, np.uint8).reshape(len(files), 4 + hw[0] * hw[1] * 3)
    st = got[:, :4].copy().view(np.int32)[:, 0]
    px = got[:, 4:].reshape(rgb.shape)
    bad = [i for i in range(len(files)) if st[i] != status[i] or not np.array_equal(px[i], rgb[i])]
    if group:
        print(r.stdout.strip())
    print(f"{name}: {len(files)} files, status {status.tolist()}, "
          f"{'all equal the reference' if not bad else f'MISMATCH at {bad}'}")
    return not bad


def main():
    if not os.path.exists(BIN):
        raise SystemExit("build it first: python -m kvedge_amd._build --asan")
    ok = True
    corpus = dc.malformed_corpus()
    ok &= check("malformed " + " ".join(corpus), list(corpus.values()), dc.MALFORMED_HW)
    for sub in dc.SUBS:
        for hw in ((16, 16), (40, 67)):
            files = [dc.pillow_file("noise", *hw, sub, dri, 95, True)
                     for dri in ("none", "row", "3")]
            ok &= check(f"{sub} {hw[0]}x{hw[1]} optimised, DRI none / row / 3", files, hw)
    corpus = pc.malformed_no_dri()
    for group in (64, 8):
        ok &= check(f"split path, groups of {group}: no DRI " + " ".join(corpus),
                    list(corpus.values()), pc.HW, group)
        ok &= check(f"split path, groups of {group}: stuffed bytes at the cuts",
                    pc.stuffed_batch(), pc.HW, group)
        for sub in dc.SUBS:
            files = [dc.pillow_file(c, 40, 67, sub, "none", q) for c, q in
                     (("smooth", 75), ("noise", 75), ("bw_blocks", 20), ("noise", 100))]
            ok &= check(f"split path, groups of {group}: {sub} 40x67 no DRI", files, (40, 67), group)
        files = [dc.pillow_file("noise", 64, 256, "444", "row", 95),
                 dc.pillow_file("noise", 64, 256, "420", "3", 30)]
        ok &= check(f"split path, groups of {group}: DRI, long and short intervals", files,
                    (64, 256), group)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
