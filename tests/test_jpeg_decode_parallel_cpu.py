"""The split path of the JPEG decoder without a GPU: the decoder's ``entropy`` keyword, and the
lane steps of csrc/kernels/jpeg_decode_core.h run lane by lane by the stand-alone self-test
program against its own serial walk and the reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import jpeg_decode_cases as dc
import jpeg_decode_parallel_cases as pc
from kvedge_amd import _build, ops


def test_entropy_keyword_and_constants():
    assert set(ops.JPEG_DECODE_ENTROPY) == {"auto", "serial", "parallel"}
    assert ops.JPEG_DECODE_SPLIT_BYTES % 16 == 0
    assert ops.JpegDecoder(1, (16, 16)).entropy == "auto"
    for bad in ("fast", None, 1):
        with pytest.raises(ValueError):
            ops.JpegDecoder(1, (16, 16), entropy=bad)
    files = [dc.pillow_file("noise", 40, 67, "420")]
    rgb, status, rows = dc.reference(files, (40, 67))
    dec = ops.JpegDecoder(1, (40, 67), rows.shape[1], entropy="parallel")
    got, st = ops.jpeg_decode(torch.from_numpy(rows.copy()), dec)
    assert torch.equal(got, torch.from_numpy(rgb.copy())) and st.tolist() == status.tolist()
    assert dec.paths.tolist() == [[0, 0]]


@pytest.mark.parametrize("group", [64, 8])
def test_lane_steps_on_the_host(tmp_path, group):
    if not (os.path.exists(_build.hipcc()) or shutil.which("hipcc")):
        pytest.skip("no hipcc")
    exe = tmp_path / "selftest"
    src = os.path.join(_build.CSRC, "runtime", "jpeg_decode_selftest_main.cpp")
    r = subprocess.run([_build.hipcc(), "-O1", "-std=c++17", "-x", "c++", f"-I{_build.CSRC}/kernels",
                        src, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = list(pc.malformed_no_dri().values()) + pc.stuffed_batch()
    rgb, status, rows = dc.reference(files, pc.HW)
    (tmp_path / "in").write_bytes(
        np.asarray([len(files), rows.shape[1], *pc.HW], np.int32).tobytes() + rows.tobytes())
    r = subprocess.run([str(exe), "--parallel", str(group), str(tmp_path / "in"),
                        str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "completed 18 intervals" in r.stdout  # good, flip_entropy and the 16 stuffed files
    got = np.fromfile(tmp_path / "out", np.uint8).reshape(len(files), -1)
    assert got[:, :4].copy().view(np.int32)[:, 0].tolist() == status.tolist()
    assert np.array_equal(got[:, 4:].reshape(rgb.shape), rgb)
