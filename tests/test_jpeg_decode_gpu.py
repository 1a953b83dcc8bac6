"""The JPEG decoder on the MI355X: pixels and status words of the three kernels against the CPU
reference, torch.equal, on the smallest files that reach each mechanism (the table in
docs/kernels.md, K29).  The malformed corpus is the one tools/jpeg_decode_hostcheck.py runs
through the same core on the CPU under sanitizers."""
import pytest
import torch

import jpeg_decode_cases as dc
from kvedge_amd import ops

pytestmark = pytest.mark.gpu

CANARY = 0x5A


def _guarded(shape, dtype):
    """A tensor of ``shape`` with one canary row before and after it in the same allocation."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), CANARY, dtype=dtype, device="cuda")
    return whole[1:-1], whole


def _decode(files, hw, lanes=16):
    """Decode on the GPU with canary rows around out and every scratch buffer; asserts pixels,
    status and canaries against the reference."""
    assert ops.load()
    rgb, status, rows = dc.reference(files, hw)
    n = len(files)
    dec = ops.JpegDecoder(n, hw, rows.shape[1], device="cuda", lanes=lanes)
    guards = []
    for name in ("tables", "mpos", "planes", "status"):
        view, whole = _guarded(getattr(dec, name).shape, getattr(dec, name).dtype)
        setattr(dec, name, view)
        guards.append(whole)
    out, whole = _guarded((n,) + tuple(hw) + (3,), torch.uint8)
    guards.append(whole)
    got, st = ops.jpeg_decode(torch.from_numpy(rows.copy()).cuda(), dec, out=out)
    torch.cuda.synchronize()
    assert torch.equal(st.cpu(), torch.from_numpy(status.copy())), (st.tolist(), status.tolist())
    diff = (got.cpu() != torch.from_numpy(rgb.copy())).flatten(1).sum(1)
    assert int(diff.sum()) == 0, f"differing bytes per file: {diff.tolist()}"
    canary = torch.tensor(CANARY, device="cuda")
    for g in guards:
        assert bool((g[0] == canary.to(g.dtype)).all()) and bool((g[-1] == canary.to(g.dtype)).all())
    return status


SHAPES = [(sub, dri, 16, 16) for sub in dc.SUBS for dri in ("none", "row", "3")] + \
         [(sub, dri, 40, 67) for sub in dc.SUBS for dri in ("none", "row", "3")]


@pytest.mark.parametrize("sub,dri,h,w", SHAPES, ids=lambda v: str(v))
def test_sampling_and_restart_interval(sub, dri, h, w):
    """One MCU, and partial MCUs both ways with an interval that does not divide the row."""
    assert _decode([dc.pillow_file("smooth", h, w, sub, dri)], (h, w)).tolist() == [0]


@pytest.mark.parametrize("lanes", ops.JPEG_DECODE_LANES)
def test_more_intervals_than_one_wave(lanes):
    """1064 x 16 at 4:2:0, one MCU row per interval: 67 intervals, 2 to 5 wavefronts."""
    assert _decode([dc.pillow_file("noise", 1064, 16, "420", "row")], (1064, 16),
                   lanes).tolist() == [0]


@pytest.mark.parametrize("sub", dc.SUBS)
def test_long_codes_and_stuffed_bytes(sub):
    """Noise at quality 95 with optimised tables: codes past the 9-bit look-ahead and many
    FF 00 pairs at the refill edges."""
    f = dc.pillow_file("noise", 40, 67, sub, "3", 95, True)
    assert f.count(b"\xff\x00") >= 8
    assert _decode([f], (40, 67)).tolist() == [0]


def test_marker_alignment():
    """A comment of 0..17 bytes moves every marker through every phase of the 16-byte load;
    the entropy data (> 4 KiB) spans more than one step of the scan."""
    files = [dc.pillow_file("noise", 64, 64, "444", "row", 95, False, b"x" * k)
             for k in range(18)]
    assert min(len(f) for f in files) > 2 * 4096
    assert _decode(files, (64, 64)).tolist() == [0] * 18


def test_tables_are_per_image():
    files = [dc.pillow_file("noise", 40, 67, "420", "row", q, opt)
             for q, opt in ((30, False), (75, True), (95, True))]
    assert _decode(files, (40, 67)).tolist() == [0, 0, 0]


def test_malformed_corpus():
    corpus = dc.malformed_corpus()
    status = _decode(list(corpus.values()), dc.MALFORMED_HW)
    got = dict(zip(corpus, status.tolist()))
    assert got["good"] == 0 and got["progressive"] == -4 and got["size_mismatch"] == -8
    assert all(got[k] < 0 for k in corpus if k.startswith("cut_"))


def test_engine_graph_jpeg_equals_rgb_feed():
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50

    assert ops.load()
    resnet = KvResNet50(init_resnet50(seed=0), "cuda")
    hw = (96, 128)
    sets = [[dc.pillow_file(c, *hw, "420", "row", q) for c in cs]
            for cs, q in ((("noise", "smooth"), 75), (("bw_blocks", "noise"), 90))]
    n = dc.row_bytes(sets[0] + sets[1])
    eng = InferenceEngine(resnet, 2, 224, device="cuda", synthetic=False, frame_hw=hw,
                          frame_codec="jpeg", jpeg_row_bytes=n).prepare(warmup=1, autotune=False)
    assert eng.graph is not None and eng.input_frames.shape == (2, n)
    rgb_eng = InferenceEngine(resnet, 2, 224, device="cuda", synthetic=False, use_graph=False,
                              frame_hw=hw)
    for files in sets:
        rgb, status, rows = dc.reference(files, hw, n)
        eng.input_frames.copy_(torch.from_numpy(rows.copy()))
        probs, top1 = eng.run()
        torch.cuda.synchronize()
        want = rgb_eng.set_frames(torch.from_numpy(rgb.copy()).cuda())
        torch.cuda.synchronize()
        assert eng.decode_status.tolist() == [0, 0]
        assert torch.equal(eng.source_frames.cpu(), torch.from_numpy(rgb.copy()))
        assert torch.equal(probs, want[0]) and torch.equal(top1, want[1])
