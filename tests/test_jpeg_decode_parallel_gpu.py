"""Long restart intervals decoded by one lane per ops.JPEG_DECODE_SPLIT_BYTES on the MI355X
(docs/kernels.md, K29): pixels and status words against the CPU reference, torch.equal, and
``dec.paths`` = (intervals the split launches completed, handed back) every time.  Files have
no restart markers unless a test says so."""
import pytest
import torch

import jpeg_decode_cases as dc
import jpeg_decode_parallel_cases as pc
from kvedge_amd import ops
from kvedge_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

CANARY = 0x5A
S = ops.JPEG_DECODE_SPLIT_BYTES
SCRATCH = ("tables", "mpos", "planes", "status", "split", "done", "paths")


def _entropy(f):
    """(offset, length) of a file's entropy-coded bytes, EOI excluded."""
    sos = dc._segment(f, 0xda)
    e0 = sos + 2 + ((f[sos + 2] << 8) | f[sos + 3])
    return e0, len(f) - 2 - e0


def _decode(files, hw, entropy="parallel"):
    """Decode with canary rows around out and every scratch tensor; asserts pixels, status and
    canaries against the reference.  Returns (status, paths) as lists."""
    assert ops.load()
    rgb, status, rows = dc.reference(files, hw)
    n = len(files)
    dec = ops.JpegDecoder(n, hw, rows.shape[1], device="cuda", entropy=entropy)
    guards = []
    for name in SCRATCH if entropy != "serial" else SCRATCH[:4]:
        t = getattr(dec, name)
        whole = torch.full((n + 2,) + tuple(t.shape[1:]), CANARY, dtype=t.dtype, device="cuda")
        setattr(dec, name, whole[1:-1])
        guards.append(whole)
    whole = torch.full((n + 2,) + tuple(hw) + (3,), CANARY, dtype=torch.uint8, device="cuda")
    guards.append(whole)
    got, st = ops.jpeg_decode(torch.from_numpy(rows.copy()).cuda(), dec, out=whole[1:-1])
    torch.cuda.synchronize()
    assert torch.equal(st.cpu(), torch.from_numpy(status.copy())), (st.tolist(), status.tolist())
    diff = (got.cpu() != torch.from_numpy(rgb.copy())).flatten(1).sum(1)
    assert int(diff.sum()) == 0, f"differing bytes per file: {diff.tolist()}"
    for g in guards:
        assert bool((g[0] == CANARY).all()) and bool((g[-1] == CANARY).all())
    return status.tolist(), ([[0, 0]] * n if entropy == "serial" else dec.paths.tolist())


@pytest.mark.parametrize("sub", dc.SUBS)
def test_one_workgroup(sub):
    """40 x 67: partial MCUs both ways, 5 to 55 subsequences."""
    files = [dc.pillow_file(c, 40, 67, sub) for c in ("smooth", "noise")]
    assert all(2 * S < _entropy(f)[1] < 64 * S for f in files)
    assert _decode(files, (40, 67)) == ([0, 0], [[1, 0], [1, 0]])


def test_many_blocks_per_subsequence():
    """Low quality: blocks of an EOB and little else, dozens of block starts per lane."""
    files = [dc.pillow_file(c, 64, 256, "444", "none", q) for c, q in (("bw_blocks", 20),
                                                                       ("smooth", 10))]
    assert all(_entropy(f)[1] * 24 < 768 * S for f in files)  # > 24 of the 768 blocks per S
    assert _decode(files, (64, 256)) == ([0, 0], [[1, 0], [1, 0]])


def _block_starts(f, hw):
    """Row byte of every block's DC symbol in a 4:4:4 file, walked by the reference's reader."""
    info = ref.jpeg_parse_header(f, hw)[1]
    e0, n = _entropy(f)
    seg, pred, starts = f[e0:e0 + n], [0, 0, 0], []
    raw = [i for i in range(n) if not (i and seg[i] == 0 and seg[i - 1] == 0xff)]  # unstuffed -> row
    rd = ref._JdBits(seg)
    for g in range(info["mw"] * info["mh"] * 3):
        starts.append(e0 + raw[rd.c >> 3])
        pred[g % 3] = ref._jd_block(rd, info["h"][info["td"][g % 3]],
                                    info["h"][2 + info["ta"][g % 3]], pred[g % 3])[1]
    return starts


def test_block_longer_than_a_subsequence():
    """Noise at quality 100, 4:4:4: blocks of up to 117 bytes, so some cover a whole
    subsequence: its lane starts and ends inside one block and owns no block start."""
    f = dc.pillow_file("noise", 40, 67, "444", "none", 100)
    e0, n = _entropy(f)
    owned = {b // S for b in _block_starts(f, (40, 67))}
    inner = range(e0 // S + 1, (e0 + n) // S)  # neither the interval's first lane nor its last
    assert sum(m not in owned for m in inner) >= 8
    assert _decode([f], (40, 67)) == ([0], [[1, 0]])


def test_long_codes_and_stuffing_at_the_cut():
    files = pc.stuffed_batch()
    rows = dc.reference(files, pc.HW)[2]
    assert sum(f.count(b"\xff\x00") for f in files) >= 8
    assert any(r[c - 1] == 0xff and r[c] == 0 for f, r in zip(files, rows)
               for c in range(-(-_entropy(f)[0] // S) * S, len(f), S))
    assert _decode(files, pc.HW) == ([0] * 16, [[1, 0]] * 16)


def test_workgroup_seams_and_per_file_lanes():
    """128 x 128 noise: more than two workgroups of 64 lanes; the second file has another size."""
    files = [dc.pillow_file("noise", 128, 128, "444", "none", 95),
             dc.pillow_file("smooth", 128, 128, "420", "none", 50)]
    assert _entropy(files[0])[1] > 2 * 64 * S > _entropy(files[1])[1] > S
    assert _decode(files, (128, 128)) == ([0, 0], [[1, 0], [1, 0]])


def test_restart_intervals_long_and_short():
    """64 x 256 with one MCU row per interval: 8 intervals of several subsequences each; with
    three MCUs per interval at low quality none reaches one, and the old kernel has them all."""
    files = [dc.pillow_file("noise", 64, 256, "444", "row", 95),
             dc.pillow_file("smooth", 64, 256, "420", "3", 30)]
    assert files[0].count(b"\xff\xd0") >= 1 and _entropy(files[0])[1] > 8 * 4 * S
    assert _decode(files, (64, 256)) == ([0, 0], [[8, 0], [0, 0]])


def test_malformed_without_restart_markers():
    """The files tools/jpeg_decode_hostcheck.py ran through the same lane steps under the
    sanitizers: whatever the serial walk calls an entropy error is handed back to it."""
    corpus = pc.malformed_no_dri()
    status, paths = _decode(list(corpus.values()), pc.HW)
    assert paths[0] == [1, 0] and status[0] == 0
    assert any(-s & ops.JPEG_DECODE_ERRORS["entropy"] for s in status)
    for s, p in zip(status, paths):
        assert sum(p) <= 1 and (not -s & ops.JPEG_DECODE_ERRORS["entropy"] or p == [0, 1])


def test_modes_agree():
    files = [dc.pillow_file("noise", 40, 67, "420"), dc.pillow_file("smooth", 40, 67, "420")]
    assert S < _entropy(files[1])[1] < 16 * S < _entropy(files[0])[1]
    assert _decode(files, (40, 67), "serial")[1] == [[0, 0], [0, 0]]
    assert _decode(files, (40, 67), "auto")[1] == [[1, 0], [0, 0]]
    assert _decode(files, (40, 67), "parallel")[1] == [[1, 0], [1, 0]]


def test_graph_replays_keep_no_state():
    assert ops.load()
    sets = [[dc.pillow_file("noise", 40, 67, "420"), pc.malformed_no_dri()["flip_entropy_late"]],
            [dc.pillow_file("smooth", 40, 67, "444"), dc.pillow_file("noise", 40, 67, "422")]]
    n = dc.row_bytes(sets[0] + sets[1])
    dec = ops.JpegDecoder(2, pc.HW, n, device="cuda", entropy="parallel")
    files = torch.zeros(2, n, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, *pc.HW, 3, dtype=torch.uint8, device="cuda")
    ops.jpeg_decode(files, dec, out=out)  # warm up outside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.jpeg_decode(files, dec, out=out)
    for fs, paths in ((sets[0], [[1, 0], [0, 1]]), (sets[1], [[1, 0], [1, 0]]), (sets[0], None)):
        rgb, status, rows = dc.reference(fs, pc.HW, n)
        files.copy_(torch.from_numpy(rows.copy()))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(rgb.copy()))
        assert dec.status.tolist() == status.tolist()
        assert paths is None or dec.paths.tolist() == paths
