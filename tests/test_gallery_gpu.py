"""Appearance search on the GPU (csrc/kernels/gallery.hip): every comparison is torch.equal
against the CPU reference -- codes, nrm2, rows and the fp32 score bits."""
import pytest
import torch

from kvedge_amd import ops
from kvedge_amd.ops import reference
from test_gallery_cpu import embed, planted_features

pytestmark = pytest.mark.gpu
BLOCK = 128  # gallery rows per block of the kernel: ties are planted across its boundaries


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_gallery(codes, count, cap=None, scale=None):
    """A device gallery holding ``codes`` (all ``cap`` rows uploaded, ``count`` of them live)."""
    cap = cap or codes.shape[0]
    gal = ops.Gallery(cap, codes.shape[1], "cuda")
    nrm2 = (codes.long() ** 2).sum(1).clamp_(min=1)
    gal.codes[:codes.shape[0]].copy_(codes)
    gal.scale[:codes.shape[0]].copy_((1.0 / torch.sqrt(nrm2.float())) if scale is None else scale)
    gal.count.fill_(count)
    return gal


def check_match(q, gal, k):
    score, row = ops.gallery_match(q.cuda(), gal, top=k)
    want = reference.gallery_match(q, gal.codes.cpu(), gal.scale.cpu(), gal.count.cpu(),
                                   torch.empty(q.shape[0], k),
                                   torch.empty(q.shape[0], k, dtype=torch.int32))
    assert torch.equal(row.cpu(), want[1]) and torch.equal(score.cpu(), want[0])
    return score.cpu(), row.cpu()


@pytest.mark.parametrize("m,hw,c", [(1, 1, 64), (3, 49, 2048), (2, 256, 4096), (5, 7, 192)])
def test_embed_quantize(m, hw, c):
    x = (torch.randn(m, 1, hw, c, generator=gen(c + hw)) * 4).to(torch.bfloat16)
    x = torch.cat([x, planted_features(c).repeat(1, 1, hw, 1)[:, :, :hw]])
    want = embed(x)
    got = ops.embed_quantize(x.cuda())
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("d", [64, 192, 2048])
@pytest.mark.parametrize("g", [1, 127, 129, 1000])
@pytest.mark.parametrize("m", [1, 33, 257])
def test_gallery_match(m, g, d, k):
    q = torch.randint(-127, 128, (m, d), generator=gen(m + g + d), dtype=torch.int8)
    codes = torch.randint(-127, 128, (g + 3, d), generator=gen(g), dtype=torch.int8)
    codes[g:] = q[0]  # the rows past count would win: they must never be reported
    score, row = check_match(q, make_gallery(codes, g), k)
    assert int(row.max()) < g and (row[:, :min(g, k)] >= 0).all()
    if g < k:
        assert (row[:, g:] == -1).all() and (score[:, g:] == 0).all()


@pytest.mark.parametrize("lo,hi", [(-127, 127), (-2, 2)])
def test_gallery_match_ties(lo, hi):
    """Copies of a row on both sides of a block boundary and in blocks of different
    workgroups come out lowest row first; with codes in -2..2 thousands of scores tie."""
    g, d = 5 * BLOCK, 64
    codes = torch.randint(lo, hi + 1, (g, d), generator=gen(7), dtype=torch.int8)
    q = torch.randint(lo, hi + 1, (4, d), generator=gen(8), dtype=torch.int8)
    sets = [(BLOCK - 1, BLOCK, 4 * BLOCK + 5), (3, 2 * BLOCK - 1, 2 * BLOCK), (0, 1, g - 1)]
    for i, rows in enumerate(sets):
        codes[list(rows)] = q[i]
    scale = torch.full((g,), 0.125)
    scale[77] = 0.0  # a row that does not count
    score, row = check_match(q, make_gallery(codes, g, scale=scale), 8)
    if lo < -2:
        for i, rows in enumerate(sets):
            assert row[i, :3].tolist() == list(rows)
    assert not (row == 77).any()


def test_gallery_match_persistent_walk():
    g, d = 70001, 64
    codes = torch.randint(-127, 128, (g, d), generator=gen(9), dtype=torch.int8)
    q = torch.randint(-127, 128, (5, d), generator=gen(10), dtype=torch.int8)
    codes[[5, 100, g - 1]] = q[0]
    codes[[0, g - 2]] = q[4]
    _, row = check_match(q, make_gallery(codes, g), 8)
    assert row[0, :3].tolist() == [5, 100, g - 1] and row[4, :2].tolist() == [0, g - 2]


def test_gallery_match_live_count_under_graph():
    d = 192
    codes, nrm2 = embed((torch.randn(40, 1, 2, d, generator=gen(11)) * 2).to(torch.bfloat16))
    gal = ops.Gallery(300, d, "cuda").enrol(codes[1:], nrm2[1:], 1)
    q = codes[:1].cuda()
    score = torch.empty(1, 2, device="cuda")
    row = torch.empty(1, 2, dtype=torch.int32, device="cuda")
    ops.gallery_match(q, gal, 2, score, row)  # warm
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gallery_match(q, gal, 2, score, row)
    for _ in range(2):
        graph.replay()
    eager = ops.gallery_match(q, gal, 2)
    assert torch.equal(row, eager[1]) and torch.equal(score, eager[0]) and int(row[0, 0]) != 39
    gal.enrol(codes[0], nrm2[0], 2)  # the query itself: row 39, cosine 1
    for _ in range(2):
        graph.replay()
    assert int(row[0, 0]) == 39 and int(row[0, 1]) == int(eager[1][0, 0])
    assert abs(float(score[0, 0]) * float(nrm2[0]) ** -0.5 - 1.0) < 1e-6


def test_gallery_match_beyond_2gib():
    cap, d = 524800, 4096
    gal = ops.Gallery.__new__(ops.Gallery)  # device tensors only: no 2 GiB host mirror
    gal.capacity, gal.dim = cap, d
    gal.codes = torch.randint(-127, 128, (cap, d), dtype=torch.int8, device="cuda")
    nrm2 = torch.empty(cap, dtype=torch.int64, device="cuda")
    for lo in range(0, cap, 65600):  # the squares in slices: no 8 GiB temporary
        nrm2[lo:lo + 65600] = (gal.codes[lo:lo + 65600].to(torch.int32) ** 2).sum(1)
    nrm2 = nrm2.float()
    gal.scale = (1.0 / torch.sqrt(nrm2.cpu())).cuda()
    gal.count = torch.tensor([cap], dtype=torch.int32, device="cuda")
    rows = [524288, 524799]
    score, row = ops.gallery_match(gal.codes[rows].clone(), gal, top=1)
    assert row.flatten().tolist() == rows
    cos = score.flatten().cpu() * torch.rsqrt(nrm2[rows].cpu())
    assert (cos - 1.0).abs().max() < 1e-6


def test_gallery_match_refusals():
    q = torch.zeros(2, 64, dtype=torch.int8, device="cuda")
    gal = make_gallery(torch.ones(4, 64, dtype=torch.int8), 4)
    score = torch.full((2, 1), 7.0, device="cuda")
    row = torch.full((2, 1), 7, dtype=torch.int32, device="cuda")
    part = torch.empty(4096, dtype=torch.int32, device="cuda")
    k = torch.ops.kvedge.gallery_match
    big = torch.empty(2 ** 20 + 1, 64, dtype=torch.int8, device="cuda")
    bad = [
        (q[:, :0].new_zeros(2, 96), gal.codes.new_zeros(4, 96), gal.scale, score, row),  # D = 96
        (q, gal.codes, gal.scale, torch.full((2, 9), 7.0, device="cuda"),
         torch.full((2, 9), 7, dtype=torch.int32, device="cuda")),                       # K = 9
        (q, big, torch.ones(2 ** 20 + 1, device="cuda"), score, row),                    # cap
        (q.cpu(), gal.codes, gal.scale, score, row),                                     # devices
    ]
    for qq, codes, scale, s, r in bad:
        with pytest.raises(RuntimeError, match="kvedge"):
            k(qq, codes, scale, gal.count, part, s, r)
        assert (s == 7).all() and (r == 7).all()
    for kw in (dict(q_codes=q.cpu()), dict(top=9), dict(q_codes=q[:, :0].new_zeros(2, 96))):
        with pytest.raises(ValueError):
            ops.gallery_match(**dict(dict(q_codes=q, gallery=gal, out_score=score, out_row=row), **kw))
    with pytest.raises(ValueError):
        ops.Gallery(2 ** 20 + 1, 64)
    assert (score == 7).all() and (row == 7).all()


def test_module_gallery_enrol_without_recapture(tmp_path):
    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    tr = FakeTransport({"model": "detect-classify", "batch": 2, "crops_per_image": 2,
                        "report_interval_s": 0.01, "conf": 0.0, "max_det": 8,
                        "gallery": str(tmp_path / "g.npz"), "gallery_threshold": -1.0})
    with ModuleApp(tr, device="cuda").start() as app:
        graph = app.engine.graph
        assert graph is not None and tr.reported["config"]["gallery_threshold"] == -1.0
        app.run(max_steps=2)
        assert app.report()["matches"] == {} and app.on_method("gallery_remove", {})[0] == 400
        assert app.on_method("gallery_enrol", {"camera": 1, "row": 0, "label": 42})[0] == 200
        assert app.on_method("gallery_enrol", {"camera": 2, "row": 0, "label": 1})[0] == 400
        app.run(max_steps=2)
        t = app.report()
        torch.cuda.synchronize()
        count = app.engine.outputs[1].cpu()
        want = [[n, k] for n in range(2) for k in range(2) if k < int(count[n])]
        # one row enrolled, threshold -1: every real crop reports it, from the same graph
        assert sorted(r[:2] for r in t["match_rows"]) == want and want
        assert {r[2] for r in t["match_rows"]} == {42} and t["matches"] == {"42": len(want)}
        assert app.engine.graph is graph and app.state["rebuilds"] == 0
        assert app.on_method("gallery_remove", {"label": 42})[1] == {"removed": 1, "rows": 0}


@pytest.fixture(scope="module")
def cascade_parts():
    from kvedge_amd.models.resnet import KvResNet50, init_resnet50
    from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n

    assert ops.load()
    return (KvYoloV8n(init_yolov8n(0), "cuda", conf=0.0, max_det=8),
            KvResNet50(init_resnet50(seed=0), "cuda"))


def test_cascade_with_gallery_eager_and_graph(cascade_parts):
    from kvedge_amd.engine import InferenceEngine
    from kvedge_amd.models.cascade import KvDetectClassify

    det, clf = cascade_parts
    frames = torch.randint(0, 256, (2, 640, 640, 3), generator=gen(12), dtype=torch.uint8).cuda()
    plain = KvDetectClassify(det, clf, 2)(frames)
    gal = ops.Gallery(256, 2048, "cuda")
    m = KvDetectClassify(det, clf, 2, gallery=gal, gallery_top=2, gallery_threshold=-1.0)
    out = m(frames)
    assert len(out) == 6 and all(torch.equal(a, b) for a, b in zip(out[:4], plain))
    assert int(out[1].min()) >= 2 and (out[4] == -1).all()
    # enrol the crops' own embeddings plus noise rows, then match by hand
    codes, nrm2 = (t.cpu() for t in m.embedding)
    noise = embed((torch.randn(100, 1, 1, 2048, generator=gen(13))).to(torch.bfloat16))
    gal.enrol(noise[0], noise[1], 5).enrol(codes, nrm2, [10, 11, 12, 13])
    label, cos = m(frames)[4:]
    crops = ops.roi_crop(frames, out[0], out[1], 2, 224)
    c2, n2 = ops.embed_quantize(clf.raw_features(crops))
    assert torch.equal(c2.cpu(), codes) and torch.equal(n2.cpu(), nrm2)
    score, row = ops.gallery_match(c2, gal, 2)
    want_cos = score * torch.rsqrt(n2.float()).view(-1, 1)
    assert torch.equal(cos.view(4, 2), want_cos)
    assert torch.equal(label.view(4, 2), gal.label[row.long()])
    assert label[..., 0].flatten().tolist() == [10, 11, 12, 13]
    assert (cos[..., 0] - 1.0).abs().max() < 1e-6
    # the same step captured by the engine
    eng = InferenceEngine(m, 2, 640, device="cuda", seed=5).prepare(warmup=1, autotune=False)
    assert eng.graph is not None
    for _ in range(2):
        got = eng.run()
    torch.cuda.synchronize()
    eager = m(eng.frames.clone())
    assert len(got) == 6 and all(torch.equal(a, b) for a, b in zip(got, eager))
