"""Walk KvResNet50 and KvYoloV8n op by op on the GPU against the CPU reference (shadow.py):
every HIP kernel at single-op tolerance where it actually runs -- the models' own buffers,
channel offsets, dispatch gates and heuristic tile picks -- in every dispatch regime, plus
every explicit tile at every model layer key (the launches the autotuner makes).

Frames are small so each test takes seconds and every stage has partial tiles: ResNet
3 x 88 x 72 is 22 x 18 after the pool, then 11 x 9, 6 x 5, 3 x 3 (1188 / 297 / 90 / 27 rows:
none a multiple of 64, stride-2 layers on odd extents).

With KVEDGE_WALK_LOG=<existing directory> every test writes its harness log there as
model_walk_<test>.json: one record per call (op, key, tile, max err, rrms), one per swept key
(accepted tiles, refused tiles and their codes) and the per-tile acceptance counts.
"""
import pytest
import torch

import kernel_rules
from kvedge_amd import ops
from kvedge_amd.models import resnet as resnet_mod
from kvedge_amd.models import yolov8 as yolo_mod
from kvedge_amd.models.resnet import KvResNet50, init_resnet50
from kvedge_amd.models.yolov8 import KvYoloV8n, init_yolov8n
from shadow import is_canary, shadow

pytestmark = pytest.mark.gpu

YOLO_CONF = 1e-3  # the seeded random-init heads score 2e-5 .. 0.4: about 40 % of anchors pass
TAIL_BLOCKS = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11]  # test_resnet_tail_and_seam_plumbing's list


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load(), "native kvedge library must be loaded on the GPU box"


def _frames(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.fixture(scope="module")
def resnet():
    return KvResNet50(init_resnet50(0, calibrate=True, calib_batch=2, calib_hw=96), "cuda")


@pytest.fixture(scope="module")
def yolo():
    return KvYoloV8n(init_yolov8n(0, calibrate=True), "cuda")


# ---------------------------------------------------------------------------
# regimes: (attribute owner, name, value) triples applied with monkeypatch.setattr
# ---------------------------------------------------------------------------
FUSED = [(resnet_mod, "TAIL1_MIN_ROWS", 0), (ops, "SEAM_MIN_WGS", 1)]
_EDGE = {"stem12_pool_frames", "conv2d", "conv_dual", "global_avgpool", "softmax_rows"}
RESNET_REGIMES = {
    # name -> (settings ("kv" = the model instance), entry point, EXACTLY the op kinds walked:
    # what a switch turns off must be gone, not only what it turns on be there)
    "edge": ([], "call", _EDGE),
    "fused": (FUSED, "call", _EDGE | {"conv_tail"}),
    "fused_mb3": (FUSED + [("kv", "microbatch", 1), ("kv", "microbatch_blocks", 3)], "call",
                  _EDGE | {"conv_tail"}),
    "fused_mb5": (FUSED + [("kv", "microbatch", 1), ("kv", "microbatch_blocks", 5)], "call",
                  _EDGE | {"conv_tail"}),
    "fuse_head": ([("kv", "fuse_head", True)], "call",
                  _EDGE - {"global_avgpool"} | {"pooled_fc"}),
    "stem16": ([("kv", "stem12", False)], "call",
               _EDGE - {"stem12_pool_frames"} | {"stem_pool_frames"}),
    "no_fuse_preprocess": ([("kv", "fuse_preprocess", False)], "raw",
                           {"preprocess", "stem_pool", "conv2d", "conv_dual", "global_avgpool"}),
    "no_fuse_stem_pool": ([("kv", "fuse_stem_pool", False)], "raw",
                          {"preprocess", "conv2d", "maxpool2d", "conv_dual", "global_avgpool"}),
}
_YOLO = {"yolo_stem2", "conv2d", "conv_dual2", "conv_pair", "sppf_pool", "yolo_decode", "nms"}
YOLO_REGIMES = {
    # name -> (settings, exactly the op kinds walked where b2 runs unfused; + c2f16 where the
    # fused form takes b2, i.e. at 320 x 320 unless the regime turns it off)
    "defaults": ([], _YOLO),
    "no_fuse_up": ([("kv", "fuse_up", False)], _YOLO - {"conv_dual2"} | {"upsample2x"}),
    "no_fuse_b1": ([("kv", "fuse_b1", False)], _YOLO - {"yolo_stem2"} | {"stem_from_frames"}),
    "no_fuse_preprocess": ([("kv", "fuse_b1", False), ("kv", "fuse_preprocess", False)],
                           _YOLO - {"yolo_stem2"} | {"preprocess"}),
    "no_fuse_pairs": ([(yolo_mod.DDetectLevel, "fuse_pairs", False)], _YOLO - {"conv_pair"}),
    "no_c2f": ([(ops, "C2F_ENABLED", False)], _YOLO),
}


def _apply(monkeypatch, kv, settings):
    for owner, name, value in settings:
        monkeypatch.setattr(kv if owner == "kv" else owner, name, value)


def _tail_blocks(kv, sh):
    """Bottleneck indices whose boundary ran as ops.conv_tail, from the log's weight pointers."""
    by_w = {}
    for i, b in enumerate(kv.blocks):
        by_w[(b.dual.w if b.dual is not None else b.c3.w).data_ptr()] = i
    return sorted({by_w[r["w_ptr"]] for r in sh.log if r["op"] == "conv_tail"})


def _walk_resnet(kv, frames, regime, monkeypatch, tag, sweep=False):
    settings, entry, kinds = RESNET_REGIMES[regime]
    _apply(monkeypatch, kv, settings)
    with shadow(monkeypatch, sweep=sweep) as sh:
        try:
            with torch.no_grad():
                out = kv(frames) if entry == "call" else kv.raw_outputs(frames)
        finally:
            sh.write_log(tag)
    torch.cuda.synchronize()
    assert sh.op_kinds() == kinds, (regime, sorted(sh.op_kinds()))
    last = out[0] if entry == "call" else out
    assert torch.isfinite(last.float()).all()
    fused = any(s[1] == "TAIL1_MIN_ROWS" for s in settings)
    assert _tail_blocks(kv, sh) == (TAIL_BLOCKS if fused else []), regime
    return sh


@pytest.mark.parametrize("regime", list(RESNET_REGIMES))
def test_resnet_walk(resnet, regime, monkeypatch):
    sh = _walk_resnet(resnet, _frames(3, 88, 72, 1), regime, monkeypatch, f"resnet_{regime}")
    w = sh.worst()
    print(f"resnet {regime}: {len(sh.log)} calls, worst rrms {w['rrms']:.3g} max err "
          f"{w['max_err']:.3g} at call {w['i']} {w['op']}")


@pytest.mark.parametrize("regime", ["edge", "fused"])
def test_resnet_walk_224(resnet, regime, monkeypatch):
    """The real geometry, one frame: 56 / 28 / 14 / 7."""
    sh = _walk_resnet(resnet, _frames(1, 224, 224, 2), regime, monkeypatch,
                      f"resnet224_{regime}")
    w = sh.worst()
    print(f"resnet224 {regime}: worst rrms {w['rrms']:.3g} at call {w['i']} {w['op']}")


def _walk_yolo(kv, frames, regime, monkeypatch, tag, sweep=False):
    settings, kinds = YOLO_REGIMES[regime]
    _apply(monkeypatch, kv, settings)
    monkeypatch.setattr(kv, "conf", YOLO_CONF)
    heads = []
    monkeypatch.setattr(kv, "keep_heads", heads)
    with shadow(monkeypatch, sweep=sweep) as sh:
        try:
            with torch.no_grad():
                det, count = kv(frames)
        finally:
            sh.write_log(tag)
    torch.cuda.synchronize()
    c2f = frames.shape[2] in (320, 640) and regime != "no_c2f"  # b2 at 80 / 160 wide
    assert sh.op_kinds() == kinds | ({"c2f16"} if c2f else set()), (regime, sorted(sh.op_kinds()))
    assert sh.log[-1]["op"] == "nms" and sh.log[-1]["kept"] > 0  # the comparison saw real rows
    assert int(count.sum()) == sh.log[-1]["kept"]
    assert all(torch.isfinite(f.float()).all() for f in heads[0])
    # concat buffers [N, h, w, 192 | 384] of heads(): the upsampled halves of cat14 (192 wide,
    # the larger map) and cat11 (384 wide, the larger map) are written by upsample2x only
    cats = [t for t in sh.allocs if t.dim() == 4 and t.shape[3] in (192, 384)
            and t.shape[1] == t.shape[2] and t.dtype == torch.bfloat16]
    h3 = max(t.shape[1] for t in cats)
    cat14 = [t for t in cats if t.shape[3] == 192 and t.shape[1] == h3]
    cat11 = [t for t in cats if t.shape[3] == 384 and t.shape[1] == h3 // 2]
    assert len(cat14) == 1 and len(cat11) == 1
    up_halves = [cat14[0][..., :128], cat11[0][..., :256]]
    if kv.fuse_up:
        assert all(bool(is_canary(h).all()) for h in up_halves), "fuse_up wrote the unused half"
    else:
        assert not any(bool(is_canary(h).any()) for h in up_halves)
    assert torch.isfinite(cat14[0][..., 128:].float()).all()
    assert torch.isfinite(cat11[0][..., 256:].float()).all()
    return sh


@pytest.mark.parametrize("regime", list(YOLO_REGIMES))
def test_yolo_walk_96(yolo, regime, monkeypatch):
    """2 x 96 x 96: P3 / P4 / P5 = 12 / 6 / 3 squared, the unfused C2f path at b2."""
    sh = _walk_yolo(yolo, _frames(2, 96, 96, 3), regime, monkeypatch, f"yolo96_{regime}")
    w = sh.worst()
    print(f"yolo96 {regime}: {len(sh.log)} calls, worst rrms {w['rrms']:.3g} max err "
          f"{w['max_err']:.3g} at call {w['i']} {w['op']}")


@pytest.mark.parametrize("regime", list(YOLO_REGIMES))
def test_yolo_walk_320(yolo, regime, monkeypatch):
    """1 x 320 x 320: b2 at 80 x 80, where the fused c2f16 form runs."""
    sh = _walk_yolo(yolo, _frames(1, 320, 320, 4), regime, monkeypatch, f"yolo320_{regime}")
    w = sh.worst()
    print(f"yolo320 {regime}: worst rrms {w['rrms']:.3g} at call {w['i']} {w['op']}")


# ---------------------------------------------------------------------------
# tile sweep: every explicit tile at every model layer key
# ---------------------------------------------------------------------------
SWEEPS = {
    "resnet_edge": ("resnet", (3, 88, 72), "edge"),
    "resnet_fused": ("resnet", (3, 88, 72), "fused"),
    "yolo96_defaults": ("yolo", (2, 96, 96), "defaults"),
    "yolo96_no_fuse_up": ("yolo", (2, 96, 96), "no_fuse_up"),
    "yolo320_defaults": ("yolo", (1, 320, 320), "defaults"),
}
_sweeps = {}  # sweep name -> Shadow, or the exception its run ended with


def _sweep(name, resnet, yolo):
    """The sweep's harness, run once per session whichever test asks first: the coverage
    test below needs all five and must not depend on file order or on -k.  A run that
    raised is not run again."""
    if name not in _sweeps:
        model, (n, h, w), regime = SWEEPS[name]
        with pytest.MonkeyPatch.context() as mp:
            try:
                if model == "resnet":
                    _sweeps[name] = _walk_resnet(resnet, _frames(n, h, w, 1), regime, mp,
                                                 f"sweep_{name}", sweep=True)
                else:
                    _sweeps[name] = _walk_yolo(yolo, _frames(n, h, w, 3), regime, mp,
                                               f"sweep_{name}", sweep=True)
            except Exception as e:  # noqa: BLE001 -- kept, and raised again for every asker
                _sweeps[name] = e
    if isinstance(_sweeps[name], Exception):
        raise _sweeps[name]
    return _sweeps[name]


# conv-table tiles that take no layer key of either model at these sizes, with the guard of
# their launcher that excludes them (test_tile_table_is_covered fails on any tile missing
# here that accepted nothing, and on any tile listed here that did accept a key)
NO_MODEL_KEY = {
    # the last seam tile is the stage 3 -> 4 form (K3 256 -> n_t 512): seam_launch() refuses
    # any other n_t (n_t != nzc * 64 -> rc=-8), and ops.SEAM_SHAPES leaves that boundary
    # unfused (block 12 is not in TAIL_BLOCKS), so no conv_tail call of the model has its key.
    # test_kernels_gpu.py::test_conv_seam runs it at (2, 14, 14, 256, 512)
    kernel_rules.N_TILES + 15: "conv_seam.hip seam_launch(): p->n_t != e.nzc * 64",
}


@pytest.mark.parametrize("name", list(SWEEPS))
def test_tile_sweep(name, resnet, yolo):
    """Each distinct (op, spec, shapes, offsets, residual) key of the forward is re-issued with
    every tile of the table (conv_tail: the seam tiles too; conv_pair: direct tiles 0-3) on
    the model's own operands.  A launcher either refuses -- and then has written nothing --
    or its result passes the same single-op comparison as the heuristic pick."""
    sh = _sweep(name, resnet, yolo)
    assert sh.sweeps
    for s in sh.sweeps:
        # the heuristic pick ran (the call as issued is compared before the sweep) and at
        # least one explicit tile takes the key
        assert s["accepted"], ("no explicit tile takes this key", s["op"], s["key"])
    print(f"sweep {name}: {len(sh.sweeps)} keys, "
          f"{sum(len(s['accepted']) for s in sh.sweeps)} accepted (key, tile) launches")


def test_tile_table_is_covered(resnet, yolo):
    """Over the five sweeps together no tile family is left unexercised, and every single tile
    that took no key is explained in NO_MODEL_KEY."""
    accepted = [_sweep(name, resnet, yolo).accepted for name in SWEEPS]
    n_tiles = int(torch.ops.kvedge.conv_num_tiles())
    n_seam = int(torch.ops.kvedge.conv_seam_num_tiles())
    assert n_tiles == kernel_rules.N_TILES
    took = {}
    for acc in accepted:
        for (op, t), k in acc.items():
            if op != "conv_pair":  # its tile numbers are the direct family's own 0-3
                took[t] = took.get(t, 0) + k
    pair = {t for acc in accepted for (op, t) in acc if op == "conv_pair"}
    assert pair, "no conv_pair tile accepted a Detect branch"
    families = dict(kernel_rules.FAMILIES, seam=range(n_tiles, n_tiles + n_seam))
    empty = [f for f, r in families.items() if not any(took.get(t) for t in r)]
    assert not empty, ("tile families no model key exercises", empty)
    idle = sorted(t for t in range(n_tiles + n_seam) if not took.get(t))
    assert idle == sorted(NO_MODEL_KEY), ("unexplained idle tiles", sorted(set(idle) - set(NO_MODEL_KEY)),
                                          "listed but not idle", sorted(set(NO_MODEL_KEY) - set(idle)))
