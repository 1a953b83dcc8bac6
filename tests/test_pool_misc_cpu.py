"""Pins the float64 oracles of pool_oracles.py before the GPU file relies on them: for every
case the GPU file runs, the oracle and the CPU path of kvedge_amd.ops (ops.reference) agree
within the bound stated for that kernel, the accept / refuse mirrors return what the case
tables expect, and the special-value inputs keep the oracle free of NaN.
"""
import itertools

import numpy as np
import pytest
import torch

import pool_oracles as po
from kvedge_amd import ops

BF16 = torch.bfloat16


def test_ulp16_and_round_bf16():
    v = torch.tensor([1.0, 1.9999, 2.0, 255.0, 0.0, 2.0 ** -126, 2.0 ** -133, -3.0],
                     dtype=torch.float64)
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133, 2.0 ** -6]
    assert po.ulp16(v).tolist() == want
    # every bf16 value is a fixed point, the midpoint of two neighbours goes to the even one
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    fin = allb[torch.isfinite(allb.float())].double()
    assert torch.equal(po.round_bf16(fin), fin)
    assert po.round_bf16(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8],
                                      dtype=torch.float64)).tolist() == [1.0, 1.0 + 2.0 ** -6]
    x = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    assert torch.equal(po.round_bf16(x.float().double()), x.float().to(BF16).double())


def test_special_data_has_what_it_claims():
    x = po.make_data((2, 8, 30, 24), "special", 1)
    f = x.float()
    assert not torch.isnan(f).any()
    assert (f == po.INF).any() and (f == -po.INF).any()
    b = po.bits(x)
    assert (b == 0).any() and (b == -32768).any()                   # +0 and -0
    sub = (f != 0) & (f.abs() < 2.0 ** -126)
    assert (sub & (f > 0)).any() and (sub & (f < 0)).any()          # subnormals of both signs
    assert (po.make_data((2, 7, 5, 8), "negative", 1).float() < 0).all()
    assert (po.make_data((2, 7, 5, 8), "neg_inf", 1).float() == -po.INF).all()


# ---- maxpool2d --------------------------------------------------------------------------
@pytest.mark.parametrize("ksp", po.MAXPOOL_KSP)
def test_maxpool_oracle_vs_reference(ksp):
    k, s, p = ksp
    shapes = po.maxpool_shapes(ksp)
    assert {(H, W) for H, W, _ in shapes} >= {(7, 5), (8, 30)} and len(shapes) >= 6
    for (H, W, C), kind, sliced in itertools.product(shapes, po.DATA, (False, True)):
        c = po.maxpool_case(ksp, H, W, C, kind, sliced)
        ctx = (ksp, H, W, C, kind, sliced)
        assert not torch.isnan(c["ref"]).any(), ctx
        if kind == "neg_inf":
            assert (c["ref"].float() == -po.INF).all(), ctx
        if sliced:
            got = ops.maxpool2d(c["x"], k, s, p, out=c["out0"].clone(), C=C, x_coff=c["x_coff"],
                                y_coff=c["y_coff"])
            po.check_slice_written(got, c["out0"], c["ref"], C, c["y_coff"], ctx)
        else:
            got = ops.maxpool2d(c["x"], k, s, p)
            assert torch.equal(got, c["ref"]) and not torch.isnan(got).any(), ctx


def test_maxpool_keeps_subnormals_and_zero_signs():
    """The oracle returns its inputs unchanged: a window of subnormals gives the largest."""
    x = po._from_bits([0x0001, 0x8001, 0x007f, 0x8000]).view(1, 2, 2, 1).repeat(1, 1, 1, 8)
    y = po.maxpool_oracle(x, 2, 2, 0)
    assert (po.bits(y) == 0x007f).all()
    x = po._from_bits([0x8001, 0x8040, 0x807f, 0xff80]).view(1, 2, 2, 1).repeat(1, 1, 1, 8)
    assert (po.bits(po.maxpool_oracle(x, 2, 2, 0)) == 0x8001 - 65536).all()


def test_maxpool_grid_stride_case():
    shape, (k, s, p) = po.MAXPOOL_GRID_STRIDE
    Ho, Wo = po.pool_out(shape[1], shape[2], k, s, p)
    assert shape[0] * Ho * Wo * shape[3] // 8 == 583680 > 2048 * 256
    x = po.make_data(shape, "randn", 5)
    assert torch.equal(ops.maxpool2d(x, k, s, p), po.maxpool_oracle(x, k, s, p))


def _slice_call(op, case, device="cpu"):
    """One SLICE_CASES call of maxpool2d (3x3/2 pad 1) or upsample2x; both tensors are views
    into larger allocations."""
    C, ldx, x_coff, ldy, y_coff, dh, _ = po.SLICE_CASES[case]
    N, H, W = 2, 6, 4
    Ho, Wo = (3, 2) if op == "maxpool2d" else (12, 8)
    x = po.view_in_slab((N, H, W, ldx), device=device, fill=1.0)
    out = po.view_in_slab((N, Ho + dh, Wo, ldy), device=device, fill=2.0)
    if op == "maxpool2d":
        ops.maxpool2d(x, 3, 2, 1, out=out, C=C, x_coff=x_coff, y_coff=y_coff)
    else:
        ops.upsample2x(x, out, C=C, x_coff=x_coff, y_coff=y_coff)
    return out, (C, y_coff)


@pytest.mark.parametrize("op", ["maxpool2d", "upsample2x"])
@pytest.mark.parametrize("case", list(po.SLICE_CASES))
def test_slice_refusals_cpu(op, case):
    C, ldx, x_coff, ldy, y_coff, dh, accepted = po.SLICE_CASES[case]
    want = (2, 3, 2) if op == "maxpool2d" else (2, 12, 8)
    got_nhw = (want[0], want[1] + dh, want[2])
    assert po.slices_accept(C, ldx, x_coff, ldy, y_coff, got_nhw, want) == accepted
    if accepted:
        out, (C, yc) = _slice_call(op, case)
        assert (out[..., yc:yc + C] == 1).all() and (out[..., :yc] == 2).all()
        assert (out[..., yc + C:] == 2).all()
    else:
        with pytest.raises(ValueError):
            _slice_call(op, case)


# ---- sppf_pool --------------------------------------------------------------------------
def test_sppf_accept_mirror():
    assert [po.sppf_lds(h, w) for h, w in po.SPPF_LARGE_MAPS] == [67584, 102400, 163840]
    assert all(po.sppf_accepts(h, w, 16) for h, w in po.SPPF_SMALL_MAPS + po.SPPF_LARGE_MAPS)
    assert po.sppf_lds(*po.SPPF_REFUSED) == 165312 and not po.sppf_accepts(*po.SPPF_REFUSED, 16)
    assert not po.sppf_accepts(5, 5, 24) and po.sppf_accepts(5, 5, 48)
    assert len(po.sppf_shapes()) == 6 * 2 * 2 + 3


@pytest.mark.parametrize("kind", po.DATA)
def test_sppf_oracle_vs_reference(kind):
    for N, H, W, C in po.sppf_shapes():
        c = po.sppf_case(N, H, W, C, kind)
        assert not torch.isnan(c["ref"]).any()
        po.check_sppf(ops.sppf_pool(c["buf"].clone(), C), c, (N, H, W, C, kind))


def test_sppf_is_mp5_mp9_mp13():
    """The chained oracle equals the single wide windows (what the models rely on)."""
    c = po.sppf_case(1, 12, 20, 16, "special")
    x = c["buf"][..., :16].contiguous()
    wide = torch.cat([po.maxpool_oracle(x, k, 1, k // 2) for k in (5, 9, 13)], dim=3)
    assert torch.equal(po.bits(wide), po.bits(c["ref"]))


# ---- global_avgpool ---------------------------------------------------------------------
@pytest.mark.parametrize("hw", po.AVG_EXACT_HW + po.AVG_BOUND_HW)
def test_avgpool_oracle_vs_reference(hw):
    for C, N in itertools.product(po.AVG_C, po.AVG_N):
        c = po.avgpool_case(N, hw[0], hw[1], C)
        assert c["x"].float().abs().max() <= 8 and torch.equal(c["x"].float(), c["x"].float().round())
        # the CPU path rounds a correctly rounded fp32 mean: inside the bound, not bit-pinned
        po.check_avgpool(ops.global_avgpool(c["x"]), c, False, (hw, C, N))


def test_avgpool_mirror_and_grid_stride_case():
    assert all(po.avgpool_accepts(C) for C in po.AVG_C)
    assert not any(po.avgpool_accepts(C) for C in po.AVG_REFUSED_C)
    N, H, W, C = po.AVG_GRID_STRIDE
    assert N * (C // 8) * 8 == 526336 > 2048 * 256
    c = po.avgpool_case(N, H, W, C)
    po.check_avgpool(ops.global_avgpool(c["x"]), c, True, "grid-stride")


# ---- softmax_rows -----------------------------------------------------------------------
def test_softmax_path_mirror():
    for cols, path in po.SOFTMAX_COLS.items():
        assert po.softmax_path(cols) == path, cols
    assert po.softmax_path(1000, aligned=False) == "strided"
    assert sorted(c for c, p in po.SOFTMAX_COLS.items() if p == "register") == [8, 16, 1000, 1016, 1024]
    assert sorted(c for c, p in po.SOFTMAX_COLS.items() if p == "strided") == [1, 7, 1001, 1032, 2000, 4096]


@pytest.mark.parametrize("cols", list(po.SOFTMAX_COLS))
def test_softmax_oracle_vs_reference(cols):
    plants = po.softmax_plants(cols)
    seen = set()
    for rows, scale, x, used in po.softmax_cases(cols):
        seen |= set(used)
        p, am = ops.softmax_rows(x)
        po.check_softmax(p, am, x, used, (cols, rows, scale))
        p64, _, first = po.softmax_oracle(x)
        assert torch.allclose(p64.sum(1), torch.ones(rows, dtype=torch.float64), atol=1e-12)
        for r, name in enumerate(used):
            if name.startswith("tie") or name in ("max_first", "max_last"):
                assert int(first[r]) == plants[name][0], (cols, name)  # the lower planted column
            if name == "all_equal":
                assert torch.allclose(p64[r], torch.full((cols,), 1.0 / cols, dtype=torch.float64))
    assert seen == set(plants), (cols, seen)
    if cols >= 128:
        assert set(plants) == {"tie_in_chunk", "tie_halves", "tie_lanes", "tie_stride64",
                               "max_first", "max_last", "all_equal", "neg_inf"}


def test_softmax_plants_sit_where_they_claim():
    for cols in (16, 1000, 1016, 1024):  # register path: lane = c // 16, half = (c % 16) // 8
        P = po.softmax_plants(cols)
        a, b = P["tie_in_chunk"]
        assert a // 8 == b // 8
        a, b = P["tie_halves"]
        assert a // 16 == b // 16 and a % 16 == 7 and b % 16 == 8
    for cols in (1000, 1016, 1024):
        a, b = po.softmax_plants(cols)["tie_lanes"]
        assert a // 16 != b // 16
    for cols in (1001, 1032, 2000, 4096):  # strided path: lane = c % 64
        a, b = po.softmax_plants(cols)["tie_stride64"]
        assert b - a == 64 and b < cols
        a, b = po.softmax_plants(cols)["tie_lanes"]
        assert a % 64 != b % 64


def test_softmax_misaligned_view():
    xv, x, used = po.softmax_misaligned()
    assert xv.is_contiguous() and xv.data_ptr() % 16 == 6 and torch.equal(xv, x)
    p, am = ops.softmax_rows(xv)
    po.check_softmax(p, am, x, used, "misaligned")


# ---- preprocess -------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [po.IMAGENET, po.UNIT])
def test_preprocess_fp32_formula_meets_the_bound(norm):
    """The kernel's fp32 formula (no FMA contraction) on all 256 x 3 byte values: inside
    ulp16/2 + 1e-6 of float64, and in fact the correctly rounded float64 value."""
    mean, std = norm
    x = po.all_bytes_frame()
    ref = po.preprocess_oracle(x, mean, std, False)[..., :3]
    model = po.preprocess_kernel_model(x, mean, std)
    ratio = ((model.double() - ref).abs() / po.preprocess_bound(ref)).max().item()
    assert ratio <= 1.0, ratio
    assert torch.equal(model.double(), po.round_bf16(ref))


@pytest.mark.parametrize("s2d", [False, True])
@pytest.mark.parametrize("norm", [po.IMAGENET, po.UNIT])
def test_preprocess_oracle_vs_reference(norm, s2d):
    mean, std = norm
    x = po.all_bytes_frame()
    for c in range(3):
        assert sorted(x[0, :, :, c].flatten().tolist()) == list(range(256))
    po.check_preprocess(ops.preprocess(x, mean=mean, std=std, s2d=s2d), x, mean, std, s2d, (norm, s2d))


@pytest.mark.parametrize("shape", po.PRE_LAYOUT_SHAPES)
def test_preprocess_layout_cpu(shape):
    x = po.layout_frame(shape)
    mean, std = po.BYTE_NORM
    y4 = ops.preprocess(x, mean=mean, std=std)
    assert torch.equal(y4[..., :3].float(), x.float()) and (po.bits(y4)[..., 3] == 0).all()
    y = ops.preprocess(x, mean=mean, std=std, s2d=True)
    N, H, W, _ = shape
    for n, by, bx, dy, dx, c in itertools.product(range(N), range(H // 2), range(W // 2),
                                                  range(2), range(2), range(3)):
        assert float(y[n, by, bx, (dy * 2 + dx) * 4 + c]) == float(x[n, 2 * by + dy, 2 * bx + dx, c])
    assert torch.equal(y.double(), po.preprocess_oracle(x, mean, std, True))


def test_preprocess_mirror_and_grid_stride_cases():
    for N, H, W, s2d, accepted in po.PRE_ACCEPT_CASES:
        assert po.preprocess_accepts(N, H, W, s2d) == accepted, (N, H, W, s2d)
    for s2d, shape in po.PRE_GRID_STRIDE.items():
        N, H, W, _ = shape
        assert (N * (H // 2) * (W // 2) if s2d else N * H * W // 2) == 525312 > 2048 * 256
        x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
        mean, std = po.IMAGENET
        po.check_preprocess(ops.preprocess(x, s2d=s2d), x, mean, std, s2d, shape)


# ---- batchnorm_nhwc ---------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
def test_bn_oracle_vs_reference(relu):
    for shape in [(3, 5, 7, C) for C in po.BN_C] + [po.BN_GRID_STRIDE]:
        c = po.bn_case(shape)
        po.check_bn(ops.batchnorm_nhwc(c["x"], c["sc"], c["sh"], relu=relu), c, relu, (shape, relu))
    assert int(np.prod(po.BN_GRID_STRIDE)) // 8 == 540800 > 2048 * 256


# ---- upsample2x -------------------------------------------------------------------------
def test_upsample_grid_stride_case_and_mirror():
    N, H, W, C = po.UPSAMPLE_GRID_STRIDE
    assert N * H * W * C // 8 == 2113536 > po.UPSAMPLE_STRIDE
    x = po.make_data(po.UPSAMPLE_GRID_STRIDE, "randn", 2)
    out = torch.empty(N, 2 * H, 2 * W, C, dtype=BF16)
    assert torch.equal(ops.upsample2x(x, out), po.upsample_oracle(x))
    small = po.make_data((2, 3, 5, 32), "randn", 3)
    want = small[..., 8:24].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(po.upsample_oracle(small, 16, 8), want)
    assert po.upsample_accepts(2 ** 31 - po.UPSAMPLE_STRIDE - 1)
    assert not po.upsample_accepts(2 ** 31 - po.UPSAMPLE_STRIDE)
    assert not po.upsample_accepts(2 ** 31 - 1)


# ---- yolo_decode ------------------------------------------------------------------------
_DECODE = list(itertools.product(po.DECODE_LEVELS, po.DECODE_NC))


def _cpu_decode(feats, nc):
    return ops.yolo_decode(list(feats), po.DECODE_STRIDES, nc)


@pytest.mark.parametrize("hw,nc", _DECODE)
def test_decode_onehot_cpu(hw, nc):
    feats, want = po.decode_onehot(hw, nc)
    b64, _, _ = po.decode_oracle(feats, po.DECODE_STRIDES, nc)
    assert (b64 - want).abs().max() < 1e-27  # the leak of the other bins
    b, _, _ = _cpu_decode(feats, nc)
    assert (b.double() - want).abs().max() <= po.DECODE_ONEHOT_BOUND


@pytest.mark.parametrize("hw,nc", _DECODE)
def test_decode_ties_cpu(hw, nc):
    feats, want = po.decode_ties(hw, nc)
    _, _, c64 = po.decode_oracle(feats, po.DECODE_STRIDES, nc)
    assert torch.equal(c64, want)
    _, _, c = _cpu_decode(feats, nc)
    assert torch.equal(c, want)


@pytest.mark.parametrize("hw,nc", _DECODE)
def test_decode_random_cpu(hw, nc):
    feats = po.decode_random(hw, nc)
    b64, s64, c64 = po.decode_oracle(feats, po.DECODE_STRIDES, nc)
    assert not torch.isnan(b64).any() and not torch.isnan(s64).any()
    b, s, c = _cpu_decode(feats, nc)
    assert (b.double() - b64).abs().max() <= po.DECODE_RANDOM_BOUND
    assert (s.double() - s64).abs().max() <= po.DECODE_SCORE_BOUND
    assert torch.equal(c, c64)


@pytest.mark.parametrize("hw", [po.DECODE_ROWSPLIT_LEVELS, po.DECODE_ROWSPLIT_SMALL])
def test_decode_rowsplit_cpu(hw):
    feats, want = po.decode_rowsplit(hw)
    if hw is po.DECODE_ROWSPLIT_LEVELS:
        assert feats[0].shape[1] * feats[0].shape[2] == 65535
    else:  # the split without its + 0.5f puts anchor al = w in row 0 at every one of these widths
        for h, w in hw:
            al = np.arange(h * w)
            assert np.array_equal(po.row_split_model(al, w), al // w)
            assert po.row_split_model(w, w, half=0.0) == 0
    b, _, _ = _cpu_decode(feats, 8)
    assert (b.double() - want).abs().max() <= po.DECODE_ONEHOT_BOUND
    b64, _, _ = po.decode_oracle(feats, po.DECODE_STRIDES, 8)
    assert (b64 - want).abs().max() < 1e-27


def test_decode_row_split_model_is_exact_below_65536():
    """int((al + 0.5f) * (1.0f / w)) == al // w for every al < 65536, every w <= 1024 and a
    dozen larger w (the claim the launcher's rc -3 rests on)."""
    al = np.arange(65536)
    for w in list(range(1, 1025)) + [1025, 1279, 1280, 2047, 2048, 4095, 8191, 8192, 16383, 32767,
                                     32768, 65535]:
        assert np.array_equal(po.row_split_model(al, w), al // w), w


def test_decode_refusal_mirror():
    assert po.decode_rc(po.DECODE_ROWSPLIT_LEVELS, 8) == 0
    assert po.decode_rc(po.DECODE_REFUSED_LEVELS, 8) == -3
    assert po.decode_rc(po.DECODE_LEVELS[0], 12) == -1
    assert po.decode_rc(po.DECODE_LEVELS[0], 512) == -2
    assert all(po.decode_rc(hw, nc) == 0 for hw, nc in _DECODE)
