"""The pool, head and pre/post-processing HIP kernels (csrc/kernels/pool_misc.hip,
yolo_decode) against the float64 oracles of pool_oracles.py, at the shapes, values and
refusals where they could go wrong: channel slices, dynamic LDS above 64 KiB, grid-stride
trips, ties, +-0 / +-inf / subnormals, and every launcher's accept / refuse rule.
test_pool_misc_cpu.py pins the same oracles against the CPU path.
"""
import itertools

import pytest
import torch

import pool_oracles as po
from kvedge_amd import ops

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert ops.load(), "native kvedge library must be loaded on the GPU box"


# ---- maxpool2d --------------------------------------------------------------------------
@pytest.mark.parametrize("ksp", po.MAXPOOL_KSP)
def test_maxpool_exact(ksp):
    """Exact on every map / channel count / data set, dense and as a channel slice of wider
    buffers (NaN prefill around the written slice keeps its bits)."""
    k, s, p = ksp
    for (H, W, C), kind, sliced in itertools.product(po.maxpool_shapes(ksp), po.DATA, (False, True)):
        c = po.maxpool_case(ksp, H, W, C, kind, sliced)
        ctx = (ksp, H, W, C, kind, sliced)
        if sliced:  # both buffers inside larger allocations: a wrong pitch stays in owned memory
            xg = po.view_in_slab(c["x"].shape, device="cuda", slack=c["x"].numel())
            og = po.view_in_slab(c["out0"].shape, device="cuda", slack=c["out0"].numel())
            xg.copy_(c["x"])
            og.copy_(c["out0"])
            got = ops.maxpool2d(xg, k, s, p, out=og, C=C, x_coff=c["x_coff"],
                                y_coff=c["y_coff"]).cpu()
            po.check_slice_written(got, c["out0"], c["ref"], C, c["y_coff"], ctx)
        else:
            got = ops.maxpool2d(c["x"].cuda(), k, s, p).cpu()
            assert not torch.isnan(got).any() and torch.equal(got, c["ref"]), ctx


def test_maxpool_returns_subnormals_unchanged():
    """Windows of subnormals and zeros only: the output is one of the inputs, bit for bit
    (up to the sign of a zero)."""
    pats = [[0x0001, 0x8001, 0x007f, 0x8000], [0x8001, 0x8040, 0x807f, 0xff80],
            [0x0040, 0x0001, 0x0000, 0x8000], [0x8001, 0xff80, 0xff80, 0xff80]]
    x = torch.stack([po._from_bits(q).view(2, 2, 1).repeat(1, 1, 8) for q in pats])
    got = ops.maxpool2d(x.cuda(), 2, 2, 0).cpu()
    ref = po.maxpool_oracle(x, 2, 2, 0)
    assert torch.equal(po.bits(got), po.bits(ref)), (po.bits(got)[..., 0].tolist(),
                                                     po.bits(ref)[..., 0].tolist())


def test_maxpool_grid_stride():
    shape, (k, s, p) = po.MAXPOOL_GRID_STRIDE
    x = po.make_data(shape, "randn", 5)
    got = ops.maxpool2d(x.cuda(), k, s, p).cpu()
    assert torch.equal(got, po.maxpool_oracle(x, k, s, p))


def _slice_tensors(op, case):
    C, ldx, x_coff, ldy, y_coff, dh, _ = po.SLICE_CASES[case]
    N, H, W = 2, 6, 4
    Ho, Wo = (3, 2) if op == "maxpool2d" else (12, 8)
    x = po.view_in_slab((N, H, W, ldx), device="cuda", fill=1.0)
    out = po.view_in_slab((N, Ho + dh, Wo, ldy), device="cuda", fill=2.0)
    return x, out, (N, H, W, Ho, Wo)


@pytest.mark.parametrize("op", ["maxpool2d", "upsample2x"])
@pytest.mark.parametrize("case", list(po.SLICE_CASES))
def test_slice_refusals(op, case):
    """ValueError from ops.* and an exception from the binding itself, before any launch;
    every tensor is a view into a larger allocation."""
    C, ldx, x_coff, ldy, y_coff, dh, accepted = po.SLICE_CASES[case]
    x, out, (N, H, W, Ho, Wo) = _slice_tensors(op, case)

    def via_ops():
        if op == "maxpool2d":
            ops.maxpool2d(x, 3, 2, 1, out=out, C=C, x_coff=x_coff, y_coff=y_coff)
        else:
            ops.upsample2x(x, out, C=C, x_coff=x_coff, y_coff=y_coff)

    def via_binding():
        if op == "maxpool2d":
            torch.ops.kvedge.maxpool2d(x, out, N, H, W, C, ldx, x_coff, ldy, y_coff, 3, 2, 1, Ho, Wo)
        else:
            torch.ops.kvedge.upsample2x(x, out, N, H, W, C, ldx, x_coff, ldy, y_coff)

    for call in (via_ops, via_binding):
        if accepted:
            out.fill_(2.0)
            call()
            got = out.cpu()
            assert (got[..., y_coff:y_coff + C] == 1).all() and (got[..., :y_coff] == 2).all()
            assert (got[..., y_coff + C:] == 2).all()
        else:
            with pytest.raises(ValueError if call is via_ops else RuntimeError):
                call()
            torch.cuda.synchronize()
            assert (out == 2).all()


@pytest.mark.parametrize("op", ["maxpool2d", "upsample2x"])
def test_binding_refuses_ld_that_is_not_the_row(op):
    """ldx / ldy handed to the binding must be the tensors' last dimension."""
    x, out, (N, H, W, Ho, Wo) = _slice_tensors(op, "ok_sliced")
    for ldx, ldy in ((24, 40), (32, 32), (40, 40), (32, 48)):
        with pytest.raises(RuntimeError):
            if op == "maxpool2d":
                torch.ops.kvedge.maxpool2d(x, out, N, H, W, 16, ldx, 8, ldy, 16, 3, 2, 1, Ho, Wo)
            else:
                torch.ops.kvedge.upsample2x(x, out, N, H, W, 16, ldx, 8, ldy, 16)
    torch.cuda.synchronize()
    assert (out == 2).all()


# ---- sppf_pool --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", po.DATA)
def test_sppf_exact(kind):
    """Every map up to the LDS cap (33x32 and above need more than 64 KiB of dynamic LDS):
    slices 1..3 fully overwritten with the exact chained pools, slice 0 keeps its bits."""
    for N, H, W, C in po.sppf_shapes():
        c = po.sppf_case(N, H, W, C, kind)
        got = ops.sppf_pool(c["buf"].cuda(), C).cpu()
        po.check_sppf(got, c, (N, H, W, C, kind))


def test_sppf_refuses_above_the_lds_cap():
    H, W = po.SPPF_REFUSED
    buf = po.view_in_slab((1, H, W, 64), device="cuda", fill=1.0)
    with pytest.raises(RuntimeError, match="sppf"):
        ops.sppf_pool(buf, 16)
    with pytest.raises(RuntimeError, match="sppf"):  # C not a multiple of 16
        ops.sppf_pool(po.view_in_slab((1, 5, 5, 96), device="cuda", fill=1.0), 24)
    torch.cuda.synchronize()
    assert (buf == 1).all()


# ---- global_avgpool ---------------------------------------------------------------------
@pytest.mark.parametrize("hw", po.AVG_EXACT_HW + po.AVG_BOUND_HW)
def test_avgpool(hw):
    exact = hw in po.AVG_EXACT_HW
    for C, N in itertools.product(po.AVG_C, po.AVG_N):
        c = po.avgpool_case(N, hw[0], hw[1], C)
        po.check_avgpool(ops.global_avgpool(c["x"].cuda()).cpu(), c, exact, (hw, C, N))


def test_avgpool_grid_stride():
    c = po.avgpool_case(*po.AVG_GRID_STRIDE)
    po.check_avgpool(ops.global_avgpool(c["x"].cuda()).cpu(), c, True, "grid-stride")


@pytest.mark.parametrize("C", po.AVG_REFUSED_C)
def test_avgpool_refuses_partial_waves(C):
    x = po.view_in_slab((2, 2, 2, C), device="cuda", fill=1.0)
    out = po.view_in_slab((2, C), device="cuda", fill=2.0)
    with pytest.raises(RuntimeError, match="avgpool"):
        ops.global_avgpool(x, out=out)
    torch.cuda.synchronize()
    assert (out == 2).all()


# ---- softmax_rows -----------------------------------------------------------------------
_softmax_worst = {}


@pytest.mark.parametrize("cols", list(po.SOFTMAX_COLS))
def test_softmax(cols):
    worst = 0.0
    for rows, scale, x, used in po.softmax_cases(cols):
        p, am = ops.softmax_rows(x.cuda())
        worst = max(worst, po.check_softmax(p.cpu(), am.cpu(), x, used, (cols, rows, scale)))
    print(f"softmax cols={cols} path={po.SOFTMAX_COLS[cols]} worst err/bound={worst:.4f}")


def test_softmax_misaligned_rows_take_the_strided_path():
    xv, x, used = po.softmax_misaligned("cuda")
    assert xv.is_contiguous() and xv.data_ptr() % 16 == 6
    p, am = ops.softmax_rows(xv)
    worst = po.check_softmax(p.cpu(), am.cpu(), x, used, "misaligned")
    print(f"softmax misaligned worst err/bound={worst:.4f}")


# ---- preprocess -------------------------------------------------------------------------
@pytest.mark.parametrize("s2d", [False, True])
@pytest.mark.parametrize("norm", [po.IMAGENET, po.UNIT])
def test_preprocess_all_bytes(norm, s2d):
    mean, std = norm
    x = po.all_bytes_frame()
    got = ops.preprocess(x.cuda(), mean=mean, std=std, s2d=s2d).cpu()
    ratio = po.check_preprocess(got, x, mean, std, s2d, (norm, s2d))
    print(f"preprocess s2d={s2d} mean={mean[0]} worst err/bound={ratio:.4f}")


@pytest.mark.parametrize("shape", po.PRE_LAYOUT_SHAPES)
def test_preprocess_layout(shape):
    x = po.layout_frame(shape)
    mean, std = po.BYTE_NORM
    y4 = ops.preprocess(x.cuda(), mean=mean, std=std).cpu()
    assert torch.equal(y4[..., :3].float(), x.float()) and (po.bits(y4)[..., 3] == 0).all()
    y = ops.preprocess(x.cuda(), mean=mean, std=std, s2d=True).cpu()
    N, H, W, _ = shape
    for n, by, bx, dy, dx, c in itertools.product(range(N), range(H // 2), range(W // 2),
                                                  range(2), range(2), range(3)):
        assert float(y[n, by, bx, (dy * 2 + dx) * 4 + c]) == float(x[n, 2 * by + dy, 2 * bx + dx, c])
    assert (po.bits(y)[..., 3::4] == 0).all()


@pytest.mark.parametrize("case", [c for c in po.PRE_ACCEPT_CASES if not c[4]])
def test_preprocess_refusals(case):
    N, H, W, s2d, _ = case
    x = po.view_in_slab((N, H, W, 3), dtype=torch.uint8, device="cuda", fill=7)
    shape = (N, H // 2, W // 2, 16) if s2d else (N, H, W, 4)
    out = po.view_in_slab(shape, device="cuda", fill=2.0)
    with pytest.raises(RuntimeError):
        ops.preprocess(x, out=out, s2d=s2d)
    torch.cuda.synchronize()
    assert (out == 2).all()


@pytest.mark.parametrize("s2d", [False, True])
def test_preprocess_grid_stride(s2d):
    shape = po.PRE_GRID_STRIDE[s2d]
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    mean, std = po.IMAGENET
    po.check_preprocess(ops.preprocess(x.cuda(), s2d=s2d).cpu(), x, mean, std, s2d, shape)


# ---- batchnorm_nhwc ---------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm(relu):
    for shape in [(3, 5, 7, C) for C in po.BN_C] + [po.BN_GRID_STRIDE]:
        c = po.bn_case(shape)
        got = ops.batchnorm_nhwc(c["x"].cuda(), c["sc"].cuda(), c["sh"].cuda(), relu=relu).cpu()
        po.check_bn(got, c, relu, (shape, relu))


# ---- upsample2x -------------------------------------------------------------------------
def test_upsample_grid_stride():
    N, H, W, C = po.UPSAMPLE_GRID_STRIDE
    x = po.make_data(po.UPSAMPLE_GRID_STRIDE, "randn", 2)
    out = torch.full((N, 2 * H, 2 * W, C), float("nan"), dtype=BF16, device="cuda")
    got = ops.upsample2x(x.cuda(), out).cpu()
    assert torch.equal(got, po.upsample_oracle(x))


# ---- yolo_decode ------------------------------------------------------------------------
_DECODE = list(itertools.product(po.DECODE_LEVELS, po.DECODE_NC))


def _gpu_decode(feats, nc):
    b, s, c = ops.yolo_decode([f.cuda() for f in feats], po.DECODE_STRIDES, nc)
    return b.cpu(), s.cpu(), c.cpu()


@pytest.mark.parametrize("hw,nc", _DECODE)
def test_decode_onehot_dfl(hw, nc):
    """(a) every box side lands on its planted bin: sign and side order of dist2bbox, the
    anchor split, strides."""
    feats, want = po.decode_onehot(hw, nc)
    b, s, c = _gpu_decode(feats, nc)
    err = (b.double() - want).abs().max().item()
    print(f"decode onehot hw={hw} nc={nc} worst box err={err:.3e}")
    assert err <= po.DECODE_ONEHOT_BOUND, err
    _, s64, c64 = po.decode_oracle(feats, po.DECODE_STRIDES, nc)
    assert torch.equal(c, c64) and (s.double() - s64).abs().max() <= po.DECODE_SCORE_BOUND


@pytest.mark.parametrize("hw,nc", _DECODE)
def test_decode_class_ties(hw, nc):
    """(b) the lower class index wins every planted tie."""
    feats, want = po.decode_ties(hw, nc)
    _, _, c = _gpu_decode(feats, nc)
    bad = (c != want).nonzero()
    assert bad.numel() == 0, (bad[:4].tolist(), c[c != want][:4].tolist(), want[c != want][:4].tolist())


@pytest.mark.parametrize("hw,nc", _DECODE)
def test_decode_random(hw, nc):
    """(c) random features against float64."""
    feats = po.decode_random(hw, nc)
    b64, s64, c64 = po.decode_oracle(feats, po.DECODE_STRIDES, nc)
    b, s, c = _gpu_decode(feats, nc)
    err = (b.double() - b64).abs().max().item()
    print(f"decode random hw={hw} nc={nc} worst box err={err:.3e}")
    assert err <= po.DECODE_RANDOM_BOUND, err
    assert (s.double() - s64).abs().max() <= po.DECODE_SCORE_BOUND
    assert torch.equal(c, c64)


@pytest.mark.parametrize("hw", [po.DECODE_ROWSPLIT_LEVELS, po.DECODE_ROWSPLIT_SMALL])
def test_decode_row_split(hw):
    """(d) 65,535 anchors in one level, and widths whose fp32 reciprocal is rounded down (the
    split's + 0.5f matters from the second row on): every box is its anchor centre times the
    stride."""
    feats, want = po.decode_rowsplit(hw)
    b, _, c = _gpu_decode(feats, 8)
    err = (b.double() - want).abs()
    assert err.max() <= po.DECODE_ONEHOT_BOUND, (err.max().item(), (err > 1e-3).nonzero()[:4].tolist())
    assert (c == 0).all()


def test_decode_refuses_65536_anchors():
    hw = po.DECODE_REFUSED_LEVELS
    assert po.decode_rc(hw, 8) == -3
    feats = [torch.zeros(1, h, w, 72, dtype=BF16, device="cuda") for h, w in hw]
    with pytest.raises(RuntimeError, match="rc=-3"):
        ops.yolo_decode(feats, po.DECODE_STRIDES, 8)
