"""float64 oracles, input builders and launcher accept/refuse mirrors for the pool, head and
pre/post-processing kernels (test_pool_misc_cpu.py, test_pool_misc_gpu.py).

Every oracle here is computed from the bf16 / uint8 inputs in ``torch.float64`` with plain
tensor arithmetic and none of the project's code, so the CPU file can pin it against
``kvedge_amd.ops.reference`` and the GPU file can hold the HIP kernels to it.  Builders are
cached: what they return is shared between tests and must not be modified.

Bounds (``ulp16(v)`` is the bf16 spacing at ``|v|``; derivations in docs/kernels.md, "Other
kernels"):

* maxpool2d, sppf_pool, upsample2x: exact (``torch.equal``: +0 and -0 compare equal), no NaN.
* global_avgpool: integer inputs in [-8, 8] make the fp32 sum exact; HW a power of two then
  makes the result the correctly rounded bf16, else ``ulp16/2 + 4 * 2^-24 * |ref|``.
* softmax_rows: ``(|x - rowmax| + SOFTMAX_K) * 2^-23 * p + 1e-37``, argmax = first maximum.
* preprocess: ``ulp16/2 + 1e-6``;  batchnorm_nhwc: ``ulp16/2 + 2^-22 * (|x*sc| + |sh|)``.
* yolo_decode: see DECODE_* below.

NaN inputs are outside every kernel's contract and appear nowhere here (only as the prefill
of output channels that must, or must not, be overwritten).
"""
import functools
import itertools

import numpy as np
import torch

BF16 = torch.bfloat16
INF = float("inf")


def ulp16(v: torch.Tensor) -> torch.Tensor:
    """bf16 spacing at |v| (float64): 2^(e - 7) for 2^e <= |v| < 2^(e+1), subnormal spacing
    2^-133 below 2^-126 and at 0."""
    v = v.double().abs()
    _, ex = torch.frexp(v)  # v = m * 2^ex with m in [0.5, 1)
    ex = torch.where(v > 0, ex, torch.full_like(ex, -125)).clamp_min(-125)
    return torch.ldexp(torch.ones_like(v), ex - 8)


def round_bf16(v: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even), kept in float64.  One rounding: a
    cast through fp32 would round twice."""
    u = ulp16(v)
    return torch.round(v.double() / u) * u  # the scaling by a power of two is exact


def bits(t: torch.Tensor) -> torch.Tensor:
    """The bf16 tensor's bit patterns (int16), for comparisons that tell -0 from +0 and
    one NaN from another."""
    assert t.dtype == BF16
    return t.contiguous().view(torch.int16)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _from_bits(patterns):
    return torch.tensor([b - 65536 if b >= 32768 else b for b in patterns],
                        dtype=torch.int16).view(BF16)


# +inf once in 16, then -inf, +0, -0 and bf16 subnormals of both signs (smallest, largest, middle)
_SPECIALS = _from_bits([0x7f80, 0xff80, 0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x807f, 0x0040,
                        0x8040, 0xff80, 0x0000, 0x8000, 0x0001, 0x8001, 0x007f])
DATA = ("randn", "negative", "neg_inf", "special")


def make_data(shape, kind, seed=0):
    """bf16 test images.  ``negative`` catches a 0 initial value; ``neg_inf`` is an image of
    -inf; ``special`` is a negative image with half its elements replaced by +-inf, +-0 and
    subnormals, so that windows whose maximum is a zero or a subnormal are common."""
    g = _gen(seed)
    x = torch.randn(shape, generator=g)
    if kind in ("negative", "special"):
        x = -x.abs() - 0.25
    x = x.to(BF16)
    if kind == "neg_inf":
        x = torch.full(shape, -INF, dtype=BF16)
    elif kind == "special":
        take = torch.rand(shape, generator=g) < 0.5
        which = torch.randint(0, _SPECIALS.numel(), shape, generator=g)
        x = torch.where(take, _SPECIALS[which], x)
    else:
        assert kind in DATA
    return x


# ---------------------------------------------------------------------------
# maxpool2d
# ---------------------------------------------------------------------------
MAXPOOL_KSP = ((3, 2, 1), (2, 2, 0), (3, 1, 1), (5, 1, 2), (3, 2, 0))
MAXPOOL_MAPS = ((7, 5), (8, 30), (1, 9), (2, 2))
MAXPOOL_C = (8, 24, 64)
MAXPOOL_GRID_STRIDE = ((1, 97, 96, 512), (2, 1, 0))  # 96*95*64 = 583,680 vectors > 2048*256


def pool_out(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def maxpool_shapes(ksp):
    """(H, W, C) of every call for one (k, s, p): the maps that leave Ho, Wo >= 1."""
    k, s, p = ksp
    return [(H, W, C) for (H, W), C in itertools.product(MAXPOOL_MAPS, MAXPOOL_C)
            if min(pool_out(H, W, k, s, p)) >= 1]


def maxpool_oracle(x, k, s, p, C=None, x_coff=0):
    """max over the k x k window of the -inf padded image, in float64; bf16 out (exact)."""
    C = C or x.shape[3] - x_coff
    xs = x[..., x_coff:x_coff + C].double()
    N, H, W, _ = xs.shape
    Ho, Wo = pool_out(H, W, k, s, p)
    xp = torch.full((N, H + 2 * p, W + 2 * p, C), -INF, dtype=torch.float64)
    xp[:, p:p + H, p:p + W] = xs
    y = torch.full((N, Ho, Wo, C), -INF, dtype=torch.float64)
    for r in range(k):
        for c in range(k):
            y = torch.maximum(y, xp[:, r:r + (Ho - 1) * s + 1:s, c:c + (Wo - 1) * s + 1:s])
    return y.to(BF16)


SLICE_LDX, SLICE_XCOFF, SLICE_LDY, SLICE_YCOFF = 16, 8, 24, 16  # ld = C + 16 / C + 24


@functools.lru_cache(maxsize=None)
def maxpool_case(ksp, H, W, C, kind, sliced, N=2):
    """x, the output buffer before the call (NaN where sliced), the oracle of the slice, and
    the call's (C, x_coff, y_coff).  The sliced form reads channels [8, 8 + C) of C + 16 and
    writes channels [16, 16 + C) of C + 24."""
    k, s, p = ksp
    Ho, Wo = pool_out(H, W, k, s, p)
    seed = 1000 * k + 100 * s + 10 * p + H + W + C
    if sliced:
        x = make_data((N, H, W, C + SLICE_LDX), kind, seed)
        out0 = torch.full((N, Ho, Wo, C + SLICE_LDY), float("nan"), dtype=BF16)
        xc, yc = SLICE_XCOFF, SLICE_YCOFF
    else:
        x = make_data((N, H, W, C), kind, seed)
        out0 = None
        xc = yc = 0
    return dict(x=x, out0=out0, ref=maxpool_oracle(x, k, s, p, C, xc), C=C, x_coff=xc, y_coff=yc)


def check_slice_written(got, out0, ref, C, y_coff, ctx):
    """Exact slice, no NaN in it, and the channels around it keep the prefill's bits."""
    sl = got[..., y_coff:y_coff + C]
    assert not torch.isnan(sl).any(), ctx
    assert torch.equal(sl, ref), ctx
    assert torch.equal(bits(got[..., :y_coff]), bits(out0[..., :y_coff])), ctx
    assert torch.equal(bits(got[..., y_coff + C:]), bits(out0[..., y_coff + C:])), ctx


def slices_accept(C, ldx, x_coff, ldy, y_coff, out_nhw, want_nhw):
    """Mirror of ops._check_slices / the bindings' check_slices (maxpool2d, upsample2x)."""
    if tuple(out_nhw) != tuple(want_nhw):
        return False
    if C <= 0 or x_coff < 0 or y_coff < 0 or any(v % 8 for v in (C, ldx, x_coff, ldy, y_coff)):
        return False
    return x_coff + C <= ldx and y_coff + C <= ldy


# name -> (C, ldx, x_coff, ldy, y_coff, rows added to the output's height, accepted)
SLICE_CASES = {
    "ok_sliced": (16, 32, 8, 40, 16, 0, True),
    "ok_flush": (16, 24, 8, 32, 16, 0, True),          # both slices end at the row's end
    "x_slice_past_row": (16, 24, 16, 40, 16, 0, False),
    "y_slice_past_row": (16, 32, 8, 24, 16, 0, False),
    "c_not_8": (12, 32, 8, 40, 16, 0, False),
    "ldx_not_8": (16, 36, 8, 40, 16, 0, False),
    "x_coff_not_8": (16, 32, 4, 40, 16, 0, False),
    "ldy_not_8": (16, 32, 8, 44, 16, 0, False),
    "y_coff_not_8": (16, 32, 8, 40, 12, 0, False),
    "out_height": (16, 32, 8, 40, 16, 1, False),
}


def view_in_slab(shape, dtype=BF16, device="cpu", fill=0.0, slack=4096):
    """A contiguous tensor of ``shape`` that is a view into the middle of a larger
    allocation: a launcher that wrongly accepts a refusal case stays inside owned memory."""
    n = int(np.prod(shape))
    slab = torch.full((n + 2 * slack,), fill, dtype=dtype, device=device)
    return slab[slack:slack + n].view(shape)


# ---------------------------------------------------------------------------
# sppf_pool
# ---------------------------------------------------------------------------
SPPF_SMALL_MAPS = ((1, 1), (1, 7), (2, 3), (5, 5), (12, 20), (20, 12))
SPPF_LARGE_MAPS = ((33, 32), (40, 40), (40, 64))  # 66 KiB, 100 KiB, 160 KiB (the cap) of LDS
SPPF_REFUSED = (41, 63)                           # 2583 px: 165,312 B
SPPF_LDS_CAP = 160 * 1024


def sppf_lds(H, W):
    return 2 * H * W * 16 * 2  # two images of a 16-channel bf16 slice


def sppf_accepts(H, W, C):
    return C % 16 == 0 and sppf_lds(H, W) <= SPPF_LDS_CAP


def sppf_shapes():
    """(N, H, W, C) of every accepted call."""
    small = [(N, H, W, C) for (H, W), C, N in itertools.product(SPPF_SMALL_MAPS, (16, 48), (1, 3))]
    return small + [(1, H, W, 16) for H, W in SPPF_LARGE_MAPS]


@functools.lru_cache(maxsize=None)
def sppf_case(N, H, W, C, kind):
    """buf [N,H,W,4C]: x in slice 0, NaN in slices 1..3; ref: the three chained 5x5 pools."""
    buf = torch.full((N, H, W, 4 * C), float("nan"), dtype=BF16)
    buf[..., :C] = make_data((N, H, W, C), kind, 7 * H + W + C + N)
    y, refs = buf[..., :C], []
    for _ in range(3):
        y = maxpool_oracle(y.contiguous(), 5, 1, 2)
        refs.append(y)
    return dict(buf=buf, ref=torch.cat(refs, dim=3))


def check_sppf(got, case, ctx):
    C = case["buf"].shape[3] // 4
    assert torch.equal(bits(got[..., :C]), bits(case["buf"][..., :C])), ctx  # slice 0 untouched
    assert not torch.isnan(got[..., C:]).any(), ctx                          # fully overwritten
    assert torch.equal(got[..., C:], case["ref"]), ctx


# ---------------------------------------------------------------------------
# global_avgpool
# ---------------------------------------------------------------------------
AVG_EXACT_HW = ((1, 1), (2, 2), (4, 4), (8, 8))   # 1/HW exact: the output is bf16(sum/HW)
AVG_BOUND_HW = ((7, 7), (3, 2), (14, 14))
AVG_C = (64, 192, 2048)
AVG_N = (1, 3, 5)
AVG_REFUSED_C = (32, 72)
AVG_GRID_STRIDE = (257, 1, 2, 2048)  # 257 * 256 * 8 = 526,336 lanes > 2048 * 256


def avgpool_accepts(C):
    return C % 64 == 0


@functools.lru_cache(maxsize=None)
def avgpool_case(N, H, W, C):
    """Integer-valued bf16 in [-8, 8]: every partial sum is an integer below 2^24."""
    x = torch.randint(-8, 9, (N, H, W, C), generator=_gen(N + 10 * H + W + C)).to(BF16)
    return dict(x=x, ref=x.double().sum(dim=(1, 2)) / (H * W))


def avgpool_bound(ref):
    """One bf16 rounding plus the two fp32 roundings of s * (1.0f / HW)."""
    return ulp16(ref) / 2 + 4 * 2.0 ** -24 * ref.abs()


def check_avgpool(got, case, exact, ctx):
    ref = case["ref"]
    assert got.dtype == BF16 and not torch.isnan(got).any(), ctx
    if exact:
        assert torch.equal(ref.float().double(), ref), ctx  # sum / 2^k needs no rounding to fp32
        assert torch.equal(bits(got), bits(ref.to(BF16))), ctx
    else:
        err = (got.double() - ref).abs()
        assert (err <= avgpool_bound(ref)).all(), (ctx, (err / avgpool_bound(ref)).max().item())


# ---------------------------------------------------------------------------
# softmax_rows
# ---------------------------------------------------------------------------
SOFTMAX_K = 32  # see docs/kernels.md for the derivation and the measured err / bound
SOFTMAX_COLS = {8: "register", 16: "register", 1000: "register", 1016: "register",
                1024: "register", 1: "strided", 7: "strided", 1001: "strided", 1032: "strided",
                2000: "strided", 4096: "strided"}
SOFTMAX_ROWS = (1, 5, 9)
SOFTMAX_SCALES = (3.0, 30.0)


def softmax_path(cols, aligned=True):
    """Mirror of softmax_kernel's choice between the register-resident row and the strided loop."""
    return "register" if cols <= 1024 and cols % 8 == 0 and aligned else "strided"


def softmax_plants(cols):
    """name -> columns of the rows planted at this width (every one that fits)."""
    P = {}
    if cols >= 4:
        c = (cols // 2) // 16 * 16 + 2
        P["tie_in_chunk"] = (c, c + 1)            # inside one lane's 8-column chunk
    if cols >= 16:
        l = cols // 32
        P["tie_halves"] = (16 * l + 7, 16 * l + 8)  # across a lane's two 8-halves
    if cols >= 6:
        P["tie_lanes"] = (3, cols - 2)
    if cols >= 128:
        P["tie_stride64"] = (cols // 3, cols // 3 + 64)  # one lane, two trips of the strided loop
    P["max_first"] = (0,)
    P["max_last"] = (cols - 1,)
    P["all_equal"] = ()
    if cols >= 2:
        P["neg_inf"] = ()
    return P


@functools.lru_cache(maxsize=None)
def softmax_cases(cols):
    """[(rows, scale, logits bf16 [rows, cols], plant of each row)] for every rows x scale; the
    plants cycle over the rows of all the matrices, so each appears in every list."""
    plants = softmax_plants(cols)
    names = list(plants)
    out, k = [], 0
    for rows, scale in itertools.product(SOFTMAX_ROWS, SOFTMAX_SCALES):
        x = (torch.randn(rows, cols, generator=_gen(cols + rows + int(scale))) * scale).to(BF16)
        used = []
        for r in range(rows):
            name = names[k % len(names)]
            k += 1
            top = float(x[r].float().max()) + 2.0
            if name == "all_equal":
                x[r] = 1.5
            elif name == "neg_inf":
                x[r, 1::3] = -INF
            else:
                for c in plants[name]:
                    x[r, c] = top
            used.append(name)
        out.append((rows, scale, x, tuple(used)))
    assert k >= len(names)
    return out


def softmax_oracle(x):
    """(p, a, first): float64 softmax, a = x - rowmax, and the first index of the row maximum."""
    xd = x.double()
    mx = xd.max(dim=1, keepdim=True).values
    a = xd - mx
    e = a.exp()
    col = torch.arange(x.shape[1]).expand_as(xd)
    first = torch.where(xd == mx, col, torch.full_like(col, x.shape[1])).min(dim=1).values
    return e / e.sum(dim=1, keepdim=True), a, first


def softmax_bound(a, p):
    b = (a.abs() + SOFTMAX_K) * 2.0 ** -23 * p + 1e-37
    return torch.where(torch.isinf(a), torch.zeros_like(b), b)  # a -inf logit: exactly 0


def check_softmax(got_p, got_arg, x, used, ctx):
    """Returns the worst err / bound (measured, for docs/kernels.md)."""
    p, a, first = softmax_oracle(x)
    assert not torch.isnan(p).any() and got_p.dtype == torch.float32, ctx
    assert not torch.isnan(got_p).any(), ctx
    assert torch.equal(got_arg.long(), first), (ctx, got_arg.tolist(), first.tolist())
    err = (got_p.double() - p).abs()
    bound = softmax_bound(a, p)
    worst = (err / bound.clamp_min(1e-300)).max().item() if (bound > 0).any() else 0.0
    bad = err > bound
    assert not bad.any(), (ctx, used, worst, bad.nonzero()[:4].tolist())
    assert (got_p[torch.isinf(x.float())] == 0).all(), ctx
    for r, name in enumerate(used):
        if name == "all_equal":
            assert int(got_arg[r]) == 0, ctx
    return worst


def softmax_misaligned(flat_device="cpu"):
    """The rows = 5, scale 3 case of cols = 1000 as a contiguous view 3 elements (6 B) into a
    flat buffer: not 16-B aligned, so the register path's guard must refuse it."""
    rows, scale, x, used = softmax_cases(1000)[2]
    assert (rows, scale) == (5, 3.0)
    flat = torch.zeros(16 + rows * 1000, dtype=BF16)
    flat[3:3 + rows * 1000] = x.reshape(-1)
    flat = flat.to(flat_device)
    return flat[3:3 + rows * 1000].view(rows, 1000), x, used


# ---------------------------------------------------------------------------
# preprocess
# ---------------------------------------------------------------------------
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
BYTE_NORM = ((0.0, 0.0, 0.0), (1.0 / 255,) * 3)  # output == the byte value, exactly
PRE_LAYOUT_SHAPES = ((3, 6, 10, 3), (1, 2, 2, 3))
PRE_GRID_STRIDE = {False: (1, 1024, 1026, 3),  # 525,312 pixel pairs > 2048 * 256
                   True: (1, 1026, 2048, 3)}   # 525,312 2x2 blocks
# (N, H, W, s2d, accepted)
PRE_ACCEPT_CASES = ((1, 3, 3, False, False), (3, 5, 7, False, False), (2, 3, 3, False, True),
                    (1, 3, 4, False, True), (1, 3, 4, True, False), (1, 4, 3, True, False),
                    (1, 5, 7, True, False), (1, 4, 6, True, True))


def preprocess_accepts(N, H, W, s2d):
    return (H % 2 == 0 and W % 2 == 0) if s2d else (N * H * W) % 2 == 0


def s2d_layout(y4):
    """[N,H,W,4] -> [N,H/2,W/2,16] with y[n,by,bx,(dy*2+dx)*4+c] = y4[n,2by+dy,2bx+dx,c]."""
    N, H, W, _ = y4.shape
    y = torch.zeros(N, H // 2, W // 2, 16, dtype=y4.dtype)
    for dy in range(2):
        for dx in range(2):
            for c in range(4):
                y[..., (dy * 2 + dx) * 4 + c] = y4[:, dy::2, dx::2, c]
    return y


def preprocess_oracle(x, mean, std, s2d):
    """float64 (p/255 - mean) / std, pad channel 0."""
    y = (x.double() / 255.0 - torch.tensor(mean, dtype=torch.float64)) / torch.tensor(
        std, dtype=torch.float64)
    y4 = torch.zeros(*x.shape[:3], 4, dtype=torch.float64)
    y4[..., :3] = y
    return s2d_layout(y4) if s2d else y4


def preprocess_bound(ref):
    """One bf16 rounding plus the three fp32 roundings scaled by 1/std <= 4.47."""
    return ulp16(ref) / 2 + 1e-6


def preprocess_kernel_model(x, mean, std):
    """The kernel's fp32 formula without FMA contraction, rounded to bf16: [.., 3] bf16."""
    m = np.asarray(mean, dtype=np.float64).astype(np.float32)
    inv = (1.0 / np.asarray(std, dtype=np.float64)).astype(np.float32)
    v = (x.numpy().astype(np.float32) * np.float32(1.0 / 255.0) - m) * inv
    assert v.dtype == np.float32
    return torch.from_numpy(v).to(BF16)


@functools.lru_cache(maxsize=None)
def all_bytes_frame():
    """[1,16,16,3]: all 256 values in every channel (another rotation per channel)."""
    v = torch.arange(256).view(16, 16)
    return torch.stack([(v + 85 * c) % 256 for c in range(3)], dim=-1).to(torch.uint8)[None]


def layout_frame(shape):
    """Bytes that encode the flat (n, y, x, c) position mod 251: neighbours in every
    direction differ, so a misplaced element shows."""
    n = int(np.prod(shape))
    return (torch.arange(n) % 251).to(torch.uint8).view(shape)


def check_preprocess(got, x, mean, std, s2d, ctx):
    """Returns the worst err / bound."""
    ref = preprocess_oracle(x, mean, std, s2d)
    assert got.shape == ref.shape and got.dtype == BF16, ctx
    assert not torch.isnan(got).any(), ctx
    err = (got.double() - ref).abs()
    ratio = (err / preprocess_bound(ref)).max().item()
    assert ratio <= 1.0, (ctx, ratio)
    assert (bits(got)[..., 3::4] == 0).all(), ctx  # pad channel: +0 bits
    return ratio


# ---------------------------------------------------------------------------
# batchnorm_nhwc
# ---------------------------------------------------------------------------
BN_C = (8, 24, 64)
BN_GRID_STRIDE = (1, 65, 65, 1024)  # 540,800 vectors > 2048 * 256


@functools.lru_cache(maxsize=None)
def bn_case(shape):
    g = _gen(sum(shape))
    C = shape[-1]
    x = torch.randn(shape, generator=g).to(BF16)
    sc = torch.rand(C, generator=g) + 0.5
    sc[::3] *= -1  # negative scales too
    sh = torch.randn(C, generator=g)
    return dict(x=x, sc=sc, sh=sh)


def check_bn(got, case, relu, ctx):
    x, sc, sh = case["x"].double(), case["sc"].double(), case["sh"].double()
    ref = x * sc + sh
    assert (ref < 0).any() and (ref > 0).any(), ctx  # ReLU has something to clamp
    if relu:
        ref = ref.clamp_min(0)
        assert (got.float() >= 0).all(), ctx
    bound = ulp16(ref) / 2 + 2.0 ** -22 * ((x * sc).abs() + sh.abs())
    assert not torch.isnan(got).any(), ctx
    err = (got.double() - ref).abs()
    assert (err <= bound).all(), (ctx, (err / bound).max().item())


# ---------------------------------------------------------------------------
# upsample2x
# ---------------------------------------------------------------------------
UPSAMPLE_GRID_STRIDE = (1, 129, 128, 1024)  # 2,113,536 vectors > 8192 * 256
UPSAMPLE_STRIDE = 8192 * 256


def upsample_accepts(work):
    """The int index may take one more grid stride past the last item: that must fit too."""
    return work + UPSAMPLE_STRIDE < 2 ** 31


def upsample_oracle(x, C=None, x_coff=0):
    C = C or x.shape[3] - x_coff
    N, H, W, _ = x.shape
    iy = torch.arange(2 * H) // 2
    ix = torch.arange(2 * W) // 2
    return x[:, iy][:, :, ix][..., x_coff:x_coff + C]


# ---------------------------------------------------------------------------
# yolo_decode
# ---------------------------------------------------------------------------
DECODE_NC = (8, 16, 24, 80)  # 24: nc/4 = 6, the scalar class loop at 4-byte quarter offsets
DECODE_LEVELS = (((9, 13), (5, 7), (3, 4)), ((16, 16), (8, 8), (4, 4)))
DECODE_STRIDES = (8, 16, 32)
DECODE_ONEHOT_BOUND = 1e-3  # px: fp32 rounding of a distance <= 15, times stride 32, plus the
#                             rounding of a 640 px coordinate, is about 2e-4
# px, random features (c): the worst |box - float64| measured on an MI355X over the eight
# (levels, nc) cases of decode_random is 6.3e-5 (4.5e-5 .. 6.3e-5 per case); the bound is 4x
# that, and would never be set above 2e-3
DECODE_RANDOM_BOUND = 2.5e-4
DECODE_SCORE_BOUND = 1e-5
DECODE_ROWSPLIT_LEVELS = ((257, 255), (1, 1), (1, 1))  # 65,535 anchors: the largest admitted
DECODE_REFUSED_LEVELS = ((256, 256), (1, 1), (1, 1))   # 65,536: rc -3
# widths whose fp32 reciprocal is rounded down: al * (1.0f / w) falls below 1 at al = w, so
# the split needs its + 0.5f already in the second row (at w = 255 it happens not to)
DECODE_ROWSPLIT_SMALL = ((3, 41), (2, 47), (2, 61))


def decode_rc(hw, nc, N=1):
    """Mirror of kv_yolo_decode's refusals, in its order (0 = launched or nothing to do)."""
    if nc % 8:
        return -1
    if 64 * (64 + nc + 8) * 2 > 64 * 1024:
        return -2
    if N * sum((h * w + 63) // 64 for h, w in hw) <= 0:
        return 0
    if any(h * w >= 65536 for h, w in hw):
        return -3
    return 0


def row_split_model(al, w, half=0.5):
    """numpy model of the kernel's int((al + 0.5f) * (1.0f / w))."""
    al = np.asarray(al, dtype=np.float32)
    return ((al + np.float32(half)) * (np.float32(1.0) / np.float32(w))).astype(np.int32)


def _anchors(h, w):
    a = torch.arange(h * w)
    return (a % w).double() + 0.5, (a // w).double() + 0.5


def decode_oracle(feats, strides, nc):
    """float64 DFL expectation, dist2bbox, first-index class maximum and its sigmoid."""
    B, S, Cl = [], [], []
    for f, s in zip(feats, strides):
        N, h, w, ch = f.shape
        assert ch == 64 + nc
        ff = f.double().reshape(N, h * w, ch)
        lg = ff[..., :64].reshape(N, h * w, 4, 16)
        e = (lg - lg.max(dim=-1, keepdim=True).values).exp()
        dist = (e * torch.arange(16, dtype=torch.float64)).sum(-1) / e.sum(-1)
        ax, ay = _anchors(h, w)
        B.append(torch.stack([ax - dist[..., 0], ay - dist[..., 1], ax + dist[..., 2],
                              ay + dist[..., 3]], dim=-1) * s)
        cl = ff[..., 64:]
        mx = cl.max(dim=-1, keepdim=True).values
        idx = torch.arange(nc).expand_as(cl)
        Cl.append(torch.where(cl == mx, idx, torch.full_like(idx, nc)).min(dim=-1).values.int())
        S.append(1.0 / (1.0 + (-mx[..., 0]).exp()))
    return torch.cat(B, 1), torch.cat(S, 1), torch.cat(Cl, 1)


@functools.lru_cache(maxsize=None)
def decode_onehot(hw, nc, N=2):
    """(a) DFL logit +40 at bin j, -40 elsewhere (the other bins' leak is below 1e-30), j
    another one per side, anchor, image and level.  Returns feats and the expected boxes."""
    feats, boxes = [], []
    for li, ((h, w), s) in enumerate(zip(hw, DECODE_STRIDES)):
        A = h * w
        f = (torch.randn(N, A, 64 + nc, generator=_gen(li + nc)) * 2).to(BF16)
        a = torch.arange(A).view(1, A, 1)
        side = torch.arange(4).view(1, 1, 4)
        n = torch.arange(N).view(N, 1, 1)
        j = (a * 7 + side * 5 + n * 3 + li) % 16  # [N, A, 4]
        dfl = torch.full((N, A, 4, 16), -40.0)
        dfl.scatter_(3, j.unsqueeze(-1), 40.0)
        f[..., :64] = dfl.view(N, A, 64).to(BF16)
        feats.append(f.view(N, h, w, 64 + nc))
        ax, ay = _anchors(h, w)
        jd = j.double()
        boxes.append(torch.stack([ax - jd[..., 0], ay - jd[..., 1], ax + jd[..., 2],
                                  ay + jd[..., 3]], dim=-1) * s)
    return tuple(feats), torch.cat(boxes, 1)


DECODE_TIES = ("other_quarter", "same_quarter", "same_vector", "all_equal", "last")


@functools.lru_cache(maxsize=None)
def decode_ties(hw, nc, N=2):
    """(b) Class ties planted in every anchor, the kind cycling with the anchor index: two
    equal top logits in different lane quarters, in one quarter, in one 4-vector of a quarter,
    all classes equal, and the maximum at nc - 1.  Returns feats and the expected cls (the
    lower index of a tie)."""
    cq = nc // 4
    feats, exp = [], []
    for li, (h, w) in enumerate(hw):
        A = h * w
        f = (torch.randn(N, A, 64 + nc, generator=_gen(50 + li + nc)) * 2).clamp(max=4.0).to(BF16)
        e = torch.zeros(N, A, dtype=torch.int32)
        for n in range(N):
            for a in range(A):
                kind = DECODE_TIES[(a + n) % 5]
                r = a // 5 + n + li
                q = r % 4
                if kind == "all_equal":
                    f[n, a, 64:] = 1.0
                    continue
                if kind == "last":
                    f[n, a, 64 + nc - 1] = 6.0
                    e[n, a] = nc - 1
                    continue
                if kind == "other_quarter":
                    c1 = r % cq
                    c2 = cq * (1 + r % 3) + (3 * r) % cq
                elif kind == "same_quarter":
                    c1 = q * cq + r % (cq - 1)
                    c2 = c1 + 1
                elif cq >= 4:  # same_vector: the 4-vectors start at multiples of 4 in a quarter
                    c1 = q * cq + (r % (cq // 4)) * 4 + 1
                    c2 = c1 + 2
                else:
                    c1, c2 = q * cq, q * cq + 1
                assert c1 < c2 < nc
                f[n, a, 64 + c1] = f[n, a, 64 + c2] = 6.0
                e[n, a] = c1
        feats.append(f.view(N, h, w, 64 + nc))
        exp.append(e)
    return tuple(feats), torch.cat(exp, 1)


@functools.lru_cache(maxsize=None)
def decode_random(hw, nc, N=2):
    """(c) Random normal features of scale 2."""
    return tuple((torch.randn(N, h, w, 64 + nc, generator=_gen(10 + i)) * 2).to(BF16)
                 for i, (h, w) in enumerate(hw))


@functools.lru_cache(maxsize=None)
def decode_rowsplit(hw=DECODE_ROWSPLIT_LEVELS, nc=8):
    """(d) All DFL mass on bin 0: every box collapses onto its anchor centre times the stride."""
    feats, boxes = [], []
    for (h, w), s in zip(hw, DECODE_STRIDES):
        f = torch.full((1, h, w, 64 + nc), -40.0, dtype=BF16)
        f[..., 0:64:16] = 40.0
        f[..., 64:] = 0.0
        feats.append(f)
        ax, ay = _anchors(h, w)
        boxes.append(torch.stack([ax, ay, ax, ay], dim=-1)[None] * s)
    return tuple(feats), torch.cat(boxes, 1)
