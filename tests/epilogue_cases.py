"""Shared construction of the conv epilogue matrix (test_ops_cpu.py, test_kernels_gpu.py).

A case is a conv plus the buffers the models hand it: either YOLOv8's C2f form (residual
and output are two channel slices of one ``cat`` buffer, written in place) or a residual
slice of one wide buffer with the output slice in another.  A variant is an activation /
residual placement / bias combination.

Exact variants (activation NONE or RELU) use integer data: weights dense in {-1, +1}, x in
{-1, 0, 1}, bias and every element of the residual buffer in [-8, 8].  While
max |conv + bias| + 8 <= 256 every partial sum, every intermediate bf16 rounding and the
output are integers of at most 9 bits, exactly representable in bf16 and fp32 in any
summation order, so a kernel must reproduce the float64 result bit for bit.
SiLU variants use random normal data and the kernel suite's tolerances.
"""
import torch
import torch.nn.functional as F

from kvedge_amd import ops
from kvedge_amd.ops import ConvSpec

# name -> (cin, cout, k, pad, (N, H, W), in_place, ld of the residual buffer, r_coff,
#          ld of the output buffer, y_coff); in_place: residual buffer == output buffer
CASES = {
    "c2f64": (64, 64, 3, 1, (2, 13, 11), True, 256, 64, 256, 128),
    "c2f16": (16, 16, 3, 1, (2, 13, 11), True, 48, 16, 48, 32),       # generic-gather mode
    "c2f128": (128, 128, 3, 1, (3, 7, 9), True, 384, 128, 384, 256),  # K = 1152: 18 K steps
    "gemm136": (128, 136, 1, 0, (2, 13, 11), False, 176, 24, 160, 16),  # N tail
    "gemm512": (256, 512, 1, 0, (2, 13, 11), False, 576, 32, 536, 16),  # 8 N tiles of 64
    # the C2f conv with residual and output in two buffers of different row pitch: in the
    # in-place cases ldr == ldy, so a 3x3 kernel that took the output's pitch for the
    # residual's (the v4 / v10 direct forms take no 1x1 with a residual) would still pass
    "conv64": (64, 64, 3, 1, (2, 13, 11), False, 136, 40, 104, 16),
    # ... and at 16 channels: the v4 residual forms with Cin <= 32 prefetch the band's
    # residual through an address expression of their own
    "conv16": (16, 16, 3, 1, (2, 13, 11), False, 56, 24, 40, 8),
}

# name -> (act bits, residual, bias)
VARIANTS = {
    "none_res": (ops.ACT_NONE, True, True),
    "relu_res": (ops.ACT_RELU, True, True),                        # act(conv + res)
    "relu_post": (ops.ACT_RELU | ops.RES_AFTER_ACT, True, True),   # act(conv) + res
    "silu_post": (ops.ACT_SILU | ops.RES_AFTER_ACT, True, True),   # the C2f bottleneck's form
    "silu_res": (ops.ACT_SILU, True, True),
    "relu_res_nobias": (ops.ACT_RELU, True, False),
    "silu_nores": (ops.ACT_SILU, False, True),
}
EXACT_VARIANTS = [v for v, (a, _, _) in VARIANTS.items() if (a & 3) != ops.ACT_SILU]
EXACT_BOUND = 256  # integers up to 2^8 are exact in bf16 (8 significand bits)

_cache = {}


def is_exact(variant):
    return variant in EXACT_VARIANTS


def build(case, variant, n=None, seed=0):
    """Inputs, the destination buffer before the call and the CPU reference's destination
    buffer after it, built once per (case, variant, n) and never modified afterwards.

    Returns a dict: spec, x, w (packed), b, res (buffer or None), r_coff, dst0 (destination
    before the call), y_coff, in_place, ref (destination after the CPU reference ran),
    and for exact variants ref64 (float64 output slice) and bound (max |conv + bias| + 8).
    """
    key = (case, variant, n, seed)
    if key in _cache:
        return _cache[key]
    cin, cout, k, pad, (N, H, W), in_place, ldr, r_coff, ldy, y_coff = CASES[case]
    if n is not None:
        N = n
    act, has_res, has_bias = VARIANTS[variant]
    exact = is_exact(variant)
    spec = ConvSpec.auto(cin, cout, k, 1, pad, act)
    g = torch.Generator().manual_seed(1000 * seed + 17 * list(CASES).index(case)
                                      + list(VARIANTS).index(variant))
    if exact:
        x = torch.randint(-1, 2, (N, H, W, cin), generator=g).to(torch.bfloat16)
        w = (torch.randint(0, 2, (cout, cin, k, k), generator=g) * 2 - 1).float()
        b = torch.randint(-8, 9, (cout,), generator=g).float()
        rbuf = torch.randint(-8, 9, (N, H, W, ldr), generator=g).to(torch.bfloat16)
    else:
        x = torch.randn(N, H, W, cin, generator=g).to(torch.bfloat16)
        w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        rbuf = torch.randn(N, H, W, ldr, generator=g).to(torch.bfloat16)
    wp = ops.pack_conv_weight(w, spec)
    if in_place:
        dst0 = rbuf
    else:  # a separate destination: NaN everywhere the conv does not write
        dst0 = torch.full((N, H, W, ldy), float("nan"), dtype=torch.bfloat16)
    c = dict(spec=spec, x=x, w=wp, b=b if has_bias else None, res=rbuf if has_res else None,
             r_coff=r_coff if has_res else 0, dst0=dst0, y_coff=y_coff, in_place=in_place,
             cout=cout)
    ref = dst0.clone()
    ops.conv2d(x, spec, wp, c["b"], res=ref if (has_res and in_place) else c["res"], out=ref,
               r_coff=c["r_coff"], y_coff=y_coff)
    c["ref"] = ref
    if exact:
        y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, 1, pad).permute(0, 2, 3, 1)
        if has_bias:
            y = y + b.double()
        c["bound"] = y.abs().max().item() + 8
        a, post = act & 3, bool(act & ops.RES_AFTER_ACT)
        r = rbuf[..., r_coff:r_coff + cout].double() if has_res else None
        if r is not None and not post:
            y = y + r
        if a == ops.ACT_RELU:
            y = y.clamp_min(0)
        if r is not None and post:
            y = y + r
        c["ref64"] = y
    _cache[key] = c
    return c


def same_bits(a, b):
    """Bitwise equality of two bf16 tensors (NaN canaries compare equal to themselves)."""
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def outside(t, y_coff, cout):
    """The channels of t outside the written slice [y_coff, y_coff + cout)."""
    return torch.cat([t[..., :y_coff], t[..., y_coff + cout:]], -1)
