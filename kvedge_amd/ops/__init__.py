"""kvedge_amd.ops — Python face of the gfx950 HIP kernel library.

Contract
--------
* GPU tensors ALWAYS go to the hand-written HIP kernels in ``kvedge_amd/_C.so``.
  If the extension is missing on a GPU box the call raises — there is no silent
  eager fallback on the device path.
* CPU tensors go to :mod:`kvedge_amd.ops.reference`, a plain-PyTorch fp32
  implementation of the *same* semantics (NHWC, packed weights, channel slices).
  That path exists so the model/engine/module plumbing is testable without a GPU
  and doubles as the numerics oracle for the kernel tests.

Layout conventions (shared by kernels and reference):
* activations: NHWC bf16, viewed as ``[N, H, W, ld]``; an op may read/write a
  channel slice ``[coff, coff + C)`` of a wider buffer (concat-free YOLO neck).
* conv weights: packed ``[Cout, Kpad]`` bf16, k-order ``(r, s, c)``; BN folded.
  Stem mode (mode 2): input padded to 4 channels, KW padded to even,
  k-order ``(r, s_padded, c4)`` so that each 8-element MFMA k-chunk is two
  adjacent pixels (16 contiguous bytes).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import reference as _ref

# KVEDGE_CHECKS=1 selects the bounds-check build (python -m kvedge_amd._build with the
# same variable set): launchers verify operand extents against their HIP allocations.
# KVEDGE_LIB=<file name in kvedge_amd/> selects another in-tree build of the same sources
# (A/B of one kernel change on one box: tools/ab_build.sh)
_LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                         "_C_checks.so" if os.environ.get("KVEDGE_CHECKS", "0") not in ("", "0")
                         else os.path.basename(os.environ.get("KVEDGE_LIB", "") or "_C.so"))
_loaded = False
_load_error: Optional[str] = None

ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2
RES_AFTER_ACT = 4  # flag: y = act(conv) + res  (default: y = act(conv + res))
MODE_GENERAL, MODE_GEMM, MODE_STEM = 0, 1, 2
BK = 64


def load(build_if_missing: bool = False) -> bool:
    """Load the native op library once. Returns True when available."""
    global _loaded, _load_error
    if _loaded:
        return True
    if not os.path.exists(_LIB_PATH) and build_if_missing:
        from .. import _build

        _build.build()
    if not os.path.exists(_LIB_PATH):
        _load_error = f"{_LIB_PATH} not built (run `python -m kvedge_amd._build`)"
        return False
    try:
        torch.ops.load_library(_LIB_PATH)
    except Exception as e:  # pragma: no cover - depends on build state
        _load_error = f"failed to load {_LIB_PATH}: {e}"
        return False
    _check_single_hip_runtime()
    global SPLITK0
    SPLITK0 = int(torch.ops.kvedge.conv_splitk_base())
    if int(torch.ops.kvedge.conv_splitk_num_tiles()) != N_SPLITK_TILES:
        _load_error = "split-K tile count differs from the native library (stale build?)"
        return False
    _loaded = True
    return True


def _check_single_hip_runtime() -> None:
    """Two libamdhip64 copies in one process (torch's + system) would split HIP state."""
    try:
        with open("/proc/self/maps") as f:
            libs = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    except OSError:
        return
    real = {os.path.realpath(p) for p in libs}
    if len(real) > 1:
        raise RuntimeError(f"kvedge: multiple HIP runtimes loaded: {sorted(real)}")


def native_available() -> bool:
    return load()


def library_path() -> str:
    return _LIB_PATH


# ---------------------------------------------------------------------------
# activation allocation (every op/model output goes through here so the native arena
# planner can see tensor lifetimes: kvedge_amd.runtime.plan_memory)
# ---------------------------------------------------------------------------
_recorder = None


def empty(*shape, dtype=None, device=None) -> torch.Tensor:
    t = torch.empty(*shape, dtype=dtype, device=device)
    if _recorder is not None:
        _recorder(t)
    return t


def set_alloc_recorder(fn) -> None:
    """Install (or clear with None) a callback seeing every activation allocation."""
    global _recorder
    _recorder = fn


def _native():
    if not load():
        raise RuntimeError(
            "kvedge_amd native kernels are required for GPU tensors but unavailable: "
            f"{_load_error}")
    return torch.ops.kvedge


# ---------------------------------------------------------------------------
# conv spec + weight packing
# ---------------------------------------------------------------------------
@dataclass
class ConvSpec:
    cin: int
    cout: int
    kh: int
    kw: int
    stride: int = 1
    pad: int = 0
    act: int = ACT_NONE
    mode: int = MODE_GENERAL
    pad_b: int = -1  # bottom/right padding when asymmetric (s2d stem); -1 = same as pad

    @property
    def pad_end(self) -> int:
        return self.pad if self.pad_b < 0 else self.pad_b

    @property
    def cin_eff(self) -> int:
        return 4 if self.mode == MODE_STEM else self.cin

    @property
    def kwp(self) -> int:
        return (self.kw + 1) // 2 * 2

    @property
    def K(self) -> int:
        if self.mode == MODE_STEM:
            return self.kh * self.kwp * 4
        return self.kh * self.kw * self.cin

    @property
    def Kpad(self) -> int:
        return (self.K + BK - 1) // BK * BK

    def out_hw(self, h: int, w: int):
        p = self.pad + self.pad_end
        return ((h + p - self.kh) // self.stride + 1, (w + p - self.kw) // self.stride + 1)

    @staticmethod
    def auto(cin, cout, k, stride=1, pad=None, act=ACT_NONE) -> "ConvSpec":
        if pad is None:
            pad = k // 2
        if cin < 8:
            mode = MODE_STEM
        elif k == 1 and stride == 1 and pad == 0:
            mode = MODE_GEMM
        else:
            mode = MODE_GENERAL
        return ConvSpec(cin, cout, k, k, stride, pad, act, mode)


def pack_conv_weight(w: torch.Tensor, spec: ConvSpec) -> torch.Tensor:
    """torch OIHW fp32 -> packed [Cout, Kpad] bf16 (k-order (r, s, c))."""
    assert w.shape == (spec.cout, spec.cin, spec.kh, spec.kw), (w.shape, spec)
    w = w.detach().float()
    if spec.mode == MODE_STEM:
        wp = torch.zeros(spec.cout, spec.kh, spec.kwp, 4, dtype=torch.float32, device=w.device)
        wp[:, :, :spec.kw, :spec.cin] = w.permute(0, 2, 3, 1)
        flat = wp.reshape(spec.cout, -1)
    else:
        flat = w.permute(0, 2, 3, 1).reshape(spec.cout, -1)
    out = torch.zeros(spec.cout, spec.Kpad, dtype=torch.float32, device=w.device)
    out[:, :flat.shape[1]] = flat
    return out.to(torch.bfloat16).contiguous()


def unpack_conv_weight(wp: torch.Tensor, spec: ConvSpec) -> torch.Tensor:
    """Inverse of :func:`pack_conv_weight` -> OIHW fp32 (bf16-rounded values)."""
    wf = wp.float()[:, :spec.K]
    if spec.mode == MODE_STEM:
        w4 = wf.reshape(spec.cout, spec.kh, spec.kwp, 4)[:, :, :spec.kw, :spec.cin]
        return w4.permute(0, 3, 1, 2).contiguous()
    return wf.reshape(spec.cout, spec.kh, spec.kw, spec.cin).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------
# Split-K workspaces (v8 tiles): fp32 slabs [ksplit][M][Cout], one per K slice of a tile
# (plain stores; the finalize kernel sums them), one workspace per (device, stream), since
# layers on one stream run in order while the multi-stream engine's slices run concurrently.
# Sized on first use (warm-up, before hipGraph capture) for the largest split (32) that fits
# under SPLITK_MAX_ELEMS; a tile whose slabs do not fit is refused by the launcher (the
# autotuner skips it), so big layers only ever take their smaller splits.
_WS: dict = {}
SPLITK_MAX_ELEMS = 32 << 20  # 128 MB of fp32 per stream at most
SPLITK_MAX_SPLIT = 32        # largest split of conv_sk.hip kSkTiles
N_SPLITK_TILES = 19          # conv_sk.hip kSkTiles
N_DE_TILES = 3               # v10 direct-epilogue tiles (conv_direct.hip): after split-K
N_SKINNY_TILES = 9           # v12 edge-batch tiles (conv_skinny.hip kSknTiles): before v14
SPLITK0 = 1 << 30            # first split-K tile index, set by load()


def is_splitk(tile: int) -> bool:
    return SPLITK0 <= tile < SPLITK0 + N_SPLITK_TILES


def splitk_workspace(device: torch.device, elems: int) -> Optional[torch.Tensor]:
    """The stream's split-K workspace for a layer of ``elems`` = M x Cout outputs (None if
    not even two slabs fit under SPLITK_MAX_ELEMS).

    Allocated ONCE per (device, stream) at the full SPLITK_MAX_ELEMS (128 MB of fp32 --
    noise in 288 GB of HBM) and never replaced: a captured hipGraph holds the raw pointer,
    not the tensor, and torch hands out pooled stream handles round-robin, so a later
    engine or the autotuner can reach the same key.  Growing the buffer would free memory
    a live graph still writes its slabs into."""
    if elems > SPLITK_MAX_ELEMS // 2:
        return None
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        ws = torch.empty(SPLITK_MAX_ELEMS, dtype=torch.float32, device=device)
        _WS[key] = ws
    return ws


def conv2d(x: torch.Tensor, spec: ConvSpec, w: torch.Tensor, bias: Optional[torch.Tensor],
           res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           x_coff: int = 0, y_coff: int = 0, r_coff: int = 0, tile: int = -1) -> torch.Tensor:
    """Fused conv + bias (+ residual) (+ act).  x: [N,H,W,ldx] bf16 -> out [N,Ho,Wo,ldy]."""
    N, H, W, ldx = x.shape
    Ho, Wo = spec.out_hw(H, W)
    if out is None:
        out = empty(N, Ho, Wo, spec.cout, dtype=torch.bfloat16, device=x.device)
    assert out.shape[:3] == (N, Ho, Wo), (out.shape, (N, Ho, Wo))
    ldy = out.shape[3]
    ldr = res.shape[-1] if res is not None else 0
    # in place (YOLO C2f: residual and output are slices of one concat buffer): the kernels'
    # workgroups read residual channels while others write output channels, in no order
    if (res is not None and res.data_ptr() == out.data_ptr() and ldr == ldy
            and r_coff < y_coff + spec.cout and y_coff < r_coff + spec.cout):
        raise ValueError(f"kvedge: residual slice [{r_coff}, {r_coff + spec.cout}) and output "
                         f"slice [{y_coff}, {y_coff + spec.cout}) of one buffer overlap")
    if x.is_cuda:
        ws = splitk_workspace(x.device, N * Ho * Wo * spec.cout) if is_splitk(tile) else None
        _native().conv(x, w, bias, res, out, N, H, W, spec.cin_eff, ldx, x_coff, Ho, Wo,
                       spec.cout, spec.kh, spec.kw, spec.stride, spec.pad, spec.K, ldy, y_coff,
                       ldr, r_coff, spec.act, spec.mode, tile, ws)
    else:
        _ref.conv2d(x, spec, w, bias, res, out, x_coff, y_coff, r_coff)
    return out


def conv_pair(x: torch.Tensor, spec: ConvSpec, w: torch.Tensor, bias: torch.Tensor,
              w2: torch.Tensor, b2: torch.Tensor, out: torch.Tensor, x_coff: int = 0,
              z_coff: int = 0, tile: int = 0) -> torch.Tensor:
    """Fused YOLO Detect-branch pair: out[..., z_coff : z_coff + C2] =
    act(conv3x3/1(x[..., x_coff:]) + bias) . w2^T + b2, the 3x3's output t kept on chip
    (csrc/kernels/conv_direct.hip, C2 forms).  spec: the 3x3 (stride 1, pad 1); w2: bf16
    [C2, Cout] (the 1x1's packed weight without K padding); tile: direct tile 0-3.
    CPU: the two reference convs in sequence, t rounded to bf16 in between."""
    assert spec.kh == 3 and spec.stride == 1 and spec.pad == 1 and spec.mode == MODE_GENERAL
    C2 = w2.shape[0]
    assert w2.shape[1] == spec.cout and out.shape[:3] == x.shape[:3]
    if x.is_cuda:
        _native().conv_pair(x, w, bias, w2, b2, out, spec.cin, x_coff, z_coff, spec.act, tile)
        return out
    t = torch.empty(*x.shape[:3], spec.cout, dtype=torch.bfloat16)
    _ref.conv2d(x, spec, w, bias, None, t, x_coff, 0, 0)
    z = t.float() @ w2.float().t() + b2.float()
    out[..., z_coff:z_coff + C2] = z.to(out.dtype)
    return out


def conv_dual(x1: torch.Tensor, x2: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor],
              act: int, stride2: int, out: Optional[torch.Tensor] = None,
              tile: int = -1) -> torch.Tensor:
    """Bottleneck conv3 + downsample in ONE GEMM (K = K1 + K2):
    out = act(x1 . W[:, :K1]^T + x2[::s, ::s] . W[:, K1:]^T + bias), all 1x1.
    The downsample's output tensor is never written or re-read."""
    N, Ho, Wo, K1 = x1.shape
    cout = w.shape[0]
    if out is None:
        out = empty(N, Ho, Wo, cout, dtype=torch.bfloat16, device=x1.device)
    if x1.is_cuda:
        ws = splitk_workspace(x1.device, N * Ho * Wo * cout) if is_splitk(tile) else None
        _native().conv_dual(x1, x2, w, bias, out, stride2, act, tile, ws)
    else:
        _ref.conv_dual(x1, x2, w, bias, act, stride2, out)
    return out


def conv_dual2(x: torch.Tensor, K1: int, x2: torch.Tensor, w: torch.Tensor,
               bias: Optional[torch.Tensor], act: int, out: torch.Tensor, x_coff: int = 0,
               x2_coff: int = 0, y_coff: int = 0, stride2: int = 1, up2: bool = False,
               tile: int = -1) -> torch.Tensor:
    """Dual-source 1x1 GEMM over channel slices: out[..., y_coff : y_coff + Cout] =
    act(x[..., x_coff : x_coff + K1] . W[:, :K1]^T + x2'[..., x2_coff : x2_coff + K2] . W[:, K1:]^T
    + bias), x2' = x2 at ``stride2``, or with ``up2`` x2 (half resolution) upsampled 2x
    nearest -- YOLO's neck C2f cv1 reads its [upsampled | skip] concat without the upsample
    launch or the concat's upsampled half (v2 LDS-DMA tiles and their v7 / v8 forms only)."""
    if x.is_cuda:
        N, Ho, Wo, _ = x.shape
        ws = splitk_workspace(x.device, N * Ho * Wo * w.shape[0]) if is_splitk(tile) else None
        _native().conv_dual2(x, x_coff, K1, x2, x2_coff, w, bias, out, y_coff, stride2,
                             1 if up2 else 0, act, tile, ws)
    else:
        _ref.conv_dual2(x, x_coff, K1, x2, x2_coff, w, bias, act, stride2, up2, out, y_coff)
    return out


def conv_tail(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act: int,
              w1: torch.Tensor, b1: Optional[torch.Tensor], res: Optional[torch.Tensor] = None,
              x2: Optional[torch.Tensor] = None, stride2: int = 1,
              out: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None,
              tile: int = -1):
    """Fused bottleneck tail: y = act(x . W^T + bias + res) -- or, with ``x2``, the dual
    conv3 + downsample GEMM of :func:`conv_dual` -- AND z = ReLU(y . w1^T + b1), the next
    block's 1x1 reduce conv, in one pass: y is written once and never re-read from HBM.
    w: packed [Cout, K] (1x1); w1: packed [n_t, Cout].  Returns (y, z)."""
    N, H, W, _ = x.shape
    cout, nt = w.shape[0], w1.shape[0]
    if out is None:
        out = empty(N, H, W, cout, dtype=torch.bfloat16, device=x.device)
    if z is None:
        z = empty(N, H, W, nt, dtype=torch.bfloat16, device=x.device)
    if x.is_cuda:
        _native().conv_tail(x, x2, w, bias, res, out, w1, b1, z, stride2, act, tile)
        return out, z
    if x2 is not None:
        _ref.conv_dual(x, x2, w, bias, act, stride2, out)
    else:
        spec = ConvSpec.auto(x.shape[3], cout, 1, 1, 0, act)
        _ref.conv2d(x, spec, w, bias, res, out, 0, 0, 0)
    spec1 = ConvSpec.auto(cout, nt, 1, 1, 0, ACT_RELU)
    _ref.conv2d(out, spec1, w1, b1, None, z, 0, 0, 0)
    return out, z


# v9 bottleneck seams (csrc/kernels/conv_seam.hip) the tail path takes: (conv3 K3, conv3
# Cout, next conv1 Cout) -- ResNet-50 stage 2, 2 -> 3 and 3.  The 3 -> 4 boundary seam
# (N1 = 512) is level with the two unfused launches at batch 640 and stays unfused
# (profiles/r4_v2_seam_probe_b640.md)
SEAM_SHAPES = {(128, 512, 128), (128, 512, 256), (256, 1024, 256)}
SEAM_ENABLED = os.environ.get("KVEDGE_SEAM", "1") != "0"
# ... only when the layer gives every CU a 128-row workgroup (edge batches: split-K instead)
SEAM_MIN_WGS = int(os.environ.get("KVEDGE_SEAM_MIN_WGS", "256"))


# v13 fused YOLOv8 C2f(32, 32, n=1, shortcut) (csrc/kernels/c2f_fused.hip): the b2 block at
# 160 x 160.  KVEDGE_C2F=0 = the four-launch path (A/B knob)
C2F_ENABLED = os.environ.get("KVEDGE_C2F", "1") != "0"


def c2f16_strip(H: int, W: int) -> int:
    """Output rows per workgroup of the fused C2f kernel (0 = no form for this shape)."""
    for S in (40, 32, 20, 16, 8, 4):
        if H % S == 0 and W in (80, 160):
            return S
    return 0


def c2f16(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, wm1: torch.Tensor,
          bm1: torch.Tensor, wm2: torch.Tensor, bm2: torch.Tensor, w2: torch.Tensor,
          b2: torch.Tensor, out: Optional[torch.Tensor] = None, x_coff: int = 0,
          y_coff: int = 0, S: int = 0) -> torch.Tensor:
    """YOLOv8 C2f(32, 32, n=1, shortcut) as one pass: t = SiLU(W1 . x + b1) (a = t[:16],
    s = t[16:]), u = SiLU(conv3x3(s) + bm1), v = s + SiLU(conv3x3(u) + bm2),
    y = SiLU(W2 . [a, s, v] + b2).  Packed bf16 weights w1 [32, >=32], wm1 / wm2 [16, >=144]
    (tap-major), w2 [32, >=48]; fp32 biases.  GPU: one launch, t / u / v never leave the chip.
    CPU: the four reference convs with bf16 intermediates (what the kernel keeps in LDS and
    registers, and what the four-launch path writes)."""
    N, H, W, _ = x.shape
    if out is None:
        out = empty(N, H, W, 32, dtype=torch.bfloat16, device=x.device)
    if x.is_cuda:
        _native().c2f16_fused(x, x_coff, w1, b1, wm1, bm1, wm2, bm2, w2, b2, out, y_coff,
                              S or c2f16_strip(H, W))
        return out
    s1 = ConvSpec.auto(32, 32, 1, 1, 0, ACT_SILU)
    sm1 = ConvSpec.auto(16, 16, 3, 1, 1, ACT_SILU)
    sm2 = ConvSpec.auto(16, 16, 3, 1, 1, ACT_SILU | RES_AFTER_ACT)
    s2 = ConvSpec.auto(48, 32, 1, 1, 0, ACT_SILU)
    cat = torch.empty(N, H, W, 48, dtype=torch.bfloat16)
    u = torch.empty(N, H, W, 16, dtype=torch.bfloat16)
    _ref.conv2d(x, s1, w1, b1, None, cat, x_coff, 0, 0)
    _ref.conv2d(cat, sm1, wm1, bm1, None, u, 16, 0, 0)
    _ref.conv2d(u, sm2, wm2, bm2, cat, cat, 0, 32, 16)
    _ref.conv2d(cat, s2, w2, b2, None, out, 0, y_coff, 0)
    return out


def stem_pool(x: torch.Tensor, spec: "ConvSpec", w: torch.Tensor, bias: torch.Tensor,
              out: Optional[torch.Tensor] = None, y_coff: int = 0) -> torch.Tensor:
    """Fused ResNet stem + max pool: maxpool3x3/2(relu(conv_s2d(x) + bias)).

    x: the space-to-depth image [N, H, W, 16] (ops.preprocess(s2d=True)); spec/w/bias:
    the s2d stem DeployedConv (4x4, stride 1, pads 2/1, Cout 64, ReLU).  -> [N, H/2, W/2, 64].
    GPU: one kernel (csrc/kernels/stem_pool.hip), the 112x112x64 stem output never
    touches HBM.  CPU: the reference conv followed by the reference pool."""
    assert spec.cin == 16 and spec.cout == 64 and spec.kh == 4 and spec.stride == 1
    assert spec.pad == 2 and spec.pad_end == 1 and spec.act == ACT_RELU and spec.Kpad == 256
    N, H, W, _ = x.shape
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = empty(N, Hp, Wp, 64, dtype=torch.bfloat16, device=x.device)
    if x.is_cuda:
        _native().stem_pool(x, w, bias, out, y_coff)
    else:
        y = conv2d(x, spec, w, bias)
        maxpool2d(y, 3, 2, 1, out=out, y_coff=y_coff)
    return out


def stem_pool_frames(frames: torch.Tensor, spec: "ConvSpec", w: torch.Tensor,
                     bias: torch.Tensor, out: Optional[torch.Tensor] = None, y_coff: int = 0,
                     mean=None, std=None) -> torch.Tensor:
    """Frames-in ResNet stem + pool: preprocess(s2d) fused into :func:`stem_pool`.

    frames: uint8 [N, H, W, 3] (H even, W % 4 == 0) -> [N, H/4, W/4, 64] (224 -> 56).
    GPU: stem_pool.hip's U8 instantiation -- the patch fetch reads the raw bytes (one
    12-B load per two s2d pixels), normalises and space-to-depths them in registers; the
    bf16 s2d image (32 B/px) is never written.  CPU: the reference preprocess + stem_pool."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    mean = IMAGENET_MEAN if mean is None else mean
    std = IMAGENET_STD if std is None else std
    if not frames.is_cuda:
        return stem_pool(preprocess(frames, mean=mean, std=std, s2d=True), spec, w, bias,
                         out=out, y_coff=y_coff)
    assert spec.cin == 16 and spec.cout == 64 and spec.kh == 4 and spec.stride == 1
    assert spec.pad == 2 and spec.pad_end == 1 and spec.act == ACT_RELU and spec.Kpad == 256
    N, H0, W0, _ = frames.shape
    H, W = H0 // 2, W0 // 2
    if out is None:
        out = empty(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64, dtype=torch.bfloat16,
                    device=frames.device)
    _native().stem_pool_frames(frames, w, bias, out, list(mean), list(std), y_coff)
    return out


def pack_stem12(wf: torch.Tensor) -> torch.Tensor:
    """Folded 7x7/2 stem weights [Cout, 3, 7, 7] -> the 12-channel s2d 4x4 form [Cout, 192]
    bf16 that csrc/kernels/stem12.hip reads.  K index = r*48 + s*12 + dy*6 + dx*3 + c for
    s2d tap (r, s) in 4x4 and s2d channel (dy, dx, c); its weight is
    wf[:, c, 2r-1+dy, 2s-1+dx] (zero where that leaves 0..6)."""
    cout, cin, k, _ = wf.shape
    assert cin == 3 and k == 7
    w = torch.zeros(cout, 4, 4, 2, 2, 3)
    for r in range(4):
        for dy in range(2):
            ky = 2 * r - 1 + dy
            if not 0 <= ky < 7:
                continue
            for s_ in range(4):
                for dx in range(2):
                    kx = 2 * s_ - 1 + dx
                    if 0 <= kx < 7:
                        w[:, r, s_, dy, dx, :] = wf[:, :, ky, kx].float()
    return w.reshape(cout, 192).to(torch.bfloat16).contiguous()


def stem12_reference(frames: torch.Tensor, w12: torch.Tensor, bias: torch.Tensor,
                     mean=None, std=None) -> torch.Tensor:
    """CPU reference of :func:`stem12_pool_frames`, step for step: normalise (fp32) -> bf16,
    12-channel space-to-depth, 4x4 stride-1 conv (pads 2 / 1) in fp32, bf16, ReLU, 3x3/2
    max pool (pad 1)."""
    mean = IMAGENET_MEAN if mean is None else mean
    std = IMAGENET_STD if std is None else std
    N, H0, W0, _ = frames.shape
    Hs, Ws = H0 // 2, W0 // 2
    m = torch.tensor(mean, dtype=torch.float32)
    inv = 1.0 / torch.tensor(std, dtype=torch.float32)
    x = (frames.float() * (inv / 255.0) + (-m * inv)).to(torch.bfloat16).float()
    x = x.view(N, Hs, 2, Ws, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(N, Hs, Ws, 12)
    xp = torch.nn.functional.pad(x, (0, 0, 2, 1, 2, 1))  # X: 2 left 1 right, Y: 2 top 1 bottom
    cols = xp.unfold(1, 4, 1).unfold(2, 4, 1)            # [N, Hs, Ws, 12, 4(r), 4(s)]
    cols = cols.permute(0, 1, 2, 4, 5, 3).reshape(N, Hs, Ws, 192)
    y = cols @ w12.float().t() + bias.float()
    y = y.to(torch.bfloat16).float().relu()
    y = torch.nn.functional.max_pool2d(y.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    return y.to(torch.bfloat16).contiguous()


def stem12_pool_frames(frames: torch.Tensor, w12: torch.Tensor, bias: torch.Tensor,
                       out: Optional[torch.Tensor] = None, y_coff: int = 0,
                       mean=None, std=None) -> torch.Tensor:
    """Frames-in ResNet stem + ReLU + 3x3/2 max pool over a 12-channel space-to-depth image
    (K = 192 instead of the 16-channel form's 256; csrc/kernels/stem12.hip).
    frames: uint8 [N, H, W, 3] (H even, W % 4 == 0); w12: :func:`pack_stem12`.
    -> [N, H/4, W/4, 64] (224 -> 56).  CPU: :func:`stem12_reference`."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    mean = IMAGENET_MEAN if mean is None else mean
    std = IMAGENET_STD if std is None else std
    N, H0, W0, _ = frames.shape
    Hs, Ws = H0 // 2, W0 // 2
    if out is None:
        out = empty(N, (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1, 64, dtype=torch.bfloat16,
                    device=frames.device)
    if not frames.is_cuda:
        out[..., y_coff:y_coff + 64] = stem12_reference(frames, w12, bias, mean, std)
        return out
    _native().stem12_pool_frames(frames, w12, bias, out, list(mean), list(std), y_coff)
    return out


def yolo_stem2_fits(frames_shape) -> bool:
    """Shapes the fused YOLO b0 + b1 kernel takes (csrc/kernels/yolo_stem2.hip)."""
    _, H, W, _ = frames_shape
    return H % 4 == 0 and W % 32 == 0 and 0 < W <= 640


def yolo_stem2(frames: torch.Tensor, spec0: "ConvSpec", w0: torch.Tensor, b0: torch.Tensor,
               spec1: "ConvSpec", w1: torch.Tensor, b1: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """YOLOv8n b0 (frames-in s2d stem, SiLU) + b1 (3x3/2 16 -> 32, SiLU) in ONE pass: b0's
    [N, H/2, W/2, 16] output stays in LDS (csrc/kernels/yolo_stem2.hip).
    frames: uint8 [N, H, W, 3] with :func:`yolo_stem2_fits`; spec0/w0/b0: a
    DeployedConv.stem_s2d(..., in_scale=1/255); spec1/w1/b1: the 3x3/2 16 -> 32 conv.
    -> [N, H/4, W/4, 32].  CPU: the two reference ops in sequence (bf16 in between)."""
    assert spec0.kh == 2 and spec0.cin == 16 and spec0.cout == 16, spec0
    assert (spec1.kh, spec1.stride, spec1.cin, spec1.cout) == (3, 2, 16, 32), spec1
    assert spec0.act == ACT_SILU and spec1.act == ACT_SILU
    N, H, W, _ = frames.shape
    if out is None:
        out = empty(N, H // 4, W // 4, 32, dtype=torch.bfloat16, device=frames.device)
    if not frames.is_cuda:
        x = stem_from_frames(frames, spec0, w0, b0)
        return conv2d(x, spec1, w1, b1, out=out)
    _native().yolo_stem2(frames, w0, b0, w1, b1, out)
    return out


def stem_from_frames(frames: torch.Tensor, spec: "ConvSpec", w: torch.Tensor,
                     bias: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
                     tile: int = -1) -> torch.Tensor:
    """Preprocess + space-to-depth + 2x2 s2d stem conv in ONE pass (YOLO b0).

    frames: uint8 [N, H, W, 3]; spec/w/bias: a DeployedConv.stem_s2d(..., in_scale=1/255)
    (weights scaled for raw 0..255 inputs, so the 1/255 normalisation costs nothing).
    GPU: the frames-in v4 direct kernel (csrc/kernels/conv_direct.hip) builds the s2d
    patch from raw bytes in LDS -- the [N, H/2, W/2, 16] bf16 image is never written.
    CPU: the reference preprocess (values 0..255) then the reference conv."""
    assert spec.kh == 2 and spec.stride == 1 and spec.cin == 16, spec
    N, H, W, _ = frames.shape
    if out is None:
        out = empty(N, H // 2, W // 2, spec.cout, dtype=torch.bfloat16, device=frames.device)
    if frames.is_cuda:
        _native().conv_frames_s2d(frames, w, bias, out, spec.act, tile)
        return out
    x = preprocess(frames, mean=(0.0, 0.0, 0.0), std=(1.0 / 255,) * 3, s2d=True)
    return conv2d(x, spec, w, bias, out=out)


def _check_slices(op: str, C: int, ldx: int, x_coff: int, out: torch.Tensor, y_coff: int,
                  out_nhw: Tuple[int, int, int]) -> None:
    """The channel-slice contract of maxpool2d / upsample2x, the same on both paths: the
    kernels move 8 channels (16 B) per access and trust the slices to lie inside their rows."""
    ldy = out.shape[3] if out.dim() == 4 else -1
    if out.dim() != 4 or tuple(out.shape[:3]) != tuple(out_nhw):
        raise ValueError(f"{op}: out must be [N, Ho, Wo, ldy] = {tuple(out_nhw)} + (ldy,), "
                         f"got {tuple(out.shape)}")
    if C <= 0 or x_coff < 0 or y_coff < 0 or any(v % 8 for v in (C, ldx, x_coff, ldy, y_coff)):
        raise ValueError(f"{op}: C, ldx, x_coff, ldy, y_coff must be multiples of 8, got "
                         f"{(C, ldx, x_coff, ldy, y_coff)}")
    if x_coff + C > ldx:
        raise ValueError(f"{op}: input slice [{x_coff}, {x_coff + C}) exceeds ldx = {ldx}")
    if y_coff + C > ldy:
        raise ValueError(f"{op}: output slice [{y_coff}, {y_coff + C}) exceeds ldy = {ldy}")


def maxpool2d(x: torch.Tensor, k: int, stride: int, pad: int, out: Optional[torch.Tensor] = None,
              C: Optional[int] = None, x_coff: int = 0, y_coff: int = 0) -> torch.Tensor:
    N, H, W, ldx = x.shape
    C = C or (ldx - x_coff)
    Ho = (H + 2 * pad - k) // stride + 1
    Wo = (W + 2 * pad - k) // stride + 1
    if out is None:
        out = empty(N, Ho, Wo, C, dtype=x.dtype, device=x.device)
    _check_slices("maxpool2d", C, ldx, x_coff, out, y_coff, (N, Ho, Wo))
    if x.is_cuda:
        _native().maxpool2d(x, out, N, H, W, C, ldx, x_coff, out.shape[3], y_coff, k, stride, pad,
                            Ho, Wo)
    else:
        _ref.maxpool2d(x[..., x_coff:x_coff + C], out, C, k, stride, pad, y_coff)
    return out


def sppf_pool(buf: torch.Tensor, C: int) -> torch.Tensor:
    """buf [N,H,W,4C] with x in slice 0 -> fills slices 1..3 with mp5/mp9/mp13."""
    N, H, W, ld = buf.shape
    assert ld == 4 * C
    if buf.is_cuda:
        _native().sppf_pool(buf, N, H, W, C)
    else:
        _ref.sppf_pool(buf, C)
    return buf


def global_avgpool(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    N, H, W, C = x.shape
    if out is None:
        out = empty(N, C, dtype=x.dtype, device=x.device)
    if x.is_cuda:
        _native().global_avgpool(x, out, N, H * W, C)
    else:
        out.copy_(x.float().mean(dim=(1, 2)).to(out.dtype))
    return out


POOLED_FC_MAX_BATCH = 16  # edge batches: the head runs as one GEMV launch up to here


def pooled_fc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor],
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Classifier head at edge batches in ONE launch: out [N, ncls] bf16 =
    fc(global_avgpool(x)) with the pooled vector rounded to bf16 as global_avgpool stores it.
    x: [N, H, W, C] bf16; w: the fc's packed [ncls, Kpad] bf16 weight (Kpad >= C).
    CPU: global_avgpool then the 1x1 conv reference."""
    N, H, W, C = x.shape
    ncls = w.shape[0]
    if out is None:
        out = empty(N, ncls, dtype=torch.bfloat16, device=x.device)
    if x.is_cuda:
        _native().pooled_fc(x, w, bias, out)
        return out
    pooled = global_avgpool(x).view(N, 1, 1, C)
    spec = ConvSpec(C, ncls, 1, 1, 1, 0, ACT_NONE, MODE_GEMM)
    _ref.conv2d(pooled, spec, w, bias, None, out.view(N, 1, 1, ncls))
    return out


def softmax_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None,
                 argmax: Optional[torch.Tensor] = None):
    if out is None:
        out = empty(x.shape, dtype=torch.float32, device=x.device)
    if argmax is None:
        argmax = empty(x.shape[0], dtype=torch.int64, device=x.device)
    if x.is_cuda:
        _native().softmax_rows(x, out, argmax)
    else:
        xf = x.float()
        out.copy_(torch.softmax(xf, dim=1))
        argmax.copy_(xf.argmax(dim=1))
    return out, argmax


def upsample2x(x: torch.Tensor, out: torch.Tensor, C: Optional[int] = None, x_coff: int = 0,
               y_coff: int = 0):
    N, H, W, ldx = x.shape
    C = C or (ldx - x_coff)
    _check_slices("upsample2x", C, ldx, x_coff, out, y_coff, (N, 2 * H, 2 * W))
    if x.is_cuda:
        _native().upsample2x(x, out, N, H, W, C, ldx, x_coff, out.shape[3], y_coff)
    else:
        up = x[..., x_coff:x_coff + C].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        out[..., y_coff:y_coff + C] = up
    return out


def yolo_decode(feats: Sequence[torch.Tensor], strides: Sequence[int], nc: int,
                boxes=None, scores=None, cls=None):
    f0, f1, f2 = feats
    N = f0.shape[0]
    hw = [(f.shape[1], f.shape[2]) for f in feats]
    A = sum(h * w for h, w in hw)
    dev = f0.device
    if boxes is None:
        boxes = empty(N, A, 4, dtype=torch.float32, device=dev)
        scores = empty(N, A, dtype=torch.float32, device=dev)
        cls = empty(N, A, dtype=torch.int32, device=dev)
    if f0.is_cuda:
        _native().yolo_decode(f0, f1, f2, hw[0][0], hw[0][1], hw[1][0], hw[1][1], hw[2][0],
                              hw[2][1], strides[0], strides[1], strides[2], nc, boxes, scores, cls)
    else:
        _ref.yolo_decode(feats, strides, nc, boxes, scores, cls)
    return boxes, scores, cls


def nms(boxes, scores, cls, conf: float = 0.25, iou: float = 0.7, max_det: int = 300,
        out=None, count=None):
    N = scores.shape[0]
    if out is None:
        out = empty(N, max_det, 6, dtype=torch.float32, device=scores.device)
        count = empty(N, dtype=torch.int32, device=scores.device)
    if scores.is_cuda:
        _native().nms(boxes, scores, cls, conf, iou, max_det, out, count)
    else:
        _ref.nms(boxes, scores, cls, conf, iou, max_det, out, count)
    return out, count


def synth_frames(out: torch.Tensor, seed: int, step) -> torch.Tensor:
    """On-device synthetic uint8 NHWC3 frames.  ``step`` int or a device int64[1] counter."""
    if out.is_cuda:
        if isinstance(step, torch.Tensor):
            _native().synth_frames_dev(out, step, seed)
        else:
            _native().synth_frames(out, seed, int(step))
    else:
        _ref.synth_frames(out, seed, step)
    return out


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def preprocess(x: torch.Tensor, out: Optional[torch.Tensor] = None, mean=IMAGENET_MEAN,
               std=IMAGENET_STD, s2d: bool = False) -> torch.Tensor:
    """uint8 NHWC3 frames -> normalized bf16, either NHWC4 (channel 3 zero) or, with
    ``s2d``, space-to-depth [N, H/2, W/2, 16] (channel (dy*2+dx)*4 + c)."""
    N, H, W, _ = x.shape
    if out is None:
        shape = (N, H // 2, W // 2, 16) if s2d else (N, H, W, 4)
        out = empty(shape, dtype=torch.bfloat16, device=x.device)
    if x.is_cuda:
        _native().preprocess(x, out, list(mean), list(std))
    else:
        _ref.preprocess(x, out, mean, std)
    return out


# ---------------------------------------------------------------------------
# camera front end: native-resolution frames -> model-size frames, boxes back to the frame
# ---------------------------------------------------------------------------
RESIZE_MAX_EXTENT = 8192  # S, R <= 8192 keeps the fixed-point resample inside int32
LETTERBOX_PAD = 114       # Ultralytics' letterbox grey


@dataclass(frozen=True)
class ResizePlan:
    """Geometry of one frame resample (:func:`frame_resize`).  Each axis is five integers
    ``(S, R, off, c0, cn)``: source extent, extent of the virtual resized image, offset of the
    destination content origin inside it (the crop offset; 0 for letterbox), first
    destination index holding content, number of destination indices holding content.
    Destination pixels outside the content are ``pad``."""
    axis_y: Tuple[int, int, int, int, int]
    axis_x: Tuple[int, int, int, int, int]
    pad: int
    src_hw: Tuple[int, int]
    dst_hw: Tuple[int, int]

    def box_map(self) -> Tuple[float, float, float, float]:
        """(cy, sy, cx, sx) of :func:`det_to_source`: source = (model - c) * s."""
        (sy_, ry, oy, c0y, _), (sx_, rx, ox, c0x, _) = self.axis_y, self.axis_x
        return float(c0y - oy), float(sy_ / ry), float(c0x - ox), float(sx_ / rx)


def _check_src_hw(src_hw, dst: int) -> Tuple[int, int]:
    hs, ws = int(src_hw[0]), int(src_hw[1])
    if not (1 <= hs <= RESIZE_MAX_EXTENT and 1 <= ws <= RESIZE_MAX_EXTENT):
        raise ValueError(f"frame size {hs}x{ws} outside 1..{RESIZE_MAX_EXTENT}")
    if not 1 <= dst <= RESIZE_MAX_EXTENT:
        raise ValueError(f"model size {dst} outside 1..{RESIZE_MAX_EXTENT}")
    return hs, ws


def letterbox_plan(src_hw, dst: int) -> ResizePlan:
    """Ultralytics letterbox into ``dst`` x ``dst``: scale by min(dst/Hs, dst/Ws) (upscaling
    allowed), centre, pad with 114."""
    hs, ws = _check_src_hw(src_hw, dst)
    r = min(dst / hs, dst / ws)
    nw = min(dst, max(1, int(round(ws * r))))
    nh = min(dst, max(1, int(round(hs * r))))
    left = int(round((dst - nw) / 2 - 0.1))
    top = int(round((dst - nh) / 2 - 0.1))
    return ResizePlan((hs, nh, 0, top, nh), (ws, nw, 0, left, nw), LETTERBOX_PAD, (hs, ws),
                      (dst, dst))


def center_crop_plan(src_hw, dst: int) -> ResizePlan:
    """torchvision's 256/224 convention: resize the shorter side to ``dst * 8 // 7`` (the
    longer one in proportion, truncated), then centre-crop ``dst`` x ``dst``."""
    hs, ws = _check_src_hw(src_hw, dst)
    short = dst * 8 // 7
    if hs <= ws:
        rh, rw = short, int(short * ws / hs)
    else:
        rh, rw = int(short * hs / ws), short
    if max(rh, rw) > RESIZE_MAX_EXTENT:
        raise ValueError(f"resized frame {rh}x{rw} exceeds {RESIZE_MAX_EXTENT}")
    oy, ox = int(round((rh - dst) / 2)), int(round((rw - dst) / 2))
    return ResizePlan((hs, rh, oy, 0, dst), (ws, rw, ox, 0, dst), 0, (hs, ws), (dst, dst))


SRC_FORMATS = ("rgb", "nv12")


def _check_nv12(src: torch.Tensor, hs: Optional[int] = None) -> Tuple[int, int]:
    """(Hs, Ws) of NV12 frames uint8 [N, Hs * 3 // 2, Ws]; ``hs``: the height they must have."""
    if src.dtype != torch.uint8 or src.dim() != 3:
        raise ValueError(f"NV12 frames are uint8 [N, Hs * 3 / 2, Ws], got {src.dtype} "
                         f"{tuple(src.shape)}")
    rows, ws = int(src.shape[1]), int(src.shape[2])
    if hs is None:
        hs = rows * 2 // 3
    if hs % 2 or ws % 2:
        raise ValueError(f"NV12 needs an even frame height and width, got {hs}x{ws}")
    if rows != hs * 3 // 2:
        raise ValueError(f"NV12 frames of height {hs} have {hs * 3 // 2} rows (Y plane + "
                         f"half-height UV plane), got {rows}")
    return hs, ws


def _check_format(src_format: str) -> None:
    if src_format not in SRC_FORMATS:
        raise ValueError(f"src_format must be one of {SRC_FORMATS}, got {src_format!r}")


def nv12_to_rgb(src: torch.Tensor) -> torch.Tensor:
    """NV12 frames uint8 [N, Hs * 3 // 2, Ws] -> RGB uint8 [N, Hs, Ws, 3]: integer BT.601
    limited range, nearest-neighbour chroma -- the conversion the NV12 kernels apply to every
    source tap (csrc/kernels/nv12.h).  A host-side reference, not a device kernel: GPU
    tensors are converted on the CPU and copied back (the serving path never materialises
    the RGB frame; it reads NV12 through ``src_format="nv12"``)."""
    _check_nv12(src)
    return _ref.nv12_to_rgb(src.cpu()).to(src.device)


def frame_resize(src: torch.Tensor, plan: ResizePlan, out: Optional[torch.Tensor] = None,
                 src_format: str = "rgb") -> torch.Tensor:
    """uint8 frames [N, Hs, Ws, 3] -> [N, Hd, Wd, 3] by ``plan``: bilinear, half-pixel
    centres, no antialias (OpenCV INTER_LINEAR sampling), 11-bit fixed point; every byte of
    ``out`` is written.  GPU (csrc/kernels/frame_resize.hip) and CPU reference are
    bit-identical.  Wd % 4 == 0.
    ``src_format="nv12"``: ``src`` is NV12 [N, Hs * 3 // 2, Ws] (Hs, Ws even) and every source
    tap is converted to RGB before the blend (csrc/kernels/frame_nv12.hip), so the result
    equals ``frame_resize(nv12_to_rgb(src), plan)`` byte for byte -- which is how the CPU
    path computes it."""
    _check_format(src_format)
    nv12 = src_format == "nv12"
    if nv12:
        hs, ws = _check_nv12(src, int(plan.src_hw[0]))
        assert ws == plan.src_hw[1], (src.shape, plan.src_hw)
    else:
        assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3
        assert tuple(src.shape[1:3]) == tuple(plan.src_hw), (src.shape, plan.src_hw)
    hd, wd = plan.dst_hw
    if wd % 4:
        raise ValueError(f"frame_resize needs a destination width % 4 == 0, got {wd}")
    if out is None:
        out = torch.empty(src.shape[0], hd, wd, 3, dtype=torch.uint8, device=src.device)
    assert out.shape == (src.shape[0], hd, wd, 3), (out.shape, plan.dst_hw)
    if src.is_cuda:
        op = _native().frame_resize_nv12 if nv12 else _native().frame_resize
        op(src, out, list(plan.axis_y), list(plan.axis_x), plan.pad)
    else:
        _ref.frame_resize(_ref.nv12_to_rgb(src) if nv12 else src, plan, out)
    return out


def det_to_source(det: torch.Tensor, count: torch.Tensor, plan: ResizePlan) -> torch.Tensor:
    """Kept boxes of :func:`nms` (det fp32 [N, max_det, 6], rows < count[n]) from model
    coordinates to source-frame pixels, in place: x = clamp((x - cx) * sx, 0, Ws),
    y = clamp((y - cy) * sy, 0, Hs).  Score, class and the rows past count are untouched."""
    cy, sy, cx, sx = plan.box_map()
    hs, ws = plan.src_hw
    if det.is_cuda:
        _native().det_to_source(det, count, [cy, sy, cx, sx], hs, ws)
    else:
        _ref.det_to_source(det, count, (cy, sy, cx, sx), hs, ws)
    return det


def roi_crop(src: torch.Tensor, det: torch.Tensor, count: torch.Tensor, k: int, size: int,
             pad: int = 0, out: Optional[torch.Tensor] = None, band: int = 0,
             src_format: str = "rgb") -> torch.Tensor:
    """The top ``k`` boxes of every image as ``size`` x ``size`` uint8 crops
    [N * k, size, size, 3]: crop ``n * k + j`` is the window of box row ``j`` of ``det[n]``
    (fp32 [N, max_det, 6], boxes in ``src`` pixels; :func:`nms` rows are ordered by score) cut
    from ``src`` [N, Hs, Ws, 3] and stretched with :func:`frame_resize`'s fixed-point bilinear.
    The window is clamped to the frame and is at least 1 x 1 for any box, non-finite ones
    included; slots ``j >= count[n]`` are ``pad``; every byte of ``out`` is written.  GPU
    (csrc/kernels/roi_crop.hip) and CPU reference are bit-identical.  ``size % 4 == 0``,
    ``1 <= k <= max_det``.  ``band``: destination rows per workgroup (GPU, 0 = built-in).
    ``src_format="nv12"``: ``src`` is NV12 [N, Hs * 3 // 2, Ws] (Hs, Ws even; boxes in its
    Hs x Ws pixels) and the result equals ``roi_crop(nv12_to_rgb(src), ...)`` byte for byte
    (csrc/kernels/frame_nv12.hip; the CPU path computes exactly that composition)."""
    _check_format(src_format)
    nv12 = src_format == "nv12"
    if nv12:
        _check_nv12(src)
    else:
        assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3
    n = src.shape[0]
    if size % 4:
        raise ValueError(f"roi_crop needs a crop size % 4 == 0, got {size}")
    if not 1 <= size <= RESIZE_MAX_EXTENT:
        raise ValueError(f"crop size {size} outside 1..{RESIZE_MAX_EXTENT}")
    if det.dim() != 3 or det.shape[0] != n or det.shape[2] != 6:
        raise ValueError(f"det must be [N, max_det, 6] for N = {n}, got {tuple(det.shape)}")
    if not 1 <= k <= det.shape[1]:
        raise ValueError(f"roi_crop needs 1 <= k <= max_det = {det.shape[1]}, got {k}")
    if not 0 <= pad <= 255:
        raise ValueError(f"pad {pad} outside 0..255")
    if out is None:
        out = empty(n * k, size, size, 3, dtype=torch.uint8, device=src.device)
    assert out.shape == (n * k, size, size, 3), (out.shape, (n * k, size, size, 3))
    if src.is_cuda:
        nat = _native()
        if band:
            (nat.roi_crop_nv12_band if nv12 else nat.roi_crop_band)(src, det, count, out, pad,
                                                                     band)
        else:
            (nat.roi_crop_nv12 if nv12 else nat.roi_crop)(src, det, count, out, pad)
    else:
        _ref.roi_crop(_ref.nv12_to_rgb(src) if nv12 else src, det, count, k, size, pad, out)
    return out


def frame_resize_nv12(src: torch.Tensor, plan: ResizePlan,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`frame_resize` of NV12 frames [N, Hs * 3 // 2, Ws]."""
    return frame_resize(src, plan, out=out, src_format="nv12")


def roi_crop_nv12(src: torch.Tensor, det: torch.Tensor, count: torch.Tensor, k: int, size: int,
                  pad: int = 0, out: Optional[torch.Tensor] = None, band: int = 0) -> torch.Tensor:
    """:func:`roi_crop` from NV12 frames [N, Hs * 3 // 2, Ws]."""
    return roi_crop(src, det, count, k, size, pad=pad, out=out, band=band, src_format="nv12")


# ---------------------------------------------------------------------------
# multi-object tracking: detections -> stable ids across frames
# ---------------------------------------------------------------------------
TRACK_MAX_TRACKS = (64, 128, 192, 256)  # slots per stream: 1..4 per lane of one wavefront
TRACK_MAX_DET = 300
TRACK_FIELDS = ("box", "vel", "cls", "id", "age", "hits", "next_id", "dropped")


class TrackState:
    """Tracker state of ``streams`` cameras with ``max_tracks`` slots each, one int32 buffer
    ``buf`` [streams, 12 * max_tracks + 4] (the layout csrc/kernels/track.hip reads:
    box | vel | cls | id | age | hits | next_id, dropped, 0, 0) and named views into it:
    ``box`` / ``vel`` [S, T, 4] (quarter pixels; per frame), ``cls`` / ``id`` / ``age`` /
    ``hits`` [S, T] (id -1 = not confirmed, hits 0 = free slot), ``next_id`` / ``dropped``
    [S] (ids handed out so far = distinct confirmed objects; detections that found no slot)."""

    def __init__(self, streams: int, max_tracks: int = 64, device="cpu"):
        if max_tracks not in TRACK_MAX_TRACKS:
            raise ValueError(f"max_tracks must be one of {TRACK_MAX_TRACKS}, got {max_tracks}")
        if streams < 1:
            raise ValueError(f"streams must be >= 1, got {streams}")
        self.streams, self.max_tracks = int(streams), int(max_tracks)
        T = self.max_tracks
        self.buf = torch.zeros(self.streams, 12 * T + 4, dtype=torch.int32, device=device)
        self.box = self.buf[:, :4 * T].unflatten(1, (T, 4))
        self.vel = self.buf[:, 4 * T:8 * T].unflatten(1, (T, 4))
        self.cls = self.buf[:, 8 * T:9 * T]
        self.id = self.buf[:, 9 * T:10 * T]
        self.age = self.buf[:, 10 * T:11 * T]
        self.hits = self.buf[:, 11 * T:12 * T]
        self.next_id = self.buf[:, 12 * T]
        self.dropped = self.buf[:, 12 * T + 1]
        self.reset()

    @property
    def device(self) -> torch.device:
        return self.buf.device

    def reset(self) -> "TrackState":
        """Forget every track and restart the ids at 0 (device ops on the current stream)."""
        self.buf.zero_()
        self.id.fill_(-1)
        return self

    def active(self) -> int:
        """Live tracks over all streams, tentative ones included (syncs with the device)."""
        return int((self.hits > 0).sum())

    def unique(self) -> int:
        """Distinct confirmed objects so far over all streams (syncs with the device)."""
        return int(self.next_id.sum())


def track_thr_q(iou: float) -> int:
    """The IoU gate in 1/1024: floor(iou * 1024 + 0.5) (0.3 -> 307)."""
    import math

    return int(math.floor(float(iou) * 1024 + 0.5))


def track_update(det: torch.Tensor, count: torch.Tensor, state: TrackState, slot0: int = 0,
                 iou: float = 0.3, max_age: int = 30, min_hits: int = 3,
                 class_aware: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One tracker step: batch row n of ``det`` fp32 [N, max_det, 6] / ``count`` int32 [N]
    (:func:`nms` output, in any pixel frame that stays the same from step to step) is the next
    frame of stream ``slot0 + n`` of ``state``.  Returns ``track_id`` int32 [N, max_det]: the
    id of the track each row continues or starts, -1 while the track is not confirmed
    (fewer than ``min_hits`` consecutive matches), when no slot was free, and for rows
    >= count[n].  A track coasts on its last velocity for up to ``max_age`` missed frames.
    ``iou``: the association gate; ``class_aware``: a detection only continues a track of its
    class.  Integer arithmetic on quarter-pixel boxes: GPU (csrc/kernels/track.hip) and CPU
    (ops.reference.track_update, where the rules are written out) are bit-identical.  Streams
    outside [slot0, slot0 + N) are not touched."""
    if not isinstance(state, TrackState):
        raise TypeError(f"state must be an ops.TrackState, got {type(state).__name__}")
    if det.dtype != torch.float32 or det.dim() != 3 or det.shape[2] != 6:
        raise ValueError(f"det must be fp32 [N, max_det, 6], got {det.dtype} {tuple(det.shape)}")
    n, max_det = int(det.shape[0]), int(det.shape[1])
    if count.dtype != torch.int32 or tuple(count.shape) != (n,):
        raise ValueError(f"count must be int32 [{n}], got {count.dtype} {tuple(count.shape)}")
    if not det.is_contiguous() or not count.is_contiguous():
        raise ValueError("det and count must be contiguous")
    if det.device != state.device or count.device != state.device:
        raise ValueError(f"det / count on {det.device} / {count.device}, state on {state.device}")
    if not 1 <= max_det <= TRACK_MAX_DET:
        raise ValueError(f"track_update needs 1 <= max_det <= {TRACK_MAX_DET}, got {max_det}")
    slot0 = int(slot0)
    if slot0 < 0 or slot0 + n > state.streams:
        raise ValueError(f"streams [{slot0}, {slot0 + n}) outside the state's {state.streams}")
    if not 0 <= int(max_age) <= 255:
        raise ValueError(f"max_age {max_age} outside 0..255")
    if not 1 <= int(min_hits) <= 255:
        raise ValueError(f"min_hits {min_hits} outside 1..255")
    thr_q = track_thr_q(iou)
    if not 1 <= thr_q <= 1024:
        raise ValueError(f"iou {iou} gives a threshold of {thr_q}/1024, outside 1..1024")
    if out is None:
        out = empty(n, max_det, dtype=torch.int32, device=det.device)
    if (out.dtype != torch.int32 or tuple(out.shape) != (n, max_det) or not out.is_contiguous()
            or out.device != det.device):
        raise ValueError(f"out must be contiguous int32 [{n}, {max_det}] on {det.device}")
    if det.is_cuda:
        _native().track_update(det, count, state.buf, out, slot0, thr_q, int(max_age),
                               int(min_hits), bool(class_aware))
    else:
        _ref.track_update(det, count, state, slot0, thr_q, int(max_age), int(min_hits),
                          bool(class_aware), out)
    return out


# ---------------------------------------------------------------------------
# lines and zones: stable ids -> crossings, occupancy, dwell
# ---------------------------------------------------------------------------
ZONE_MAX_LINES = 8
ZONE_MAX_ZONES = 8
ZONE_MAX_VERTICES = 8
ZONE_COUNTERS = ("line_fwd", "line_back", "zone_enter", "zone_exit", "zone_occ", "zone_dwell")
ZONE_TABLE_STRIDE = 188
ZONE_ANCHORS = {"bottom": 0, "centre": 1, "center": 1, 0: 0, 1: 1}


def _zone_q(xy) -> list:
    """A pixel point (x, y) -> the tracker's quarter pixels (reference.track_quantize)."""
    if len(xy) != 2:
        raise ValueError(f"a point is (x, y), got {xy!r}")
    return _ref.track_quantize(torch.tensor([float(xy[0]), float(xy[1])])).tolist()


class ZoneSet:
    """The virtual lines and polygon zones of ``streams`` cameras: one int32 table ``table``
    [streams, 188] on ``device`` (the layout csrc/kernels/zones.hip reads) and named views into
    it: ``line`` [S, 8, 4] (ax, ay, bx, by), ``line_cls`` [S, 8], ``vertex`` [S, 8, 8, 2],
    ``n_vertex`` [S, 8], ``zone_cls`` [S, 8] (-1 = any class), ``n_lines`` / ``n_zones`` /
    ``anchor`` [S].  Coordinates are given in pixels and stored in the tracker's quarter
    pixels.  An index that was never set holds a line with A == B or a zone without vertices:
    neither ever counts."""

    def __init__(self, streams: int, device="cpu"):
        if streams < 1:
            raise ValueError(f"streams must be >= 1, got {streams}")
        self.streams = int(streams)
        self._host = torch.zeros(self.streams, ZONE_TABLE_STRIDE, dtype=torch.int32)
        self.table = self._host if torch.device(device).type == "cpu" else self._host.to(device)
        for name, v in self._views(self.table).items():
            setattr(self, name, v)
        self.clear()

    @staticmethod
    def _views(tab: torch.Tensor) -> dict:
        return {"line": tab[:, 0:32].unflatten(1, (8, 4)), "line_cls": tab[:, 32:40],
                "vertex": tab[:, 40:168].unflatten(1, (8, 8, 2)), "n_vertex": tab[:, 168:176],
                "zone_cls": tab[:, 176:184], "n_lines": tab[:, 184], "n_zones": tab[:, 185],
                "anchor": tab[:, 186]}

    @property
    def device(self) -> torch.device:
        return self.table.device

    def _push(self) -> None:
        if self.table is not self._host:
            self.table.copy_(self._host)

    def _rows(self, camera):
        if camera is None:
            return slice(None)
        if not 0 <= int(camera) < self.streams:
            raise ValueError(f"camera {camera} outside 0..{self.streams - 1}")
        return slice(int(camera), int(camera) + 1)

    def clear(self) -> "ZoneSet":
        """Drop every line and zone (the anchor mode stays)."""
        anchor = self._host[:, 186].clone()
        self._host.zero_()
        h = self._views(self._host)
        h["line_cls"].fill_(-1)
        h["zone_cls"].fill_(-1)
        h["anchor"].copy_(anchor)
        self._push()
        return self

    def set_anchor(self, anchor) -> "ZoneSet":
        """``"bottom"`` (0: bottom-centre of the box, feet on the ground plane) or
        ``"centre"`` (1)."""
        if anchor not in ZONE_ANCHORS:
            raise ValueError(f"anchor must be 'bottom' or 'centre', got {anchor!r}")
        self._host[:, 186] = ZONE_ANCHORS[anchor]
        self._push()
        return self

    def set_line(self, camera, index: int, a, b, cls: int = -1) -> "ZoneSet":
        """Line ``index`` of ``camera`` (None: of every camera) from pixel point ``a`` to
        ``b``.  With side(P) = cross(b - a, P - a) >= 0, a move from side true to side false
        is "forward", the other way "backward".  ``cls``: only tracks of that class count
        (-1: any)."""
        if not 0 <= int(index) < ZONE_MAX_LINES:
            raise ValueError(f"line index {index} outside 0..{ZONE_MAX_LINES - 1}")
        if not -1 <= int(cls) <= 65535:
            raise ValueError(f"class {cls} outside -1..65535")
        rows, h = self._rows(camera), self._views(self._host)
        h["line"][rows, index] = torch.tensor(_zone_q(a) + _zone_q(b), dtype=torch.int32)
        h["line_cls"][rows, index] = int(cls)
        h["n_lines"][rows] = h["n_lines"][rows].clamp_min(int(index) + 1)
        self._push()
        return self

    def set_zone(self, camera, index: int, polygon, cls: int = -1) -> "ZoneSet":
        """Zone ``index`` of ``camera`` (None: of every camera): a polygon of 3..8 pixel
        vertices, convex or not.  ``cls``: only that class counts (-1: any)."""
        if not 0 <= int(index) < ZONE_MAX_ZONES:
            raise ValueError(f"zone index {index} outside 0..{ZONE_MAX_ZONES - 1}")
        polygon = list(polygon)
        if not 3 <= len(polygon) <= ZONE_MAX_VERTICES:
            raise ValueError(f"a zone has 3..{ZONE_MAX_VERTICES} vertices, got {len(polygon)}")
        if not -1 <= int(cls) <= 65535:
            raise ValueError(f"class {cls} outside -1..65535")
        rows, h = self._rows(camera), self._views(self._host)
        v = torch.zeros(ZONE_MAX_VERTICES, 2, dtype=torch.int32)
        v[:len(polygon)] = torch.tensor([_zone_q(p) for p in polygon], dtype=torch.int32)
        h["vertex"][rows, index] = v
        h["n_vertex"][rows, index] = len(polygon)
        h["zone_cls"][rows, index] = int(cls)
        h["n_zones"][rows] = h["n_zones"][rows].clamp_min(int(index) + 1)
        self._push()
        return self


class ZoneState:
    """Line / zone state of ``streams`` cameras over a tracker of ``max_tracks`` slots: one
    int32 buffer ``buf`` [streams, 4 * max_tracks + 48] (the layout csrc/kernels/zones.hip
    reads) and named views: ``entry`` [S, T, 4] = ``seen_id`` (-1 = none), ``anchor`` [S, T, 2]
    (quarter pixels at the last sighting), ``zmask``; ``counters`` [S, 48] = ``line_fwd``
    ``line_back`` ``zone_enter`` ``zone_exit`` ``zone_occ`` ``zone_dwell`` [S, 8] each,
    cumulative and wrapping modulo 2^32 (``zone_occ``: the current value)."""

    def __init__(self, streams: int, max_tracks: int = 64, device="cpu"):
        if max_tracks not in TRACK_MAX_TRACKS:
            raise ValueError(f"max_tracks must be one of {TRACK_MAX_TRACKS}, got {max_tracks}")
        if streams < 1:
            raise ValueError(f"streams must be >= 1, got {streams}")
        self.streams, self.max_tracks = int(streams), int(max_tracks)
        T = self.max_tracks
        self.buf = torch.zeros(self.streams, 4 * T + 48, dtype=torch.int32, device=device)
        self.entry = self.buf[:, :4 * T].unflatten(1, (T, 4))
        self.seen_id = self.entry[..., 0]
        self.anchor = self.entry[..., 1:3]
        self.zmask = self.entry[..., 3]
        self.counters = self.buf[:, 4 * T:]
        for i, name in enumerate(ZONE_COUNTERS):
            setattr(self, name, self.counters[:, 8 * i:8 * i + 8])
        self.reset()

    @property
    def device(self) -> torch.device:
        return self.buf.device

    def reset(self) -> "ZoneState":
        """Forget every entry and zero the counters (device ops on the current stream)."""
        self.buf.zero_()
        self.seen_id.fill_(-1)
        return self


def zone_update(det: torch.Tensor, count: torch.Tensor, track_state: TrackState,
                zone_state: ZoneState, zones: ZoneSet, slot0: int = 0,
                out_mask: Optional[torch.Tensor] = None,
                out_counts: Optional[torch.Tensor] = None):
    """One line / zone step, after the same step's :func:`track_update` on the same ``det`` /
    ``count`` / ``track_state`` (which is only read).  Updates the counters of streams
    [slot0, slot0 + N) in ``zone_state`` -- line crossings by direction, zone entries, exits,
    occupancy, dwell frames -- and returns ``(zone_mask, zone_counts)``: int32 [N, max_det],
    bit z set when the anchor of the row's box lies in zone z (rows >= count[n]: 0), and int32
    [N, 48], the stream's counters after the step in the order of ``ZONE_COUNTERS``.  Integer
    arithmetic on quarter pixels: GPU (csrc/kernels/zones.hip) and CPU
    (ops.reference.zone_update, where the rules are written out) are bit-identical."""
    if not isinstance(track_state, TrackState):
        raise TypeError(f"track_state must be an ops.TrackState, got {type(track_state).__name__}")
    if not isinstance(zone_state, ZoneState):
        raise TypeError(f"zone_state must be an ops.ZoneState, got {type(zone_state).__name__}")
    if not isinstance(zones, ZoneSet):
        raise TypeError(f"zones must be an ops.ZoneSet, got {type(zones).__name__}")
    if det.dtype != torch.float32 or det.dim() != 3 or det.shape[2] != 6:
        raise ValueError(f"det must be fp32 [N, max_det, 6], got {det.dtype} {tuple(det.shape)}")
    n, max_det = int(det.shape[0]), int(det.shape[1])
    if count.dtype != torch.int32 or tuple(count.shape) != (n,):
        raise ValueError(f"count must be int32 [{n}], got {count.dtype} {tuple(count.shape)}")
    if not det.is_contiguous() or not count.is_contiguous():
        raise ValueError("det and count must be contiguous")
    for name, dev in (("count", count.device), ("track_state", track_state.device),
                      ("zone_state", zone_state.device), ("zones", zones.device)):
        if dev != det.device:
            raise ValueError(f"det on {det.device}, {name} on {dev}")
    if not 1 <= max_det <= TRACK_MAX_DET:
        raise ValueError(f"zone_update needs 1 <= max_det <= {TRACK_MAX_DET}, got {max_det}")
    if (zone_state.streams, zone_state.max_tracks) != (track_state.streams,
                                                       track_state.max_tracks):
        raise ValueError("zone_state and track_state differ in streams or max_tracks")
    if zones.streams != track_state.streams:
        raise ValueError(f"zones cover {zones.streams} streams, the state {track_state.streams}")
    slot0 = int(slot0)
    if slot0 < 0 or slot0 + n > track_state.streams:
        raise ValueError(f"streams [{slot0}, {slot0 + n}) outside the state's "
                         f"{track_state.streams}")
    if out_mask is None:
        out_mask = empty(n, max_det, dtype=torch.int32, device=det.device)
    if out_counts is None:
        out_counts = empty(n, 48, dtype=torch.int32, device=det.device)
    for name, t, shape in (("out_mask", out_mask, (n, max_det)),
                           ("out_counts", out_counts, (n, 48))):
        if (t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous()
                or t.device != det.device):
            raise ValueError(f"{name} must be contiguous int32 {list(shape)} on {det.device}")
    if det.is_cuda:
        _native().zone_update(det, count, track_state.buf, zone_state.buf, zones.table, out_mask,
                              out_counts, slot0)
    else:
        _ref.zone_update(det, count, track_state, zone_state, zones, slot0, out_mask, out_counts)
    return out_mask, out_counts


# ---------------------------------------------------------------------------
# frame watch: the frames themselves -> motion grid, dark / flat / frozen / scene alarms
# ---------------------------------------------------------------------------
WATCH_CELLS = (8, 16, 32)
WATCH_ROW_STEPS = (1, 2, 4)
WATCH_MAX_BG_SHIFT = 8
WATCH_MAX_EXTENT = 4096
WATCH_CONDITIONS = _ref.WATCH_CONDITIONS
WATCH_PARAMS = _ref.WATCH_PARAMS
WATCH_PARAM_RANGES = _ref.WATCH_PARAM_RANGES
WATCH_STATS = ("mean16", "sharp16", "moving", "cells", "conditions", "alarms")
WATCH_HEADER = 24
# motion 10 luma levels in 1 % of the cells, scene change at half of them, dark below level
# 24, flat below a mean neighbour difference of 1.5 levels, alarms after 8 frames
WATCH_DEFAULTS = {"motion_thr16": 160, "motion_share_q": 10, "scene_share_q": 512,
                  "dark16": 384, "flat16": 24, "hold": 8}


def watch_level16(level: float) -> int:
    """A luma (or gradient) level in 1/16: floor(level * 16 + 0.5)."""
    import math

    return int(math.floor(float(level) * 16 + 0.5))


def watch_share_q(share: float) -> int:
    """A share of the cells in 1/1024: floor(share * 1024 + 0.5)."""
    import math

    return int(math.floor(float(share) * 1024 + 0.5))


def check_watch_params(**params) -> dict:
    """Range-check threshold words by name (``WATCH_PARAMS``) against the ranges the kernel
    clamps them into; returns them as ints."""
    out = {}
    for name, v in params.items():
        if name not in WATCH_PARAMS:
            raise ValueError(f"unknown watch parameter {name!r}; known: {WATCH_PARAMS}")
        lo, hi = WATCH_PARAM_RANGES[WATCH_PARAMS.index(name)]
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"watch parameter {name} = {v!r} outside {lo}..{hi}")
        out[name] = v
    return out


class WatchState:
    """Frame-watch state of ``streams`` cameras of ``frame_hw`` = (Hs, Ws) pixels: one int32
    buffer ``buf`` [streams, 24 + 3 * GH * GW] (the layout csrc/kernels/frame_watch.hip reads),
    GH = ceil(Hs / cell), GW = ceil(Ws / cell), and named views into it: ``primed`` [S],
    ``run`` / ``raised`` [S, 5] (in the order of ``WATCH_CONDITIONS``; ``raised`` wraps modulo
    2^32), ``params`` [S, 6] (``WATCH_PARAMS``: the thresholds the kernel reads every step, so
    :meth:`set_params` takes effect from the next step without recapturing), ``acc`` / ``sum`` /
    ``grad`` [S, GH, GW] (the background accumulator, scaled by 2^bg_shift, and the last
    frame's per-cell sums).  ``cell`` in 8 / 16 / 32, ``row_step`` in 1 / 2 / 4 (every
    row_step-th frame row is read), ``bg_shift`` k in 0..8 (background = acc >> k; 0 = plain
    frame differencing)."""

    def __init__(self, streams: int, frame_hw, cell: int = 16, row_step: int = 1,
                 bg_shift: int = 4, device="cpu"):
        if streams < 1:
            raise ValueError(f"streams must be >= 1, got {streams}")
        hs, ws = int(frame_hw[0]), int(frame_hw[1])
        if not (1 <= hs <= WATCH_MAX_EXTENT and 2 <= ws <= WATCH_MAX_EXTENT):
            raise ValueError(f"frame_watch frames are 1..{WATCH_MAX_EXTENT} x "
                             f"2..{WATCH_MAX_EXTENT}, got {hs}x{ws}")
        if cell not in WATCH_CELLS:
            raise ValueError(f"cell must be one of {WATCH_CELLS}, got {cell}")
        if row_step not in WATCH_ROW_STEPS:
            raise ValueError(f"row_step must be one of {WATCH_ROW_STEPS}, got {row_step}")
        if isinstance(bg_shift, bool) or not 0 <= int(bg_shift) <= WATCH_MAX_BG_SHIFT:
            raise ValueError(f"bg_shift {bg_shift} outside 0..{WATCH_MAX_BG_SHIFT}")
        self.streams, self.frame_hw = int(streams), (hs, ws)
        self.cell, self.row_step, self.bg_shift = int(cell), int(row_step), int(bg_shift)
        self.grid = (-(-hs // self.cell), -(-ws // self.cell))
        C = self.grid[0] * self.grid[1]
        H = WATCH_HEADER
        self.buf = torch.zeros(self.streams, H + 3 * C, dtype=torch.int32, device=device)
        self.primed = self.buf[:, 0]
        self.run = self.buf[:, 1:6]
        self.raised = self.buf[:, 6:11]
        self.params = self.buf[:, 16:22]
        self.acc = self.buf[:, H:H + C].unflatten(1, self.grid)
        self.sum = self.buf[:, H + C:H + 2 * C].unflatten(1, self.grid)
        self.grad = self.buf[:, H + 2 * C:].unflatten(1, self.grid)
        self.set_params(None, **WATCH_DEFAULTS)

    @property
    def device(self) -> torch.device:
        return self.buf.device

    def reset(self) -> "WatchState":
        """Forget the background, the last frame and every counter; the thresholds stay
        (device ops on the current stream)."""
        self.buf[:, :16].zero_()
        self.buf[:, WATCH_HEADER:].zero_()
        return self

    def set_params(self, camera=None, **params) -> "WatchState":
        """Set thresholds of ``camera`` (None: of every camera) by name: ``motion_thr16``
        (1/16 luma, 0..4080), ``motion_share_q`` / ``scene_share_q`` (1/1024 of the cells,
        0..1024), ``dark16`` / ``flat16`` (1/16 luma, 0..4096), ``hold`` (frames, 1..255)."""
        vals = check_watch_params(**params)
        if camera is None:
            rows = slice(None)
        elif not 0 <= int(camera) < self.streams:
            raise ValueError(f"camera {camera} outside 0..{self.streams - 1}")
        else:
            rows = slice(int(camera), int(camera) + 1)
        for name, v in vals.items():
            self.params[rows, WATCH_PARAMS.index(name)] = v
        return self


def frame_watch(src: torch.Tensor, state: WatchState, slot0: int = 0, src_format: str = "rgb",
                out_stats: Optional[torch.Tensor] = None,
                out_mask: Optional[torch.Tensor] = None):
    """One frame-watch step: batch row n of ``src`` -- uint8 RGB [N, Hs, Ws, 3], or NV12
    [N, Hs * 3 // 2, Ws] with ``src_format="nv12"`` (only the luma rows are read) -- is the next
    frame of stream ``slot0 + n`` of ``state``.  Returns ``(stats, motion_mask)``: int32 [N, 16]
    = mean16, sharp16, moving, cells, conditions, alarms, run[5], raised[5] (bits and counters
    in the order of ``WATCH_CONDITIONS``) and uint8 [N, GH, GW], 1 where the cell moved against
    the running background.  Every element of both is written; streams outside
    [slot0, slot0 + N) are not touched.  Integer arithmetic: GPU
    (csrc/kernels/frame_watch.hip) and CPU (ops.reference.frame_watch, where the rules are
    written out) are bit-identical."""
    if not isinstance(state, WatchState):
        raise TypeError(f"state must be an ops.WatchState, got {type(state).__name__}")
    _check_format(src_format)
    if src.dtype != torch.uint8:
        raise ValueError(f"frames must be uint8, got {src.dtype}")
    if src_format == "nv12":
        hw = _check_nv12(src)
    else:
        if src.dim() != 4 or src.shape[3] != 3:
            raise ValueError(f"RGB frames are uint8 [N, Hs, Ws, 3], got {tuple(src.shape)}")
        hw = (int(src.shape[1]), int(src.shape[2]))
    if hw != state.frame_hw:
        raise ValueError(f"frames of {hw[0]}x{hw[1]}, the state was made for "
                         f"{state.frame_hw[0]}x{state.frame_hw[1]}")
    if not src.is_contiguous():
        raise ValueError("frames must be contiguous")
    if src.device != state.device:
        raise ValueError(f"frames on {src.device}, state on {state.device}")
    n = int(src.shape[0])
    slot0 = int(slot0)
    if slot0 < 0 or slot0 + n > state.streams:
        raise ValueError(f"streams [{slot0}, {slot0 + n}) outside the state's {state.streams}")
    if out_stats is None:
        out_stats = empty(n, 16, dtype=torch.int32, device=src.device)
    if out_mask is None:
        out_mask = empty(n, *state.grid, dtype=torch.uint8, device=src.device)
    for name, t, dt, shape in (("out_stats", out_stats, torch.int32, (n, 16)),
                               ("out_mask", out_mask, torch.uint8, (n, *state.grid))):
        if (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()
                or t.device != src.device):
            raise ValueError(f"{name} must be contiguous {dt} {list(shape)} on {src.device}")
    if src.is_cuda:
        _native().frame_watch(src, state.buf, out_stats, out_mask, slot0, src_format == "nv12",
                              state.cell, state.row_step, state.bg_shift)
    else:
        _ref.frame_watch(src, state, slot0, src_format, out_stats, out_mask)
    return out_stats, out_mask


# ---------------------------------------------------------------------------
# camera snapshots: baseline JPEG files of frames that are already on the device
# ---------------------------------------------------------------------------
JPEG_SUBSAMPLINGS = _ref.JPEG_SUBSAMPLINGS
JPEG_MAX_EXTENT = 8192
JPEG_HEADER_BYTES = _ref.JPEG_HEADER_BYTES
JPEG_BLOCK_BYTES = 416


def jpeg_max_bytes(hw, subsampling: str = "420") -> int:
    """Worst-case size of a file of :func:`jpeg_encode`, derived and not measured.

    One 8 x 8 block: the DC difference is a Huffman code of at most 11 bits (the longest DC code
    of the Annex K tables, chrominance category 11) and at most 11 magnitude bits; each of the
    63 AC coefficients costs at most a 16-bit code and 10 magnitude bits.  A ZRL (at most 16
    bits) stands for 16 zero coefficients and an EOB for at least one, so neither can exceed the
    26 bits per coefficient already counted: 22 + 63 * 26 = 1660 bits, 207.5 bytes.  An
    interval of nb blocks is therefore at most nb * 208 bytes after its last byte is padded with
    1-bits, and every one of them may be an FF that is stuffed: nb * 416.  Per interval one
    more byte is allowed for the padding (it is already inside the bound above whenever
    nb * 1660 is no multiple of 8; kept so that the bound does not rest on that) and 2 bytes for
    the RSTn marker (the last interval has none); the header and the 2-byte EOI are added once."""
    _, mh, mw, bpm = _ref.jpeg_geometry(hw, subsampling)
    return JPEG_HEADER_BYTES + mh * (mw * bpm * JPEG_BLOCK_BYTES + 1 + 2) + 2


def thumbnail_plan(src_hw, width: int) -> ResizePlan:
    """Full-frame stretch of ``src_hw`` = (Hs, Ws) frames to ``width`` x round(width * Hs / Ws),
    both rounded up to a multiple of 4 (:func:`frame_resize` needs Wd % 4 == 0); no padding."""
    width = int(width)
    hs, ws = _check_src_hw(src_hw, max(width, 1))
    if width < 1:
        raise ValueError(f"thumbnail width {width} must be >= 1")
    wd = -(-width // 4) * 4
    hd = -(-max(1, int(round(width * hs / ws))) // 4) * 4
    if max(wd, hd) > RESIZE_MAX_EXTENT:
        raise ValueError(f"thumbnail {hd}x{wd} exceeds {RESIZE_MAX_EXTENT}")
    return ResizePlan((hs, hd, 0, 0, hd), (ws, wd, 0, 0, wd), 0, (hs, ws), (hd, wd))


class JpegEncoder:
    """Everything :func:`jpeg_encode` needs outside the caller's tensors, for up to
    ``max_images`` images of ``hw`` = (H, W) pixels per call, all in device memory:
    ``qtab`` int32 [2, 64] (luminance / chrominance quantisers, natural order), ``huff`` int32
    [4, 256] (code | length << 16 of the four Annex K tables), ``header`` uint8 [611] (SOI, DQT
    x2, SOF0, DHT x4, DRI, SOS) and the workspaces ``coef`` int16 [max_images, intervals,
    blocks, 64], ``scratch`` uint8 [max_images, intervals, blocks * 416 + 16] and ``seglen``
    int32 [max_images, intervals] (one restart interval per MCU row).  The kernels read the
    tables and the header at run time, so :meth:`set_quality` takes effect from the next call
    -- or the next replay of a captured step -- without recapturing."""

    def __init__(self, hw, max_images: int, subsampling: str = "420", quality: int = 75,
                 device="cpu"):
        self.mcu, self.intervals, mw, bpm = _ref.jpeg_geometry(hw, subsampling)
        if isinstance(max_images, bool) or int(max_images) < 1:
            raise ValueError(f"max_images must be >= 1, got {max_images!r}")
        self.hw = (int(hw[0]), int(hw[1]))
        self.max_images, self.subsampling = int(max_images), subsampling
        self.blocks = mw * bpm
        self.max_bytes = jpeg_max_bytes(self.hw, subsampling)
        if self.max_bytes > 2 ** 31 - 1:
            raise ValueError(f"a {self.hw[0]}x{self.hw[1]} image can exceed 2 GiB as a file")
        dev = torch.device(device)
        self.qtab = torch.zeros(2, 64, dtype=torch.int32, device=dev)
        self.huff = torch.from_numpy(_ref.jpeg_huff_codes()).to(dev)
        self.header = torch.zeros(JPEG_HEADER_BYTES, dtype=torch.uint8, device=dev)
        self.quality = None
        self.set_quality(quality)
        M, I, B = self.max_images, self.intervals, self.blocks
        if dev.type == "cuda":
            self.coef = torch.empty(M, I, B, 64, dtype=torch.int16, device=dev)
            self.scratch = torch.empty(M, I, B * JPEG_BLOCK_BYTES + 16, dtype=torch.uint8,
                                       device=dev)
            self.seglen = torch.empty(M, I, dtype=torch.int32, device=dev)
        else:
            self.coef = self.scratch = self.seglen = None  # the reference needs none

    @property
    def device(self) -> torch.device:
        return self.qtab.device

    def set_quality(self, quality: int) -> "JpegEncoder":
        """Rewrite the two quantisation tables and the header's DQT bytes for ``quality`` in
        1..100 (copies into the existing device tensors on the current stream)."""
        q = _ref.jpeg_quant_tables(quality)
        head = torch.frombuffer(bytearray(_ref.jpeg_header(self.hw, self.subsampling, q)),
                                dtype=torch.uint8)
        if self.quality is None:
            self.header.copy_(head)
        else:
            for o in _ref.JPEG_DQT_OFFSETS:
                self.header[o:o + 64].copy_(head[o:o + 64])
        self.qtab.copy_(torch.from_numpy(q))
        self.quality = int(quality)
        return self


def jpeg_encode(images: torch.Tensor, enc: JpegEncoder, out: Optional[torch.Tensor] = None,
                lengths: Optional[torch.Tensor] = None, slot0: int = 0):
    """Baseline JPEG files of ``images`` uint8 [M, H, W, 3] RGB (contiguous, (H, W) == enc.hw,
    M <= enc.max_images).  Returns ``(buf, length)``: ``buf`` uint8 [rows >= M, cap] is ``out``
    or a new [M, jpeg_max_bytes] tensor, ``length`` int32 [rows] is ``lengths`` or new;
    ``buf[m, :length[m]]`` is file m, complete and openable by any decoder (no JFIF segment).
    A file that does not fit ``cap`` gives ``length[m] = -needed`` and leaves row m alone.
    Bytes past a file and the rows past M are left as they were.  Three launches on the
    current stream, no host synchronisation, capturable (csrc/kernels/jpeg_encode.hip); GPU
    and CPU (ops.reference.jpeg_encode, where the format is written out) agree byte for
    byte.  ``slot0``: image m works in rows ``slot0 + m`` of the encoder's workspaces
    (slot0 + M <= enc.max_images), so calls on different streams may overlap when their rows
    are disjoint -- the engine's batch slices."""
    if not isinstance(enc, JpegEncoder):
        raise TypeError(f"enc must be an ops.JpegEncoder, got {type(enc).__name__}")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError(f"images are uint8 [M, H, W, 3], got {images.dtype} "
                         f"{tuple(images.shape)}")
    if tuple(images.shape[1:3]) != enc.hw:
        raise ValueError(f"images of {images.shape[1]}x{images.shape[2]}, the encoder was made "
                         f"for {enc.hw[0]}x{enc.hw[1]}")
    m, slot0 = int(images.shape[0]), int(slot0)
    if slot0 < 0 or slot0 + m > enc.max_images:
        raise ValueError(f"images [{slot0}, {slot0 + m}) outside the {enc.max_images} the "
                         f"encoder was made for")
    if not images.is_contiguous():
        raise ValueError("images must be contiguous")
    if images.device != enc.device:
        raise ValueError(f"images on {images.device}, encoder on {enc.device}")
    if out is None:
        out = empty(m, enc.max_bytes, dtype=torch.uint8, device=images.device)
    if lengths is None:
        lengths = empty(int(out.shape[0]) if out.dim() == 2 else m, dtype=torch.int32,
                        device=images.device)
    if (out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] < m or out.shape[1] < 1
            or not out.is_contiguous() or out.device != images.device):
        raise ValueError(f"out must be contiguous uint8 [>= {m}, cap] on {images.device}")
    if (lengths.dtype != torch.int32 or lengths.dim() != 1 or lengths.shape[0] < m
            or not lengths.is_contiguous() or lengths.device != images.device):
        raise ValueError(f"lengths must be contiguous int32 [>= {m}] on {images.device}")
    if images.is_cuda:
        rows = slice(slot0, slot0 + m)
        _native().jpeg_encode(images, enc.qtab, enc.huff, enc.header, enc.coef[rows],
                              enc.scratch[rows], enc.seglen[rows], out, lengths,
                              enc.subsampling == "420")
    else:
        files = _ref.jpeg_encode(images, enc.subsampling, qtabs=enc.qtab.numpy(),
                                 header=bytes(enc.header.tolist()))
        cap = int(out.shape[1])
        for i, f in enumerate(files):
            if len(f) > cap:
                lengths[i] = -len(f)
            else:
                out[i, :len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8)
                lengths[i] = len(f)
    return out, lengths


# ---------------------------------------------------------------------------
# snapshot annotation: boxes, labels and a privacy mosaic drawn into the thumbnails
# ---------------------------------------------------------------------------
ANNOTATE_TABLE_STRIDE = _ref.ANN_TABLE_STRIDE
ANNOTATE_MAX_CLASSES = ANNOTATE_MAX_POLYGONS = ANNOTATE_MAX_VERTICES = _ref.ANN_MAX
ANNOTATE_LABELS = {"none": 0, "class": 1, "id": 2, "both": 3}
ANNOTATE_COLOUR_BY = {"class": 0, "track": 1}
ANNOTATE_BLOCKS = (4, 8, 16)
ANNOTATE_MAX_SRC = _ref.ANN_MAX_SRC
# sixteen colours that stay apart on a thumbnail, (R, G, B)
ANNOTATE_PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200),
                    (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
                    (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255),
                    (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195))


class AnnotateStyle:
    """How the snapshots of ``streams`` cameras are drawn: one int32 table ``table``
    [streams, 168] on ``device`` (the layout csrc/kernels/annotate.hip reads), its host mirror
    ``host`` and named views: ``boxes`` ``labels`` ``colour_by`` ``thickness`` ``scale``
    ``block`` ``max_draw`` ``n_polygons`` [S], ``privacy_classes`` [S, 8] (-1 = unused),
    ``n_vertex`` [S, 8], ``vertex`` [S, 8, 8, 2] (given in pixels of the frame the boxes live
    in, stored in the tracker's quarter pixels) and ``palette`` [S, 16] (R | G << 8 | B << 16);
    plus one font table ``font`` int32 [88] for all of them (5 x 7 glyphs of ``0-9`` and ``:``).
    ``camera=None`` in a setter means every camera.  The kernel reads the tables at run time:
    a setter takes effect from the next call, or the next replay of a captured step."""

    def __init__(self, streams: int, device="cpu"):
        if isinstance(streams, bool) or int(streams) < 1:
            raise ValueError(f"streams must be >= 1, got {streams!r}")
        self.streams = int(streams)
        dev = torch.device(device)
        self.host = torch.zeros(self.streams, ANNOTATE_TABLE_STRIDE, dtype=torch.int32)
        self.font_host = torch.from_numpy(_ref.annotate_font())
        self.table = self.host if dev.type == "cpu" else self.host.to(dev)
        self.font = self.font_host if dev.type == "cpu" else self.font_host.to(dev)
        for name, v in self._views(self.table).items():
            setattr(self, name, v)
        h = self._views(self.host)
        h["boxes"].fill_(1)
        h["labels"].fill_(ANNOTATE_LABELS["both"])
        h["thickness"].fill_(1)
        h["scale"].fill_(1)
        h["block"].fill_(8)
        h["max_draw"].fill_(32)
        h["privacy_classes"].fill_(-1)
        h["palette"].copy_(torch.tensor([r | g << 8 | b << 16 for r, g, b in ANNOTATE_PALETTE],
                                        dtype=torch.int32))
        self._push()

    @staticmethod
    def _views(tab: torch.Tensor) -> dict:
        r = _ref
        return {"boxes": tab[:, r.ANN_BOXES], "labels": tab[:, r.ANN_LABELS],
                "colour_by": tab[:, r.ANN_COLOUR_BY], "thickness": tab[:, r.ANN_THICKNESS],
                "scale": tab[:, r.ANN_SCALE], "block": tab[:, r.ANN_BLOCK],
                "max_draw": tab[:, r.ANN_MAX_DRAW], "n_polygons": tab[:, r.ANN_N_POLY],
                "privacy_classes": tab[:, r.ANN_PRIV_CLS:r.ANN_PRIV_CLS + 8],
                "n_vertex": tab[:, r.ANN_N_VERT:r.ANN_N_VERT + 8],
                "vertex": tab[:, r.ANN_VERT:r.ANN_VERT + 128].unflatten(1, (8, 8, 2)),
                "palette": tab[:, r.ANN_PALETTE:r.ANN_PALETTE + 16]}

    @property
    def device(self) -> torch.device:
        return self.table.device

    def _push(self) -> None:
        if self.table is not self.host:
            self.table.copy_(self.host)

    def _rows(self, camera):
        if camera is None:
            return slice(None)
        if isinstance(camera, bool) or not 0 <= int(camera) < self.streams:
            raise ValueError(f"camera {camera} outside 0..{self.streams - 1}")
        return slice(int(camera), int(camera) + 1)

    def _set(self, camera, name: str, value) -> "AnnotateStyle":
        self._views(self.host)[name][self._rows(camera)] = value
        self._push()
        return self

    def set_boxes(self, on: bool, camera=None) -> "AnnotateStyle":
        """Draw the outlines of the first ``max_draw`` boxes, or not."""
        return self._set(camera, "boxes", 1 if on else 0)

    def set_labels(self, parts: str, camera=None) -> "AnnotateStyle":
        """``"class"``, ``"id"``, ``"both"`` (``cls:id``) or ``"none"``."""
        if parts not in ANNOTATE_LABELS:
            raise ValueError(f"labels must be one of {tuple(ANNOTATE_LABELS)}, got {parts!r}")
        return self._set(camera, "labels", ANNOTATE_LABELS[parts])

    def set_colour_by(self, key: str, camera=None) -> "AnnotateStyle":
        """Box colour from the ``"class"`` or from the ``"track"`` id (rows without an id fall
        back to the class)."""
        if key not in ANNOTATE_COLOUR_BY:
            raise ValueError(f"colour_by must be 'class' or 'track', got {key!r}")
        return self._set(camera, "colour_by", ANNOTATE_COLOUR_BY[key])

    @staticmethod
    def _int(name: str, v, lo: int, hi: int) -> int:
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
        return int(v)

    def set_thickness(self, t: int, camera=None) -> "AnnotateStyle":
        """Outline thickness in thumbnail pixels, 1..4."""
        return self._set(camera, "thickness", self._int("thickness", t, 1, 4))

    def set_label_scale(self, s: int, camera=None) -> "AnnotateStyle":
        """Glyph scale 1..2: cells of 6 x 8 or 12 x 16 pixels."""
        return self._set(camera, "scale", self._int("label scale", s, 1, 2))

    def set_privacy_block(self, block: int, camera=None) -> "AnnotateStyle":
        """Mosaic block side in thumbnail pixels: 4, 8 or 16."""
        if isinstance(block, bool) or block not in ANNOTATE_BLOCKS:
            raise ValueError(f"privacy block must be one of {ANNOTATE_BLOCKS}, got {block!r}")
        return self._set(camera, "block", int(block))

    def set_max_draw(self, rows: int, camera=None) -> "AnnotateStyle":
        """Only the first ``rows`` boxes get an outline or a label (privacy covers all)."""
        return self._set(camera, "max_draw", self._int("max_draw", rows, 0, TRACK_MAX_DET))

    def set_privacy_classes(self, classes, camera=None) -> "AnnotateStyle":
        """Up to 8 class ids whose boxes are pixelated (an empty list: none)."""
        classes = [self._int("privacy class", c, 0, 65535) for c in classes]
        if len(classes) > ANNOTATE_MAX_CLASSES:
            raise ValueError(f"at most {ANNOTATE_MAX_CLASSES} privacy classes, got "
                             f"{len(classes)}")
        row = torch.full((ANNOTATE_MAX_CLASSES,), -1, dtype=torch.int32)
        row[:len(classes)] = torch.tensor(classes, dtype=torch.int32)
        return self._set(camera, "privacy_classes", row)

    def set_privacy_polygon(self, index: int, polygon, camera=None) -> "AnnotateStyle":
        """Privacy polygon ``index`` (0..7): 3..8 pixel vertices, convex or not, in the frame
        the boxes live in; every mosaic block with a pixel centre inside is pixelated."""
        index = self._int("polygon index", index, 0, ANNOTATE_MAX_POLYGONS - 1)
        polygon = list(polygon)
        if not 3 <= len(polygon) <= ANNOTATE_MAX_VERTICES:
            raise ValueError(f"a polygon has 3..{ANNOTATE_MAX_VERTICES} vertices, got "
                             f"{len(polygon)}")
        rows, h = self._rows(camera), self._views(self.host)
        v = torch.zeros(ANNOTATE_MAX_VERTICES, 2, dtype=torch.int32)
        v[:len(polygon)] = torch.tensor([_zone_q(p) for p in polygon], dtype=torch.int32)
        h["vertex"][rows, index] = v
        h["n_vertex"][rows, index] = len(polygon)
        h["n_polygons"][rows] = h["n_polygons"][rows].clamp_min(index + 1)
        self._push()
        return self

    def clear_privacy_polygons(self, camera=None) -> "AnnotateStyle":
        rows, h = self._rows(camera), self._views(self.host)
        h["vertex"][rows] = 0
        h["n_vertex"][rows] = 0
        h["n_polygons"][rows] = 0
        self._push()
        return self

    def set_palette(self, colours, camera=None) -> "AnnotateStyle":
        """Sixteen (R, G, B) colours; a box takes entry ``key & 15``."""
        colours = [tuple(self._int("colour", c, 0, 255) for c in rgb) for rgb in colours]
        if len(colours) != 16 or any(len(c) != 3 for c in colours):
            raise ValueError("the palette has 16 (R, G, B) entries")
        return self._set(camera, "palette", torch.tensor(
            [r | g << 8 | b << 16 for r, g, b in colours], dtype=torch.int32))


def annotate(images: torch.Tensor, style: AnnotateStyle, det: Optional[torch.Tensor] = None,
             count: Optional[torch.Tensor] = None, track_id: Optional[torch.Tensor] = None,
             src_hw=None, slot0: int = 0) -> torch.Tensor:
    """Draw what the device knows into the thumbnails ``images`` uint8 [N, H, W, 3]
    (contiguous, W % 4 == 0, H and W <= RESIZE_MAX_EXTENT), in place, and return them: the
    outlines and ``cls:id`` labels of the boxes ``det`` fp32 [N, max_det, 6] / ``count`` int32
    [N] / ``track_id`` int32 [N, max_det] (optional), and a mosaic over every box of a privacy
    class and over the privacy polygons of ``style``.  ``src_hw`` = (Hs, Ws) <= 4096 is the pixel
    frame the boxes and polygons live in (default: the thumbnail's own).  With ``det=None`` only
    the polygons apply.  Row n is drawn in the style of camera ``slot0 + n``.  One launch on
    the current stream, no host synchronisation, capturable (csrc/kernels/annotate.hip); GPU
    and CPU (ops.reference.annotate, where the rules are written out) agree byte for byte."""
    if not isinstance(style, AnnotateStyle):
        raise TypeError(f"style must be an ops.AnnotateStyle, got {type(style).__name__}")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError(f"images are uint8 [N, H, W, 3], got {images.dtype} "
                         f"{tuple(images.shape)}")
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    if not (1 <= h <= RESIZE_MAX_EXTENT and 1 <= w <= RESIZE_MAX_EXTENT) or w % 4:
        raise ValueError(f"thumbnails of {h}x{w}: 1..{RESIZE_MAX_EXTENT}, width a multiple of 4")
    if not images.is_contiguous():
        raise ValueError("images must be contiguous")
    if images.device != style.device:
        raise ValueError(f"images on {images.device}, style on {style.device}")
    slot0 = int(slot0)
    if slot0 < 0 or slot0 + n > style.streams:
        raise ValueError(f"cameras [{slot0}, {slot0 + n}) outside the style's {style.streams}")
    hs, ws = (h, w) if src_hw is None else (int(src_hw[0]), int(src_hw[1]))
    if not (1 <= hs <= ANNOTATE_MAX_SRC and 1 <= ws <= ANNOTATE_MAX_SRC):
        raise ValueError(f"src_hw {hs}x{ws} outside 1..{ANNOTATE_MAX_SRC}")
    if det is None:
        if count is not None or track_id is not None:
            raise ValueError("count and track_id come with det")
    else:
        if det.dtype != torch.float32 or det.dim() != 3 or det.shape[2] != 6 or det.shape[0] != n:
            raise ValueError(f"det must be fp32 [{n}, max_det, 6], got {det.dtype} "
                             f"{tuple(det.shape)}")
        max_det = int(det.shape[1])
        if not 1 <= max_det <= TRACK_MAX_DET:
            raise ValueError(f"annotate needs 1 <= max_det <= {TRACK_MAX_DET}, got {max_det}")
        if count is None or count.dtype != torch.int32 or tuple(count.shape) != (n,):
            raise ValueError(f"count must be int32 [{n}]")
        if track_id is not None and (track_id.dtype != torch.int32
                                     or tuple(track_id.shape) != (n, max_det)):
            raise ValueError(f"track_id must be int32 [{n}, {max_det}], got {track_id.dtype} "
                             f"{tuple(track_id.shape)}")
        for name, t in (("det", det), ("count", count), ("track_id", track_id)):
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if t is not None and t.device != images.device:
                raise ValueError(f"images on {images.device}, {name} on {t.device}")
    if images.is_cuda:
        _native().annotate(images, style.table, style.font, det, count, track_id, hs, ws, slot0)
    else:
        _ref.annotate(images, style.host, style.font_host, det, count, track_id, (hs, ws), slot0)
    return images


def batchnorm_nhwc(x, scale, shift, relu=False, out=None):
    if out is None:
        out = torch.empty_like(x)
    if x.is_cuda:
        _native().batchnorm_nhwc(x, out, scale, shift, relu)
    else:
        y = x.float() * scale + shift
        out.copy_((y.clamp_min(0) if relu else y).to(out.dtype))
    return out
