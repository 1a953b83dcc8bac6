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
    if isinstance(plan, ViewSlots):  # per-camera views: through the mesh
        return view_to_source(det, count, plan.views, plan.slot0)
    cy, sy, cx, sx = plan.box_map()
    hs, ws = plan.src_hw
    if det.is_cuda:
        _native().det_to_source(det, count, [cy, sy, cx, sx], hs, ws)
    else:
        _ref.det_to_source(det, count, (cy, sy, cx, sx), hs, ws)
    return det


# ---------------------------------------------------------------------------
# per-camera views: a mesh-driven warp (ROI, rotation, lens dewarp, perspective)
# ---------------------------------------------------------------------------
VIEW_CELL = 16           # destination pixels per mesh cell
VIEW_NODE_LIM = 1 << 20  # node values are clamped to [-2^20, 2^20): 1/64 source pixel
VIEW_FITS = ("letterbox", "stretch", "crop")
VIEW_KEYS = ("roi", "rotate", "mirror", "homography", "lens", "pad")
_LENS_KEYS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
_FISHEYE_KEYS = ("f", "cx", "cy", "fov")


def _check_view_hw(src_hw, dst_hw):
    (hs, ws), (hd, wd) = (int(src_hw[0]), int(src_hw[1])), (int(dst_hw[0]), int(dst_hw[1]))
    if not (1 <= hs <= RESIZE_MAX_EXTENT and 1 <= ws <= RESIZE_MAX_EXTENT):
        raise ValueError(f"frame size {hs}x{ws} outside 1..{RESIZE_MAX_EXTENT}")
    if not (1 <= hd <= RESIZE_MAX_EXTENT and 1 <= wd <= RESIZE_MAX_EXTENT):
        raise ValueError(f"view size {hd}x{wd} outside 1..{RESIZE_MAX_EXTENT}")
    if hd % VIEW_CELL or wd % VIEW_CELL:
        raise ValueError(f"view size {hd}x{wd} must be a multiple of {VIEW_CELL} in both axes")
    return (hs, ws), (hd, wd)


def _fit_axis(fit: str, d: int, view: float, scale: float):
    """One axis of the view rectangle (``view`` long) inside ``d`` destination pixels: (first
    destination coordinate that holds it, view units per destination pixel)."""
    if fit == "stretch":
        return 0.0, view / d
    if fit == "crop":  # scale = the resized extent of this axis (center_crop_plan)
        return -float(int(round((scale - d) / 2))), view / scale
    n = min(d, max(1, int(round(view * scale))))  # letterbox_plan's rounding
    return float(int(round((d - n) / 2 - 0.1))), view / n


def _lens_points(x, y, lens, ws: int):
    """Ideal (rectilinear) source positions -> positions in the camera's distorted frame,
    both in pixel-corner coordinates; the models themselves use OpenCV's pixel centres."""
    import numpy as np

    if not isinstance(lens, dict):
        raise ValueError(f"lens must be an object, got {type(lens).__name__}")
    fish = lens.get("fisheye")
    keys, src = (_FISHEYE_KEYS, fish) if fish is not None else (_LENS_KEYS, lens)
    if not isinstance(src, dict) or (fish is not None and len(lens) != 1):
        raise ValueError('a fisheye lens is {"fisheye": {"f", "cx", "cy", "fov"}}')
    unknown = sorted(set(src) - set(keys))
    if unknown:
        raise ValueError(f"unknown lens keys {unknown}; known: {keys}")
    p = {}
    for k in keys:
        v = src.get(k, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise ValueError(f"lens {k} = {v!r} is not a finite number")
        p[k] = float(v)
    x, y = x - 0.5, y - 0.5
    if fish is not None:
        if p["f"] <= 0 or not 0 < p["fov"] < 180:
            raise ValueError("fisheye needs f > 0 and 0 < fov < 180 (degrees)")
        # the ideal view is a pinhole that sees ``fov`` degrees across the frame width;
        # equidistant: the distorted radius is f * (angle from the axis)
        fp = (ws / 2) / np.tan(np.radians(p["fov"]) / 2)
        xr, yr = x - p["cx"], y - p["cy"]
        r = np.hypot(xr, yr)
        k = np.where(r > 1e-9, p["f"] * np.arctan(r / fp) / np.maximum(r, 1e-9), p["f"] / fp)
        return p["cx"] + xr * k + 0.5, p["cy"] + yr * k + 0.5
    if p["fx"] <= 0 or p["fy"] <= 0:
        raise ValueError("lens needs fx > 0 and fy > 0")
    xn, yn = (x - p["cx"]) / p["fx"], (y - p["cy"]) / p["fy"]
    r2 = xn * xn + yn * yn
    rad = 1 + r2 * (p["k1"] + r2 * (p["k2"] + r2 * p["k3"]))
    xd = xn * rad + 2 * p["p1"] * xn * yn + p["p2"] * (r2 + 2 * xn * xn)
    yd = yn * rad + p["p1"] * (r2 + 2 * yn * yn) + 2 * p["p2"] * xn * yn
    return p["fx"] * xd + p["cx"] + 0.5, p["fy"] * yd + p["cy"] + 0.5


def view_mesh(src_hw, dst_hw, *, roi=None, rotate: int = 0, mirror: bool = False,
              homography=None, lens=None, fit: str = "letterbox"):
    """The mesh of one camera view (:class:`CameraViews`): int32 numpy [Hd/16 + 1, Wd/16 + 1, 2],
    node (gy, gx) = the source position (x, y), in 1/64 pixel and pixel-corner coordinates,
    that destination point (16 gx, 16 gy) samples.  Computed in float64 and rounded once.
    From the destination to the source it composes: the inverse of ``fit`` ("letterbox": the
    view rectangle scaled uniformly into the destination and centred with
    :func:`letterbox_plan`'s rounding; "crop": :func:`center_crop_plan`'s resize and centre
    crop, square destinations; "stretch"); ``mirror`` (left-right, of the view) and ``rotate``
    (0 / 90 / 180 / 270: the view is the source turned counter-clockwise, ``np.rot90``);
    ``roi`` = (x0, y0, x1, y1), the source rectangle the view shows (digital zoom; default the
    whole frame; the letterbox bars show what the frame holds beyond it); ``homography``, 3 x 3,
    ideal source position -> source position; ``lens``, ideal -> distorted position: Brown-Conrady
    in OpenCV's convention {fx, fy, cx, cy, k1, k2, p1, p2, k3} or an equidistant fisheye
    {"fisheye": {f, cx, cy, fov}} seen as a pinhole of ``fov`` degrees across the frame width.
    With no options the mesh reproduces :func:`frame_resize` with the corresponding plan
    (exactly where the scale is an integer ratio)."""
    import numpy as np

    (hs, ws), (hd, wd) = _check_view_hw(src_hw, dst_hw)
    if fit not in VIEW_FITS:
        raise ValueError(f"fit must be one of {VIEW_FITS}, got {fit!r}")
    if isinstance(rotate, bool) or rotate not in (0, 90, 180, 270):
        raise ValueError(f"rotate must be 0, 90, 180 or 270, got {rotate!r}")
    if roi is None:
        roi = (0.0, 0.0, float(ws), float(hs))
    try:
        x0, y0, x1, y1 = (float(v) for v in roi)
    except (TypeError, ValueError):
        raise ValueError(f"roi must be (x0, y0, x1, y1), got {roi!r}") from None
    if not (np.isfinite([x0, y0, x1, y1]).all() and x1 > x0 and y1 > y0):
        raise ValueError(f"empty roi {roi!r}: needs x1 > x0 and y1 > y0")
    rw, rh = x1 - x0, y1 - y0
    vw, vh = (rh, rw) if rotate in (90, 270) else (rw, rh)
    if fit == "crop":
        if hd != wd:
            raise ValueError(f"fit='crop' needs a square view, got {hd}x{wd}")
        short = hd * 8 // 7  # center_crop_plan: shorter side -> short, the other in proportion
        sx, sy = (short * vw / vh, float(short)) if vh <= vw else (float(short), short * vh / vw)
        sx, sy = float(int(sx)), float(int(sy))
    else:
        sx = sy = min(hd / vh, wd / vw)
    cx0, kx = _fit_axis(fit, wd, vw, sx)
    cy0, ky = _fit_axis(fit, hd, vh, sy)
    gx = (np.arange(wd // VIEW_CELL + 1, dtype=np.float64) * VIEW_CELL - cx0) * kx
    gy = (np.arange(hd // VIEW_CELL + 1, dtype=np.float64) * VIEW_CELL - cy0) * ky
    xv, yv = np.meshgrid(gx, gy)  # view coordinates of every node
    if mirror:
        xv = vw - xv
    if rotate == 90:
        xv, yv = rw - yv, xv
    elif rotate == 180:
        xv, yv = rw - xv, rh - yv
    elif rotate == 270:
        xv, yv = yv, rh - xv
    x, y = x0 + xv, y0 + yv
    if homography is not None:
        try:
            h = np.asarray(homography, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("homography must be 3 x 3 numbers") from None
        if h.shape != (3, 3) or not np.isfinite(h).all():
            raise ValueError(f"homography must be 3 x 3 finite numbers, got shape {h.shape}")
        if abs(np.linalg.det(h)) <= 1e-12 * max(1.0, np.abs(h).max()) ** 3:
            raise ValueError("singular homography")
        w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
        if (w <= 0).any():
            raise ValueError("homography sends part of the view behind the camera")
        x, y = ((h[0, 0] * x + h[0, 1] * y + h[0, 2]) / w,
                (h[1, 0] * x + h[1, 1] * y + h[1, 2]) / w)
    if lens is not None:
        x, y = _lens_points(x, y, lens, ws)
    nodes = np.rint(np.stack([x, y], -1) * 64.0)
    return np.clip(np.nan_to_num(nodes, nan=-VIEW_NODE_LIM), -VIEW_NODE_LIM,
                   VIEW_NODE_LIM - 1).astype(np.int32)


def view_mesh_from(src_hw, dst_hw, view, fit: str = "letterbox"):
    """(mesh, pad) of one twin / JSON view entry: null (the plain ``fit``) or an object with
    ``VIEW_KEYS``.  Raises ValueError on anything else."""
    if view is None:
        view = {}
    if not isinstance(view, dict):
        raise ValueError(f"a view is an object or null, got {type(view).__name__}")
    unknown = sorted(set(view) - set(VIEW_KEYS))
    if unknown:
        raise ValueError(f"unknown view keys {unknown}; known: {VIEW_KEYS}")
    pad = view.get("pad", None)
    if pad is None:
        pad = 0 if fit == "crop" else LETTERBOX_PAD
    if isinstance(pad, bool) or not isinstance(pad, int) or not 0 <= pad <= 255:
        raise ValueError(f"view pad {pad!r} outside 0..255")
    mirror = view.get("mirror", False)
    if not isinstance(mirror, bool):
        raise ValueError(f"view mirror must be true or false, got {mirror!r}")
    mesh = view_mesh(src_hw, dst_hw, roi=view.get("roi"), rotate=view.get("rotate", 0),
                     mirror=mirror, homography=view.get("homography"), lens=view.get("lens"),
                     fit=fit)
    return mesh, pad


class CameraViews:
    """The views of ``streams`` cameras of ``src_hw`` = (Hs, Ws) pixels into ``dst_hw`` =
    (Hd, Wd) model pixels (multiples of 16): ``mesh`` int32 [streams, Hd/16 + 1, Wd/16 + 1, 2]
    (:func:`view_mesh`) and ``pad`` int32 [streams], the tensors csrc/kernels/frame_warp.hip
    reads every step -- so :meth:`set` takes effect from the next step without recapturing.
    Every camera starts with the plain ``fit`` view."""

    def __init__(self, streams: int, src_hw, dst_hw, device="cpu", fit: str = "letterbox"):
        if streams < 1:
            raise ValueError(f"streams must be >= 1, got {streams}")
        self.src_hw, self.dst_hw = _check_view_hw(src_hw, dst_hw)
        self.streams, self.fit = int(streams), fit
        plain, pad = view_mesh_from(self.src_hw, self.dst_hw, None, fit)
        self.mesh = torch.from_numpy(plain).repeat(self.streams, 1, 1, 1).to(device)
        self.pad = torch.full((self.streams,), pad, dtype=torch.int32, device=device)

    @property
    def device(self) -> torch.device:
        return self.mesh.device

    def set(self, stream: int, mesh, pad: int = LETTERBOX_PAD) -> "CameraViews":
        """Give camera ``stream`` the view ``mesh`` ([Hd/16 + 1, Wd/16 + 1, 2] integers; every
        node value is clamped to [-2^20, 2^20), so no word in device memory can overflow the
        kernel's arithmetic) and the padding grey ``pad``."""
        if isinstance(stream, bool) or not 0 <= int(stream) < self.streams:
            raise ValueError(f"camera {stream} outside 0..{self.streams - 1}")
        if isinstance(pad, bool) or not isinstance(pad, int) or not 0 <= pad <= 255:
            raise ValueError(f"pad {pad!r} outside 0..255")
        m = torch.as_tensor(mesh)
        if m.is_floating_point() or m.dtype == torch.bool or tuple(m.shape) != tuple(
                self.mesh.shape[1:]):
            raise ValueError(f"a view mesh is integer {list(self.mesh.shape[1:])}, got {m.dtype} "
                             f"{list(m.shape)}")
        m = m.to(torch.int64).clamp(-VIEW_NODE_LIM, VIEW_NODE_LIM - 1).to(torch.int32)
        self.mesh[int(stream)].copy_(m)
        self.pad[int(stream)] = pad
        return self

    def set_view(self, stream: int, view) -> "CameraViews":
        """:meth:`set` from a twin / JSON entry (:func:`view_mesh_from`)."""
        return self.set(stream, *view_mesh_from(self.src_hw, self.dst_hw, view, self.fit))


@dataclass(frozen=True)
class ViewSlots:
    """Batch rows of a slice as cameras ``slot0 ..`` of ``views``: what the engine hands the
    models in place of a ResizePlan, so that :func:`det_to_source` maps their boxes through
    the mesh (:func:`view_to_source`)."""
    views: CameraViews
    slot0: int = 0

    @property
    def src_hw(self):
        return self.views.src_hw

    @property
    def dst_hw(self):
        return self.views.dst_hw


def _check_views(views, n: int, slot0: int, device) -> int:
    if not isinstance(views, CameraViews):
        raise TypeError(f"views must be an ops.CameraViews, got {type(views).__name__}")
    slot0 = int(slot0)
    if slot0 < 0 or slot0 + n > views.streams:
        raise ValueError(f"cameras [{slot0}, {slot0 + n}) outside the views' {views.streams}")
    if views.device != device:
        raise ValueError(f"frames on {device}, views on {views.device}")
    return slot0


def frame_warp(src: torch.Tensor, views: CameraViews, out: Optional[torch.Tensor] = None,
               slot0: int = 0, src_format: str = "rgb") -> torch.Tensor:
    """uint8 frames [N, Hs, Ws, 3] -> [N, Hd, Wd, 3], batch row n through the view of camera
    ``slot0 + n`` of ``views``: a bilinear mesh gives every destination pixel a source position
    in 2^-16 pixel, sampled with :func:`frame_resize`'s 11-bit bilinear; positions outside the
    frame are the camera's ``pad``; every byte of ``out`` is written.  The rule is written out
    in ops.reference.frame_warp; GPU (csrc/kernels/frame_warp.hip) and CPU are bit-identical.
    ``src_format="nv12"``: ``src`` is NV12 [N, Hs * 3 // 2, Ws] and the result equals
    ``frame_warp(nv12_to_rgb(src), ...)`` byte for byte."""
    _check_format(src_format)
    nv12 = src_format == "nv12"
    if not isinstance(views, CameraViews):
        raise TypeError(f"views must be an ops.CameraViews, got {type(views).__name__}")
    if nv12:
        hw = _check_nv12(src, views.src_hw[0])
    else:
        if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
            raise ValueError(f"RGB frames are uint8 [N, Hs, Ws, 3], got {src.dtype} "
                             f"{tuple(src.shape)}")
        hw = (int(src.shape[1]), int(src.shape[2]))
    if hw != views.src_hw:
        raise ValueError(f"frames of {hw[0]}x{hw[1]}, the views were made for "
                         f"{views.src_hw[0]}x{views.src_hw[1]}")
    n = int(src.shape[0])
    slot0 = _check_views(views, n, slot0, src.device)
    if out is None:
        out = torch.empty(n, *views.dst_hw, 3, dtype=torch.uint8, device=src.device)
    if tuple(out.shape) != (n, *views.dst_hw, 3) or out.dtype != torch.uint8:
        raise ValueError(f"out must be uint8 {[n, *views.dst_hw, 3]}, got {out.dtype} "
                         f"{list(out.shape)}")
    if src.is_cuda:
        _native().frame_warp(src, out, views.mesh, views.pad, slot0, nv12)
    else:
        _ref.frame_warp(_ref.nv12_to_rgb(src) if nv12 else src, views.mesh[slot0:slot0 + n],
                        views.pad[slot0:slot0 + n], out)
    return out


def view_to_source(det: torch.Tensor, count: torch.Tensor, views: CameraViews,
                   slot0: int = 0) -> torch.Tensor:
    """Kept boxes of :func:`nms` (det fp32 [N, max_det, 6], rows < count[n]) from the view
    pixels of camera ``slot0 + n`` to source-frame pixels, in place.  Each edge is quantised to
    quarter view pixels with the tracker's rule (NaN -> 0; at most 4096 pixels) and clamped to
    the view; the four corners and the four edge midpoints go through the mesh and the row
    becomes their axis-aligned hull, clamped to the frame.  Exact for roi, rotation and mirror
    views; for lens and perspective views it is the hull of those eight samples, which a
    strongly curved edge can leave by a fraction of its sag.  Score, class and the rows past
    count are untouched.  GPU and CPU (ops.reference.view_to_source) are bit-identical."""
    if det.dtype != torch.float32 or det.dim() != 3 or det.shape[2] != 6:
        raise ValueError(f"det must be fp32 [N, max_det, 6], got {det.dtype} {tuple(det.shape)}")
    n = int(det.shape[0])
    slot0 = _check_views(views, n, slot0, det.device)
    if det.is_cuda:
        _native().view_to_source(det, count, views.mesh, *views.src_hw, *views.dst_hw, slot0)
    else:
        _ref.view_to_source(det, count, views.mesh[slot0:slot0 + n], views.dst_hw, views.src_hw)
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
# sliced detection: tile views of a frame, and the merge of what the tiles saw
# ---------------------------------------------------------------------------
MERGE_MAX_CANDIDATES = 4096  # groups * R: what one workgroup sorts in LDS
MERGE_MODES = ("nmm", "nms")
MERGE_METRICS = ("ios", "iou")
SLICE_MAX_GRID = 4


def det_merge(det: torch.Tensor, count: torch.Tensor, groups: int, *, mode: str = "nmm",
              metric: str = "ios", thr: float = 0.5, class_aware: bool = True,
              max_det: Optional[int] = None, out: Optional[torch.Tensor] = None,
              out_count: Optional[torch.Tensor] = None):
    """Merge ``groups`` :func:`nms` outputs per camera -- the tiles of a sliced frame and the
    full frame -- into one list: ``det`` fp32 [groups * N, R, 6] / ``count`` int32 [groups * N],
    group-major (row g * N + n is group g of camera n), all boxes already in one pixel frame
    -> (det fp32 [N, max_det, 6], count int32 [N]); ``max_det`` defaults to R.  Candidates go
    by score (then group, then row); one that matches an earlier kept one -- same class
    (``class_aware``), overlap over the union (``metric="iou"``) or over the smaller box
    ("ios", which lets a whole box absorb the half a tile border cut off) of at least ``thr``
    -- is absorbed by the earliest such one; ``mode="nms"`` keeps the kept rows as they are,
    "nmm" grows each kept box to the hull of what it absorbed.  The sweep ends at ``max_det``
    kept rows; rows past the new count are zero.  Integer arithmetic on quarter-pixel boxes, the
    tracker's: the rule is written out in ops.reference.det_merge, which the GPU
    (csrc/kernels/det_merge.hip) equals bit for bit.  ``1 <= max_det <= R <= TRACK_MAX_DET``
    and ``groups * R <= MERGE_MAX_CANDIDATES``: nothing is truncated silently."""
    if mode not in MERGE_MODES:
        raise ValueError(f"mode must be one of {MERGE_MODES}, got {mode!r}")
    if metric not in MERGE_METRICS:
        raise ValueError(f"metric must be one of {MERGE_METRICS}, got {metric!r}")
    if det.dtype != torch.float32 or det.dim() != 3 or det.shape[2] != 6:
        raise ValueError(f"det must be fp32 [groups * N, R, 6], got {det.dtype} {tuple(det.shape)}")
    if isinstance(groups, bool) or int(groups) < 1 or det.shape[0] % int(groups):
        raise ValueError(f"det has {det.shape[0]} rows, no multiple of groups = {groups!r}")
    groups = int(groups)
    gn, r = int(det.shape[0]), int(det.shape[1])
    n = gn // groups
    if count.dtype != torch.int32 or tuple(count.shape) != (gn,):
        raise ValueError(f"count must be int32 [{gn}], got {count.dtype} {tuple(count.shape)}")
    if not det.is_contiguous() or not count.is_contiguous():
        raise ValueError("det and count must be contiguous")
    if count.device != det.device:
        raise ValueError(f"det on {det.device}, count on {count.device}")
    if not 1 <= r <= TRACK_MAX_DET or groups * r > MERGE_MAX_CANDIDATES:
        raise ValueError(f"det_merge needs 1 <= R <= {TRACK_MAX_DET} and groups * R <= "
                         f"{MERGE_MAX_CANDIDATES}, got {groups} x {r}")
    max_det = r if max_det is None else int(max_det)
    if not 1 <= max_det <= r:
        raise ValueError(f"det_merge needs 1 <= max_det <= R = {r}, got {max_det}")
    thr_q = track_thr_q(thr)
    if not 1 <= thr_q <= 1024:
        raise ValueError(f"thr {thr} gives a threshold of {thr_q}/1024, outside 1..1024")
    if out is None:
        out = empty(n, max_det, 6, dtype=torch.float32, device=det.device)
    if out_count is None:
        out_count = empty(n, dtype=torch.int32, device=det.device)
    if (out.dtype != torch.float32 or tuple(out.shape) != (n, max_det, 6)
            or not out.is_contiguous() or out.device != det.device):
        raise ValueError(f"out must be contiguous fp32 [{n}, {max_det}, 6] on {det.device}")
    if (out_count.dtype != torch.int32 or tuple(out_count.shape) != (n,)
            or not out_count.is_contiguous() or out_count.device != det.device):
        raise ValueError(f"out_count must be contiguous int32 [{n}] on {det.device}")
    args = (groups, thr_q, metric == "iou", bool(class_aware), mode == "nmm")
    if det.is_cuda:
        _native().det_merge(det, count, out, out_count, *args)
    else:
        _ref.det_merge(det, count, *args, out, out_count)
    return out, out_count


def _slice_axis(size: int, k: int, overlap: float):
    import math

    se = size - (size & 1)
    w = -(-se // k)
    w = min(se, w + (w & 1))
    while k > 1:
        step = 2 * -(-(se - w) // (2 * (k - 1)))  # the largest even step between origins
        if step <= w - math.floor(overlap * w):
            break
        w += 2
    return w, [2 * ((i * (se - w)) // (2 * (k - 1))) if k > 1 else 0 for i in range(k)]


def check_slice_grid(grid, overlap):
    """(cols, rows, overlap) of a tile grid, or ValueError: 1..SLICE_MAX_GRID tiles per axis,
    neighbours sharing 0..0.5 of a tile."""
    try:
        cols, rows = (int(v) for v in grid)
        overlap = float(overlap)
    except (TypeError, ValueError):
        raise ValueError(f"grid is (cols, rows) and overlap a number, got {grid!r}, "
                         f"{overlap!r}") from None
    if not (1 <= cols <= SLICE_MAX_GRID and 1 <= rows <= SLICE_MAX_GRID):
        raise ValueError(f"grid {cols}x{rows} outside 1..{SLICE_MAX_GRID} per axis")
    if not 0.0 <= overlap <= 0.5:
        raise ValueError(f"overlap {overlap} outside 0..0.5")
    return cols, rows, overlap


def slice_rois(src_hw, grid=(2, 2), overlap: float = 0.2):
    """The ``cols * rows`` tiles of a ``grid`` = (cols, rows) over a frame of ``src_hw`` =
    (Hs, Ws), row-major, as integer ROIs (x0, y0, w, h).  The rule, per axis of S pixels (an odd
    S loses its last pixel) with k tiles: w is the smallest even size, from ceil(S / k) up, whose
    largest step between origins, 2 * ceil((S - w) / (2 (k - 1))), still leaves neighbours
    floor(overlap * w) shared pixels; origin i is (i * (S - w) / (k - 1)) rounded down to even.
    So all tiles have one even size and even origins (NV12), the first and last are flush with
    the frame, neighbours share at least floor(overlap * w) pixels, and k = 1 is the frame."""
    cols, rows, overlap = check_slice_grid(grid, overlap)
    try:
        hs, ws = (int(v) for v in src_hw)
    except (TypeError, ValueError):
        raise ValueError(f"src_hw is (Hs, Ws), got {src_hw!r}") from None
    if hs < 2 * rows or ws < 2 * cols:
        raise ValueError(f"a frame of {hs}x{ws} is too small for a {cols}x{rows} grid")
    w, xs = _slice_axis(ws, cols, overlap)
    h, ys = _slice_axis(hs, rows, overlap)
    return [(x, y, w, h) for y in ys for x in xs]


def slice_views(streams: int, src_hw, dst_hw, grid=(2, 2), overlap: float = 0.2,
                device="cpu") -> CameraViews:
    """The tile views of ``streams`` cameras as one :class:`CameraViews` of
    ``cols * rows * streams`` slots: slot ``g * streams + n`` is tile g (:func:`slice_rois`) of
    camera n, letterboxed into ``dst_hw``.  ``frame_warp(src[lo:hi], views, out=...,
    slot0=g * streams + lo)`` fills tile g of a slice, and :func:`view_to_source` with the same
    slot maps its boxes back to frame pixels."""
    rois, s = slice_rois(src_hw, grid, overlap), int(streams)
    views = CameraViews(len(rois) * s, src_hw, dst_hw, device=device)
    for g, (x, y, w, h) in enumerate(rois):
        mesh, pad = view_mesh_from(views.src_hw, views.dst_hw, {"roi": [x, y, x + w, y + h]})
        views.mesh[g * s:(g + 1) * s] = torch.from_numpy(mesh).to(views.device)
        views.pad[g * s:(g + 1) * s] = pad
    return views


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
# low-light enhancement: per-camera CLAHE on luma (csrc/kernels/frame_enhance.hip)
# ---------------------------------------------------------------------------
ENHANCE_MODES = _ref.ENHANCE_MODES
ENHANCE_PARAMS = _ref.ENHANCE_PARAMS
ENHANCE_PARAM_RANGES = _ref.ENHANCE_PARAM_RANGES
ENHANCE_MAX_TILES = _ref.ENHANCE_MAX_TILES
ENHANCE_MAX_EXTENT = _ref.ENHANCE_MAX_EXTENT
ENHANCE_STATS = ("mean16", "alpha")
# on at full strength, clip limit 2.0; auto ramps in between mean luma 64 (off) and 24 (full),
# the watch's default dark level
ENHANCE_DEFAULTS = {"mode": 1, "strength": 256, "clip_q8": 512, "lo16": 384, "hi16": 1024}


def enhance_strength_q(strength: float) -> int:
    """A blend strength 0..1 in 1/256: floor(strength * 256 + 0.5)."""
    import math

    return int(math.floor(float(strength) * 256 + 0.5))


class FrameEnhance:
    """Low-light enhancement of ``streams`` cameras of ``hw`` = (H, W) pixel frames on a grid
    of ``tiles`` = (TY, TX) tiles, and the device memory csrc/kernels/frame_enhance.hip works
    in: ``params`` int32 [streams, 8] (``ENHANCE_PARAMS``, read and clamped every step, so the
    setters take effect from the next step without recapturing), ``axis`` int32
    [W + H + TY + 2] (per column and per row the table cell and the weight, ``cell | w << 8``,
    then the first row of every row band), ``luts`` uint8 [streams, TY TX, 256] and ``sums``
    int32 [streams, TY TX] (the per-tile tables and luma sums between the two launches)."""

    def __init__(self, streams: int, hw, tiles=(8, 8), device="cpu"):
        if streams < 1:
            raise ValueError(f"streams must be >= 1, got {streams}")
        h, w = int(hw[0]), int(hw[1])
        if not (1 <= h <= ENHANCE_MAX_EXTENT and 1 <= w <= ENHANCE_MAX_EXTENT):
            raise ValueError(f"frame_enhance frames are 1..{ENHANCE_MAX_EXTENT} pixels on each "
                             f"axis, got {h}x{w}")
        ty, tx = int(tiles[0]), int(tiles[1])
        if not (1 <= ty <= ENHANCE_MAX_TILES and 1 <= tx <= ENHANCE_MAX_TILES):
            raise ValueError(f"tiles are 1..{ENHANCE_MAX_TILES} on each axis, got {tiles}")
        th, tw = -(-h // ty), -(-w // tx)
        if (ty - 1) * th >= h or (tx - 1) * tw >= w:
            raise ValueError(f"a {ty}x{tx} grid of {th}x{tw} tiles leaves a tile of a {h}x{w} "
                             f"frame empty")
        import numpy as np

        self.streams, self.hw, self.tiles = int(streams), (h, w), (ty, tx)
        # LDS histogram copies per wave in the table launch (1, 2, 4 or 8; docs/kernels.md)
        self.hist_copies = 4
        self.params = torch.zeros(self.streams, 8, dtype=torch.int32, device=device)
        self.luts = torch.zeros(self.streams, ty * tx, 256, dtype=torch.uint8, device=device)
        self.sums = torch.zeros(self.streams, ty * tx, dtype=torch.int32, device=device)
        words = []
        for size, t in ((w, tx), (h, ty)):
            # cell k of an axis reads tiles (max(k - 1, 0), min(k, t - 1)): 0 before the first
            # tile centre, t past the last one
            s = -(-size // t)
            a = 2 * np.arange(size) + 1 - s
            cell = np.where(a <= 0, 0, np.minimum(a // (2 * s), t - 1) + 1)
            words.append(cell | (_ref.enhance_axis(size, t)[2] << 8))
        ycell = words[1] & 0xff
        words.append(np.searchsorted(ycell, np.arange(ty + 2)))  # band b = rows of cell b
        self.axis = torch.from_numpy(np.concatenate(words).astype(np.int32)).to(device)
        for name, v in ENHANCE_DEFAULTS.items():
            self._set(None, name, v)

    @property
    def device(self) -> torch.device:
        return self.params.device

    def _set(self, camera, name: str, v: int) -> "FrameEnhance":
        i = ENHANCE_PARAMS.index(name)
        lo, hi = ENHANCE_PARAM_RANGES[i]
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"enhance parameter {name} = {v!r} outside {lo}..{hi}")
        if camera is None:
            rows = slice(None)
        elif not 0 <= int(camera) < self.streams:
            raise ValueError(f"camera {camera} outside 0..{self.streams - 1}")
        else:
            rows = slice(int(camera), int(camera) + 1)
        self.params[rows, i] = v
        return self

    def set_mode(self, mode, camera=None) -> "FrameEnhance":
        """``mode``: "off", "on" (blend at ``strength``) or "auto" (``strength`` scaled by how
        dark the frame is, :meth:`set_levels`), or its number."""
        if isinstance(mode, str):
            if mode not in ENHANCE_MODES:
                raise ValueError(f"mode must be one of {ENHANCE_MODES}, got {mode!r}")
            mode = ENHANCE_MODES.index(mode)
        return self._set(camera, "mode", mode)

    def set_strength(self, strength: int, camera=None) -> "FrameEnhance":
        """Blend weight in 1/256, 0..256 (:func:`enhance_strength_q`)."""
        return self._set(camera, "strength", strength)

    def set_clip(self, clip: float, camera=None) -> "FrameEnhance":
        """Clip limit as a multiple of the flat histogram's bin height, 1.0..64.0."""
        if isinstance(clip, bool) or not 1.0 <= float(clip) <= 64.0:
            raise ValueError(f"clip {clip!r} outside 1.0..64.0")
        return self._set(camera, "clip_q8", int(float(clip) * 256 + 0.5))

    def set_levels(self, dark: float, bright: float, camera=None) -> "FrameEnhance":
        """Auto mode's ramp in luma levels: full strength at a mean luma of ``dark`` or below,
        none at ``bright`` or above; at least one level apart."""
        lo16, hi16 = watch_level16(dark), watch_level16(bright)
        if hi16 - lo16 < _ref.ENHANCE_MIN_SPAN:
            raise ValueError(f"levels dark {dark} / bright {bright} are less than one luma "
                             f"level apart")
        # both checked before either is stored
        for name, v in (("lo16", lo16), ("hi16", hi16)):
            lo, hi = ENHANCE_PARAM_RANGES[ENHANCE_PARAMS.index(name)]
            if not lo <= v <= hi:
                raise ValueError(f"enhance parameter {name} = {v} outside {lo}..{hi}")
        return self._set(camera, "lo16", lo16)._set(camera, "hi16", hi16)


def frame_enhance(images: torch.Tensor, enh: FrameEnhance, slot0: int = 0,
                  out: Optional[torch.Tensor] = None,
                  out_stats: Optional[torch.Tensor] = None):
    """Low-light enhancement of one step: batch row n of ``images`` -- uint8 RGB [N, H, W, 3]
    -- is camera ``slot0 + n`` of ``enh``.  Contrast-limited adaptive histogram equalisation of
    the luma on ``enh.tiles``, blended in at the camera's ``alpha`` (0..256); R, G and B move
    by the same amount, so the chroma stays.  ``out`` None works in place (a camera whose
    alpha is 0 is then not written at all), else every byte of ``out`` is written.  Returns
    ``(out or images, stats)``, stats int32 [N, 2] = mean16 (mean luma in 1/16), alpha, every
    element written.  Integer arithmetic: GPU (csrc/kernels/frame_enhance.hip) and CPU
    (ops.reference.frame_enhance, where the rules are written out) are byte-identical."""
    if not isinstance(enh, FrameEnhance):
        raise TypeError(f"enh must be an ops.FrameEnhance, got {type(enh).__name__}")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError(f"images are uint8 RGB [N, H, W, 3], got {images.dtype} "
                         f"{tuple(images.shape)}")
    hw = (int(images.shape[1]), int(images.shape[2]))
    if hw != enh.hw:
        raise ValueError(f"images of {hw[0]}x{hw[1]}, the enhancer was made for "
                         f"{enh.hw[0]}x{enh.hw[1]}")
    if not images.is_contiguous():
        raise ValueError("images must be contiguous")
    if images.device != enh.device:
        raise ValueError(f"images on {images.device}, enhancer on {enh.device}")
    n = int(images.shape[0])
    slot0 = int(slot0)
    if slot0 < 0 or slot0 + n > enh.streams:
        raise ValueError(f"cameras [{slot0}, {slot0 + n}) outside the enhancer's {enh.streams}")
    if out is not None and (out.dtype != torch.uint8 or out.shape != images.shape
                            or not out.is_contiguous() or out.device != images.device):
        raise ValueError(f"out must be contiguous uint8 {list(images.shape)} on {images.device}")
    if out_stats is None:
        out_stats = empty(n, 2, dtype=torch.int32, device=images.device)
    if (out_stats.dtype != torch.int32 or tuple(out_stats.shape) != (n, 2)
            or not out_stats.is_contiguous() or out_stats.device != images.device):
        raise ValueError(f"out_stats must be contiguous int32 {[n, 2]} on {images.device}")
    dst = images if out is None else out
    if images.is_cuda:
        _native().frame_enhance(images, dst, enh.params, enh.axis, enh.luts, enh.sums, out_stats,
                                slot0, enh.tiles[0], enh.tiles[1], enh.hist_copies)
    else:
        _ref.frame_enhance(images, enh, slot0, out, out_stats)
    return dst, out_stats


# ---------------------------------------------------------------------------
# motion regions: the watch's motion grid -> connected blobs as detection rows
# ---------------------------------------------------------------------------
BLOB_MAX_CELLS = _ref.BLOB_MAX_CELLS
BLOB_MAX_BLOBS = _ref.BLOB_MAX_BLOBS
BLOB_CLASS = _ref.BLOB_CLASS
BLOB_CONNECTIVITY = (4, 8)


def check_blob_grid(frame_hw, cell: int) -> Tuple[int, int]:
    """The (GH, GW) grid of ``frame_hw`` at ``cell``, refused above ``BLOB_MAX_CELLS`` cells."""
    hs, ws = int(frame_hw[0]), int(frame_hw[1])
    if not (1 <= hs <= WATCH_MAX_EXTENT and 1 <= ws <= WATCH_MAX_EXTENT):
        raise ValueError(f"motion regions need frames of 1..{WATCH_MAX_EXTENT}, got {hs}x{ws}")
    if cell not in WATCH_CELLS:
        raise ValueError(f"cell must be one of {WATCH_CELLS}, got {cell}")
    grid = (-(-hs // cell), -(-ws // cell))
    if grid[0] * grid[1] > BLOB_MAX_CELLS:
        raise ValueError(f"motion regions label at most {BLOB_MAX_CELLS} cells; {hs}x{ws} at "
                         f"cell {cell} is {grid[0]}x{grid[1]} = {grid[0] * grid[1]}")
    return grid


class MotionRegions:
    """What ops.motion_blobs reads per camera, for ``streams`` cameras of ``frame_hw`` = (Hs, Ws)
    pixels on a ``cell``-pixel grid: ``params`` int32 [S, 4] = min_cells, cls, 0, 0 and
    ``ignore`` uint8 [S, GH, GW] (non-zero: the cell never counts as moving) on ``device``, with
    host mirrors.  ``camera=None`` in a setter means every camera.  The kernel reads both at run
    time and clamps min_cells into 1..GH GW and cls into 0..65535: a setter takes effect from
    the next call, or the next replay of a captured step."""

    def __init__(self, streams: int, frame_hw, cell: int = 16, device="cpu"):
        if isinstance(streams, bool) or int(streams) < 1:
            raise ValueError(f"streams must be >= 1, got {streams!r}")
        self.grid = check_blob_grid(frame_hw, cell)
        self.streams, self.cell = int(streams), int(cell)
        self.frame_hw = (int(frame_hw[0]), int(frame_hw[1]))
        cpu = torch.device(device).type == "cpu"
        self._params = torch.zeros(self.streams, 4, dtype=torch.int32)
        self._ignore = torch.zeros(self.streams, *self.grid, dtype=torch.uint8)
        self._params[:, 0], self._params[:, 1] = 1, BLOB_CLASS
        self.params = self._params if cpu else self._params.to(device)
        self.ignore = self._ignore if cpu else self._ignore.to(device)

    @property
    def device(self) -> torch.device:
        return self.params.device

    def _rows(self, camera):
        if camera is None:
            return slice(None)
        if isinstance(camera, bool) or not 0 <= int(camera) < self.streams:
            raise ValueError(f"camera {camera} outside 0..{self.streams - 1}")
        return slice(int(camera), int(camera) + 1)

    def _set_param(self, word: int, name: str, v, lo: int, hi: int, camera):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{name} = {v!r} outside {lo}..{hi}")
        self._params[self._rows(camera), word] = v
        if self.params is not self._params:
            self.params.copy_(self._params)
        return self

    def set_min_cells(self, v: int, camera=None) -> "MotionRegions":
        """Blobs of fewer cells are dropped."""
        return self._set_param(0, "min_cells", v, 1, self.grid[0] * self.grid[1], camera)

    def set_class(self, v: int, camera=None) -> "MotionRegions":
        """The class written into the blob rows."""
        return self._set_param(1, "class", v, 0, 65535, camera)

    def set_ignore(self, camera, mask) -> "MotionRegions":
        """``mask`` bool [GH, GW]: True = ignore the cell; with ``camera=None`` for every
        camera, or bool [S, GH, GW] for all of them at once (one upload)."""
        mask = torch.as_tensor(mask)
        whole = camera is None and tuple(mask.shape) == (self.streams, *self.grid)
        if mask.dtype != torch.bool or not (whole or tuple(mask.shape) == self.grid):
            raise ValueError(f"the ignore mask is bool {list(self.grid)}, got {mask.dtype} "
                             f"{tuple(mask.shape)}")
        self._ignore[self._rows(camera)] = mask.cpu().to(torch.uint8)
        if self.ignore is not self._ignore:
            self.ignore.copy_(self._ignore)
        return self

    def rasterise(self, polygons) -> torch.Tensor:
        """bool [GH, GW]: the cells whose centre lies in one of ``polygons`` (lists of 3 or
        more pixel points), by the zones' crossing-number rule on quarter pixels."""
        gh, gw = self.grid
        py = ((2 * torch.arange(gh, dtype=torch.int64) + 1) * 2 * self.cell)[:, None].expand(gh, gw)
        px = ((2 * torch.arange(gw, dtype=torch.int64) + 1) * 2 * self.cell)[None, :].expand(gh, gw)
        hit = torch.zeros(gh, gw, dtype=torch.bool)
        for poly in polygons:
            poly = [tuple(_zone_q(p)) for p in poly]
            if len(poly) < 3:
                raise ValueError(f"an ignore polygon has 3 or more vertices, got {len(poly)}")
            hit |= _ref.point_in_polygon(px, py, poly)
        return hit

    def set_ignore_polygons(self, camera, polygons) -> "MotionRegions":
        """Ignore the cells of ``camera`` that :meth:`rasterise` finds under ``polygons``."""
        return self.set_ignore(camera, self.rasterise(polygons))

    def clear_ignore(self, camera=None) -> "MotionRegions":
        return self.set_ignore(camera, torch.zeros(self.grid, dtype=torch.bool))


def motion_blobs(mask: torch.Tensor, regions: MotionRegions, slot0: int = 0, max_blobs: int = 16,
                 connectivity: int = 8, out_det: Optional[torch.Tensor] = None,
                 out_count: Optional[torch.Tensor] = None,
                 out_labels: Optional[torch.Tensor] = None):
    """Motion regions of one step: camera n of ``mask`` -- uint8 [N, GH, GW], ops.frame_watch's
    motion_mask -- is stream ``slot0 + n`` of ``regions``.  The moving cells that are not
    ignored are grouped under 4- or 8-connectivity; of the blobs of at least min_cells cells
    the ``max_blobs`` (1..64) largest are reported, ties by the lower first cell.  Returns
    ``(blob_det, blob_count, labels)``: fp32 [N, max_blobs, 6] = the blob's pixel box x1, y1,
    x2, y2, its cell count and the regions' class (rows from blob_count on all zero), int32
    [N], and int32 [N, GH, GW], the cell's row in blob_det or -1.  Every element is written.
    GPU (csrc/kernels/motion_blobs.hip) and CPU (ops.reference.motion_blobs, a flood fill) are
    bit-identical."""
    if not isinstance(regions, MotionRegions):
        raise TypeError(f"regions must be an ops.MotionRegions, got {type(regions).__name__}")
    if mask.dtype != torch.uint8 or mask.dim() != 3:
        raise ValueError(f"mask must be uint8 [N, GH, GW], got {mask.dtype} {tuple(mask.shape)}")
    if tuple(mask.shape[1:]) != regions.grid:
        raise ValueError(f"mask grid {tuple(mask.shape[1:])}, the regions were made for "
                         f"{regions.grid}")
    if regions.grid[0] * regions.grid[1] > BLOB_MAX_CELLS:
        raise ValueError(f"motion regions label at most {BLOB_MAX_CELLS} cells")
    if not mask.is_contiguous():
        raise ValueError("mask must be contiguous")
    if mask.device != regions.device:
        raise ValueError(f"mask on {mask.device}, regions on {regions.device}")
    if isinstance(max_blobs, bool) or not 1 <= int(max_blobs) <= BLOB_MAX_BLOBS:
        raise ValueError(f"max_blobs {max_blobs!r} outside 1..{BLOB_MAX_BLOBS}")
    if connectivity not in BLOB_CONNECTIVITY:
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    n, R = int(mask.shape[0]), int(max_blobs)
    slot0 = int(slot0)
    if slot0 < 0 or slot0 + n > regions.streams:
        raise ValueError(f"streams [{slot0}, {slot0 + n}) outside the regions' {regions.streams}")
    if out_det is None:
        out_det = empty(n, R, 6, dtype=torch.float32, device=mask.device)
    if out_count is None:
        out_count = empty(n, dtype=torch.int32, device=mask.device)
    if out_labels is None:
        out_labels = empty(n, *regions.grid, dtype=torch.int32, device=mask.device)
    for name, t, dt, shape in (("out_det", out_det, torch.float32, (n, R, 6)),
                               ("out_count", out_count, torch.int32, (n,)),
                               ("out_labels", out_labels, torch.int32, (n, *regions.grid))):
        if (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()
                or t.device != mask.device):
            raise ValueError(f"{name} must be contiguous {dt} {list(shape)} on {mask.device}")
    if mask.is_cuda:
        _native().motion_blobs(mask, regions.params, regions.ignore, out_det, out_count,
                               out_labels, slot0, regions.cell, *regions.frame_hw,
                               int(connectivity))
    else:
        _ref.motion_blobs(mask, regions.params, regions.ignore, slot0, regions.cell,
                          regions.frame_hw, int(connectivity), out_det, out_count, out_labels)
    return out_det, out_count, out_labels


# ---------------------------------------------------------------------------
# appearance search: int8 embeddings of the crops matched to a gallery on the device
# ---------------------------------------------------------------------------
GALLERY_MAX_CAPACITY = 1 << 20
GALLERY_MAX_TOP = 8
GALLERY_MAX_QUERIES = 65535


def _check_embed_dim(d: int) -> int:
    if isinstance(d, bool) or not (64 <= int(d) <= 4096 and int(d) % 64 == 0):
        raise ValueError(f"the embedding width is a multiple of 64 in 64..4096, got {d!r}")
    return int(d)


def _check_out(name, t, dt, shape, device):
    if t.dtype != dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be contiguous {dt} {list(shape)} on {device}")


def embed_quantize(features: torch.Tensor, out_codes: Optional[torch.Tensor] = None,
                   out_nrm2: Optional[torch.Tensor] = None):
    """Feature maps bf16 [M, H, W, C] (NHWC, contiguous; C % 64 == 0 in 64..4096, H W in
    1..256) -> ``(codes, nrm2)``: int8 [M, C] and int32 [M] = sum codes^2.  Average pooling as
    an exact int32 sum of rint(clamp(x) * 256), then one shared exponent per row so that the
    largest channel lands in 64..127 (ops.reference.embed_quantize writes the rule out).  GPU
    (csrc/kernels/gallery.hip) and CPU are bit-identical; one launch, capturable."""
    if features.dtype != torch.bfloat16 or features.dim() != 4 or not features.is_contiguous():
        raise ValueError(f"features must be contiguous bf16 [M, H, W, C], got {features.dtype} "
                         f"{tuple(features.shape)}")
    m, h, w, c = (int(v) for v in features.shape)
    _check_embed_dim(c)
    if not 1 <= h * w <= 256:
        raise ValueError(f"embed_quantize pools 1..256 positions, got {h}x{w}")
    if m > GALLERY_MAX_QUERIES:
        raise ValueError(f"at most {GALLERY_MAX_QUERIES} rows, got {m}")
    dev = features.device
    if out_codes is None:
        out_codes = empty(m, c, dtype=torch.int8, device=dev)
    if out_nrm2 is None:
        out_nrm2 = empty(m, dtype=torch.int32, device=dev)
    _check_out("out_codes", out_codes, torch.int8, (m, c), dev)
    _check_out("out_nrm2", out_nrm2, torch.int32, (m,), dev)
    if features.is_cuda:
        _native().embed_quantize(features, out_codes, out_nrm2)
    else:
        _ref.embed_quantize(features, out_codes, out_nrm2)
    return out_codes, out_nrm2


class Gallery:
    """The enrolled embeddings ops.gallery_match scores against, for up to ``capacity`` (1..2^20)
    rows of ``dim`` int8 codes, in device memory with host mirrors: ``codes`` int8 [capacity,
    dim], ``scale`` fp32 [capacity] = 1 / sqrt(nrm2) (computed on the host, so both sides read
    the same bits), ``label`` int32 [capacity] and ``count`` int32 [1].  The kernel reads
    ``count`` at run time: :meth:`enrol`, :meth:`remove` and :meth:`clear` take effect from the
    next call, or the next replay of a captured step, without recapturing."""

    def __init__(self, capacity: int, dim: int, device="cpu"):
        if isinstance(capacity, bool) or not 1 <= int(capacity) <= GALLERY_MAX_CAPACITY:
            raise ValueError(f"capacity must be 1..{GALLERY_MAX_CAPACITY}, got {capacity!r}")
        self.capacity, self.dim = int(capacity), _check_embed_dim(dim)
        cpu = torch.device(device).type == "cpu"
        self._codes = torch.zeros(self.capacity, self.dim, dtype=torch.int8)
        self._nrm2 = torch.zeros(self.capacity, dtype=torch.int32)
        self._scale = torch.zeros(self.capacity, dtype=torch.float32)
        self._label = torch.full((self.capacity,), -1, dtype=torch.int32)
        self._count = torch.zeros(1, dtype=torch.int32)
        self.codes = self._codes if cpu else self._codes.to(device)
        self.scale = self._scale if cpu else self._scale.to(device)
        self.label = self._label if cpu else self._label.to(device)
        self.count = self._count if cpu else self._count.to(device)

    @property
    def device(self) -> torch.device:
        return self.codes.device

    def __len__(self) -> int:
        return int(self._count[0])

    def labels(self) -> torch.Tensor:
        """The enrolled rows' labels, int32 [len] (a host copy)."""
        return self._label[:len(self)].clone()

    def _upload(self, lo: int, hi: int) -> None:
        """Rows [lo, hi) and the count to the device; the count goes last."""
        if self.codes is not self._codes:
            for dev, host in ((self.codes, self._codes), (self.scale, self._scale),
                              (self.label, self._label)):
                if hi > lo:
                    dev[lo:hi].copy_(host[lo:hi])
            self.count.copy_(self._count)

    def enrol(self, codes, nrm2, label) -> "Gallery":
        """Append rows: ``codes`` int8 [R, dim] (or [dim]), ``nrm2`` int32 [R] = sum codes^2 as
        ops.embed_quantize returned it, ``label`` an int >= 0 or int [R].  A row of nrm2 == 0
        has no direction and is refused; so is a row past the capacity."""
        codes = torch.as_tensor(codes).detach().cpu()
        if codes.dim() == 1:
            codes = codes[None]
        nrm2 = torch.as_tensor(nrm2).detach().cpu().reshape(-1).to(torch.int64)
        r = int(codes.shape[0])
        if codes.dtype != torch.int8 or codes.dim() != 2 or codes.shape[1] != self.dim:
            raise ValueError(f"codes must be int8 [R, {self.dim}], got {codes.dtype} "
                             f"{tuple(codes.shape)}")
        label = torch.as_tensor(label).detach().cpu().reshape(-1).to(torch.int64)
        if label.numel() == 1:
            label = label.expand(r)
        if nrm2.numel() != r or label.numel() != r:
            raise ValueError(f"{r} rows of codes, {nrm2.numel()} of nrm2, {label.numel()} labels")
        if not torch.equal(nrm2, (codes.long() ** 2).sum(1)):
            raise ValueError("nrm2 is not the sum of the codes' squares")
        if bool((nrm2 == 0).any()):
            raise ValueError("a row with nrm2 == 0 cannot be enrolled")
        if bool((label < 0).any()) or bool((label >= 2 ** 31).any()):
            raise ValueError("labels are 0..2^31-1")
        lo = len(self)
        if lo + r > self.capacity:
            raise ValueError(f"the gallery holds {self.capacity} rows; {lo} enrolled, {r} more asked")
        self._codes[lo:lo + r] = codes
        self._nrm2[lo:lo + r] = nrm2.to(torch.int32)
        self._scale[lo:lo + r] = 1.0 / torch.sqrt(nrm2.to(torch.float32))
        self._label[lo:lo + r] = label.to(torch.int32)
        self._count[0] = lo + r
        self._upload(lo, lo + r)
        return self

    def remove(self, label: int) -> int:
        """Drop every row of ``label``, close the gaps (the order of the rest is kept) and lower
        ``count``; returns the number of rows dropped."""
        n = len(self)
        keep = torch.nonzero(self._label[:n] != int(label)).reshape(-1)
        k = int(keep.numel())
        if k == n:
            return 0
        for host in (self._codes, self._nrm2, self._scale, self._label):
            host[:k] = host[keep]
        self._scale[k:n] = 0.0
        self._label[k:n] = -1
        self._count[0] = k
        self._upload(0, n)
        return n - k

    def clear(self) -> "Gallery":
        n = len(self)
        self._scale[:n] = 0.0
        self._label[:n] = -1
        self._count[0] = 0
        self._upload(0, n)
        return self

    def save(self, path) -> None:
        """codes, nrm2 and labels of the enrolled rows as an ``.npz``."""
        import numpy as np
        n = len(self)
        with open(path, "wb") as f:
            np.savez(f, codes=self._codes[:n].numpy(), nrm2=self._nrm2[:n].numpy(),
                     labels=self._label[:n].numpy())

    @staticmethod
    def load(path, capacity: int = 0, device="cpu") -> "Gallery":
        """The gallery of an ``.npz`` written by :meth:`save`; ``capacity`` 0 = its rows (at
        least 1)."""
        import numpy as np
        with np.load(path) as z:
            codes, nrm2, labels = (torch.from_numpy(z[k].copy()) for k in ("codes", "nrm2", "labels"))
        if codes.dim() != 2 or codes.dtype != torch.int8:
            raise ValueError(f"{path}: codes must be int8 [R, dim]")
        g = Gallery(capacity or max(1, int(codes.shape[0])), int(codes.shape[1]), device)
        if codes.shape[0]:
            g.enrol(codes, nrm2, labels)
        return g


def gallery_match(q_codes: torch.Tensor, gallery: Gallery, top: int = 1,
                  out_score: Optional[torch.Tensor] = None,
                  out_row: Optional[torch.Tensor] = None):
    """The ``top`` (1..8) best rows of ``gallery`` for every query of ``q_codes`` int8 [M, dim]
    (M in 1..65535).  Returns ``(score, row)``: fp32 [M, top] = float32(integer dot product) *
    gallery.scale[row] and int32 [M, top], ordered by score descending, then row ascending;
    slots past the number of enrolled rows hold 0 / -1.  ``score * rsqrt(nrm2 of the query)``
    is the cosine.  The gallery's count is read on the device at run time.  Two launches, no
    host synchronisation, capturable (csrc/kernels/gallery.hip: i8 MFMA, the gallery is read
    once for M <= 256); GPU and CPU (ops.reference.gallery_match) are bit-identical."""
    if not isinstance(gallery, Gallery):
        raise TypeError(f"gallery must be an ops.Gallery, got {type(gallery).__name__}")
    if q_codes.dtype != torch.int8 or q_codes.dim() != 2 or not q_codes.is_contiguous():
        raise ValueError(f"q_codes must be contiguous int8 [M, D], got {q_codes.dtype} "
                         f"{tuple(q_codes.shape)}")
    m, d = int(q_codes.shape[0]), int(q_codes.shape[1])
    _check_embed_dim(d)
    if d != gallery.dim:
        raise ValueError(f"queries of width {d}, the gallery holds {gallery.dim}")
    if not 1 <= m <= GALLERY_MAX_QUERIES:
        raise ValueError(f"1..{GALLERY_MAX_QUERIES} queries, got {m}")
    if isinstance(top, bool) or not 1 <= int(top) <= GALLERY_MAX_TOP:
        raise ValueError(f"top {top!r} outside 1..{GALLERY_MAX_TOP}")
    if q_codes.device != gallery.device:
        raise ValueError(f"q_codes on {q_codes.device}, the gallery on {gallery.device}")
    k, dev = int(top), q_codes.device
    if out_score is None:
        out_score = empty(m, k, dtype=torch.float32, device=dev)
    if out_row is None:
        out_row = empty(m, k, dtype=torch.int32, device=dev)
    _check_out("out_score", out_score, torch.float32, (m, k), dev)
    _check_out("out_row", out_row, torch.int32, (m, k), dev)
    if q_codes.is_cuda:
        # the workgroups' partial lists [M, workgroups, top] of (score, row): per call, so that
        # calls on different streams never share one
        part = empty(m * int(_native().gallery_workgroups(gallery.capacity)) * k * 2,
                     dtype=torch.int32, device=dev)
        _native().gallery_match(q_codes, gallery.codes, gallery.scale, gallery.count, part,
                                out_score, out_row)
    else:
        _ref.gallery_match(q_codes, gallery.codes, gallery.scale, gallery.count, out_score,
                           out_row)
    return out_score, out_row


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
# MJPEG camera sources: baseline JPEG files decoded on the device
# ---------------------------------------------------------------------------
JPEG_DECODE_ERRORS = _ref.JPEG_DECODE_ERRORS
JPEG_DECODE_TABLE_BYTES = 6256  # sizeof(JdTables), csrc/kernels/jpeg_decode_core.h
JPEG_DECODE_LANES = (16, 32, 64)
JPEG_DECODE_ENTROPY = ("serial", "auto", "parallel")  # the native op's mode 0 / 1 / 2
# S: a long restart interval is cut at the row's multiples of S into one lane each
# (kJdSplitBytes, csrc/kernels/jpeg_decode_core.h).  "parallel" splits intervals longer than S,
# "auto" those longer than 16 S (kJdAutoSplitBytes: the measured crossover, docs/kernels.md K29).
JPEG_DECODE_SPLIT_BYTES = 64


def jpeg_row_bytes(hw) -> int:
    """Default size of a compressed-frame row: H * W // 2 rounded up to 16 (a third of the
    NV12 frame; camera JPEGs are near a tenth of it)."""
    return max(16, -(-(int(hw[0]) * int(hw[1]) // 2) // 16) * 16)


class JpegDecoder:
    """Everything :func:`jpeg_decode` needs outside the caller's tensors, for ``streams``
    files of ``hw`` = (H, W) pixels in rows of ``row_bytes`` bytes (a multiple of 16), all in
    device memory: ``tables`` uint8 [streams, 6256] (per file: scan geometry, error bits, its
    quantisation and Huffman tables), ``mpos`` int32 [streams, ceil(H / 8) * ceil(W / 8)]
    (offsets of the restart markers; the worst case is 4:4:4 with one MCU per interval),
    ``planes`` uint8 [streams, 3, H16, W16] (the Y / Cb / Cr samples before upsampling, H16 /
    W16 = H / W rounded up to 16) and ``status`` int32 [streams].  The op allocates nothing.
    ``lanes``: restart intervals per wavefront of the decode launch (16, 32 or 64); fewer
    lanes give more wavefronts when streams x intervals is small.

    ``entropy``: who decodes a long restart interval (a file without restart markers is one).
    ``"serial"``: one lane, as every short interval; ``"parallel"``: one lane per
    JPEG_DECODE_SPLIT_BYTES of every interval longer than that; ``"auto"``: of every interval
    longer than sixteen times that; fixed when the decoder is made.  The split launches keep their
    lanes in ``split`` int32 [streams, 16 + 10 * L] with L = 3 * (row_bytes //
    JPEG_DECODE_SPLIT_BYTES) + 3 lanes (the size is the native library's; header: lanes in use,
    most synchronisation rounds of a workgroup, seam rounds, seam passes, then 12 counts of
    workgroups by their synchronisation rounds, 11 and more in the last), mark
    every interval in ``done`` int32 [streams, like mpos] (0 left to the serial walk, 1 completed,
    2 handed back to it) and count them in ``paths`` int32 [streams, 2] = (completed, handed
    back).  The CPU reference ignores ``entropy``; ``paths`` stays zero there and with
    ``"serial"``."""

    def __init__(self, streams: int, hw, row_bytes: Optional[int] = None, device="cpu",
                 lanes: int = 16, entropy: str = "auto"):
        h, w = int(hw[0]), int(hw[1])
        if not (1 <= h <= JPEG_MAX_EXTENT and 1 <= w <= JPEG_MAX_EXTENT):
            raise ValueError(f"JPEG image size {h}x{w} outside 1..{JPEG_MAX_EXTENT}")
        if isinstance(streams, bool) or not 1 <= int(streams) <= 65535:
            raise ValueError(f"streams must be in 1..65535, got {streams!r}")
        row_bytes = jpeg_row_bytes((h, w)) if row_bytes is None else int(row_bytes)
        if row_bytes < 16 or row_bytes % 16 or row_bytes > 0x7ffffff0:
            raise ValueError(f"row_bytes must be a multiple of 16 in 16..2^31-16, got {row_bytes}")
        if lanes not in JPEG_DECODE_LANES:
            raise ValueError(f"lanes must be one of {JPEG_DECODE_LANES}, got {lanes!r}")
        if entropy not in JPEG_DECODE_ENTROPY:
            raise ValueError(f"entropy must be one of {JPEG_DECODE_ENTROPY}, got {entropy!r}")
        self.streams, self.hw, self.row_bytes, self.lanes = int(streams), (h, w), row_bytes, lanes
        self._entropy = entropy
        dev = torch.device(device)
        self.status = torch.zeros(self.streams, dtype=torch.int32, device=dev)
        self.paths = torch.zeros(self.streams, 2, dtype=torch.int32, device=dev)
        self.split = self.done = None
        if dev.type == "cuda":
            h16, w16 = -(-h // 16) * 16, -(-w // 16) * 16
            self.tables = torch.zeros(self.streams, JPEG_DECODE_TABLE_BYTES, dtype=torch.uint8,
                                      device=dev)
            self.mpos = torch.zeros(self.streams, -(-h // 8) * -(-w // 8), dtype=torch.int32,
                                    device=dev)
            self.planes = torch.zeros(self.streams, 3, h16, w16, dtype=torch.uint8, device=dev)
            if entropy != "serial":
                self.split = torch.zeros(self.streams,
                                         _native().jpeg_decode_split_ints(row_bytes),
                                         dtype=torch.int32, device=dev)
                self.done = torch.zeros_like(self.mpos)
        else:
            self.tables = self.mpos = self.planes = None  # the reference needs none

    @property
    def device(self) -> torch.device:
        return self.status.device

    @property
    def entropy(self) -> str:
        return self._entropy


def jpeg_decode(files: torch.Tensor, dec: JpegDecoder, out: Optional[torch.Tensor] = None,
                slot0: int = 0):
    """Baseline JPEG ``files`` uint8 [N, dec.row_bytes] (one file per row from SOI, bytes after
    EOI ignored) -> ``(rgb, status)``: ``rgb`` uint8 [N, H, W, 3] is ``out`` or new, ``status``
    int32 [N] is rows ``slot0 .. slot0 + N`` of ``dec.status``: 0, or minus the sum of the
    JPEG_DECODE_ERRORS bits.  A header error (unsupported form, wrong size, missing table,
    truncated header) zero-fills the image; an entropy error zeroes the rest of its restart
    interval.  What is accepted and every rule is written out at ops.reference.jpeg_decode; GPU
    and CPU agree byte for byte, status and malformed files included.  Three launches on the
    current stream (csrc/kernels/jpeg_decode.hip), seven unless ``dec.entropy`` is "serial" (the
    split launches for long restart intervals, which also write ``dec.paths``); no allocation
    when ``out`` is given, no host synchronisation, capturable.  File n works in row
    ``slot0 + n`` of the decoder's scratch."""
    if not isinstance(dec, JpegDecoder):
        raise TypeError(f"dec must be an ops.JpegDecoder, got {type(dec).__name__}")
    if (files.dtype != torch.uint8 or files.dim() != 2 or files.shape[1] != dec.row_bytes
            or not files.is_contiguous()):
        raise ValueError(f"files are contiguous uint8 [N, {dec.row_bytes}], got {files.dtype} "
                         f"{tuple(files.shape)}")
    n, slot0 = int(files.shape[0]), int(slot0)
    if slot0 < 0 or slot0 + n > dec.streams:
        raise ValueError(f"files [{slot0}, {slot0 + n}) outside the {dec.streams} the decoder "
                         f"was made for")
    if files.device != dec.device:
        raise ValueError(f"files on {files.device}, decoder on {dec.device}")
    if files.data_ptr() % 16:
        raise ValueError("files must be 16-byte aligned")
    h, w = dec.hw
    if out is None:
        out = empty(n, h, w, 3, dtype=torch.uint8, device=files.device)
    if (out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous()
            or out.device != files.device):
        raise ValueError(f"out must be contiguous uint8 [{n}, {h}, {w}, 3] on {files.device}")
    rows = slice(slot0, slot0 + n)
    status = dec.status[rows]
    if files.is_cuda and dec.entropy != "serial":
        _native().jpeg_decode_split(files, dec.tables[rows], dec.mpos[rows], dec.planes[rows],
                                    out, status, dec.split[rows], dec.done[rows], dec.paths[rows],
                                    dec.lanes, JPEG_DECODE_ENTROPY.index(dec.entropy), 7)
    elif files.is_cuda:
        _native().jpeg_decode(files, dec.tables[rows], dec.mpos[rows], dec.planes[rows], out,
                              status, dec.lanes)
    else:
        rgb, st = _ref.jpeg_decode(files, dec.hw)
        out.copy_(torch.from_numpy(rgb))
        status.copy_(torch.from_numpy(st))
    return out, status


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
