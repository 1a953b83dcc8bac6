"""YOLOv8n detection model (ultralytics yolov8.yaml, scale n) — reference + deployed forms.

BASELINE.json config 4 ("YOLOv8n detection edge module, conv + NMS CDNA4 HIP kernels").
Architecture facts (depth 0.33, width 0.25, max 1024 ch, 80 classes, reg_max 16) are
public model facts; no ultralytics code is used (the package is not installed and
there is no network).  Weights are random-init, seeded; the Detect head biases use
the usual prior (box 1.0, cls log(5/nc/(640/s)^2)) so random nets give sparse,
realistic candidate counts for NMS.

Deployed forward is CONCAT-FREE: every Concat / C2f split of the graph is a channel
slice of one NHWC buffer; producers write their slice directly (conv y_coff, upsample
y_coff) and consumers read slices (x_coff).  The two Detect branch stems that read
the same level feature are merged into one conv (Cout 64+80).  Hot path kernels:
K2/K3 convs with SiLU epilogue, K5b SPPF (3 pools in one pass), K8 upsample, K9
decode, K10 NMS.
"""
from __future__ import annotations

import os

import math
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .layers import DeployedConv, _record, _recorder_active, calibrate_bn, count_flops

ACT_SILU, ACT_NONE = ops.ACT_SILU, ops.ACT_NONE
NC = 80
REG_MAX = 16
STRIDES = (8, 16, 32)


# ---------------------------------------------------------------------------
# reference modules (NCHW fp32)
# ---------------------------------------------------------------------------
class Conv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, k // 2, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)

    def forward(self, x):
        return F.silu(self.bn(self.conv(x)))


class Bottleneck(nn.Module):
    def __init__(self, c1, c2, shortcut=True):
        super().__init__()
        self.cv1 = Conv(c1, c2, 3)
        self.cv2 = Conv(c2, c2, 3)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        y = self.cv2(self.cv1(x))
        return x + y if self.add else y


class C2f(nn.Module):
    def __init__(self, c1, c2, n=1, shortcut=False):
        super().__init__()
        self.c = c2 // 2
        self.cv1 = Conv(c1, 2 * self.c, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        for m in self.m:
            y.append(m(y[-1]))
        return self.cv2(torch.cat(y, 1))


class SPPF(nn.Module):
    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1)
        self.cv2 = Conv(c_ * 4, c2, 1)
        self.k = k

    def forward(self, x):
        y = [self.cv1(x)]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], self.k, 1, self.k // 2))
        return self.cv2(torch.cat(y, 1))


class Detect(nn.Module):
    def __init__(self, nc=NC, ch=(64, 128, 256)):
        super().__init__()
        self.nc = nc
        c2 = max(16, ch[0] // 4, REG_MAX * 4)
        c3 = max(ch[0], min(nc, 100))
        self.cv2 = nn.ModuleList(
            nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * REG_MAX, 1))
            for x in ch)
        self.cv3 = nn.ModuleList(
            nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, nc, 1)) for x in ch)

    def bias_init(self):
        for a, b, s in zip(self.cv2, self.cv3, STRIDES):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[:self.nc] = math.log(5 / self.nc / (640 / s) ** 2)

    def forward(self, feats):
        return [torch.cat([self.cv2[i](f), self.cv3[i](f)], 1) for i, f in enumerate(feats)]


class YoloV8nRef(nn.Module):
    """Returns the three raw Detect outputs [N, 64+nc, h, w] (strides 8/16/32)."""

    def __init__(self, nc=NC):
        super().__init__()
        self.nc = nc
        self.b0 = Conv(3, 16, 3, 2)
        self.b1 = Conv(16, 32, 3, 2)
        self.b2 = C2f(32, 32, 1, True)
        self.b3 = Conv(32, 64, 3, 2)
        self.b4 = C2f(64, 64, 2, True)
        self.b5 = Conv(64, 128, 3, 2)
        self.b6 = C2f(128, 128, 2, True)
        self.b7 = Conv(128, 256, 3, 2)
        self.b8 = C2f(256, 256, 1, True)
        self.b9 = SPPF(256, 256, 5)
        self.h12 = C2f(384, 128, 1, False)
        self.h15 = C2f(192, 64, 1, False)
        self.h16 = Conv(64, 64, 3, 2)
        self.h18 = C2f(192, 128, 1, False)
        self.h19 = Conv(128, 128, 3, 2)
        self.h21 = C2f(384, 256, 1, False)
        self.detect = Detect(nc, (64, 128, 256))

    def forward(self, x):
        x = self.b1(self.b0(x))
        x = self.b2(x)
        p3b = self.b4(self.b3(x))
        p4b = self.b6(self.b5(p3b))
        p5b = self.b9(self.b8(self.b7(p4b)))
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
        h12 = self.h12(torch.cat([up(p5b), p4b], 1))
        p3 = self.h15(torch.cat([up(h12), p3b], 1))
        p4 = self.h18(torch.cat([self.h16(p3), h12], 1))
        p5 = self.h21(torch.cat([self.h19(p4), p5b], 1))
        return self.detect([p3, p4, p5])


def init_yolov8n(seed: int = 0, calibrate: bool = True, calib_batch: int = 2,
                 calib_hw: int = 320) -> YoloV8nRef:
    torch.manual_seed(seed)
    m = YoloV8nRef()
    m.detect.bias_init()
    if calibrate:
        g = torch.Generator().manual_seed(seed)
        fr = torch.randint(0, 256, (calib_batch, calib_hw, calib_hw, 3), generator=g,
                           dtype=torch.uint8)
        calibrate_bn(m, [fr.float().permute(0, 3, 1, 2) / 255.0])
    m.eval()
    return m


def frames_to_yolo(frames_u8: torch.Tensor) -> torch.Tensor:
    return (frames_u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------
# deployed (NHWC bf16, concat-free)
# ---------------------------------------------------------------------------
def _dc(m: Conv, device) -> DeployedConv:
    return DeployedConv.from_modules(m.conv, m.bn, ACT_SILU, device)


class DeployedUpDual:
    """A neck C2f's cv1 over [upsample2x(low) | skip] as ONE dual-source GEMM (ops.conv_dual2,
    up2): the skip tensor is read at full resolution, the low-resolution map at (h / 2, w / 2)
    -- no upsample launch, and the concat's upsampled half is never written or read.  The
    packed weight's columns are permuted to [skip | upsampled]."""

    def __init__(self, cv1: DeployedConv, c_up: int):
        w = cv1.w[:, :cv1.spec.K]
        self.c_up, self.c_skip = c_up, cv1.spec.K - c_up
        self.w = torch.cat([w[:, c_up:], w[:, :c_up]], 1).contiguous()
        self.b = cv1.b
        self.act = cv1.spec.act
        self.tile = -1

    def __call__(self, skip, skip_coff, low, low_coff, out, y_coff=0, tile=None):
        ops.conv_dual2(skip, self.c_skip, low, self.w, self.b, self.act, out, x_coff=skip_coff,
                       x2_coff=low_coff, y_coff=y_coff, up2=True,
                       tile=self.tile if tile is None else tile)
        if _recorder_active():
            key = ("dual_up", tuple(skip.shape), skip_coff, tuple(low.shape), low_coff,
                   tuple(out.shape), y_coff, tuple(self.w.shape))
            fn = lambda t, o=out: ops.conv_dual2(  # noqa: E731
                skip, self.c_skip, low, self.w, self.b, self.act, o, x_coff=skip_coff,
                x2_coff=low_coff, y_coff=y_coff, up2=True, tile=t)
            _record(self, key, fn)
        return out


class DC2f:
    def __init__(self, m: C2f, device):
        self.c = m.c
        self.n = len(m.m)
        self.cv1 = _dc(m.cv1, device)
        self.cv2 = _dc(m.cv2, device)
        self.m = []
        for b in m.m:
            c2 = _dc(b.cv2, device)
            if b.add:  # x + SiLU(bn(conv)): residual after the activation
                c2.spec.act |= ops.RES_AFTER_ACT
            self.m.append((_dc(b.cv1, device), c2, b.add))

    def fused_ok(self, x) -> bool:
        """The whole block as ONE v13 launch (ops.c2f16): C2f(32, 32, n=1, shortcut) -- the
        b2 block at 160 x 160 -- on the GPU."""
        N, H, W, _ = x.shape
        return (ops.C2F_ENABLED and x.is_cuda and self.c == 16 and self.n == 1 and
                self.m[0][2] and self.cv1.spec.cin == 32 and self.cv2.spec.cout == 32 and
                ops.c2f16_strip(H, W) > 0)

    def up_call(self, skip, skip_coff, low, low_coff, c_up, out=None, y_coff=0):
        """The block over [upsample2x(low[..., low_coff : + c_up]) | skip[..., skip_coff :]]
        with cv1 as one dual-source GEMM (DeployedUpDual): same result as writing the
        upsampled map into the concat and calling the block on it."""
        if getattr(self, "_up", None) is None:
            self._up = DeployedUpDual(self.cv1, c_up)
        N, H, W, _ = skip.shape
        c, n = self.c, self.n
        cat = ops.empty(N, H, W, (2 + n) * c, dtype=torch.bfloat16, device=skip.device)
        self._up(skip, skip_coff, low, low_coff, cat, 0)
        return self._rest(cat, out, y_coff)

    def _rest(self, cat, out, y_coff):
        c = self.c
        for i, (b1, b2, add) in enumerate(self.m):
            t = b1(cat, x_coff=(1 + i) * c)
            b2(t, res=cat if add else None, r_coff=(1 + i) * c, out=cat, y_coff=(2 + i) * c)
        return self.cv2(cat, out=out, y_coff=y_coff)

    def __call__(self, x, x_coff=0, out=None, y_coff=0):
        N, H, W, _ = x.shape
        c, n = self.c, self.n
        if self.fused_ok(x):
            b1, b2, _ = self.m[0]
            return ops.c2f16(x, self.cv1.w, self.cv1.b, b1.w, b1.b, b2.w, b2.b, self.cv2.w,
                             self.cv2.b, out=out, x_coff=x_coff, y_coff=y_coff)
        cat = ops.empty(N, H, W, (2 + n) * c, dtype=torch.bfloat16, device=x.device)
        self.cv1(x, x_coff=x_coff, out=cat, y_coff=0)
        return self._rest(cat, out, y_coff)

    def convs(self):
        out = [self.cv1, self.cv2]
        for b1, b2, _ in self.m:
            out += [b1, b2]
        return out


class DSPPF:
    def __init__(self, m: SPPF, device):
        self.cv1 = _dc(m.cv1, device)
        self.cv2 = _dc(m.cv2, device)
        self.c_ = m.cv1.conv.out_channels

    def __call__(self, x, out=None, y_coff=0):
        N, H, W, _ = x.shape
        buf = ops.empty(N, H, W, 4 * self.c_, dtype=torch.bfloat16, device=x.device)
        self.cv1(x, out=buf, y_coff=0)
        ops.sppf_pool(buf, self.c_)
        return self.cv2(buf, out=out, y_coff=y_coff)

    def convs(self):
        return [self.cv1, self.cv2]


class DeployedPair:
    """A Detect branch's 3x3 (+SiLU) and 1x1 convs run as ONE kernel (ops.conv_pair): the
    3x3's output never leaves the chip.  ``tile`` = v4 direct tile (autotuned)."""

    # (Cin, Cout, C2) shapes with a direct pair instantiation (csrc/kernels/conv_direct.hip)
    SHAPES = {(64, 64, 64), (80, 80, 80)}

    def __init__(self, c1: DeployedConv, c2: DeployedConv):
        self.c1, self.c2 = c1, c2
        s1, s2 = c1.spec, c2.spec
        self.fits = (s1.kh == 3 and s1.stride == 1 and s1.act == ACT_SILU and s2.kh == 1 and
                     s2.act == ACT_NONE and (s1.cin, s1.cout, s2.cout) in self.SHAPES)
        # the 1x1's packed weight without its K padding: [C2, Cout]
        self.w2 = c2.w[:, :s1.cout].contiguous()
        self.tile = 1  # DMA form

    def __call__(self, x, out, x_coff=0, z_coff=0, tile=None):
        ops.conv_pair(x, self.c1.spec, self.c1.w, self.c1.b, self.w2, self.c2.b, out,
                      x_coff=x_coff, z_coff=z_coff, tile=self.tile if tile is None else tile)
        if _recorder_active():
            s = self.c1.spec
            key = ("pair", s.cin, s.cout, self.w2.shape[0], tuple(x.shape), x_coff,
                   tuple(out.shape), z_coff)
            fn = lambda t, o=out: ops.conv_pair(x, s, self.c1.w, self.c1.b, self.w2,  # noqa: E731
                                                self.c2.b, o, x_coff=x_coff, z_coff=z_coff,
                                                tile=t)
            _record(self, key, fn)
        return out


class DDetectLevel:
    """One Detect level: merged branch stems (64 box + 80 cls) -> two 3x3 -> two 1x1
    heads writing [box 64 | cls 80] slices of one [N,h,w,144] buffer."""

    def __init__(self, d: Detect, i: int, device):
        a, b = d.cv2[i], d.cv3[i]
        wa, ba = _fold(a[0])
        wb, bb = _fold(b[0])
        merged = nn.Conv2d(wa.shape[1], wa.shape[0] + wb.shape[0], 3, 1, 1, bias=True)
        with torch.no_grad():
            merged.weight.copy_(torch.cat([wa, wb], 0))
            merged.bias.copy_(torch.cat([ba, bb], 0))
        self.stem = DeployedConv.from_modules(merged, None, ACT_SILU, device)
        self.ca = wa.shape[0]
        self.a1 = _dc(a[1], device)
        self.b1 = _dc(b[1], device)
        self.a2 = DeployedConv.from_modules(a[2], None, ACT_NONE, device)
        self.b2 = DeployedConv.from_modules(b[2], None, ACT_NONE, device)
        self.nc = d.nc
        # fused branch pairs (3x3 + SiLU -> 1x1 into the head map, the 3x3 output kept on
        # chip: ops.conv_pair) where a v4 direct pair form exists; KVEDGE_YOLO_PAIR=0 = A/B off
        self.pairs = [DeployedPair(self.a1, self.a2), DeployedPair(self.b1, self.b2)]

    fuse_pairs: bool = os.environ.get("KVEDGE_YOLO_PAIR", "1") != "0"

    def __call__(self, p):
        N, h, w, _ = p.shape
        s = self.stem(p)
        feat = ops.empty(N, h, w, 4 * REG_MAX + self.nc, dtype=torch.bfloat16, device=p.device)
        for pair, xo, zo in ((self.pairs[0], 0, 0), (self.pairs[1], self.ca, 4 * REG_MAX)):
            if self.fuse_pairs and p.is_cuda and pair.fits:
                pair(s, feat, x_coff=xo, z_coff=zo)
            else:
                pair.c2(pair.c1(s, x_coff=xo), out=feat, y_coff=zo)
        return feat

    def convs(self):
        return [self.stem, self.a1, self.b1, self.a2, self.b2]


def _fold(m: Conv):
    from .layers import fold_bn

    return fold_bn(m.conv, m.bn)


class KvYoloV8n:
    """Deployed YOLOv8n: frames u8 [N,640,640,3] -> (dets fp32 [N,300,6], count int32 [N])."""

    image_size = 640

    def __init__(self, ref: YoloV8nRef, device="cuda", conf=0.25, iou=0.7, max_det=300):
        self.device = torch.device(device)
        self.nc = ref.nc
        self.conf, self.iou, self.max_det = conf, iou, max_det
        d = self.device
        self.b0 = DeployedConv.stem_s2d(ref.b0.conv, ref.b0.bn, ACT_SILU, d)  # K12b s2d stem
        # the same stem reading raw frames (preprocess fused into the conv, GPU path)
        self.b0_frames = DeployedConv.stem_s2d(ref.b0.conv, ref.b0.bn, ACT_SILU, d,
                                               in_scale=1.0 / 255)
        self.b1, self.b3, self.b5, self.b7 = (_dc(m, d) for m in (ref.b1, ref.b3, ref.b5, ref.b7))
        self._ref = ref
        self._flops = {}
        self.b2, self.b4, self.b6, self.b8 = (DC2f(m, d) for m in (ref.b2, ref.b4, ref.b6, ref.b8))
        self.b9 = DSPPF(ref.b9, d)
        self.h12, self.h15, self.h18, self.h21 = (DC2f(m, d) for m in
                                                  (ref.h12, ref.h15, ref.h18, ref.h21))
        self.h16, self.h19 = _dc(ref.h16, d), _dc(ref.h19, d)
        self.levels = [DDetectLevel(ref.detect, i, d) for i in range(3)]

    @staticmethod
    def build(seed: int = 0, device="cuda", calibrate: bool = True) -> "KvYoloV8n":
        return KvYoloV8n(init_yolov8n(seed, calibrate=calibrate), device)

    def convs(self) -> List[DeployedConv]:
        out = [self.b0, self.b0_frames, self.b1, self.b3, self.b5, self.b7, self.h16, self.h19]
        for m in (self.b2, self.b4, self.b6, self.b8, self.b9, self.h12, self.h15, self.h18,
                  self.h21):
            out += m.convs()
        for lv in self.levels:
            out += lv.convs()
        return out

    def flops_per_image(self, hw: int = 640) -> int:
        """Model FLOPs (2*MAC of all convs) of the reference architecture."""
        if hw not in self._flops:
            self._flops[hw] = count_flops(self._ref, (1, 3, hw, hw))
        return self._flops[hw]

    def frame_plan(self, src_hw, image_size: int = 0) -> "ops.ResizePlan":
        """Native-resolution frames [Hs, Ws] -> the model's square input: letterbox (pad 114,
        the Ultralytics convention).  ``image_size``: 0 = the model's own."""
        return ops.letterbox_plan(src_hw, image_size or self.image_size)

    def to_source(self, outputs, plan: "ops.ResizePlan"):
        """(det, count) in model coordinates -> the same tensors with the kept boxes in
        source-frame pixels (in place, ops.det_to_source)."""
        det, count = outputs
        ops.det_to_source(det, count, plan)
        return det, count

    def preprocess(self, frames_u8: torch.Tensor) -> torch.Tensor:
        return ops.preprocess(frames_u8, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), s2d=True)

    fuse_preprocess: bool = True  # GPU: frames -> b0 output in one kernel

    def stem(self, frames_u8: torch.Tensor) -> torch.Tensor:
        """uint8 frames -> b0 output [N,320,320,16]."""
        if self.fuse_preprocess and frames_u8.is_cuda:
            b = self.b0_frames
            return ops.stem_from_frames(frames_u8, b.spec, b.w, b.b)
        return self.b0(self.preprocess(frames_u8))

    # GPU: frames -> b1 output in one kernel (b0 never leaves LDS); KVEDGE_YOLO_FUSE_B1=0 = A/B off
    fuse_b1: bool = os.environ.get("KVEDGE_YOLO_FUSE_B1", "1") != "0"

    def stem_b1(self, frames_u8: torch.Tensor) -> torch.Tensor:
        """uint8 frames -> b1 output [N,160,160,32]: the fused b0 + b1 kernel
        (csrc/kernels/yolo_stem2.hip) where the shape allows, else stem() then b1."""
        if self.fuse_b1 and frames_u8.is_cuda and ops.yolo_stem2_fits(frames_u8.shape):
            b0, b1 = self.b0_frames, self.b1
            return ops.yolo_stem2(frames_u8, b0.spec, b0.w, b0.b, b1.spec, b1.w, b1.b)
        return self.b1(self.stem(frames_u8))

    # GPU: the neck's two upsample + concat steps folded into h12 / h15's cv1
    # (DeployedUpDual); KVEDGE_YOLO_FUSE_UP=0 = A/B off
    fuse_up: bool = os.environ.get("KVEDGE_YOLO_FUSE_UP", "1") != "0"

    def heads(self, x: torch.Tensor, stem_done: bool = False, b1_done: bool = False):
        """x: preprocessed bf16 s2d [N,320,320,16] (or, with stem_done, the b0 output; with
        b1_done, the b1 output) -> three [N,h,w,144] head outputs."""
        N = x.shape[0]
        dev = x.device
        bf = torch.bfloat16
        if not b1_done:
            x = self.b1(x if stem_done else self.b0(x))  # [N,160,160,32]
        x = self.b2(x)
        x = self.b3(x)                                # [N,80,80,64]
        H3 = x.shape[1]
        H4, H5 = H3 // 2, H3 // 4
        cat14 = ops.empty(N, H3, H3, 192, dtype=bf, device=dev)   # [up(h12) 128 | p3b 64]
        cat11 = ops.empty(N, H4, H4, 384, dtype=bf, device=dev)   # [up(p5b) 256 | p4b 128]
        cat17 = ops.empty(N, H4, H4, 192, dtype=bf, device=dev)   # [h16 64 | h12 128]
        cat20 = ops.empty(N, H5, H5, 384, dtype=bf, device=dev)   # [h19 128 | p5b 256]
        self.b4(x, out=cat14, y_coff=128)                          # p3b
        x = self.b5(cat14, x_coff=128)                             # [N,40,40,128]
        self.b6(x, out=cat11, y_coff=256)                          # p4b
        x = self.b7(cat11, x_coff=256)                             # [N,20,20,256]
        x = self.b8(x)
        self.b9(x, out=cat20, y_coff=128)                          # p5b
        if self.fuse_up and dev.type == "cuda":
            # the upsampled halves of cat11 / cat14 are never written: h12 / h15 read p5b and
            # h12 at half resolution inside their cv1 GEMM (DeployedUpDual)
            self.h12.up_call(cat11, 256, cat20, 128, 256, out=cat17, y_coff=64)     # h12
            p3 = self.h15.up_call(cat14, 128, cat17, 64, 128)                     # [N,80,80,64]
        else:
            ops.upsample2x(cat20, cat11, C=256, x_coff=128, y_coff=0)
            self.h12(cat11, out=cat17, y_coff=64)                      # h12
            ops.upsample2x(cat17, cat14, C=128, x_coff=64, y_coff=0)
            p3 = self.h15(cat14)                                       # [N,80,80,64]
        self.h16(p3, out=cat17, y_coff=0)
        p4 = self.h18(cat17)                                       # [N,40,40,128]
        self.h19(p4, out=cat20, y_coff=0)
        p5 = self.h21(cat20)                                       # [N,20,20,256]
        return [lv(p) for lv, p in zip(self.levels, (p3, p4, p5))]

    def raw_outputs(self, frames_u8: torch.Tensor) -> torch.Tensor:
        """uint8 frames -> the three Detect head maps flattened and concatenated
        [N, 8400*144] (pre-decode, pre-NMS): what the C4 replica check hashes."""
        feats = self.heads(self.stem_b1(frames_u8), b1_done=True)
        N = frames_u8.shape[0]
        return torch.cat([f.reshape(N, -1) for f in feats], dim=1)

    # tests: a list here collects every call's three head maps.  Maps made during a hipGraph
    # capture live in the graph's pool and hold each replay's values, so a parity test can
    # read the GRAPH's own head maps instead of an eager re-run
    keep_heads = None

    def __call__(self, frames_u8: torch.Tensor):
        feats = self.heads(self.stem_b1(frames_u8), b1_done=True)
        if self.keep_heads is not None:
            self.keep_heads.append(feats)
        boxes, scores, cls = ops.yolo_decode(feats, STRIDES, self.nc)
        return ops.nms(boxes, scores, cls, self.conf, self.iou, self.max_det)
