"""Plain-PyTorch fp32 reference of every kvedge kernel (CPU path + numerics oracle).

Semantics mirror csrc/kernels/*.hip exactly (layouts, channel slices, padding,
tie-breaking) so GPU kernel tests can compare against these on the same inputs.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2


def _act(y: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return y.clamp_min(0)
    if act == ACT_SILU:
        return y * torch.sigmoid(y)
    return y


def conv2d(x, spec, w, bias, res, out, x_coff=0, y_coff=0, r_coff=0):
    from . import unpack_conv_weight, MODE_STEM

    xin = x[..., x_coff:x_coff + spec.cin_eff].float()
    if spec.mode == MODE_STEM:
        xin = xin[..., :spec.cin]
    wt = unpack_conv_weight(w, spec).to(xin.device)
    xp = F.pad(xin.permute(0, 3, 1, 2), (spec.pad, spec.pad_end, spec.pad, spec.pad_end))
    y = F.conv2d(xp, wt, None, spec.stride, 0).permute(0, 2, 3, 1)
    if bias is not None:
        y = y + bias.float()
    act, post = spec.act & 3, bool(spec.act & 4)
    if res is not None and not post:
        y = y + res[..., r_coff:r_coff + spec.cout].float()
    y = _act(y, act)
    if res is not None and post:
        y = y.to(out.dtype).float() + res[..., r_coff:r_coff + spec.cout].float()
    out[..., y_coff:y_coff + spec.cout] = y.to(out.dtype)
    return out


def maxpool2d(x, out, C, k, stride, pad, y_coff=0):
    xin = x[..., :C].float().permute(0, 3, 1, 2)
    y = F.max_pool2d(xin, k, stride, pad).permute(0, 2, 3, 1)
    out[..., y_coff:y_coff + C] = y.to(out.dtype)
    return out


def sppf_pool(buf, C):
    x = buf[..., :C].float().permute(0, 3, 1, 2)
    y1 = F.max_pool2d(x, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    y3 = F.max_pool2d(y2, 5, 1, 2)
    for i, y in enumerate((y1, y2, y3), start=1):
        buf[..., i * C:(i + 1) * C] = y.permute(0, 2, 3, 1).to(buf.dtype)
    return buf


def yolo_decode(feats, strides, nc, boxes, scores, cls):
    outs_b, outs_s, outs_c = [], [], []
    for f, s in zip(feats, strides):
        N, h, w, ch = f.shape
        ff = f.float().reshape(N, h * w, ch)
        box = ff[..., :64].reshape(N, h * w, 4, 16).softmax(-1)
        dist = (box * torch.arange(16, dtype=torch.float32, device=f.device)).sum(-1)
        ys, xs = torch.meshgrid(torch.arange(h, device=f.device), torch.arange(w, device=f.device),
                                indexing="ij")
        ax = xs.reshape(-1).float() + 0.5
        ay = ys.reshape(-1).float() + 0.5
        b = torch.stack([ax - dist[..., 0], ay - dist[..., 1], ax + dist[..., 2],
                         ay + dist[..., 3]], -1) * s
        logits = ff[..., 64:64 + nc]
        mx, arg = logits.max(-1)
        outs_b.append(b)
        outs_s.append(torch.sigmoid(mx))
        outs_c.append(arg.int())
    boxes.copy_(torch.cat(outs_b, 1))
    scores.copy_(torch.cat(outs_s, 1))
    cls.copy_(torch.cat(outs_c, 1))
    return boxes, scores, cls


def _iou(a, b):
    iw = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp_min(0)
    ih = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp_min(0)
    inter = iw * ih
    aa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    ab = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return inter / (aa + ab - inter).clamp_min(1e-9)


def nms(boxes, scores, cls, conf, iou, max_det, out, count, max_wh=7680.0):
    """Greedy class-aware NMS; order = score desc, index asc (same as the kernel)."""
    out.zero_()
    N, A = scores.shape
    for n in range(N):
        s = scores[n].float()
        idx = torch.nonzero(s > conf).flatten()
        if idx.numel() == 0:
            count[n] = 0
            continue
        order = sorted(idx.tolist(), key=lambda i: (-float(s[i]), i))
        order = torch.tensor(order, dtype=torch.long)
        b = boxes[n, order].float()
        c = cls[n, order].float()
        bo = b + (c * max_wh)[:, None]
        keep = []
        for i in range(order.numel()):
            if len(keep) >= max_det:
                break
            if keep:
                ious = _iou(bo[i][None], bo[torch.tensor(keep)])
                if bool((ious > iou).any()):
                    continue
            keep.append(i)
        for r, i in enumerate(keep):
            out[n, r, :4] = b[i]
            out[n, r, 4] = s[order[i]]
            out[n, r, 5] = c[i]
        count[n] = len(keep)
    return out, count


_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def synth_frames(out, seed, step):
    if isinstance(step, torch.Tensor):  # int64[1] counter, or [2]: counter + done-count slot
        st = int(step[0].item())
        step[0] += 1
    else:
        st = int(step)
    n8 = out.numel() // 8
    i = np.arange(n8, dtype=np.uint64)
    with np.errstate(over="ignore"):
        mix = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ (np.uint64(st) * np.uint64(0xD1B54A32D192ED03))
    h = _splitmix64(mix ^ i)
    out.copy_(torch.from_numpy(h.view(np.uint8).copy()).reshape(out.shape))
    return out


def preprocess(x, out, mean, std):
    xf = x.float() / 255.0
    m = torch.tensor(mean, dtype=torch.float32)
    s = torch.tensor(std, dtype=torch.float32)
    y = (xf - m) * (1.0 / s)
    y4 = torch.zeros(*y.shape[:3], 4, dtype=torch.float32)
    y4[..., :3] = y
    if out.shape[-1] == 16:  # space-to-depth: channel (dy*2+dx)*4 + c
        N, H, W, _ = y4.shape
        y4 = y4.view(N, H // 2, 2, W // 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(
            N, H // 2, W // 2, 16)
    out.copy_(y4.to(out.dtype))
    return out


def _resize_axis(axis, D):
    """Per destination index of one axis (S, R, off, c0, cn): content mask, the two source
    taps and the 11-bit weight of the second one -- the integer formulas of
    csrc/kernels/frame_resize.hip, in int64."""
    S, R, off, c0, cn = axis
    d = torch.arange(D, dtype=torch.int64)
    content = (d >= c0) & (d < c0 + cn)
    v = d - c0 + off
    num = (2 * v + 1) * S - R
    q = torch.div(num, 2 * R, rounding_mode="floor")
    r = num - q * (2 * R)
    w = torch.div(r * 2048 + R, 2 * R, rounding_mode="floor")
    w = torch.where((q < 0) | (q >= S - 1), torch.zeros_like(w), w)
    q = q.clamp(0, S - 1)  # (also keeps the taps of padding indices in range)
    return content, q, (q + 1).clamp(max=S - 1), w


def frame_resize(src, plan, out):
    """Fixed-point bilinear resample (half-pixel centres, no antialias) of uint8 frames
    [N, Hs, Ws, 3] into out [N, Hd, Wd, 3]; padding pixels are plan.pad."""
    Hd, Wd = plan.dst_hw
    cy, y0, y1, wy = _resize_axis(plan.axis_y, Hd)
    cx, x0, x1, wx = _resize_axis(plan.axis_x, Wd)
    top_rows, bot_rows = src[:, y0], src[:, y1]          # [N, Hd, Ws, 3] uint8
    a, b = top_rows[:, :, x0].long(), top_rows[:, :, x1].long()
    c, d = bot_rows[:, :, x0].long(), bot_rows[:, :, x1].long()
    wx = wx.view(1, 1, Wd, 1)
    wy = wy.view(1, Hd, 1, 1)
    top = a * (2048 - wx) + b * wx
    bot = c * (2048 - wx) + d * wx
    y = (top * (2048 - wy) + bot * wy + (1 << 21)) >> 22
    content = (cy.view(Hd, 1) & cx.view(1, Wd)).view(1, Hd, Wd, 1)
    out.copy_(torch.where(content, y, torch.full_like(y, plan.pad)).to(torch.uint8))
    return out


def nv12_to_rgb(src):
    """NV12 frames uint8 [N, Hs * 3 // 2, Ws] (Hs, Ws even; rows 0 .. Hs - 1 are Y, row
    Hs + (y >> 1) holds U at byte x & ~1 and V at (x & ~1) + 1 for pixel (y, x)) -> RGB uint8
    [N, Hs, Ws, 3]: integer BT.601 limited range with nearest-neighbour chroma, the integers
    of csrc/kernels/nv12.h (int32 arithmetic shift = floor)."""
    N, rows, Ws = src.shape
    Hs = rows * 2 // 3
    if Hs % 2 or Ws % 2 or Hs * 3 // 2 != rows:
        raise ValueError(f"NV12 frames are [N, Hs * 3 / 2, Ws] with even Hs and Ws, "
                         f"got {tuple(src.shape)}")
    c = 298 * (src[:, :Hs].to(torch.int32) - 16) + 128
    uv = src[:, Hs:].reshape(N, Hs // 2, Ws // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)  # [N, Hs, Ws, 2]
    d, e = uv[..., 0], uv[..., 1]
    rgb = torch.stack([c + 409 * e, c - 100 * d - 208 * e, c + 516 * d], dim=-1) >> 8
    return rgb.clamp_(0, 255).to(torch.uint8)


def det_to_source(det, count, box_map, Hs, Ws):
    """In place on rows < count[n]: x = clamp((x - cx) * sx, 0, Ws), y likewise (fp32)."""
    cy, sy, cx, sx = box_map
    N, max_det, _ = det.shape
    live = (torch.arange(max_det).view(1, max_det) < count.view(N, 1).long()).unsqueeze(-1)
    sub = torch.tensor([cx, cy, cx, cy], dtype=torch.float32)
    mul = torch.tensor([sx, sy, sx, sy], dtype=torch.float32)
    hi = torch.tensor([Ws, Hs, Ws, Hs], dtype=torch.float32)
    box = det[..., :4]
    new = torch.minimum(((box - sub) * mul).clamp_min(0.0), hi)
    det[..., :4] = torch.where(live, new, box)
    return det


def roi_windows(boxes, Hs, Ws):
    """Float boxes [..., >= 4] (x1, y1, x2, y2) -> integer windows [..., 4] (x0, y0, w, h):
    clamp in fp32 (NaN -> 0 first, as the kernel's fmaxf(NaN, 0)), floor / ceil, at least
    1 x 1 and always inside the Hs x Ws frame."""
    b = torch.nan_to_num(boxes[..., :4].float(), nan=0.0)
    lim = torch.tensor([Ws, Hs, Ws, Hs], dtype=torch.float32)
    b = torch.minimum(b.clamp_min(0.0), lim)
    x0 = b[..., 0].floor().long().clamp(max=Ws - 1)
    y0 = b[..., 1].floor().long().clamp(max=Hs - 1)
    xe = torch.maximum(b[..., 2].ceil().long(), x0 + 1).clamp(max=Ws)
    ye = torch.maximum(b[..., 3].ceil().long(), y0 + 1).clamp(max=Hs)
    return torch.stack([x0, y0, xe - x0, ye - y0], dim=-1)


def roi_crop(src, det, count, K, D, pad, out):
    """Crop n * K + k of out [N*K, D, D, 3]: the window of box row k of det[n] cut from
    src[n] and stretched to D x D by frame_resize; slots k >= count[n] are ``pad``."""
    from . import ResizePlan

    N, Hs, Ws, _ = src.shape
    max_det = det.shape[1]
    win = roi_windows(det, Hs, Ws)
    for n in range(N):
        valid = min(max(int(count[n]), 0), max_det)
        for k in range(K):
            crop = out[n * K + k:n * K + k + 1]
            if k >= valid:
                crop.fill_(pad)
                continue
            x0, y0, w, h = (int(v) for v in win[n, k])
            plan = ResizePlan((h, D, 0, 0, D), (w, D, 0, 0, D), pad, (h, w), (D, D))
            frame_resize(src[n:n + 1, y0:y0 + h, x0:x0 + w], plan, crop)
    return out


TRACK_Q_MAX = 16384  # quarter pixels: 4096 px, the largest frame the module accepts


def track_quantize(x):
    """fp32 coordinates -> quarter pixels, int64: q(x) = min(max(floor(x * 4 + 0.5), 0), 16384)
    in fp32 with NaN -> 0 (the kernel's fmaxf(NaN, 0)); x * 4 is exact."""
    v = torch.floor(x.float() * 4.0 + 0.5)
    v = torch.nan_to_num(v, nan=0.0, posinf=float(TRACK_Q_MAX), neginf=0.0)
    return v.clamp(0.0, float(TRACK_Q_MAX)).to(torch.int64)


def track_class(c):
    """fp32 class column of det -> int64 (clamped to 0..65535, NaN -> 0, truncated)."""
    v = torch.nan_to_num(c.float(), nan=0.0, posinf=65535.0, neginf=0.0)
    return v.clamp(0.0, 65535.0).to(torch.int64)


def _box_area(b):
    return (b[..., 2] - b[..., 0]).clamp_min(0) * (b[..., 3] - b[..., 1]).clamp_min(0)


def track_update(det, count, state, slot0, thr_q, max_age, min_hits, class_aware, out):
    """One IoU-tracker update: THE definition the HIP kernel (csrc/kernels/track.hip) equals
    bit for bit.  det fp32 [N, max_det, 6] / count int32 [N]: row n is the next frame of stream
    ``slot0 + n`` of ``state`` (an ops.TrackState on the CPU; its views are updated in place);
    out int32 [N, max_det] gets every row's track id.  Per stream, in this order:

    1. predict: slots live at entry (hits > 0): pred = clamp(box + vel * (age + 1), 0, 16384);
    2. associate: rows r < count in order (NMS orders them by score); a slot is a candidate when
       it was live at entry, is not claimed yet, has the row's class (``class_aware``),
       inter > 0 and inter * 1024 >= thr_q * union (int64, no divide); the best is the largest
       inter / union by cross-multiplication, the lower slot on equality.  Match:
       vel = trunc((q(det) - box) / (age + 1)), box = q(det), age = 0, hits += 1, cls = row's;
       an unconfirmed track (id < 0) with hits >= min_hits gets id = next_id++;
    3. age: live at entry and unclaimed: age += 1; freed (all zero, id -1) when age > max_age
       or while still unconfirmed;
    4. birth: unmatched rows in order take the lowest free slot (box = q(det), vel 0, age 0,
       hits 1; id = next_id++ only when min_hits <= 1); none free: id -1, dropped += 1;
    5. out[n, r] = -1 for r >= count[n] (count clamped to 0..max_det)."""
    N, max_det, _ = det.shape
    i32 = torch.int32
    for n in range(N):
        s = slot0 + n
        box, vel = state.box[s].long(), state.vel[s].long()
        cls, tid = state.cls[s].long(), state.id[s].long()
        age, hits = state.age[s].long(), state.hits[s].long()
        next_id, dropped = int(state.next_id[s]), int(state.dropped[s])
        cnt = min(max(int(count[n]), 0), max_det)
        dq = track_quantize(det[n, :cnt, :4])
        dc = track_class(det[n, :cnt, 5])
        live = hits > 0
        pred = (box + vel * (age + 1).unsqueeze(1)).clamp(0, TRACK_Q_MAX)
        parea = _box_area(pred)
        claimed = torch.zeros_like(live)
        ids = torch.full((max_det,), -1, dtype=torch.int64)
        unmatched = []
        for r in range(cnt):
            d = dq[r]
            iw = (torch.minimum(pred[:, 2], d[2]) - torch.maximum(pred[:, 0], d[0])).clamp_min(0)
            ih = (torch.minimum(pred[:, 3], d[3]) - torch.maximum(pred[:, 1], d[1])).clamp_min(0)
            inter = iw * ih
            union = parea + _box_area(d) - inter
            cand = live & ~claimed & (inter > 0) & (inter * 1024 >= thr_q * union)
            if class_aware:
                cand &= cls == dc[r]
            idx = cand.nonzero().flatten()
            if idx.numel() == 0:
                unmatched.append(r)
                continue
            ci, cu = inter[idx], union[idx]
            # beaten[i]: some candidate j has inter_j / union_j > inter_i / union_i
            beaten = (ci.view(1, -1) * cu.view(-1, 1) > ci.view(-1, 1) * cu.view(1, -1)).any(1)
            m = int(idx[(~beaten).nonzero()[0, 0]])  # lowest slot among the best
            vel[m] = torch.div(d - box[m], age[m] + 1, rounding_mode="trunc")
            box[m] = d
            age[m] = 0
            hits[m] += 1
            cls[m] = dc[r]
            if tid[m] < 0 and hits[m] >= min_hits:
                tid[m] = next_id
                next_id += 1
            claimed[m] = True
            ids[r] = tid[m]
        missed = live & ~claimed
        age[missed] += 1
        free = missed & ((age > max_age) | (tid < 0))
        box[free], vel[free] = 0, 0
        cls[free], age[free], hits[free] = 0, 0, 0
        tid[free] = -1
        for r in unmatched:
            empty = (hits == 0).nonzero().flatten()
            if empty.numel() == 0:
                dropped += 1
                continue
            m = int(empty[0])
            box[m], vel[m] = dq[r], 0
            cls[m], age[m], hits[m] = dc[r], 0, 1
            if min_hits <= 1:
                tid[m] = next_id
                next_id += 1
            ids[r] = tid[m]
        state.box[s], state.vel[s] = box.to(i32), vel.to(i32)
        state.cls[s], state.id[s] = cls.to(i32), tid.to(i32)
        state.age[s], state.hits[s] = age.to(i32), hits.to(i32)
        state.next_id[s], state.dropped[s] = next_id, dropped
        out[n] = ids.to(i32)
    return out


ZONE_MAX = 8  # lines, zones and vertices per zone, per camera


def zone_anchor(box, centre):
    """Anchor of quarter-pixel boxes int64 [..., 4]: bottom-centre ((x1 + x2) >> 1, y2), or the
    centre ((x1 + x2) >> 1, (y1 + y2) >> 1).  Returns (px, py)."""
    px = (box[..., 0] + box[..., 2]) >> 1
    py = (box[..., 1] + box[..., 3]) >> 1 if centre else box[..., 3]
    return px, py


def point_in_polygon(px, py, poly):
    """Crossing number in integers: px, py int64 tensors (any shape), poly a list of (x, y)
    ints.  The edge (xi, yi) -> (xj, yj) toggles a point when (yi > py) != (yj > py) and px is
    strictly left of it: t = (xj - xi) (py - yi) - (px - xi) (yj - yi) has the sign of
    yj - yi.  No divide; points on an edge fall wherever this puts them."""
    inside = torch.zeros_like(px, dtype=torch.bool)
    xj, yj = poly[-1]
    for xi, yi in poly:
        dy = yj - yi
        t = (xj - xi) * (py - yi) - (px - xi) * dy
        left = (t > 0) if dy > 0 else (t < 0)
        inside ^= ((yi > py) != (yj > py)) & left
        xj, yj = xi, yi
    return inside


def _zone_masks(px, py, cls, tab):
    """Bit z: zone z of the table row holds (px, py) and its class filter passes cls."""
    m = torch.zeros_like(px)
    n_zones = min(max(int(tab["n_zones"]), 0), ZONE_MAX)
    for z in range(n_zones):
        nv = min(max(int(tab["n_vertex"][z]), 0), ZONE_MAX)
        if nv < 3:
            continue
        poly = [(int(x), int(y)) for x, y in tab["vertex"][z, :nv].tolist()]
        zc = int(tab["zone_cls"][z])
        hit = point_in_polygon(px, py, poly)
        if zc != -1:
            hit &= cls == zc
        m |= hit.long() << z
    return m


def _cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def line_crossing(p0, p1, a, b):
    """The move p0 -> p1 over the segment a -> b, all (x, y) ints: +1 forward, -1 backward,
    0 none.  side(P) = cross(b - a, P - a) >= 0 and sp(X) = cross(p1 - p0, X - p0) >= 0; a
    crossing needs side(p0) != side(p1) and sp(a) != sp(b).  Both half-open: a path through the
    end point two chained segments share counts on exactly one of them.  a == b: side() is
    true everywhere, never a crossing."""
    s0 = _cross(b[0] - a[0], b[1] - a[1], p0[0] - a[0], p0[1] - a[1]) >= 0
    s1 = _cross(b[0] - a[0], b[1] - a[1], p1[0] - a[0], p1[1] - a[1]) >= 0
    pa = _cross(p1[0] - p0[0], p1[1] - p0[1], a[0] - p0[0], a[1] - p0[1]) >= 0
    pb = _cross(p1[0] - p0[0], p1[1] - p0[1], b[0] - p0[0], b[1] - p0[1]) >= 0
    if s0 == s1 or pa == pb:
        return 0
    return 1 if s0 else -1


def _wrap32(v):
    return ((int(v) + (1 << 31)) % (1 << 32)) - (1 << 31)


def zone_update(det, count, track_state, zone_state, zones, slot0, out_mask, out_counts):
    """Line crossings and zone occupancy after the same step's track_update: THE definition the
    HIP kernel (csrc/kernels/zones.hip) equals bit for bit.  ``track_state`` (ops.TrackState) is
    only read; ``zone_state`` (ops.ZoneState) and the outputs are written; ``zones``
    (ops.ZoneSet) is the region table; all on the CPU.  Row n is stream ``slot0 + n``.

    The table's n_lines, n_zones and vertex counts are clamped to 0..8 (fewer than 3 vertices:
    an empty zone), anchor 1 is the centre and anything else bottom-centre.  Per slot t, with
    cur = id if hits > 0 and id >= 0 else -1 and the entry (seen_id, ax, ay, zmask):

    1. seen_id != cur and seen_id >= 0 (track gone, or slot reused): zone_exit[z] += 1 for
       every bit of zmask; the entry is cleared to (-1, 0, 0, 0);
    2. cur >= 0 and age == 0 (seen this frame): P1 = anchor(box), m1 = the zones holding P1
       whose class filter passes cls.  seen_id == cur: every class-passing line is tested with
       P0 = (ax, ay) -> line_fwd / line_back; zone_enter gets m1 & ~zmask, zone_exit gets
       zmask & ~m1.  Otherwise (first sighting): zone_enter gets m1, no line test.
       The entry becomes (cur, P1, m1);
    3. coasting tracks (age > 0) keep their entry;
    4. zone_occ[z] = entries with seen_id >= 0 and bit z; zone_dwell[z] += zone_occ[z].

    Counters are int32 and wrap modulo 2^32.  out_mask [N, max_det]: zones holding the anchor of
    each row r < count[n] (the row's own quantised box and class), 0 elsewhere; out_counts
    [N, 48]: line_fwd line_back zone_enter zone_exit zone_occ zone_dwell after the step."""
    N, max_det, _ = det.shape
    for n in range(N):
        s = slot0 + n
        tab = {k: getattr(zones, k)[s] for k in
               ("line", "line_cls", "vertex", "n_vertex", "zone_cls", "n_lines", "n_zones",
                "anchor")}
        centre = int(tab["anchor"]) == 1
        n_lines = min(max(int(tab["n_lines"]), 0), ZONE_MAX)
        box, cls = track_state.box[s].long(), track_state.cls[s].long()
        tid, age, hits = track_state.id[s], track_state.age[s], track_state.hits[s]
        px, py = zone_anchor(box, centre)
        m_slot = _zone_masks(px, py, cls, tab)
        delta = [0] * 32  # line_fwd, line_back, zone_enter, zone_exit
        tid, age, hits, cls_l = tid.tolist(), age.tolist(), hits.tolist(), cls.tolist()
        px_l, py_l, m_slot = px.tolist(), py.tolist(), m_slot.tolist()
        lines = [(tab["line"][ln].tolist(), int(tab["line_cls"][ln])) for ln in range(n_lines)]
        entry = zone_state.entry[s].tolist()
        for t in range(len(entry)):
            cur = tid[t] if hits[t] > 0 and tid[t] >= 0 else -1
            seen, ax, ay, zmask = entry[t]
            if seen != cur and seen >= 0:
                for z in range(ZONE_MAX):
                    delta[24 + z] += (zmask >> z) & 1
                seen, ax, ay, zmask = -1, 0, 0, 0
            if cur >= 0 and age[t] == 0:
                p1, m1 = (px_l[t], py_l[t]), m_slot[t]
                if seen == cur:
                    for ln, ((x0, y0, x1, y1), lc) in enumerate(lines):
                        if lc != -1 and lc != cls_l[t]:
                            continue
                        c = line_crossing((ax, ay), p1, (x0, y0), (x1, y1))
                        if c:
                            delta[ln if c > 0 else 8 + ln] += 1
                    enter, leave = m1 & ~zmask, zmask & ~m1
                else:
                    enter, leave = m1, 0
                for z in range(ZONE_MAX):
                    delta[16 + z] += (enter >> z) & 1
                    delta[24 + z] += (leave >> z) & 1
                seen, ax, ay, zmask = cur, p1[0], p1[1], m1
            entry[t] = [seen, ax, ay, zmask]
        zone_state.entry[s] = torch.tensor(entry, dtype=torch.int32)
        ctr = zone_state.counters[s]
        for i in range(32):
            ctr[i] = _wrap32(int(ctr[i]) + delta[i])
        live = zone_state.seen_id[s] >= 0
        for z in range(ZONE_MAX):
            occ = int((live & (((zone_state.zmask[s] >> z) & 1) == 1)).sum())
            ctr[32 + z] = occ
            ctr[40 + z] = _wrap32(int(ctr[40 + z]) + occ)
        out_counts[n] = ctr
        cnt = min(max(int(count[n]), 0), max_det)
        out_mask[n] = 0
        if cnt:
            dq = track_quantize(det[n, :cnt, :4])
            rx, ry = zone_anchor(dq, centre)
            out_mask[n, :cnt] = _zone_masks(rx, ry, track_class(det[n, :cnt, 5]), tab).to(
                torch.int32)
    return out_mask, out_counts


WATCH_CONDITIONS = ("motion", "scene", "dark", "flat", "frozen")
WATCH_PARAMS = ("motion_thr16", "motion_share_q", "scene_share_q", "dark16", "flat16", "hold")
WATCH_PARAM_RANGES = ((0, 4080), (0, 1024), (0, 1024), (0, 4096), (0, 4096), (1, 255))


def watch_luma(src, src_format="rgb"):
    """Luma int32 [N, Hs, Ws] of uint8 frames: the Y plane of NV12 [N, Hs * 3 // 2, Ws] as it
    is (the chroma rows are never read), (77 R + 150 G + 29 B + 128) >> 8 of RGB [N, Hs, Ws, 3]."""
    if src_format == "nv12":
        return src[:, :src.shape[1] * 2 // 3].to(torch.int32)
    c = src.to(torch.int32)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def watch_cells(luma, cell, row_step):
    """Per-cell (n, sum, grad, pairs), int64 [N, GH, GW] each, of luma [N, Hs, Ws]: over the
    sampled rows y % row_step == 0 of every cell x cell pixel cell (the last row / column of
    cells may be partial), n the sampled pixels, sum their luma, grad the sum of
    |Y(x+1, y) - Y(x, y)| over horizontal neighbours both in the cell, pairs their number."""
    N, Hs, Ws = luma.shape
    GH, GW = -(-Hs // cell), -(-Ws // cell)
    ch = cell // row_step  # sampled rows of a whole cell (row_step divides cell)
    y = luma[:, ::row_step].to(torch.int64)
    one = torch.ones_like(y)
    d = (y[:, :, 1:] - y[:, :, :-1]).abs()
    inside = (torch.arange(Ws - 1) % cell != cell - 1).to(torch.int64)  # left pixel not last
    d = d * inside
    dn = one[:, :, 1:] * inside

    def cells(t):
        t = torch.nn.functional.pad(t, (0, GW * cell - t.shape[2], 0, GH * ch - t.shape[1]))
        return t.reshape(N, GH, ch, GW, cell).sum(dim=(2, 4))

    return cells(one), cells(y), cells(d), cells(dn)


def frame_watch(src, state, slot0, src_format, out_stats, out_mask):
    """Per-camera frame watch: THE definition the HIP kernel (csrc/kernels/frame_watch.hip)
    equals bit for bit.  ``src`` uint8 RGB [N, Hs, Ws, 3] or NV12 [N, Hs * 3 // 2, Ws];
    ``state`` an ops.WatchState on the CPU (cell, row_step, bg_shift k and the per-stream
    threshold row ``params``); row n is the next frame of stream ``slot0 + n``.  All integer.

    Per cell (watch_cells): v = (16 sum + n // 2) // n in 1/16 luma.  On a primed stream the
    cell moved when |v - (acc >> k)| > motion_thr16 -- the background from before this frame --
    and then acc += v - (acc >> k); on an unprimed stream acc = v << k and no cell moves.  The
    stream is frozen when it is primed and every cell's (sum, grad) equals the stored pair; the
    pairs are then stored and the stream is primed.

    Per camera (Python ints, so exact): mean16 = (16 S_sum + P // 2) // P over the P sampled
    pixels, sharp16 = (16 S_grad + Q // 2) // Q over the Q pairs, moving = moved cells, cells =
    GH GW.  Conditions: bit 0 motion = moving > 0 and moving * 1024 >= motion_share_q * cells,
    bit 1 scene the same with scene_share_q, bit 2 dark = mean16 < dark16, bit 3 flat =
    sharp16 < flat16, bit 4 frozen.  run[c] = min(run[c] + 1, 65535) while the condition holds,
    else 0; alarm bit c = run[c] >= hold; raised[c] (wrapping int32) += 1 in the frame where
    run[c] == hold.  The thresholds are clamped into WATCH_PARAM_RANGES whatever the row holds.

    out_stats [N, 16] = mean16, sharp16, moving, cells, conditions, alarms, run[5], raised[5];
    out_mask uint8 [N, GH, GW] = 1 where the cell moved."""
    k = state.bg_shift
    n_px, c_sum, c_grad, c_pairs = watch_cells(watch_luma(src, src_format), state.cell,
                                               state.row_step)
    v = (16 * c_sum + n_px // 2) // n_px
    for n in range(src.shape[0]):
        s = slot0 + n
        par = [min(max(int(p), lo), hi)
               for p, (lo, hi) in zip(state.params[s].tolist(), WATCH_PARAM_RANGES)]
        thr, share_m, share_s, dark16, flat16, hold = par
        primed = int(state.primed[s]) != 0
        acc = state.acc[s].to(torch.int64)
        bg = acc >> k
        if primed:
            moved = (v[n] - bg).abs() > thr
            acc = acc + v[n] - bg
        else:
            moved = torch.zeros_like(v[n], dtype=torch.bool)
            acc = v[n] << k
        same = bool((state.sum[s] == c_sum[n]).all() and (state.grad[s] == c_grad[n]).all())
        state.acc[s] = acc.to(torch.int32)
        state.sum[s] = c_sum[n].to(torch.int32)
        state.grad[s] = c_grad[n].to(torch.int32)
        P, Q = int(n_px[n].sum()), int(c_pairs[n].sum())
        mean16 = (16 * int(c_sum[n].sum()) + P // 2) // P
        sharp16 = (16 * int(c_grad[n].sum()) + Q // 2) // Q
        moving, cells = int(moved.sum()), moved.numel()
        cond = [moving > 0 and moving * 1024 >= share_m * cells,
                moving > 0 and moving * 1024 >= share_s * cells,
                mean16 < dark16, sharp16 < flat16, primed and same]
        bits = alarms = 0
        for c, on in enumerate(cond):
            run = min(int(state.run[s, c]) + 1, 65535) if on else 0
            bits |= int(on) << c
            alarms |= int(run >= hold) << c
            if run == hold:
                state.raised[s, c] = _wrap32(int(state.raised[s, c]) + 1)
            state.run[s, c] = run
        state.primed[s] = 1
        out_stats[n] = torch.tensor([mean16, sharp16, moving, cells, bits, alarms]
                                    + state.run[s].tolist() + state.raised[s].tolist(),
                                    dtype=torch.int32)
        out_mask[n] = moved.to(torch.uint8)
    return out_stats, out_mask


def conv_dual2(x, x_coff, K1, x2, x2_coff, w, bias, act, stride2, up2, out, y_coff):
    K2 = w.shape[1] - K1
    a = x[..., x_coff:x_coff + K1].float()
    b = x2[..., x2_coff:x2_coff + K2].float()
    b = b.repeat_interleave(2, 1).repeat_interleave(2, 2) if up2 else b[:, ::stride2, ::stride2]
    wf = w.float()
    y = a @ wf[:, :K1].t() + b @ wf[:, K1:].t()
    if bias is not None:
        y = y + bias.float()
    out[..., y_coff:y_coff + w.shape[0]] = _act(y, act & 3).to(out.dtype)
    return out


def conv_dual(x1, x2, w, bias, act, stride2, out):
    K1 = x1.shape[-1]
    wf = w.float()
    y = x1.float() @ wf[:, :K1].t() + x2[:, ::stride2, ::stride2].float() @ wf[:, K1:].t()
    if bias is not None:
        y = y + bias.float()
    out.copy_(_act(y, act & 3).to(out.dtype))
    return out


# ---------------------------------------------------------------------------
# baseline JPEG encoder (csrc/kernels/jpeg_encode.hip): the format and its tables
# ---------------------------------------------------------------------------
JPEG_SUBSAMPLINGS = ("420", "444")
# zigzag position -> natural (row * 8 + column) index
JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
               41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15,
               23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# JPEG spec Annex K.1: luminance and chrominance quantisation tables, natural order
JPEG_QBASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
     14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
     24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99))
# JPEG spec Annex K.3: the four typical Huffman tables as (codes per length 1..16, symbols);
# order: DC luminance, DC chrominance, AC luminance, AC chrominance
JPEG_HUFF = (
    ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61,
      0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52,
      0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25,
      0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
      0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
      0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
      0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
      0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8,
      0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61,
      0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33,
      0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18,
      0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
      0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63,
      0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
      0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
      0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7,
      0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)))
JPEG_DQT_OFFSETS = (7, 76)  # of the 64 table bytes of each DQT segment in the header
JPEG_HEADER_BYTES = 611


def jpeg_quant_tables(quality: int) -> np.ndarray:
    """int32 [2, 64] (luminance, chrominance; natural order): the Annex K tables scaled the
    libjpeg way, s = 5000 // q below 50 else 200 - 2 q, entry = (base * s + 50) // 100
    clamped to 1..255."""
    q = int(quality)
    if isinstance(quality, bool) or not 1 <= q <= 100:
        raise ValueError(f"JPEG quality {quality!r} outside 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(JPEG_QBASE, np.int64) * s + 50) // 100, 1, 255).astype(np.int32)


def jpeg_huff_codes() -> np.ndarray:
    """int32 [4, 256]: code | length << 16 of every symbol of the four tables (0 where the
    table has no such symbol), codes assigned as the spec's Annex C does."""
    out = np.zeros((4, 256), np.int32)
    for t, (bits, vals) in enumerate(JPEG_HUFF):
        code, k = 0, 0
        for ln in range(1, 17):
            for _ in range(bits[ln - 1]):
                out[t, vals[k]] = code | (ln << 16)
                code += 1
                k += 1
            code <<= 1
        assert k == len(vals)
    return out


def jpeg_geometry(hw, subsampling: str):
    """(mcu, MCU rows = restart intervals, MCUs per row, blocks per MCU)."""
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {JPEG_SUBSAMPLINGS}, got {subsampling!r}")
    h, w = int(hw[0]), int(hw[1])
    if not (1 <= h <= 8192 and 1 <= w <= 8192):
        raise ValueError(f"JPEG image size {h}x{w} outside 1..8192")
    mcu = 16 if subsampling == "420" else 8
    return mcu, -(-h // mcu), -(-w // mcu), 6 if subsampling == "420" else 3


def jpeg_header(hw, subsampling: str, qtabs) -> bytes:
    """SOI, DQT x2, SOF0 (true size), DHT x4, DRI (one MCU row), SOS: JPEG_HEADER_BYTES."""
    _, _, mw, _ = jpeg_geometry(hw, subsampling)
    h, w = int(hw[0]), int(hw[1])
    zz = list(JPEG_ZIGZAG)
    out = bytearray(b"\xff\xd8")
    for t in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(qtabs[t][i]) for i in zz)
    samp = 0x22 if subsampling == "420" else 0x11
    out += (b"\xff\xc0\x00\x11\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + b"\x03"
            + bytes([1, samp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (bits, vals), tc_th in zip(JPEG_HUFF, (0x00, 0x01, 0x10, 0x11)):
        out += (b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc_th]) + bytes(bits)
                + bytes(vals))
    out += b"\xff\xdd\x00\x04" + mw.to_bytes(2, "big")
    out += b"\xff\xda\x00\x0c\x03" + bytes([1, 0x00, 2, 0x11, 3, 0x11]) + b"\x00\x3f\x00"
    assert len(out) == JPEG_HEADER_BYTES
    return bytes(out)


def _jpeg_dct_pass(d, first: bool):
    """One 8-point pass of the Loeffler-Ligtenberg-Moschytz forward DCT in 13-bit fixed point
    along the last axis (int64 in, int64 out).  The first (row) pass leaves 2 extra bits, the
    second (column) pass removes them again and leaves the factor 8 of the 2-D transform."""
    CB, P1 = 13, 2
    sh = CB - P1 if first else CB + P1

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6 = d0 + d7, d0 - d7, d1 + d6, d1 - d6
    t2, t5, t3, t4 = d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << P1, (t10 - t11) << P1
    else:
        o[0], o[4] = descale(t10 + t11, P1), descale(t10 - t11, P1)
    z1 = (t12 + t13) * 4433
    o[2] = descale(z1 + t13 * 6270, sh)
    o[6] = descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = descale(t4 + z1 + z3, sh)
    o[5] = descale(t5 + z2 + z4, sh)
    o[3] = descale(t6 + z2 + z3, sh)
    o[1] = descale(t7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def jpeg_coefficients(image: np.ndarray, subsampling: str, qtabs) -> np.ndarray:
    """Quantised zigzag coefficients int16 [intervals, blocks per interval, 64] of one uint8
    [H, W, 3] RGB image in scan order (MCU by MCU: Y00 Y01 Y10 Y11 Cb Cr for 4:2:0, Y Cb Cr for
    4:4:4).  JFIF full-range BT.601 in 16-bit fixed point, edge replication to whole MCUs,
    4:2:0 chroma (a + b + c + d + 2) >> 2, level shift by 128, the integer DCT above,
    q = sign(c) * ((|c| + 4 Q) // (8 Q)), DC clamped to +-1024 and AC to +-1023."""
    mcu, mh, mw, bpm = jpeg_geometry(image.shape[:2], subsampling)
    px = np.pad(image.astype(np.int64),
                ((0, mh * mcu - image.shape[0]), (0, mw * mcu - image.shape[1]), (0, 0)), "edge")
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if subsampling == "420":
        cb, cr = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
                  for c in (cb, cr))

    def blocks(p):  # [R, C] -> [R / 8, C / 8, 8, 8]
        return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)

    yb, cbb, crb = blocks(y - 128), blocks(cb - 128), blocks(cr - 128)
    if subsampling == "420":
        yb = yb.reshape(mh, 2, mw, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(mh, mw, 4, 8, 8)
    else:
        yb = yb[:, :, None]
    scan = np.concatenate([yb, cbb[:, :, None], crb[:, :, None]], axis=2)  # [mh, mw, bpm, 8, 8]
    c = _jpeg_dct_pass(scan, True)                                         # rows
    c = _jpeg_dct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)         # columns
    q = np.asarray(qtabs, np.int64).reshape(2, 8, 8)
    qsel = np.stack([q[0]] * (bpm - 2) + [q[1], q[1]])
    v = np.sign(c) * ((np.abs(c) + 4 * qsel) // (8 * qsel))
    v = v.reshape(mh, mw * bpm, 64)
    v[..., 0] = np.clip(v[..., 0], -1024, 1024)
    v[..., 1:] = np.clip(v[..., 1:], -1023, 1023)
    return v[..., list(JPEG_ZIGZAG)].astype(np.int16)


def jpeg_scan(coef: np.ndarray, subsampling: str, stats=None):
    """Entropy-code int16 [intervals, blocks, 64] zigzag coefficients: one byte string per
    restart interval (DC prediction from 0, Huffman codes MSB first, padded with 1-bits to a
    byte, FF stuffed as FF 00).  ``stats``: a dict whose counters are advanced."""
    huff = jpeg_huff_codes().tolist()
    comp = (0, 0, 0, 0, 1, 2) if subsampling == "420" else (0, 1, 2)
    bpm = len(comp)
    segs = []
    for row in coef.tolist():
        acc, nbits = 0, 0
        pred = [0, 0, 0]
        for i, blk in enumerate(row):
            c = comp[i % bpm]
            dc, ac = huff[min(c, 1)], huff[2 + min(c, 1)]
            diff = blk[0] - pred[c]
            pred[c] = blk[0]
            s = abs(diff).bit_length()
            e = dc[s]
            acc = (((acc << (e >> 16)) | (e & 0xffff)) << s) | ((diff if diff >= 0 else diff - 1)
                                                                & ((1 << s) - 1))
            nbits += (e >> 16) + s
            if stats is not None:
                stats["max_dc_cat"] = max(stats["max_dc_cat"], s)
                stats["dc_nonzero"] += diff != 0
            run = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    e = ac[0xf0]
                    acc = (acc << (e >> 16)) | (e & 0xffff)
                    nbits += e >> 16
                    run -= 16
                    if stats is not None:
                        stats["zrl"] += 1
                s = abs(v).bit_length()
                e = ac[(run << 4) | s]
                acc = (((acc << (e >> 16)) | (e & 0xffff)) << s) | ((v if v >= 0 else v - 1)
                                                                    & ((1 << s) - 1))
                nbits += (e >> 16) + s
                run = 0
                if stats is not None:
                    stats["max_ac_cat"] = max(stats["max_ac_cat"], s)
            if run:
                e = ac[0x00]
                acc = (acc << (e >> 16)) | (e & 0xffff)
                nbits += e >> 16
                if stats is not None:
                    stats["eob"] += 1
        fill = -nbits % 8
        if stats is not None:
            stats["bits"] += nbits
        raw = ((acc << fill) | ((1 << fill) - 1)).to_bytes((nbits + fill) // 8, "big")
        if stats is not None:
            stats["stuffed"] += raw.count(b"\xff")
        segs.append(raw.replace(b"\xff", b"\xff\x00"))
    return segs


def jpeg_encode(images, subsampling: str = "420", quality: int = 75, stats: bool = False,
                qtabs=None, header=None):
    """Baseline JPEG files of uint8 [M, H, W, 3] RGB images: THE definition the HIP kernels
    (csrc/kernels/jpeg_encode.hip) equal byte for byte.  Returns a list of M ``bytes``; with
    ``stats`` also a list of M dicts counting stuffed bytes, ZRL symbols, EOBs, nonzero DC
    differences, the largest DC / AC categories and the scan's bits before padding.  ``qtabs`` int [2, 64] (natural order) and
    ``header`` (bytes) override the tables and header that ``quality`` gives -- the encoder's
    device copies on the CPU path.

    File: header (jpeg_header), then one interleaved scan with a restart interval of one MCU
    row: interval i > 0 is preceded by RST((i - 1) % 8); EOI.  No JFIF / EXIF segment."""
    arr = images.numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
        raise ValueError(f"images are uint8 [M, H, W, 3], got {arr.dtype} {arr.shape}")
    if qtabs is None:
        qtabs = jpeg_quant_tables(quality)
    if header is None:
        header = jpeg_header(arr.shape[1:3], subsampling, qtabs)
    files, counts = [], []
    for img in arr:
        st = dict(stuffed=0, zrl=0, eob=0, dc_nonzero=0, max_dc_cat=0, max_ac_cat=0, bits=0)
        segs = jpeg_scan(jpeg_coefficients(img, subsampling, qtabs), subsampling, st)
        out = bytearray(header)
        for i, s in enumerate(segs):
            if i:
                out += bytes([0xff, 0xd0 + ((i - 1) & 7)])
            out += s
        out += b"\xff\xd9"
        files.append(bytes(out))
        counts.append(st)
    return (files, counts) if stats else files


# ---------------------------------------------------------------------------
# snapshot annotation: boxes, labels and privacy mosaic drawn into the thumbnails
# ---------------------------------------------------------------------------
# style table, int32 per camera (the layout csrc/kernels/annotate.hip reads)
ANN_BOXES, ANN_LABELS, ANN_COLOUR_BY, ANN_THICKNESS, ANN_SCALE, ANN_BLOCK = 0, 1, 2, 3, 4, 5
ANN_MAX_DRAW, ANN_N_POLY, ANN_PRIV_CLS, ANN_N_VERT, ANN_VERT, ANN_PALETTE = 6, 7, 8, 16, 24, 152
ANN_TABLE_STRIDE = 168
ANN_MAX = 8           # privacy classes, polygons and vertices per polygon, per camera
ANN_MAX_DET = 300
ANN_MAX_SRC = 4096    # the frame the boxes live in: quarter pixels stay inside 0..16384
ANN_LABELS_MODES = ("none", "class", "id", "both")  # bit 0: class, bit 1: id
ANN_GLYPHS = "0123456789:"
# 5 x 7 glyphs, one row per word, bit 4 = the left column; the 8th row of a glyph is blank
_ANN_FONT_ROWS = (
    "01110 10001 10011 10101 11001 10001 01110",  # 0
    "00100 01100 00100 00100 00100 00100 01110",  # 1
    "01110 10001 00001 00010 00100 01000 11111",  # 2
    "11111 00010 00100 00010 00001 10001 01110",  # 3
    "00010 00110 01010 10010 11111 00010 00010",  # 4
    "11111 10000 11110 00001 00001 10001 01110",  # 5
    "00110 01000 10000 11110 10001 10001 01110",  # 6
    "11111 00001 00010 00100 01000 01000 01000",  # 7
    "01110 10001 10001 01110 10001 10001 01110",  # 8
    "01110 10001 10001 01111 00001 00010 01100",  # 9
    "00000 00100 00100 00000 00100 00100 00000",  # :
)
ANN_FONT_WORDS = 8 * len(ANN_GLYPHS)


def annotate_font() -> np.ndarray:
    """The font table int32 [88]: glyph g (``ANN_GLYPHS``) in words 8 g .. 8 g + 7."""
    f = np.zeros(ANN_FONT_WORDS, np.int32)
    for g, rows in enumerate(_ANN_FONT_ROWS):
        for i, row in enumerate(rows.split()):
            f[8 * g + i] = int(row, 2)
    return f


def annotate_block(v: int) -> int:
    """The mosaic block a table word stands for: 16, 8 or 4 whatever it holds."""
    return 16 if v >= 16 else 8 if v >= 8 else 4


def annotate_rects(det, src_hw, hw):
    """Quantised boxes fp32 [..., >= 4] in a (Hs, Ws) frame -> thumbnail rectangles int64
    [..., 4] = (x0, y0, x1, y1), half open, never empty, covering every pixel of the (H, W)
    thumbnail the box touches."""
    (hs, ws), (h, w) = src_hw, hw
    q = track_quantize(det[..., :4])
    out = torch.empty_like(q)
    for a, (src, dst) in enumerate(((ws, w), (hs, h))):
        q1 = q[..., a].clamp_max(4 * src)
        q2 = q[..., a + 2].clamp_max(4 * src)
        lo = torch.clamp((q1 * dst) // (4 * src), max=dst - 1)
        hi = (q2 * dst + 4 * src - 1) // (4 * src)
        out[..., a] = lo
        out[..., a + 2] = torch.minimum(torch.maximum(hi, lo + 1), torch.tensor(dst))
    return out


def annotate_text(labels: int, cls: int, tid: int) -> str:
    """The label of a row: class digits, ':' when both parts show, digits of id % 100000; the
    id part and the colon are dropped while id < 0 ('' = no label)."""
    parts = []
    if labels & 1:
        parts.append(str(cls))
    if labels & 2 and tid >= 0:
        parts.append(str(tid % 100000))
    return ":".join(parts)


def annotate(images, table, font, det=None, count=None, track_id=None, src_hw=None, slot0=0):
    """Draw into uint8 [N, H, W, 3] thumbnails, in place: THE definition the HIP kernel
    (csrc/kernels/annotate.hip) equals byte for byte.  ``table`` int32 [S, 168] is the style
    of every camera (row n of ``images`` uses row ``slot0 + n``), ``font`` int32 [88]; ``det``
    fp32 [N, max_det, 6] / ``count`` int32 [N] / ``track_id`` int32 [N, max_det] or None are
    the boxes in a ``src_hw`` = (Hs, Ws) pixel frame (default: the thumbnail's own).

    Every output pixel is a function of the input picture and the tables.  From the top:
    labels (lowest row index first), outlines (lowest row index first), the mosaic of the
    privacy blocks, the picture.  Every count, size and index of the table is clamped as the
    kernel clamps it."""
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    hs, ws = (h, w) if src_hw is None else (int(src_hw[0]), int(src_hw[1]))
    font = np.asarray(font).astype(np.int64)
    ys, xs = torch.arange(h, dtype=torch.int64), torch.arange(w, dtype=torch.int64)
    # pixel centres in quarter pixels of the source frame
    cx = (((2 * xs + 1) * 2 * ws) // w)[None, :].expand(h, w)
    cy = (((2 * ys + 1) * 2 * hs) // h)[:, None].expand(h, w)
    for i in range(n):
        tab = [int(v) for v in table[slot0 + i].tolist()]
        img = images[i].numpy()
        src = img.copy()
        boxes, labels = tab[ANN_BOXES] != 0, tab[ANN_LABELS] & 3
        by_track = tab[ANN_COLOUR_BY] == 1
        t = min(max(tab[ANN_THICKNESS], 1), 4)
        s = min(max(tab[ANN_SCALE], 1), 2)
        blk = annotate_block(tab[ANN_BLOCK])
        max_draw = min(max(tab[ANN_MAX_DRAW], 0), ANN_MAX_DET)
        priv = [c for c in tab[ANN_PRIV_CLS:ANN_PRIV_CLS + ANN_MAX] if c >= 0]
        cnt, rect, cls, tid = 0, None, None, None
        if det is not None:
            cnt = min(max(int(count[i]), 0), int(det.shape[1]))
            rect = annotate_rects(det[i], (hs, ws), (h, w)).tolist()
            cls = track_class(det[i, :, 5]).tolist()
            tid = track_id[i].tolist() if track_id is not None else [-1] * int(det.shape[1])
        # privacy: the pixels that are hidden, then whole blocks
        hit = np.zeros((h, w), bool)
        for r in range(cnt):
            if cls[r] in priv:
                x0, y0, x1, y1 = rect[r]
                hit[y0:y1, x0:x1] = True
        for z in range(min(max(tab[ANN_N_POLY], 0), ANN_MAX)):
            nv = min(max(tab[ANN_N_VERT + z], 0), ANN_MAX)
            if nv < 3:
                continue
            v = tab[ANN_VERT + 16 * z:ANN_VERT + 16 * z + 2 * nv]
            hit |= point_in_polygon(cx, cy, list(zip(v[0::2], v[1::2]))).numpy()
        for by in range(0, h, blk):
            for bx in range(0, w, blk):
                if hit[by:by + blk, bx:bx + blk].any():
                    cell = src[by:by + blk, bx:bx + blk].astype(np.int64).reshape(-1, 3)
                    img[by:by + blk, bx:bx + blk] = (cell.sum(0) + len(cell) // 2) // len(cell)
        # outlines and labels, highest row first so that the lowest ends on top
        drawn = range(min(cnt, max_draw) - 1, -1, -1)
        colour = {}
        for r in drawn:
            key = tid[r] if by_track and tid[r] >= 0 else cls[r]
            c = tab[ANN_PALETTE + (key & 15)]
            colour[r] = (c & 255, (c >> 8) & 255, (c >> 16) & 255)
        if boxes:
            for r in drawn:
                x0, y0, x1, y1 = rect[r]
                ring = np.ones((y1 - y0, x1 - x0), bool)
                ring[t:y1 - y0 - t, t:x1 - x0 - t] = False
                img[y0:y1, x0:x1][ring] = colour[r]
        for r in drawn:
            text = annotate_text(labels, cls[r], tid[r])
            if not text:
                continue
            x0, y0 = rect[r][0], rect[r][1]
            lw, lh = s * (6 * len(text) + 1), 9 * s
            cr, cg, cb = colour[r]
            ink = 0 if (77 * cr + 150 * cg + 29 * cb) >> 8 >= 128 else 255
            lab = np.empty((lh, lw, 3), np.uint8)
            lab[:] = colour[r]
            for k, ch in enumerate(text):
                g = ANN_GLYPHS.index(ch)
                for gy in range(7):
                    for gx in range(5):
                        if (font[8 * g + gy] >> (4 - gx)) & 1:
                            yy, xx = s * (1 + gy), s * (1 + 6 * k + gx)
                            lab[yy:yy + s, xx:xx + s] = ink
            img[y0:y0 + lh, x0:x0 + lw] = lab[:h - y0, :w - x0]
    return images
