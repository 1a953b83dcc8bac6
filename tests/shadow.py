"""Shadow executor: walk a deployed model op by op against the CPU reference
(test_model_walk_cpu.py, test_model_walk_gpu.py).

``with shadow(monkeypatch) as sh: model(frames)`` wraps every public ``kvedge_amd.ops``
function the two models call.  For each outermost call it

1. copies every tensor argument to the CPU (aliases stay aliases: a C2f conv's ``res`` and
   ``out`` are one concat buffer on both sides),
2. runs the call as issued (on a CUDA model: the HIP kernel),
3. runs the same ``ops`` function on the CPU copies (``kvedge_amd.ops.reference``) --
   teacher forcing: the reference sees exactly what the kernel saw, so no error
   accumulates across layers,
4. compares every tensor argument and every returned tensor by the rule of its dtype
   (``kernel_rules`` for bf16; the single-kernel tests' bounds for fp32 / integer results),
5. checks the canaries: ``ops.empty`` is patched so every buffer starts as one fixed NaN bit
   pattern.  Where the reference left a tensor's bits as they were before the call (canary
   or an earlier layer's values) the kernel's bits must be the same -- no stray write; where
   the reference wrote a finite value the kernel's must be finite -- no read of unwritten
   memory,
6. logs (ordinal, op, key, tile, max err, rrms) and raises ShadowError with that context.

``sweep=True`` additionally re-issues each distinct conv key with every explicit tile.
"""
import contextlib
import dataclasses
import functools
import inspect
import json
import os
import re

import torch

from kernel_rules import MAX_REL, RRMS_TOL
from kvedge_amd import ops

OPS = ("conv2d", "conv_pair", "conv_dual", "conv_dual2", "conv_tail", "c2f16",
       "stem_pool", "stem_pool_frames", "stem12_pool_frames", "yolo_stem2", "stem_from_frames",
       "maxpool2d", "sppf_pool", "global_avgpool", "pooled_fc", "softmax_rows", "upsample2x",
       "yolo_decode", "nms", "preprocess")
SWEEP_OPS = ("conv2d", "conv_dual", "conv_dual2", "conv_pair", "conv_tail")
PAIR_TILES = 4  # v4 direct tiles 0-3 of ops.conv_pair

# quiet NaNs with a payload no arithmetic produces
CANARY_BF16 = 0x7FE5
CANARY_F32 = 0x7FE5A5A5
CANARY_INT = -0x5A5A5A5  # integer buffers: no rule hangs on it, it only makes runs repeatable

# names of the tensors an op returns, for the ones it allocated itself
RET_NAMES = {"conv_tail": ("out", "z"), "softmax_rows": ("out", "argmax"),
             "yolo_decode": ("boxes", "scores", "cls"), "nms": ("out", "count")}
# fp32 results: (op, tensor) -> max |err| strictly below, the single-kernel tests' bounds
# (test_kernels_gpu.py: test_yolo_decode_and_nms, test_maxpool_avgpool_softmax)
F32_BOUNDS = {("yolo_decode", "boxes"): 2e-2, ("yolo_decode", "scores"): 1e-5,
              ("nms", "out"): 1e-4, ("softmax_rows", "out"): 1e-5}
# pure data movement: the single-kernel tests ask for equal values
EXACT_OPS = ("maxpool2d", "sppf_pool", "upsample2x")


class ShadowError(AssertionError):
    pass


def _bits(t):
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t.contiguous()


def _canary(dtype):
    if dtype == torch.bfloat16:
        return CANARY_BF16
    if dtype == torch.float32:
        return CANARY_F32
    return None


def poison(t):
    """Fill a buffer with its dtype's canary."""
    if t.dtype == torch.bfloat16:
        t.view(torch.int16).fill_(CANARY_BF16)
    elif t.dtype == torch.float32:
        t.view(torch.int32).fill_(CANARY_F32)
    elif t.dtype in (torch.int32, torch.int64):
        t.fill_(CANARY_INT)
    elif t.dtype == torch.uint8:
        t.fill_(0xA5)
    return t


def is_canary(t):
    """Elementwise: does a bf16 / fp32 tensor still hold the canary bits?"""
    return _bits(t) == _canary(t.dtype)


def _tensors(arguments):
    """(name, tensor) of every tensor among an op's bound arguments (lists one level deep)."""
    for name, v in arguments.items():
        if isinstance(v, torch.Tensor):
            yield name, v
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                if isinstance(e, torch.Tensor):
                    yield f"{name}[{i}]", e


def _key_of(arguments):
    key = []
    for name, v in arguments.items():
        if name == "tile":
            continue
        if isinstance(v, torch.Tensor):
            key.append((name, tuple(v.shape)))
        elif isinstance(v, (list, tuple)) and v and isinstance(v[0], torch.Tensor):
            key.append((name, tuple(tuple(e.shape) for e in v)))
        elif dataclasses.is_dataclass(v):
            key.append((name, dataclasses.astuple(v)))
        elif isinstance(v, (list, tuple)):
            key.append((name, tuple(v)))
        else:
            key.append((name, v))
    return tuple(key)


class Shadow:
    def __init__(self, sweep=False, exact=False, faults=None, tiles=None):
        self.sweep = sweep
        self.exact = exact            # CPU model: reference vs reference, bit for bit
        self.faults = faults or {}    # op name -> fn(orig, *args, **kw): a wrong "device" side
        self.tiles = tiles            # sweep over these tiles instead of the whole table
        self.depth = 0
        self.ordinal = 0
        self.log = []                 # one record per shadowed call
        self.sweeps = []              # one record per swept key
        self.accepted = {}            # (op, tile) -> keys accepted
        self.allocs = []
        self._swept = set()
        self._ws_poisoned = False
        self._orig_empty = ops.empty

    # -- allocation ------------------------------------------------------------------
    def empty(self, *shape, dtype=None, device=None):
        t = poison(self._orig_empty(*shape, dtype=dtype, device=device))
        if self.depth == 0:
            self.allocs.append(t)  # the model's own buffers (concat buffers among them)
        return t

    # -- comparison ------------------------------------------------------------------
    def _compare(self, ctx, op, name, got, ref, pre, aux=None):
        """got: the issued call's tensor after the call; ref: the reference's; pre: the CPU
        snapshot from before the call (None: a buffer the op allocated, all canary).
        Returns (max err, rrms); raises ShadowError."""
        if got.shape != ref.shape or got.dtype != ref.dtype:
            raise ShadowError(f"{ctx} {name}: {tuple(got.shape)} {got.dtype} vs reference "
                              f"{tuple(ref.shape)} {ref.dtype}")
        if got.numel() == 0:
            return 0.0, 0.0
        dev = got.device
        ref = ref.to(dev)
        gb, rb = _bits(got), _bits(ref)
        can = _canary(got.dtype)
        if can is None:  # integer tensors (frames, classes, counts, argmax): equal
            bad = gb != rb
            if bool(bad.any()):
                self._fail(ctx, name, "integer values differ", bad, got, ref)
            return 0.0, 0.0
        # "kept" = the reference left the element as it was: still the canary, or the same bits
        # as before the call.  Those must match bit for bit; everything else is held to the
        # tolerance.  An element the reference REWROTE with bits equal to its pre-call value
        # also counts as kept (stricter, never looser).  The models write only into fresh
        # canary regions -- the in-place C2f conv too: its output slice of the concat buffer
        # is unwritten until then -- so this costs nothing today; if a "stray write" is ever
        # reported inside an op's own output slice over a non-canary pre-state, look here first
        kept = rb == can
        if pre is not None:
            kept = kept | (rb == _bits(pre.to(dev)))
        stray = kept & (gb != rb)
        wrote = ~kept
        rf, gf = ref.float(), got.float()
        ref_bad = wrote & ~torch.isfinite(rf)
        unread = wrote & ~ref_bad & ~torch.isfinite(gf)
        ok = wrote & ~ref_bad & ~unread
        zero = torch.zeros((), device=dev)
        err = torch.where(ok, (gf - rf).abs(), zero)
        rsq = torch.where(ok, rf * rf, zero)
        stats = torch.stack([stray.sum().float(), ref_bad.sum().float(), unread.sum().float(),
                             err.max(), torch.where(ok, rf.abs(), zero).max(),
                             (err.double() ** 2).sum().float(), rsq.double().sum().float(),
                             (gb != rb).sum().float()]).tolist()
        n_stray, n_refbad, n_unread, max_err, scale, esq, rsq, n_diff = stats
        rr = (esq ** 0.5) / max(rsq ** 0.5, 1e-12)
        if n_refbad:
            self._fail(ctx, name, "the REFERENCE wrote non-finite values (the model itself "
                       "reads unwritten memory)", ref_bad, got, ref)
        if n_stray:
            self._fail(ctx, name, "stray write: bits changed where the reference left the "
                       "buffer as it was", stray, got, ref)
        if n_unread:
            self._fail(ctx, name, "non-finite where the reference wrote finite values (read "
                       "of unwritten memory?)", unread, got, ref)
        if self.exact:
            if n_diff:
                self._fail(ctx, name, "not bit-identical", gb != rb, got, ref)
            return max_err, rr
        if op == "global_avgpool" and name == "out" and aux is not None:
            # test_maxpool_avgpool_softmax: one bf16 rounding of the fp32 mean
            m = aux.to(dev)
            bad = (gf - m).abs() > 2.0 ** -8 * m.abs() + 1e-4
            if bool(bad.any()):
                self._fail(ctx, name, "more than one bf16 rounding from the fp32 mean", bad, got,
                           ref)
        elif got.dtype == torch.bfloat16:
            if op in EXACT_OPS:
                if max_err != 0.0:
                    self._fail(ctx, name, "values differ (pure data movement)", err > 0, got, ref)
            elif not (max_err <= MAX_REL * (scale + 1e-6) and rr <= RRMS_TOL):
                self._fail(ctx, name, f"max err {max_err:.4g} (bound {MAX_REL * (scale + 1e-6):.4g}"
                           f"), rrms {rr:.3g} (bound {RRMS_TOL})", err > MAX_REL * (scale + 1e-6)
                           if max_err > MAX_REL * (scale + 1e-6) else err > 0, got, ref)
        else:
            bound = F32_BOUNDS.get((op, name))
            if bound is None:
                if n_diff:  # an fp32 tensor no rule covers (bias, mean): must not change
                    self._fail(ctx, name, "fp32 tensor without a rule changed", gb != rb, got, ref)
            elif not max_err < bound:
                self._fail(ctx, name, f"max err {max_err:.4g} (bound {bound})", err >= bound, got,
                           ref)
        return max_err, rr

    def _fail(self, ctx, name, what, mask, got, ref):
        idx = mask.nonzero()[:6].cpu()
        rows = [(tuple(i.tolist()), float(got[tuple(i)].float()), float(ref[tuple(i)].float()))
                for i in idx]
        raise ShadowError(f"{ctx}: tensor {name!r} {tuple(got.shape)}: {what}; "
                          f"{int(mask.sum())} of {mask.numel()} elements, first (index, got, "
                          f"reference): {rows}")

    # -- the wrapper -----------------------------------------------------------------
    def wrap(self, name, orig):
        sig = inspect.signature(orig)

        @functools.wraps(orig)
        def wrapper(*args, **kw):
            if self.depth:  # an op's CPU path calling another op: part of the outer call
                return orig(*args, **kw)
            self.depth += 1
            try:
                return self._shadowed(name, orig, sig, args, kw)
            finally:
                self.depth -= 1
        return wrapper

    def _run(self, name, orig, arguments):
        """The call as issued (or its deliberately wrong stand-in), synchronised."""
        fault = self.faults.get(name)
        ret = fault(orig, **arguments) if fault else orig(**arguments)
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        return ret

    def _shadowed(self, name, orig, sig, args, kw):
        ba = sig.bind(*args, **kw)
        ba.apply_defaults()
        arguments = dict(ba.arguments)
        i = self.ordinal
        self.ordinal += 1
        key = _key_of(arguments)
        tile = arguments.get("tile")
        ctx = f"call {i} {name} tile {tile} key {key}"
        # 1. snapshot (aliases kept)
        memo, pre = {}, {}

        def to_cpu(t):
            k = (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)
            if k not in memo:
                memo[k] = t.detach().to("cpu", copy=True)
                pre[k] = memo[k].clone()
            return memo[k]

        def pre_of(t):
            return pre[(t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)]

        cpu_args = {}
        for n, v in arguments.items():
            if isinstance(v, torch.Tensor):
                cpu_args[n] = to_cpu(v)
            elif isinstance(v, (list, tuple)) and v and isinstance(v[0], torch.Tensor):
                cpu_args[n] = type(v)(to_cpu(e) for e in v)
            else:
                cpu_args[n] = v
        dev_pre = {n: pre_of(t) for n, t in _tensors(arguments)}
        # 2. the call as issued
        try:
            ret = self._run(name, orig, arguments)
        except Exception as e:  # noqa: BLE001 -- the model's own call must never fail
            raise ShadowError(f"{ctx}: the call as issued raised {type(e).__name__}: {e}") from e
        # 3. the reference on the CPU copies
        ref_ret = orig(**cpu_args)
        # 4. + 5. compare arguments, then the tensors the op allocated itself
        aux = None
        if name == "global_avgpool":
            aux = dev_pre["x"].float().mean(dim=(1, 2))
        worst = (0.0, 0.0)
        pairs = []  # (tensor name, issued tensor, reference tensor, pre or None)
        arg_ids = {}
        for (n, t), (_, r) in zip(_tensors(arguments), _tensors(cpu_args)):
            pairs.append((n, t, r, dev_pre[n]))
            arg_ids[id(t)] = n
        rets = ret if isinstance(ret, (list, tuple)) else (ret,)
        ref_rets = ref_ret if isinstance(ref_ret, (list, tuple)) else (ref_ret,)
        names = RET_NAMES.get(name, ("out",))
        outs = {}  # output name -> (issued tensor, reference tensor, pre or None)
        for j, (t, r) in enumerate(zip(rets, ref_rets)):
            if not isinstance(t, torch.Tensor):
                continue
            n = names[j] if j < len(names) else f"ret{j}"
            if id(t) in arg_ids:
                outs[n] = (t, r, dev_pre[arg_ids[id(t)]])
            else:
                pairs.append((n, t, r, None))
                outs[n] = (t, r, None)
        seen = set()
        for n, t, r, p in pairs:
            if id(t) in seen:
                continue
            seen.add(id(t))
            e, rr = self._compare(ctx, name, n, t, r, p, aux)
            worst = (max(worst[0], e), max(worst[1], rr))
        rec = {"i": i, "op": name, "key": repr(key), "tile": tile, "max_err": worst[0],
               "rrms": worst[1]}
        w = arguments.get("w")
        if isinstance(w, torch.Tensor):
            rec["w_ptr"] = w.data_ptr()
        if name == "nms":
            rec["kept"] = int(rets[1].sum())
        self.log.append(rec)
        # optional tile sweep, once per distinct key
        if self.sweep and name in SWEEP_OPS and (name, key) not in self._swept:
            self._swept.add((name, key))
            self._sweep(ctx, name, orig, arguments, outs, i, key)
        return ret

    # -- tile sweep ------------------------------------------------------------------
    def _sweep_tiles(self, name):
        if self.tiles is not None:
            return list(self.tiles)
        if name == "conv_pair":
            return list(range(PAIR_TILES))
        n = int(torch.ops.kvedge.conv_num_tiles())
        tiles = list(range(n))
        if name == "conv_tail":
            tiles += [n + s for s in range(int(torch.ops.kvedge.conv_seam_num_tiles()))]
        return tiles

    def _sweep(self, ctx, name, orig, arguments, outs, ordinal, key):
        call = dict(arguments)
        for n, (t, _, _) in outs.items():
            call[n] = t  # the buffers the first call wrote become the explicit destinations
        dev = next(iter(outs.values()))[0].device
        if dev.type == "cuda" and not self._ws_poisoned:
            # split-K slabs: no output may depend on the workspace's old contents
            ws = ops.splitk_workspace(dev, 1)
            ws.fill_(float("nan"))
            self._ws_poisoned = True
        before = {n: (None if p is None else p.to(dev)) for n, (_, _, p) in outs.items()}
        refs = {n: r.to(dev) for n, (_, r, _) in outs.items()}

        def restore():
            for n, (t, _, _) in outs.items():
                if before[n] is None:
                    poison(t)
                else:
                    t.copy_(before[n])

        accepted, refused = [], {}
        for tile in self._sweep_tiles(name):
            tctx = f"{ctx} SWEEP tile {tile}"
            restore()
            call["tile"] = tile
            try:
                self._run(name, orig, call)
            except RuntimeError as e:
                m = re.search(r"failed rc=(-?\d+)", str(e))
                if m is None or int(m.group(1)) == -7:
                    raise ShadowError(f"{tctx}: not a refusal: {e}") from e
                if dev.type == "cuda":
                    torch.cuda.synchronize()
                for n, (t, _, _) in outs.items():
                    was = _bits(before[n]) if before[n] is not None else None
                    same = (_bits(t) == (_canary(t.dtype) if was is None else was))
                    if not bool(same.all()):
                        raise ShadowError(
                            f"{tctx}: the launcher refused (rc={m.group(1)}) but {n!r} changed: "
                            f"{int((~same).sum())} of {same.numel()} elements")
                refused[tile] = int(m.group(1))
                continue
            except Exception as e:  # noqa: BLE001
                raise ShadowError(f"{tctx}: {type(e).__name__}: {e}") from e
            for n, (t, _, _) in outs.items():
                self._compare(tctx, name, n, t, refs[n], before[n])
            accepted.append(tile)
            self.accepted[(name, tile)] = self.accepted.get((name, tile), 0) + 1
        # downstream layers see the verified result of the call as issued
        restore()
        call["tile"] = arguments.get("tile")
        self._run(name, orig, call)
        self.sweeps.append({"i": ordinal, "op": name, "key": repr(key),
                            "issued_tile": arguments.get("tile"), "accepted": accepted,
                            "refused": refused})

    # -- reporting -------------------------------------------------------------------
    def op_kinds(self):
        return {r["op"] for r in self.log}

    def worst(self):
        """The record with the largest rrms."""
        return max(self.log, key=lambda r: r["rrms"]) if self.log else None

    def write_log(self, name, directory=None):
        """Write the call and sweep records as JSON into ``directory`` (default: the
        directory KVEDGE_WALK_LOG names); nothing is written when it is unset or missing."""
        directory = directory or os.environ.get("KVEDGE_WALK_LOG", "")
        if not directory or not os.path.isdir(directory):
            return
        doc = {"calls": self.log, "sweeps": self.sweeps,
               "accepted": {f"{op}:{t}": n for (op, t), n in sorted(self.accepted.items())}}
        with open(os.path.join(directory, f"model_walk_{name}.json"), "w") as f:
            json.dump(doc, f, indent=1)


@contextlib.contextmanager
def shadow(monkeypatch, sweep=False, exact=False, faults=None, tiles=None):
    sh = Shadow(sweep=sweep, exact=exact, faults=faults, tiles=tiles)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "empty", sh.empty)
        for name in OPS:
            mp.setattr(ops, name, sh.wrap(name, getattr(ops, name)))
        yield sh
