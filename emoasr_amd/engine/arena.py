"""The flat parameter / gradient arena, the small host-to-device helpers, and the stash records that the engine's modules and
layer_rt.py share."""
import math
import weakref
from typing import NamedTuple

import torch

from .. import ops

_ALIGN = 64  # arena slot alignment in elements (256 B in f32, 128 B in bf16)


def _cfg(cfg, key, default=None):
    return getattr(cfg, key) if hasattr(cfg, key) else default


_ARENAS = weakref.WeakSet()


def arena_of(params):
    """the live ParamArena that owns these parameter tensors (their .data are views of its flat buffer);
    LookupError before the model has been bound on the device"""
    params = list(params)
    if params:
        ptr = params[0].data_ptr()
        for a in list(_ARENAS):
            lo = a.flat.data_ptr()
            if lo <= ptr < lo + a.size * 4 and a.bound():
                return a
    raise LookupError("emoasr_amd: these parameters are not bound to a device arena yet (move the model to the GPU and "
                      "run model.engine() or one forward pass)")


class ParamArena:
    """Re-homes a module's parameters into one flat f32 buffer (and their .grad into a
    second one) so that (a) the optimizer, the gradient norm and the RCCL all-reduce work
    on a single contiguous range, (b) q/k/v projection weights are adjacent and usable as
    one fused [3d, d] GEMM operand, (c) the bf16 compute copy is one cast kernel."""

    def __init__(self, module, compute_dtype):
        named = list(module.named_parameters())
        self.module_order = [n for n, _ in named]  # position in module.parameters(): torch optimizers index by it
        order, seen = [], set()
        byname = dict(named)
        for name, _ in named:
            if name in seen:
                continue
            group = None
            if name.endswith("linear_q.weight"):
                base = name[: -len("linear_q.weight")]
                group = [base + f"linear_{x}.{kind}" for kind in ("weight", "bias") for x in "qkv"]
            elif name.endswith("self.query.weight"):  # BERT-style LM layers
                base = name[: -len("query.weight")]
                group = [base + f"{x}.{kind}" for kind in ("weight", "bias") for x in ("query", "key", "value")]
            if group is not None and all(g in byname for g in group):
                for g in group:
                    order.append(g)
                    seen.add(g)
                continue
            order.append(name)
            seen.add(name)
        self.names = order
        self.params = [byname[n] for n in order]
        dev = self.params[0].device
        assert dev.type == "cuda", "emoasr_amd: move the model to the GPU first (no CPU path)"
        self.offsets = {}
        off = 0
        for n, p in zip(order, self.params):
            self.offsets[n] = off
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.size = off
        self.flat = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32)
        self.compute_dtype = compute_dtype
        self.shadow = self.flat if compute_dtype == torch.float32 else torch.zeros(off, device=dev, dtype=compute_dtype)
        self.pviews, self.gviews = {}, {}
        self._vcache = {}
        with torch.no_grad():
            for n, p in zip(order, self.params):
                o = self.offsets[n]
                v = self.flat[o:o + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
                self.pviews[n] = v
                self.gviews[n] = self.grad[o:o + p.numel()].view(p.shape)
                p.grad = self.gviews[n]
        self.refresh_shadow()
        _ARENAS.add(self)

    def bound(self):
        """do the module's parameters still live in this arena?  Every call checks EVERY parameter (0.16 ms for the 455 tensors of
        the L2 model: nothing against a training step), so a single re-assigned parameter (p.data = ..., weight tying, a partial
        load with assign=True) is seen before the next forward / update runs on stale arena storage.  Only inside a
        hold_shadow(True) window -- an evaluation loop whose caller has promised not to touch the parameters, where that
        0.16 ms was a tenth of a batch-1 decode -- a few sentinels answer (moving the module re-creates ALL parameters), with
        the full check every 16th call."""
        n = len(self.params)
        if getattr(self, "_hold", False) and n > 16:
            self._bound_calls = getattr(self, "_bound_calls", 0) + 1
            if self._bound_calls % 16 != 1:
                idx = (0, n // 7, 2 * n // 7, 3 * n // 7, 4 * n // 7, 5 * n // 7, 6 * n // 7, n - 1)
                return all(self.params[i].data_ptr() == self.pviews[self.names[i]].data_ptr() for i in idx)
        return all(p.data_ptr() == self.pviews[n].data_ptr() for n, p in zip(self.names, self.params))

    def refresh_shadow(self):
        if self.shadow is not self.flat and not getattr(self, "_hold", False):
            ops.strided_copy(self.flat, out=self.shadow)
            if getattr(self, "_tpairs", None):
                ops.transpose_cast_batched(self._tpairs)

    def transposed(self, first, last=None, shape=None):
        """a compute-dtype copy of parameter `first` (or of the span first..last viewed as `shape` = [rows, cols]) stored
        TRANSPOSED, kept current by refresh_shadow (one batched launch for all of them).  -> [cols, rows]"""
        key = (first, last)
        reg = self.__dict__.setdefault("_tcache", {})
        if key not in reg:
            src = self.pviews[first] if last is None else self._span(self.flat, first, last, shape)
            src = src.view(shape) if (shape is not None and last is None) else src
            src = src.view(src.shape[0], -1)
            dst = torch.empty(src.shape[1], src.shape[0], device=src.device, dtype=self.shadow.dtype)
            self.__dict__.setdefault("_tpairs", []).append((src, dst))
            ops.transpose_cast_batched([(src, dst)])
            reg[key] = dst
        return reg[key]

    def hold_shadow(self, on):
        """The caller promises not to change the parameters while `on` (an evaluation loop, decode.test): the compute-dtype copy
        of the weights is refreshed once now and not again at every forward (a 94 MB conversion per utterance otherwise)."""
        self._hold = False
        if on:
            self.refresh_shadow()
        self._hold = bool(on)

    def attach_grads(self):
        """Make sure every p.grad is its arena view (zero_grad(set_to_none=True) drops them)."""
        missing = [n for n, p in zip(self.names, self.params) if p.grad is None or p.grad.data_ptr() != self.gviews[n].data_ptr()]
        if not missing:
            return
        if len(missing) == len(self.names):
            self.grad.zero_()
        for n, p in zip(self.names, self.params):
            if n in missing:
                if len(missing) != len(self.names):
                    self.gviews[n].zero_()
                p.grad = self.gviews[n]

    # views are created once and cached: the arena never moves
    def _cached(self, key, make):
        v = self._vcache.get(key)
        if v is None:
            v = self._vcache[key] = make()
        return v

    def _span(self, buf, first, last, shape):
        o0 = self.offsets[first]
        o1 = self.offsets[last] + self.pviews[last].numel()
        n = 1
        for s in shape:
            n *= s
        assert o1 - o0 == n, f"parameters {first}..{last} are not contiguous in the arena"
        return buf[o0:o1].view(shape)

    def w(self, name, shape=None):
        """compute-dtype view of a parameter (GEMM operand)"""
        def make():
            o = self.offsets[name]
            p = self.pviews[name]
            return self.shadow[o:o + p.numel()].view(shape if shape is not None else p.shape)
        return self._cached(("w", name, shape), make)

    def w_span(self, first, last, shape):
        return self._cached(("ws", first, last, shape), lambda: self._span(self.shadow, first, last, shape))

    def p(self, name):
        return self.pviews[name]

    def p_span(self, first, last, shape):
        return self._cached(("ps", first, last, shape), lambda: self._span(self.flat, first, last, shape))

    def g(self, name, shape=None):
        if shape is None:
            return self.gviews[name]
        return self._cached(("g", name, shape), lambda: self.gviews[name].view(shape))

    def g_span(self, first, last, shape):
        return self._cached(("gs", first, last, shape), lambda: self._span(self.grad, first, last, shape))


class ArenaView:
    """A ParamArena seen through a key prefix: the names an engine uses for its module (`encoder.*`, `decoder.*`) address the
    parameters of that module inside a larger model's arena (`lm.gmodel.encoder.*`), so that the whole model keeps ONE arena -- one
    fused optimizer update, one gradient norm.  names / params / offsets cover the prefixed parameters only; the buffers are the
    whole arena's."""

    def __init__(self, arena, prefix):
        self.arena, self.prefix = arena, prefix
        n = len(prefix)
        keep = [i for i, name in enumerate(arena.names) if name.startswith(prefix)]
        self.names = [arena.names[i][n:] for i in keep]
        self.params = [arena.params[i] for i in keep]
        self.offsets = {name[n:]: o for name, o in arena.offsets.items() if name.startswith(prefix)}
        self.pviews = {name[n:]: v for name, v in arena.pviews.items() if name.startswith(prefix)}
        self.gviews = {name[n:]: v for name, v in arena.gviews.items() if name.startswith(prefix)}

    flat = property(lambda self: self.arena.flat)
    grad = property(lambda self: self.arena.grad)
    shadow = property(lambda self: self.arena.shadow)
    size = property(lambda self: self.arena.size)
    compute_dtype = property(lambda self: self.arena.compute_dtype)

    def bound(self):
        return self.arena.bound()

    def refresh_shadow(self):
        self.arena.refresh_shadow()

    def hold_shadow(self, on):
        self.arena.hold_shadow(on)

    def attach_grads(self):
        self.arena.attach_grads()

    def transposed(self, first, last=None, shape=None):
        return self.arena.transposed(self.prefix + first, None if last is None else self.prefix + last, shape)

    def w(self, name, shape=None):
        return self.arena.w(self.prefix + name, shape)

    def w_span(self, first, last, shape):
        return self.arena.w_span(self.prefix + first, self.prefix + last, shape)

    def p(self, name):
        return self.arena.pviews[self.prefix + name]

    def p_span(self, first, last, shape):
        return self.arena.p_span(self.prefix + first, self.prefix + last, shape)

    def g(self, name, shape=None):
        return self.arena.g(self.prefix + name, shape)

    def g_span(self, first, last, shape):
        return self.arena.g_span(self.prefix + first, self.prefix + last, shape)


def sinusoid(positions, d, device):
    positions = positions.to(torch.float32).view(-1, 1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    out = torch.zeros(positions.shape[0], d)
    out[:, 0::2] = torch.sin(positions * div)
    out[:, 1::2] = torch.cos(positions * div)
    return out.to(device)


class _Stash:
    pass


# What the encoder sublayers' forwards leave for their backwards: the engine builds them from its kernels' outputs, layer_rt.LayerStash
# from views of the C++ layer runtime's workspaces.  They are tuples, so `x, mean, rstd, ... = record` holds.  x: the sublayer's
# input (the residual); mean, rstd, h: its LayerNorm; s_out: the seed of the output dropout.
# u: w1's pre-activation (option "ffn_save_dact": act'(u) * dropout_scale), a: the dropped activation, s_in: the inner dropout's seed
FFNStash = NamedTuple("FFNStash", [(f, object) for f in "x mean rstd h u a s_in s_out".split()])
# pp: the projected relative positions | None, s_att: the attention dropout's seed, sts: the stored scores S^T (EMOASR_ATTN_STORED=1) | None
AttnStash = NamedTuple("AttnStash", [(f, object) for f in "x mean rstd h qkv pp o lse s_att s_out sts".split()])
# g: pointwise_conv1's output, gl: GLU(g) | None (fused into the convolution), c: the depthwise convolution's output, z: BatchNorm + swish
ConvStash = NamedTuple("ConvStash", [(f, object) for f in "x mean rstd h g gl c bmean bvar z s_out".split()])
# one encoder layer; ffm, conv and fin = (x, mean, rstd) of the final LayerNorm are None in a Transformer layer
LayerRecord = NamedTuple("LayerRecord", [(f, object) for f in "ffm att conv ff fin".split()])


def h2d_pack(arrays, device):
    """several small host arrays (int32 / int64 / float32) -> device tensors through ONE pinned staging buffer and ONE asynchronous
    H2D copy (every piece 8-byte aligned); the per-step index tables of a stacked pass were six copies of a few hundred bytes"""
    ts = [torch.as_tensor(a).contiguous() for a in arrays]
    offs, total = [], 0
    for t in ts:
        offs.append(total)
        total += (t.numel() * t.element_size() + 7) // 8 * 8
    host = torch.empty(max(total, 8), dtype=torch.uint8).pin_memory()
    for t, o in zip(ts, offs):
        host[o:o + t.numel() * t.element_size()] = t.view(-1).view(torch.uint8)
    dev = host.to(device, non_blocking=True)
    return [dev[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape) for t, o in zip(ts, offs)]


def h2d_i32(values, device):
    """small host array -> int32 device tensor through pinned memory (asynchronous H2D); a tensor already on a device is converted
    where it lies"""
    t = torch.as_tensor(values, dtype=torch.int32)
    if torch.device(device).type == "cpu" or t.is_cuda:
        return t
    return t.pin_memory().to(device, non_blocking=True)
