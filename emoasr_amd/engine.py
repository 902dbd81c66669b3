"""Explicit forward/backward sequencing of the HIP kernels for the CTC models
(Conv2d front-end -> Transformer/Conformer encoder -> CTC head).

There is no autograd graph inside: forward() stashes what backward() needs, backward()
walks the layers in reverse calling the hand-written gradient kernels and accumulates
parameter gradients straight into a flat f32 gradient arena.  torch supplies device
memory and the stream only.

Reference behaviour being reproduced (file:line in /root/reference):
  encoder      asr/modeling/encoders/transformer.py:84-113, encoders/conv.py:20-28
  conformer    asr/modeling/conformer.py:47-54,77-95,121-143,191-229
  transformer  asr/modeling/transformer.py:43-45,96-99,117-118,143-153
  CTC          asr/modeling/decoders/ctc.py:103-115,176-201
"""
import math
import weakref
import os

import torch
from ctypes import c_void_p

from . import ops
from .ops import ACT_NONE, ACT_RELU, ACT_SWISH
from .recurrence import lstm_layer_bwd, lstm_layer_fwd

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


def sinusoid(positions, d, device):
    positions = positions.to(torch.float32).view(-1, 1)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    out = torch.zeros(positions.shape[0], d)
    out[:, 0::2] = torch.sin(positions * div)
    out[:, 1::2] = torch.cos(positions * div)
    return out.to(device)


class _Stash:
    pass


class _DecoderMixinPlaceholder:
    pass


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
    """small host array -> int32 device tensor through pinned memory (asynchronous H2D)"""
    t = torch.as_tensor(values, dtype=torch.int32)
    if torch.device(device).type == "cpu":
        return t
    return t.pin_memory().to(device, non_blocking=True)


class CTCEngine(_DecoderMixinPlaceholder):
    """Forward / backward of encoder + CTC head on HIP kernels."""

    def __init__(self, cfg, module, compute_dtype=torch.bfloat16, bn_buffers=None, f32_split=False):
        self.cfg = cfg
        # f32 storage with every product as three bf16 MFMAs over (hi, lo) operand pairs (csrc/gemm.hip SplitCfg): the
        # throughput mode that meets the 1e-3 bar; compute_dtype stays torch.float32
        self.split = bool(f32_split) and compute_dtype == torch.float32
        self.d = cfg.enc_hidden_size
        self.h = _cfg(cfg, "enc_num_attention_heads", 0)   # (an RNN encoder's config has no attention fields)
        self.nl = cfg.enc_num_layers
        self.conformer = cfg.encoder_type == "conformer"
        # bidirectional LSTM stack (encoders/rnn.py; _RNNEncMixin below) in place of the Transformer / Conformer layers
        self.rnn_enc = cfg.encoder_type == "rnn"
        self.rel = _cfg(cfg, "pos_encode_type", "abs") == "rel"
        # nn.Embedding front-end over token ids (encoders/transformer.py:35-36,87-89: the phone encoder of lm/modeling/p2w.py)
        self.embed_in = _cfg(cfg, "input_layer", "conv2d") == "embed"
        # intermediate branch after layer `inter_layer` (encoders/transformer.py:75-82); 0 = none
        inter_on = (_cfg(cfg, "mtl_inter_ctc_weight", 0) or 0) > 0 or (_cfg(cfg, "mtl_phone_ctc_weight", 0) or 0) > 0
        self.inter_layer = int(cfg.inter_ctc_layer_id) if inter_on else 0
        self.eouts_inter = None
        self._implicit_dgrad = os.environ.get("EMOASR_CONV2_DGRAD", "implicit") == "implicit"
        # the first convolution's weight gradient folded into the large-tile data gradient (emoasr_conv2_dgrad_w1; A/B switch)
        self._conv1_fold = os.environ.get("EMOASR_CONV1_FOLD", "1") != "0"
        # library options this engine's own launch sequence depends on, as they stand now (lib.load() applied the environment's
        # overrides); fixed per engine: "conv_fused" (csrc/convfused.hip, bit-identical), "ffn_save_dact" (the feed-forward blocks
        # save act'(u) * dropout_scale instead of u, csrc/common.h: EMO_ACT_SAVE_DACT), "conv_big" (csrc/gemm_big.hip)
        from . import lib as _lib
        self._conv_fused = _lib.get_option("conv_fused") != 0
        self._ffn_save_dact = _lib.get_option("ffn_save_dact") != 0
        self._conv_big = _lib.get_option("conv_big") != 0
        self.p_enc = float(_cfg(cfg, "dropout_enc_rate", 0.0))
        self.p_att = float(_cfg(cfg, "dropout_attn_rate", 0.0))
        self.dtype = compute_dtype
        self.module = module
        self.arena = ParamArena(module, compute_dtype)
        self._tables = {}
        self._scratch_cache = {}
        # weight gradients of one encoder layer as one grouped launch (EMOASR_WGRAD_GROUP=0: one by one)
        self._group_wgrads = os.environ.get("EMOASR_WGRAD_GROUP", "1") != "0"
        self._defer_wgrads = False
        self._wq = []
        self._ln_deferred = []
        # data parallelism: callable(lo) told after every encoder layer's backward that all gradients at
        # arena offsets >= lo are final (train.GradBuckets.ready overlaps their all-reduce with the rest)
        self.grad_hook = None
        self._layer_lo = None
        # Conformer layers sequenced in C++ (EMOASR_CPP_LAYER=0: one FFI call per kernel from Python)
        self._cpp_layers = os.environ.get("EMOASR_CPP_LAYER", "1") != "0"
        self._layer_rt = None
        # EMOASR_WGRAD_SIDE=1: run them on a side stream (measured slower on MI355X: 13.97 vs 13.62 ms/step)
        self._side_wgrads = os.environ.get("EMOASR_WGRAD_SIDE", "0") != "0"
        self._side, self._inflight = None, []
        # keep the scaled scores S^T of the forward for the backward (1) or recompute them (0)
        self.attn_store_scores = os.environ.get("EMOASR_ATTN_STORED", "0") == "1"
        # bf16 attention backward as ONE score recomputation (EMOASR_ATTN_FUSED=0: the materialised three-GEMM path)
        self.attn_fused = os.environ.get("EMOASR_ATTN_FUSED", "1") != "0"
        self._bufs = {}
        # greedy decoding in bf16 takes the arg-max over f32 logits (EMOASR_F32_HEAD=0: over logits rounded to bf16)
        self.f32_head = os.environ.get("EMOASR_F32_HEAD", "1") != "0"
        self.seed = 0x5EED
        if _cfg(cfg, "decoder_type", "ctc") == "transformer":
            self._dec_init()
        if _cfg(cfg, "decoder_type", "ctc") == "rnn_transducer":
            self._rnnt_init()
        if _cfg(cfg, "decoder_type", "ctc") == "las":
            self._las_init()
        self.step_count = 0

    # ------------------------------------------------------------------ helpers
    def ensure_bound(self):
        if not self.arena.bound():
            # the parameters were moved / re-created (model.cpu().cuda(), .to(dtype), load_state_dict on another
            # device): re-home them and drop everything derived from the old arena's addresses
            self.arena = ParamArena(self.module, self.dtype)
            self._layer_lo = None
            self._layer_rt = None
            self._bufs = {}
            self._scratch_cache = {}

    def _pos_table(self, T, device, max_len=5000):
        """sinusoid table slice for T frames; the full table is built once (like the reference's
        max_len=5000 tables, conformer.py:17,23 / transformer.py:16,22) and sliced per batch."""
        max_len = max(max_len, T)
        key = (self.rel, max_len, str(device))
        if key not in self._tables:
            if self.rel:
                tab = sinusoid(torch.arange(max_len - 1, -max_len, -1), self.d, device)  # row r <-> rel = max_len-1-r
            else:
                tab = sinusoid(torch.arange(max_len), self.d, device)
            self._tables[key] = tab
        tab = self._tables[key]
        if self.rel:
            return tab[max_len - T: max_len - 1 + T]  # rows <-> rel = T-1 ... -(T-1)
        return tab[:T]

    def _seed(self, site):
        return (self.seed * 1000003 + self.step_count * 4099 + site) & 0xFFFFFFFFFFFF

    def _apply_mode(self):
        """this engine's mode of the f32 products for the calling thread: exact f32 MFMAs, or "f32x3" -- the dtype code lib.F32X3 that
        ops.dt() then puts into every C call (the library itself keeps no mode)"""
        ops.split_products(self.split)   # this thread's f32 products from here on: the dtype code of every call (ops.dt)

    def _scope(self):
        return ops.stream_scope(self.split)

    def _buffers(self, name):
        b = self._bufs.get(name)
        if b is None or not b.is_cuda:
            self._bufs = dict(self.module.named_buffers())
            b = self._bufs[name]
        return b

    # ------------------------------------------------------------------ forward
    def forward(self, xs, xlens_host, training, stash=None):
        """xs f32 [B,T,F] (device), xlens_host: python list / CPU tensor.
        -> eouts [B,T',d] (compute dtype), elens (list), stash (or None)"""
        with self._scope():
            if self.rnn_enc:
                return self._rnn_enc_forward(xs, xlens_host, training, stash)
            return self._forward(xs, xlens_host, training, stash)

    def _forward(self, xs, xlens_host, training, stash):
        self.ensure_bound()  # (may swap in a new arena: bind `A` only afterwards)
        A, d, dt = self.arena, self.d, self.dtype
        A.refresh_shadow()
        stash = training if stash is None else stash
        self._keep = stash
        st = _Stash() if stash else None
        p_enc = self.p_enc if training else 0.0
        p_att = self.p_att if training else 0.0
        B, T = xs.shape[:2]
        dev = xs.device
        xlens_host = [int(v) for v in xlens_host]
        if self.embed_in:
            return self._forward_embed(xs, xlens_host, training, stash, st)
        elens_host = [((v - 1) // 2 - 1) // 2 for v in xlens_host]
        elens = h2d_i32(elens_host, dev)
        x, y1, y2, w2r, wlr = self._frontend_fwd(xs)
        T2, F2 = y2.shape[1], y2.shape[2]
        M = B * T2
        # ---- positional encoding --------------------------------------------------
        tab = self._pos_table(T2, dev)
        scale = math.sqrt(d)
        s_pe = self._seed(1)
        if self.rel:
            x = ops.posenc(x.view(B, T2, d), None, scale, p_enc, s_pe).view(M, d)
            pos_t = ops.scale_dropout(ops.strided_copy(tab, out_dtype=dt), 1.0, p_enc, self._seed(2)) \
                if p_enc > 0 else ops.strided_copy(tab, out_dtype=dt)
        else:
            x = ops.posenc(x.view(B, T2, d), tab, scale, p_enc, s_pe).view(M, d)
            pos_t = None
        if st is not None:
            st.xs, st.y1, st.y2, st.w2r, st.wlr, st.pos_t = xs, y1, y2, w2r, wlr, pos_t
            st.B, st.T2, st.F2, st.M, st.elens = B, T2, F2, M, elens
            st.layers = []
            st.s_pe = s_pe
        if self._cpp_layers and self.conformer and self.rel and not self.attn_store_scores:
            # one C-ABI call per layer (csrc/layer.hip); intermediates land in per-layer workspaces and
            # become tensors only when the backward sweep asks for them (layer_rt.LayerStash)
            if self._layer_rt is None:
                from .layer_rt import ConformerLayerRuntime
                self._layer_rt = ConformerLayerRuntime(self)
            cur = x
            for li in range(self.nl):
                cur = self._layer_rt.forward(li, cur, B, T2, elens, pos_t, p_enc, p_att, training, self._keep)
                if st is not None:
                    st.layers.append(cur)
                if li + 1 == self.inter_layer:
                    x_inter = cur.tv("y")
            x = cur.tv("y")
        else:
            for li in range(self.nl):
                x, ls = self._layer_fwd(li, x, B, T2, elens, pos_t, p_enc, p_att, training)
                if st is not None:
                    st.layers.append(ls)
                if li + 1 == self.inter_layer:
                    x_inter = x
        # the intermediate branch goes through the SAME final LayerNorm (encoders/transformer.py:104-107)
        self.eouts_inter = None
        if self.inter_layer > 0:
            ei, mi, ri = ops.layernorm_fwd(x_inter, A.p("encoder.norm.weight"), A.p("encoder.norm.bias"), 1e-12, stash)
            self.eouts_inter = ei.view(B, T2, d)
            if st is not None:
                st.x_inter, st.int_mean, st.int_rstd = x_inter, mi, ri
        eouts, mean, rstd = ops.layernorm_fwd(x, A.p("encoder.norm.weight"), A.p("encoder.norm.bias"), 1e-12, stash)
        if st is not None:
            st.x_final, st.fin_mean, st.fin_rstd = x, mean, rstd
        return eouts.view(B, T2, d), elens_host, elens, st

    def _forward_embed(self, ids, xlens_host, training, stash, st):
        """the absolute-position Transformer stack over token ids int32 [B,P] (input_layer "embed": x = embed(ids) * sqrt(d) + pe,
        dropout -- the reference's PositionalEncoder -- and elens = xlens)"""
        A, d = self.arena, self.d
        B, T = ids.shape
        dev = ids.device
        M = B * T
        p_enc = self.p_enc if training else 0.0
        p_att = self.p_att if training else 0.0
        elens = h2d_i32(xlens_host, dev)
        s_pe = self._seed(1)
        x = ops.embed_fwd(ids, A.w("encoder.embed.weight"), self._pos_table(T, dev), math.sqrt(d), p_enc, s_pe).view(M, d)
        if st is not None:
            st.ids, st.B, st.T2, st.M, st.elens, st.s_pe, st.p_enc, st.layers = ids, B, T, M, elens, s_pe, p_enc, []
        for li in range(self.nl):
            x, ls = self._layer_fwd(li, x, B, T, elens, None, p_enc, p_att, training)
            if st is not None:
                st.layers.append(ls)
        self.eouts_inter = None
        eouts, mean, rstd = ops.layernorm_fwd(x, A.p("encoder.norm.weight"), A.p("encoder.norm.bias"), 1e-12, stash)
        if st is not None:
            st.x_final, st.fin_mean, st.fin_rstd = x, mean, rstd
        return eouts.view(B, T, d), xlens_host, elens, st

    def _frontend_fwd(self, xs):
        """Conv2d subsampling (encoders/conv.py:20-28, channels-last) of xs f32 [B,T,F] -> (x [B*T',d] compute dtype, and the
        y1, y2, w2r, wlr that _frontend_bwd needs)"""
        A, d, dt = self.arena, self.d, self.dtype
        B = xs.shape[0]
        pre = "encoder.conv."
        C = d
        w1 = A.p(pre + "conv.0.weight").view(C, 9)
        y1 = ops.conv1_fwd(xs, w1, A.p(pre + "conv.0.bias"), dt)
        w2r = ops.strided_copy(A.p(pre + "conv.2.weight").permute(0, 2, 3, 1), out_dtype=dt).view(C, 9 * C)
        y2 = ops.conv2_fwd(y1, w2r, bias=A.p(pre + "conv.2.bias"), act=ACT_RELU)
        T2, F2 = y2.shape[1], y2.shape[2]
        wl = A.p(pre + "output.weight")  # [d, C*F2] channel-major -> [d, F2*C]
        wlr = ops.strided_copy(wl.view(d, C, F2).permute(0, 2, 1), out_dtype=dt).view(d, F2 * C)
        M = B * T2
        x = ops.gemm_nt(y2.view(M, F2 * C), wlr, bias=A.p(pre + "output.bias"))
        return x, y1, y2, w2r, wlr

    def _ffn_fwd(self, name, x, res_scale, act, norm_name, eps, p_enc, site, training):
        A = self.arena
        h, mean, rstd = ops.layernorm_fwd(x, A.p(norm_name + ".weight"), A.p(norm_name + ".bias"), eps, self._keep)
        u = torch.empty(x.shape[0], A.p(name + ".w1.weight").shape[0], device=x.device, dtype=x.dtype) if self._keep else None
        s_in, s_out = self._seed(site), self._seed(site + 1)
        a = ops.gemm_nt(h, A.w(name + ".w1.weight"), bias=A.p(name + ".w1.bias"),
                        act=act | (ops.ACT_SAVE_DACT if (self._ffn_save_dact and u is not None) else 0), pre_out=u,
                        drop_p=p_enc, seed=s_in)   # (save_dact: `u` holds act'(u) * dropout_scale, what _ffn_bwd multiplies by)
        y = ops.gemm_nt(a, A.w(name + ".w2.weight"), bias=A.p(name + ".w2.bias"), residual=x, res_scale=res_scale,
                        drop_p=p_enc, seed=s_out)
        return y, (x, mean, rstd, h, u, a, s_in, s_out)

    def _attn_fwd(self, name, x, B, T, elens, pos_t, norm_name, eps, p_enc, p_att, site, training, dims=None,
                  causal=False):
        A = self.arena
        d, H = dims if dims is not None else (self.d, self.h)
        h, mean, rstd = ops.layernorm_fwd(x, A.p(norm_name + ".weight"), A.p(norm_name + ".bias"), eps, self._keep)
        wqkv = A.w_span(name + ".linear_q.weight", name + ".linear_v.weight", (3 * d, d))
        bqkv = A.p_span(name + ".linear_q.bias", name + ".linear_v.bias", (3 * d,))
        qkv = ops.gemm_nt(h, wqkv, bias=bqkv).view(B, T, 3 * d)
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        s_att, s_out = self._seed(site), self._seed(site + 1)
        scale = 1.0 / math.sqrt(d // H)
        if pos_t is not None:
            pp = ops.gemm_nt(pos_t, A.w(name + ".linear_pos.weight"))
            bu, bv = A.p(name + ".pos_bias_u").view(-1), A.p(name + ".pos_bias_v").view(-1)
        else:
            pp = bu = bv = None
        if self._keep and self.attn_store_scores:
            o, lse, sts = ops.attn_fwd(q, k, v, H, scale, pos=pp, bias_u=bu, bias_v=bv, klens=elens, drop_p=p_att,
                                       seed=s_att, store_scores=True, causal=causal)
        else:
            o, lse = ops.attn_fwd(q, k, v, H, scale, pos=pp, bias_u=bu, bias_v=bv, klens=elens, drop_p=p_att,
                                  seed=s_att, causal=causal)
            sts = None
        y = ops.gemm_nt(o.view(B * T, d), A.w(name + ".linear_out.weight"), bias=A.p(name + ".linear_out.bias"),
                        residual=x, res_scale=1.0, drop_p=p_enc, seed=s_out)
        return y, (x, mean, rstd, h, qkv, pp, o, lse, s_att, s_out, sts)

    def _conv_fwd(self, name, x, B, T, norm_name, p_enc, site, training):
        A, d = self.arena, self.d
        h, mean, rstd = ops.layernorm_fwd(x, A.p(norm_name + ".weight"), A.p(norm_name + ".bias"), 1e-5, self._keep)
        g = ops.gemm_nt(h, A.w(name + ".pointwise_conv1.weight", (2 * d, d)), bias=A.p(name + ".pointwise_conv1.bias"))
        wd = A.p(name + ".depthwise_conv.weight")
        bn = name + ".batch_norm"
        rm, rv = self._buffers(bn + ".running_mean"), self._buffers(bn + ".running_var")
        wdk, bd = wd.view(d, wd.shape[-1]), A.p(name + ".depthwise_conv.bias")
        fused = self._conv_fused and g.dtype == torch.bfloat16  # GLU inside the convolution's staging pass (convfused.hip)
        gl = None if fused else ops.glu_fwd(g)
        if fused:
            c, bmean, bvar = ops.glu_dwconv_fwd(g, B, T, wdk, bd, rm, rv, 0.1, self._buffers(bn + ".num_batches_tracked"),
                                                training)
        elif training:  # batch statistics come out of the conv kernel (per-block partials + one merge)
            c, bmean, bvar = ops.dwconv_bn_stats_fwd(gl.view(B, T, d), wdk, bd, rm, rv, 0.1,
                                                     self._buffers(bn + ".num_batches_tracked"))
        else:
            c, bmean, bvar = ops.dwconv_fwd(gl.view(B, T, d), wdk, bd), rm, rv
        c = c.view(B * T, d)
        z = ops.bn_swish_fwd(c, bmean, bvar, A.p(bn + ".weight"), A.p(bn + ".bias"), 1e-5)
        s_out = self._seed(site)
        y = ops.gemm_nt(z, A.w(name + ".pointwise_conv2.weight", (d, d)), bias=A.p(name + ".pointwise_conv2.bias"),
                        residual=x, res_scale=1.0, drop_p=p_enc, seed=s_out)
        return y, (x, mean, rstd, h, g, gl, c, bmean, bvar, z, s_out)

    def _layer_fwd(self, li, x, B, T, elens, pos_t, p_enc, p_att, training):
        name = f"encoder.transformers.{li}"
        site = 100 + li * 20
        A = self.arena
        if self.conformer:
            x, s_ffm = self._ffn_fwd(name + ".feed_forward_macaron", x, 0.5, ACT_SWISH, name + ".norm_ff_macaron", 1e-5,
                                     p_enc, site, training)
            if self.rel:
                x, s_att = self._attn_fwd(name + ".self_attn", x, B, T, elens, pos_t, name + ".norm_self_attn", 1e-5,
                                          p_enc, p_att, site + 2, training)
                x, s_conv = self._conv_fwd(name + ".conv", x, B, T, name + ".norm_conv", p_enc, site + 4, training)
            else:
                x, s_conv = self._conv_fwd(name + ".conv", x, B, T, name + ".norm_conv", p_enc, site + 4, training)
                x, s_att = self._attn_fwd(name + ".self_attn", x, B, T, elens, None, name + ".norm_self_attn", 1e-5,
                                          p_enc, p_att, site + 2, training)
            x, s_ff = self._ffn_fwd(name + ".feed_forward", x, 0.5, ACT_SWISH, name + ".norm_ff", 1e-5, p_enc, site + 6,
                                    training)
            y, mean, rstd = ops.layernorm_fwd(x, A.p(name + ".norm_final.weight"), A.p(name + ".norm_final.bias"), 1e-5,
                                              self._keep)
            return y, (s_ffm, s_att, s_conv, s_ff, (x, mean, rstd))
        x, s_att = self._attn_fwd(name + ".self_attn", x, B, T, elens, None, name + ".norm1", 1e-12, p_enc, p_att,
                                  site + 2, training)
        x, s_ff = self._ffn_fwd(name + ".feed_forward", x, 1.0, ACT_RELU, name + ".norm2", 1e-12, p_enc, site + 6, training)
        return x, (None, s_att, None, s_ff, None)

    # ------------------------------------------------------------------ CTC head
    def head_logits(self, eouts, head="decoder.output", out_f32=False):
        """out_f32 (decoding in bf16 only): the logits leave the product as f32 instead of being rounded to bf16 -- an arg-max
        over 10 000 bf16 logits flips on every pair closer than one bf16 ulp (0.03-0.06 at |logit| ~ 8); see bench `bf16_vs_f32`"""
        self._apply_mode()
        B, T, d = eouts.shape
        A = self.arena
        w = A.w(head + ".weight")
        V = w.shape[0]
        out = None
        if V % 8:  # ragged vocabulary (phone heads): rows padded to the GEMMs' 16-byte leading-dimension rule
            out = torch.empty(B * T, (V + 7) // 8 * 8, device=eouts.device, dtype=eouts.dtype)[:, :V]
            out_f32 = False
        if out_f32 and eouts.dtype != torch.float32:
            logits = ops.gemm_nt(eouts.reshape(B * T, d), w, bias=A.p(head + ".bias"), out_f32=True)
        else:
            logits = ops.gemm_nt(eouts.reshape(B * T, d), w, out=out, bias=A.p(head + ".bias"))
        return logits.view(B, T, V)

    def ctc_loss(self, logits, elens, ys_host, ylens_host, blank, want_grad, gscale_over_b=None):
        """-> (loss 0-dim f32 tensor = sum_b nll_b / B with infeasible utterances zeroed, ctx)"""
        self._apply_mode()
        B, T, V = logits.shape
        dev = logits.device
        ylens_host = [int(v) for v in ylens_host]
        Lmax = max(max(ylens_host), 1)
        labels = torch.as_tensor(ys_host)[:, :Lmax].to(torch.int32)
        if labels.shape[1] < Lmax:
            labels = torch.nn.functional.pad(labels, (0, Lmax - labels.shape[1]))
        labels = h2d_i32(labels.contiguous(), dev)
        ylens = h2d_i32(ylens_host, dev)
        lse = ops.row_lse(logits.view(B * T, V))
        lp, alpha, beta, nll = ops.ctc_forward(logits, lse, labels, elens, ylens, blank)
        loss = torch.where(torch.isfinite(nll), nll, torch.zeros_like(nll)).sum() / B
        ctx = (logits, lse, labels, elens, ylens, blank, lp, alpha, beta, nll) if want_grad else None
        return loss, ctx

    def ctc_grad(self, ctx, gscale, gscale_dev=None):
        self._apply_mode()
        logits, lse, labels, elens, ylens, blank, lp, alpha, beta, nll = ctx
        return ops.ctc_grad(logits, lse, labels, elens, ylens, blank, lp, alpha, beta, nll, gscale / logits.shape[0],
                            gscale_dev)

    def greedy(self, logits, elens, blank):
        best, hyp, hyplen = ops.ctc_greedy(logits, elens, blank)
        return best, hyp, hyplen

    # ------------------------------------------------------------------ stacked micro-batches
    def stacked_ok(self):
        """can ctc_train_stacked take this model?  (bf16 relative-position Conformer + plain CTC head, the layer runtime and
        the single-pass attention backward on, no intermediate / distillation branches)"""
        cfg = self.cfg
        return (self.encoder_stacked_ok() and _cfg(cfg, "decoder_type", "ctc") == "ctc"
                and not (_cfg(cfg, "kd_weight", 0) or 0) > 0)

    def ctc_train_stacked(self, batches, blank, scales=None, head="decoder.output"):
        """Forward + CTC loss + backward of several micro-batches in ONE stacked pass (asr/train_asr.py:106-128 runs them one
        after the other and sums their gradients: `accum_grad`).  Rows of all micro-batches are concatenated for every row-wise
        kernel (Linear / LayerNorm / pointwise convolutions / vocabulary head); attention, the depthwise convolution's padding
        and the BatchNorm statistics stay per micro-batch (include/emoasr_hip.h: emoasr_segments_t), so the result is the sum
        of the separate passes' gradients up to summation order.

        batches: [(xs f32 [B,T,F] on the device, xlens, ys (host int tensor [B,L]), ylens), ...] (at most lib.MAX_SEGMENTS)
        scales:  weight of every micro-batch's loss in the gradient (default 1 / len(batches) = loss / accum_grad)
        -> losses f32 [n] (device): loss_s = sum_b nll_b / B_s, infeasible utterances zeroed, as nn.CTCLoss(zero_infinity)
        Parameter gradients are ACCUMULATED into the gradient arena (p.grad)."""
        assert self.stacked_ok(), "ctc_train_stacked: unsupported configuration (see stacked_ok)"
        self._defer_wgrads = self._group_wgrads
        try:
            with self._scope():
                return self._ctc_train_stacked(batches, blank, scales, head)
        finally:
            self._defer_wgrads = False
            self._wq = []
            self._ln_deferred = []

    def _stack_dtype_ok(self, single=False):
        """bf16 always; f32 (exact or split products, the materialised attention backward per micro-batch) unless switched off:
        EMOASR_F32_CPP_BWD=0 sequences the f32 gradient kernels from the host, EMOASR_F32_STACKED=0 runs f32 micro-batches one by one"""
        if self.dtype == torch.bfloat16:
            return True
        if os.environ.get("EMOASR_F32_CPP_BWD", "1") == "0":
            return False
        return single or os.environ.get("EMOASR_F32_STACKED", "1") != "0"

    def encoder_stacked_ok(self):
        """can the ENCODER take several micro-batches in one stacked pass (any decoder on top)?"""
        return (self.conformer and self.rel and self._stack_dtype_ok() and self._cpp_layers and self.attn_fused
                and not self.attn_store_scores and not self._side_wgrads and self.inter_layer == 0
                and os.environ.get("EMOASR_CPP_BWD", "1") != "0" and self._implicit_dgrad and self._conv_big
                and self.d % 256 == 0 and os.environ.get("EMOASR_STACKED", "1") != "0")

    def _encoder_fwd_stacked(self, xs_list, xlens_list, elens_dev=None):
        """Conv2d front-end per micro-batch, everything after it over the stacked rows.
        -> (eouts [M, d], stash): segment k = rows st.rows[k] .. st.rows[k + 1] as [B_k, T_k, d]"""
        from . import lib
        self.ensure_bound()
        A, d, dt = self.arena, self.d, self.dtype
        A.refresh_shadow()
        A.attach_grads()
        self.step_count += 1
        self._keep = True
        n = len(xs_list)
        assert 1 <= n <= lib.MAX_SEGMENTS
        dev = xs_list[0].device
        p_enc, p_att = self.p_enc, self.p_att
        pre = "encoder.conv."
        C = d
        # ---- Conv2d subsampling per micro-batch (its own padded length), outputs stacked row-wise ----------------
        w1 = A.p(pre + "conv.0.weight").view(C, 9)
        w2r = ops.strided_copy(A.p(pre + "conv.2.weight").permute(0, 2, 3, 1), out_dtype=dt).view(C, 9 * C)
        y1s, segs, xlens_all = [], [], []
        for xs, xlens in zip(xs_list, xlens_list):
            B, T, Fd = xs.shape
            T1, F1 = (T - 3) // 2 + 1, (Fd - 3) // 2 + 1
            T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
            segs.append((B, T2))
            xlens_all += [int(v) for v in xlens]
        rows = [0]
        for b, t in segs:
            rows.append(rows[-1] + b * t)
        M = rows[-1]
        elens_host = [((v - 1) // 2 - 1) // 2 for v in xlens_all]
        elens = elens_dev if elens_dev is not None else h2d_i32(elens_host, dev)
        if self._layer_rt is None:
            from .layer_rt import ConformerLayerRuntime
            self._layer_rt = ConformerLayerRuntime(self)
        Btot, Tmax = sum(b for b, _ in segs), max(t for _, t in segs)
        # the layers' attention keep masks as bits, all hashed now on the attention's side stream: under the front-end's products
        masks = None
        if p_att > 0 and dt == torch.bfloat16 and os.environ.get("EMOASR_MASKS_UPFRONT", "1") != "0":
            masks = self._layer_rt.hash_attn_masks(self.nl, Btot, Tmax, elens, p_att, tuple(segs))
        y2 = torch.empty(M, F2 * C, device=dev, dtype=dt)
        for k, xs in enumerate(xs_list):
            y1 = ops.conv1_fwd(xs, w1, A.p(pre + "conv.0.bias"), dt)
            ops.conv2_fwd(y1, w2r, out=y2[rows[k]:rows[k + 1]], bias=A.p(pre + "conv.2.bias"), act=ACT_RELU)
            y1s.append(y1)
        wl = A.p(pre + "output.weight")  # [d, C*F2] channel-major -> [d, F2*C]
        wlr = ops.strided_copy(wl.view(d, C, F2).permute(0, 2, 1), out_dtype=dt).view(d, F2 * C)
        x = ops.gemm_nt(y2, wlr, bias=A.p(pre + "output.bias"))
        s_pe = self._seed(1)
        x = ops.posenc(x.view(1, M, d), None, math.sqrt(d), p_enc, s_pe).view(M, d)
        # every micro-batch has its own relative-position table (rows <-> rel = T-1 ... -(T-1)), dropped out independently
        tab = torch.cat([self._pos_table(t, dev) for _, t in segs], 0)
        pos_t = ops.strided_copy(tab, out_dtype=dt)
        if p_enc > 0:
            pos_t = ops.scale_dropout(pos_t, 1.0, p_enc, self._seed(2))
        # ---- encoder layers: one C-ABI call each over the stacked rows ------------------------------------------------
        cur, layers = x, []
        for li in range(self.nl):
            cur = self._layer_rt.forward(li, cur, Btot, Tmax, elens, pos_t, p_enc, p_att, True, True, segs=tuple(segs),
                                         att_mask=None if masks is None else masks[li])
            layers.append(cur)
        x_final = cur.tv("y")
        eouts, fin_mean, fin_rstd = ops.layernorm_fwd(x_final, A.p("encoder.norm.weight"), A.p("encoder.norm.bias"), 1e-12, True)
        st = _Stash()
        st.xs_list, st.y1s, st.y2, st.wlr, st.segs, st.rows, st.M, st.F2 = xs_list, y1s, y2, wlr, segs, rows, M, F2
        st.elens, st.elens_host, st.s_pe, st.layers = elens, elens_host, s_pe, layers
        st.pos_t = pos_t   # (the layers' C structs hold its raw address: it must live until the backward sweep is done)
        st.att_masks = masks   # (likewise)
        st.x_final, st.fin_mean, st.fin_rstd, st.Btot, st.Tmax = x_final, fin_mean, fin_rstd, Btot, Tmax
        return eouts, st

    def _encoder_bwd_stacked(self, st, deouts):
        """deouts [M, d] (compute dtype): gradient w.r.t. the stacked encoder output; accumulates every encoder gradient"""
        A, d, dt = self.arena, self.d, self.dtype
        dev = deouts.device
        M, F2, C, rows = st.M, st.F2, self.d, st.rows
        pre = "encoder.conv."
        dx, _ = self._ln_bwd(deouts, st.x_final, "encoder.norm", st.fin_mean, st.fin_rstd, None, None)
        lnf = ops.lib.size_query("emoasr_layernorm_bwd_scratch_floats", d)
        ln_parts = torch.empty(self.nl, 5, lnf, device=dev, dtype=torch.float32)
        dx_bufs = [torch.empty(M, d, device=dev, dtype=dt) for _ in range(2)]
        for li in reversed(range(self.nl)):
            out = dx_bufs[li & 1]
            self._layer_rt.backward(li, st.layers[li], dx, out, ln_parts[li], self._ln_deferred)
            dx = out
            if self.grad_hook is not None:
                self._flush_wgrads()
                ops.layernorm_bwd_finalize(self._ln_deferred)
                self._hook_after_layer(li)
        self._flush_wgrads()
        self._layer_rt.join_wgrads()
        ops.layernorm_bwd_finalize(self._ln_deferred)
        if self.grad_hook is not None and self._layer_rt.wgrad_side:
            self.grad_hook(self._layer_offset(0))
        # positional scaling, Linear (all rows at once), then the two convolutions per micro-batch
        dlin = ops.scale_dropout(dx, math.sqrt(d), self.p_enc, st.s_pe)
        dwl = torch.zeros(d, F2 * C, device=dev, dtype=torch.float32)  # (f, c) order
        ops.gemm_tn(dlin, st.y2, out=dwl, accumulate=True, colsum=A.g(pre + "output.bias"))
        ops.strided_copy(dwl.view(d, F2, C).permute(0, 2, 1), out=A.g(pre + "output.weight").view(d, C, F2), accumulate=True)
        dy2 = ops.gemm_nn(dlin, st.wlr, dact_pre=st.y2, dact=ACT_RELU)
        dw2 = torch.zeros(C, 9 * C, device=dev, dtype=torch.float32)
        kc = dt == torch.bfloat16   # the large-tile kernel's data gradient (all four parity classes in one launch) is bf16 only
        if kc:
            wt = ops.strided_copy(A.p(pre + "conv.2.weight").permute(1, 2, 3, 0), out_dtype=dt).view(C, 9 * C)
        else:
            w2r = ops.strided_copy(A.p(pre + "conv.2.weight").permute(0, 2, 3, 1), out_dtype=dt).view(C, 9 * C)
        dw1, db1 = A.g(pre + "conv.0.weight").view(C, 9), A.g(pre + "conv.0.bias")
        # conv2's weight gradient over all micro-batches as one reduction (bf16, C % 256 == 0: one launch of the 256-tile kernel
        # pays the split-K atomics into dw2 once; the library falls back to one launch per micro-batch when "tn_big" is off)
        seg_wgrad = kc and C % 256 == 0 and len(st.xs_list) <= ops.lib.CONV2_WGRAD_SEGMENTS
        if seg_wgrad:
            ops.conv2_wgrad_seg([(dy2[rows[k]:rows[k + 1]].view(-1, C), st.y1s[k]) for k in range(len(st.xs_list))], dw2,
                                dbias=A.g(pre + "conv.2.bias"))
        for k, xs in enumerate(st.xs_list):
            dy2_k = dy2[rows[k]:rows[k + 1]].view(-1, C)
            if not seg_wgrad:
                ops.conv2_wgrad(dy2_k, st.y1s[k], dw2, dbias=A.g(pre + "conv.2.bias"), accumulate=True)
            if kc and self._conv1_fold:   # conv1's weight gradient in the data gradient's epilogue: dy1 never reaches HBM
                ops.conv2_dgrad_w1(dy2_k, wt, st.y1s[k], xs, dw1, db1, accumulate=True)
                continue
            dy1 = ops.conv2_dgrad_kc(dy2_k, wt, st.y1s[k]) if kc else ops.conv2_dgrad(dy2_k, w2r, st.y1s[k])
            ops.conv1_wgrad(xs, dy1, dw1, db1, accumulate=True)
        ops.strided_copy(dw2.view(C, 3, 3, C).permute(0, 3, 1, 2), out=A.g(pre + "conv.2.weight"), accumulate=True)

    def encoder_forward_stacked(self, xs_list, xlens_list):
        """the encoder over several micro-batches in one stacked pass, for ANY decoder on top (modeling/functions.py:
        encoder_apply_stacked wraps it into autograd).  -> (eouts [M, d], stash)"""
        assert self.encoder_stacked_ok(), "encoder_forward_stacked: unsupported configuration (see encoder_stacked_ok)"
        with self._scope():
            return self._encoder_fwd_stacked(xs_list, xlens_list)

    def encoder_backward_stacked(self, st, deouts):
        self._defer_wgrads = self._group_wgrads
        try:
            with self._scope():
                self._encoder_bwd_stacked(st, deouts)
        finally:
            self._defer_wgrads = False
            self._wq = []
            self._ln_deferred = []

    def _ctc_train_stacked(self, batches, blank, scales, head):
        A = self.arena
        n = len(batches)
        scales = [1.0 / n] * n if scales is None else [float(v) for v in scales]
        # every index table of the pass (encoder lengths, labels, per-utterance rows / padded lengths / gradient scales) goes up
        # in ONE pinned copy before the first kernel
        dev = batches[0][0].device
        segs_h, rows_h = [], [0]
        for xs, _, _, _ in batches:
            Bk, Tk, Fd = xs.shape
            T1 = (Tk - 3) // 2 + 1
            segs_h.append((Bk, (T1 - 3) // 2 + 1))
            rows_h.append(rows_h[-1] + Bk * segs_h[-1][1])
        elens_h = [((int(v) - 1) // 2 - 1) // 2 for b in batches for v in b[1]]
        ylens_all = [int(v) for _, _, _, yl in batches for v in yl]
        Lmax = max(max(ylens_all), 1)
        lab = torch.zeros(sum(b for b, _ in segs_h), Lmax, dtype=torch.int32)
        row0, tpad, uscale, b0 = [], [], [], 0
        segw = torch.zeros(n, sum(b for b, _ in segs_h), dtype=torch.float32)   # [segment, utterance]: 1 / B_k on the segment's own
        for k, (_, _, ys, ylens) in enumerate(batches):
            B, T2 = segs_h[k]
            yk = torch.as_tensor(ys)[:, :Lmax].to(torch.int32)
            lab[b0:b0 + B, : yk.shape[1]] = yk
            row0 += [rows_h[k] + b * T2 for b in range(B)]
            tpad += [T2] * B
            uscale += [scales[k] / B] * B
            segw[k, b0:b0 + B] = 1.0 / B
            b0 += B
        elens_d, labels, yl, row0_d, tpad_d, uscale_d, segw_d = h2d_pack(
            [torch.tensor(elens_h, dtype=torch.int32), lab, torch.tensor(ylens_all, dtype=torch.int32),
             torch.tensor(row0, dtype=torch.int64), torch.tensor(tpad, dtype=torch.int32),
             torch.tensor(uscale, dtype=torch.float32), segw], dev)
        eouts, st = self._encoder_fwd_stacked([b[0] for b in batches], [b[1] for b in batches], elens_dev=elens_d)
        segs, rows, elens, Btot, Tmax = st.segs, st.rows, st.elens, st.Btot, st.Tmax
        assert list(segs) == segs_h and list(rows) == rows_h
        # ---- vocabulary head over all rows; CTC lattices per micro-batch -----------------------------------------------
        w = A.w(head + ".weight")
        V = w.shape[0]
        assert V % 8 == 0, "ctc_train_stacked: vocabulary must be a multiple of 8"
        # the vocabulary projection with the soft-max denominators out of its epilogue: one pass over the 703 MB of logits
        logits, lse = ops.gemm_nt_lse(eouts, w, A.p(head + ".bias"))
        # the gradient rows are padded to a multiple of 64 columns (zero pad): full-line stores, and its product with the weight
        # becomes an NT product over the padded columns that the large-tile kernel takes (35 145 x 256 x 10 048: 224 us against
        # 371 us on the 64 x 64 NN kernel, tools/big_n256_probe.py)
        Vp = (V + 63) // 64 * 64
        dlp = torch.empty(logits.shape[0], Vp, device=dev, dtype=logits.dtype)
        if Vp > V:
            dlp[:, V:].zero_()
        dlogits = dlp[:, :V]
        lp, alpha, beta, nll = ops.ctc_forward_rows(logits, lse, labels, elens, yl, blank, row0_d, Tmax)
        # per-micro-batch losses (sum of the utterances' nll / B, infeasible ones zeroed) as ONE masked row reduction instead of a
        # slice, a sum and a division per segment (17 tiny launches between the lattice and the gradient kernel); deterministic
        losses = (segw_d * torch.nan_to_num(nll, nan=0.0, posinf=0.0, neginf=0.0)).sum(1)
        ops.ctc_grad_rows(logits, lse, labels, elens, yl, blank, lp, alpha, beta, nll, 1.0, row0_d, tpad_d, uscale_d, dlogits)
        # ---- backward ------------------------------------------------------------------------------------------------
        if self.dtype == torch.bfloat16 and os.environ.get("EMOASR_HEAD_NT", "1") != "0":
            self._wgrad(dlogits, eouts, A.g(head + ".weight", tuple(w.shape)), 1.0, A.g(head + ".bias"), 1.0)
            w_t = torch.zeros(w.shape[1], Vp, device=dev, dtype=w.dtype)
            w_t[:, :V].copy_(w.t())
            deouts = ops.gemm_nt(dlp, w_t)
        else:
            deouts = self._lin_bwd(dlogits, eouts, head + ".weight", head + ".bias")
        if self.grad_hook is not None:   # the head's gradients are final
            self._flush_wgrads()
            self.grad_hook(A.offsets[head + ".weight"])
        self._encoder_bwd_stacked(st, deouts)
        return losses

    # ------------------------------------------------------------------ backward
    def _lin_bwd(self, dy, x_in, wname, bname, alpha=1.0, **epi):
        """gradients of y = x_in @ W^T + b given dy (already including any dropout mask);
        returns dx = alpha * dy @ W with the optional epilogue."""
        A = self.arena
        w = A.w(wname)
        w2 = w.view(w.shape[0], -1)
        self._wgrad(dy, x_in, A.g(wname, tuple(w2.shape)), alpha, A.g(bname), alpha)
        return ops.gemm_nn(dy, w2, alpha=alpha, **epi)

    def _wgrad(self, dy, x_in, out, alpha=1.0, colsum=None, colsum_scale=1.0):
        """out += alpha * dy^T @ x_in (+ bias gradient).  Inside the encoder backward the products of
        one layer are queued and run as ONE grouped launch (_flush_wgrads): each alone is 16..64
        tiles.  The queue holds references, so operands stay alive (and nothing in the layer
        backward writes them in place) until the flush."""
        if self._defer_wgrads:
            self._wq.append((dy, x_in, out, alpha, colsum, colsum_scale))
        else:
            ops.gemm_tn(dy, x_in, out=out, alpha=alpha, accumulate=True, colsum=colsum, colsum_scale=colsum_scale)

    def _hook_after_layer(self, li):
        """gradient hook after layer li's backward call.  With the layers' weight-gradient launches on the side stream
        (layer_rt.wgrad_side) the hook runs ONE LAYER BEHIND the sweep: layer li's launch has just been issued, every earlier one is
        waited for, so what is final are the gradients from layer li + 1 up."""
        if not self._layer_rt.wgrad_side:
            self.grad_hook(self._layer_offset(li))
            return
        self._layer_rt.join_wgrads(keep=1)
        if li + 1 < self.nl:
            self.grad_hook(self._layer_offset(li + 1))

    def _layer_offset(self, li):
        """lowest gradient-arena offset of encoder layer li's parameters"""
        if self._layer_lo is None:
            lo = {}
            for n, o in self.arena.offsets.items():
                if n.startswith("encoder.transformers."):
                    k = int(n.split(".")[2])
                    lo[k] = min(lo.get(k, o), o)
            self._layer_lo = lo
        return self._layer_lo[li]

    def _flush_wgrads(self):
        """Run the queued weight-gradient products as one grouped launch -- on a side stream when
        enabled: nothing on the critical path reads weight gradients before the optimizer, while
        the dgrad chain of the next layer is a string of small kernels that leave most CUs idle.
        The operands stay referenced in _inflight until backward() has joined the side stream."""
        if not self._wq:
            return
        if self._side_wgrads:
            main = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream(device=main.device)
            ev = torch.cuda.Event()
            ev.record(main)
            self._side.wait_event(ev)
            ops.gemm_tn_grouped(self._wq, stream=self._side.cuda_stream)
            self._inflight.append(self._wq)
        else:
            ops.gemm_tn_grouped(self._wq)
        self._wq = []

    def _join_side(self):
        if self._inflight:
            ev = torch.cuda.Event()
            ev.record(self._side)
            torch.cuda.current_stream().wait_event(ev)
            self._inflight = []

    def _branch_grad(self, dx, scale, p, seed, pre=None):
        """gradient entering a residual branch x + scale*dropout(f): returns (dy, alpha).
        pre: the same dropout(dx * scale) already produced by the LayerNorm backward that made dx."""
        if p > 0:
            return (pre if pre is not None else ops.scale_dropout(dx, scale, p, seed)), 1.0
        return dx, scale

    def _ln_bwd(self, dh, x, norm_name, mean, rstd, dx, nxt=None):
        """LayerNorm backward closing a sublayer.  nxt = (scale, p, seed) of the residual branch the
        backward sweep enters next: its dropout mask is applied here too (second output), which
        saves that branch's scale_dropout pass.  Inside the encoder backward the dgamma / dbeta
        folds of all LayerNorms are deferred to one grouped launch.  -> (dx_new, dy_next or None)"""
        A = self.arena
        branch = nxt if (nxt is not None and nxt[1] > 0) else None
        out = ops.layernorm_bwd(dh, x, A.p(norm_name + ".weight"), mean, rstd, dx, A.g(norm_name + ".weight"),
                                A.g(norm_name + ".bias"), branch=branch,
                                deferred=self._ln_deferred if self._defer_wgrads else None)
        return out if branch is not None else (out, None)

    def _ffn_bwd(self, name, norm_name, st, dx, res_scale, act, p=None, pre=None, nxt=None):
        x, mean, rstd, h, u, a, s_in, s_out = st
        p = self.p_enc if p is None else p
        dy, alpha = self._branch_grad(dx, res_scale, p, s_out, pre)
        if self._ffn_save_dact:
            du = self._lin_bwd(dy, a, name + ".w2.weight", name + ".w2.bias", alpha, dact_pre=u, dact=ops.DACT_MUL)
        else:
            du = self._lin_bwd(dy, a, name + ".w2.weight", name + ".w2.bias", alpha, dact_pre=u, dact=act, drop_p=p, seed=s_in)
        dh = self._lin_bwd(du, h, name + ".w1.weight", name + ".w1.bias")
        r = self._ln_bwd(dh, x, norm_name, mean, rstd, dx, nxt)
        return r if nxt is not None else r[0]

    def _attn_bwd(self, name, norm_name, st, dx, B, T, elens, pos_t, dims=None, causal=False, p_res=None, p_att=None,
                  pre=None, nxt=None):
        A = self.arena
        d, H = dims if dims is not None else (self.d, self.h)
        p_res = self.p_enc if p_res is None else p_res
        p_att = self.p_att if p_att is None else p_att
        x, mean, rstd, h, qkv, pp, o, lse, s_att, s_out, sts = st
        dy, alpha = self._branch_grad(dx, 1.0, p_res, s_out, pre)
        do = self._lin_bwd(dy, o.view(B * T, d), name + ".linear_out.weight", name + ".linear_out.bias", alpha)
        dqkv = torch.empty_like(qkv)
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        dq, dk, dv = dqkv[..., :d], dqkv[..., d:2 * d], dqkv[..., 2 * d:]
        scale = 1.0 / math.sqrt(d // H)
        if pp is not None:
            dpos = torch.zeros(pp.shape, device=pp.device, dtype=torch.float32)
            bu, bv = A.p(name + ".pos_bias_u").view(-1), A.p(name + ".pos_bias_v").view(-1)
            gbu, gbv = A.g(name + ".pos_bias_u").view(-1), A.g(name + ".pos_bias_v").view(-1)
        else:
            dpos = bu = bv = gbu = gbv = None
        if self.attn_fused and sts is None and ops.fused_attn_bwd_ok(q, pp, bu, bv, causal):
            # single-pass backward (csrc/attention.hip: attn_bwd_fused_kernel): no P^T / dS^T / dBD images, no follow-up GEMMs
            ops.attn_bwd(do.view(B, T, d), o, lse, q, k, v, H, scale, dq, dk, dv, pos=pp, bias_u=bu, bias_v=bv,
                         klens=elens, drop_p=p_att, seed=s_att, dpos=dpos, dbias_u=gbu, dbias_v=gbv, materialise="fused")
        else:
            scratch = self._scratch_for(B, H, T, T, qkv.dtype, qkv.device, pp is not None, elens, causal)
            ops.attn_bwd(do.view(B, T, d), o, lse, q, k, v, H, scale, dq, dk, dv, pos=pp, bias_u=bu, bias_v=bv,
                         klens=elens, causal=causal, drop_p=p_att, seed=s_att, dpos=dpos, dbias_u=gbu, dbias_v=gbv,
                         scratch=scratch, st=sts)
        if pp is not None:
            dpos_t = dpos if self.dtype == torch.float32 else ops.strided_copy(dpos, out_dtype=self.dtype)
            self._wgrad(dpos_t, pos_t, A.g(name + ".linear_pos.weight"))
        dqkv2 = dqkv.view(B * T, 3 * d)
        self._wgrad(dqkv2, h, A.g_span(name + ".linear_q.weight", name + ".linear_v.weight", (3 * d, d)),
                    1.0, A.g_span(name + ".linear_q.bias", name + ".linear_v.bias", (3 * d,)))
        wqkv = A.w_span(name + ".linear_q.weight", name + ".linear_v.weight", (3 * d, d))
        dh = ops.gemm_nn(dqkv2, wqkv)
        r = self._ln_bwd(dh, x, norm_name, mean, rstd, dx, nxt)
        return r if nxt is not None else r[0]

    def _scratch_for(self, B, H, Tq, Tk, dtype, device, rel, klens, causal):
        """attention-backward scratch, zeroed once per (shape, mask): every layer of a step masks the
        same entries, so the buffers are reused across layers."""
        key = (B, H, Tq, Tk, dtype, rel, id(klens), causal)
        sc = self._scratch_cache.get(key)
        if sc is None:
            if len(self._scratch_cache) > 4:
                self._scratch_cache.clear()
            sc = self._scratch_cache[key] = ops.AttnScratch(B, H, Tq, Tk, dtype, device, rel)
            sc._klens = klens  # keep the mask tensor alive while its id() keys the cache
        return sc

    def _conv_bwd(self, name, norm_name, st, dx, B, T, pre=None, nxt=None):
        A, d = self.arena, self.d
        x, mean, rstd, h, g, gl, c, bmean, bvar, z, s_out = st
        dy, alpha = self._branch_grad(dx, 1.0, self.p_enc, s_out, pre)
        dz = self._lin_bwd(dy, z, name + ".pointwise_conv2.weight", name + ".pointwise_conv2.bias", alpha)
        bn = name + ".batch_norm"
        wd = A.p(name + ".depthwise_conv.weight")
        K = wd.shape[-1]
        if self._conv_fused and g.dtype == torch.bfloat16:
            dg = ops.conv_bwd_fused(dz, c, bmean, bvar, A.p(bn + ".weight"), A.p(bn + ".bias"), 1e-5, A.g(bn + ".weight"),
                                    A.g(bn + ".bias"), g, wd.view(d, K), A.g(name + ".depthwise_conv.weight").view(d, K),
                                    A.g(name + ".depthwise_conv.bias"), B, T)
        else:
            dc = ops.bn_swish_bwd(dz, c, bmean, bvar, A.p(bn + ".weight"), A.p(bn + ".bias"), 1e-5, A.g(bn + ".weight"),
                                  A.g(bn + ".bias"))
            dgl = ops.dwconv_bwd_x(dc.view(B, T, d), wd.view(d, K))
            ops.dwconv_bwd_w(dc.view(B, T, d), gl.view(B, T, d), A.g(name + ".depthwise_conv.weight").view(d, K),
                             A.g(name + ".depthwise_conv.bias"), accumulate=True)
            dg = ops.glu_bwd(g, dgl.view(B * T, d))
        dh = self._lin_bwd(dg, h, name + ".pointwise_conv1.weight", name + ".pointwise_conv1.bias")
        r = self._ln_bwd(dh, x, norm_name, mean, rstd, dx, nxt)
        return r if nxt is not None else r[0]

    def backward(self, st, deouts, deouts_inter=None):
        """deouts: gradient w.r.t. encoder output [B,T',d] (compute dtype); deouts_inter: gradient w.r.t. the
        intermediate branch (or None).  Accumulates into the gradient arena (p.grad views)."""
        self._apply_mode()
        self._defer_wgrads = self._group_wgrads
        try:
            with self._scope():
                if self.rnn_enc:
                    return self._rnn_enc_backward(st, deouts)
                return self._backward(st, deouts, deouts_inter)
        finally:
            self._defer_wgrads = False
            self._wq = []
            self._ln_deferred = []
            self._join_side()

    def _cpp_bwd_ok(self, st):
        """the whole-layer C++ backward takes bf16 relative-position Conformer layers whose forward ran through the
        C++ layer runtime (EMOASR_CPP_BWD=0: sequence the gradient kernels from here)"""
        from .layer_rt import LayerStash
        return (self._cpp_layers and self.conformer and self.rel and self._stack_dtype_ok(True) and self.attn_fused
                and not self._side_wgrads and os.environ.get("EMOASR_CPP_BWD", "1") != "0"
                and bool(st.layers) and all(isinstance(s, LayerStash) and s.io is not None for s in st.layers)
                and st.layers[0].io.training)

    def _backward(self, st, deouts, deouts_inter=None):
        A, d = self.arena, self.d
        A.attach_grads()
        B, T, M = st.B, st.T2, st.M
        # Every LayerNorm backward of the sweep also emits the dropout-masked gradient of the residual
        # branch entered next (nxt = (scale, p, seed of that branch's output dropout)).
        p = self.p_enc
        nl = self.nl

        def br(li, which):  # branch spec of sublayer `which` of layer li
            s_ffm, s_att, s_conv, s_ff, _ = st.layers[li]
            if which == "ff":
                return (0.5 if self.conformer else 1.0, p, s_ff[7])
            if which == "ffm":
                return (0.5, p, s_ffm[7])
            if which == "att":
                return (1.0, p, s_att[9])
            return (1.0, p, s_conv[10])

        # the intermediate branch's gradient joins dx where the sweep reaches the output of layer `inter`-1;
        # a dropout-masked branch gradient carried across that point would be stale, so it is not produced
        inter = self.inter_layer if deouts_inter is not None else 0
        first = None if (self.conformer or inter == nl) else br(nl - 1, "ff")
        dx, pre = self._ln_bwd(deouts.reshape(M, d), st.x_final, "encoder.norm", st.fin_mean, st.fin_rstd, None, first)
        cpp_bwd = self._cpp_bwd_ok(st)
        if cpp_bwd:
            from .layer_rt import LayerStash  # noqa: F401
            lnf = ops.lib.size_query("emoasr_layernorm_bwd_scratch_floats", d)
            ln_parts = torch.empty(nl, 5, lnf, device=dx.device, dtype=torch.float32)
            dx_bufs = [torch.empty(M, d, device=dx.device, dtype=dx.dtype) for _ in range(2)]
        for li in reversed(range(nl)):
            name = f"encoder.transformers.{li}"
            if cpp_bwd:
                # one C-ABI call per layer (csrc/layer.hip: emoasr_conformer_layer_bwd), incl. its grouped weight gradients
                if li + 1 == inter:
                    dx, _ = self._ln_bwd(deouts_inter.reshape(M, d), st.x_inter, "encoder.norm", st.int_mean, st.int_rstd, dx)
                out = dx_bufs[li & 1]
                self._layer_rt.backward(li, st.layers[li], dx, out, ln_parts[li], self._ln_deferred)
                dx = out
                if self.grad_hook is not None and li + 1 <= (inter if inter > 0 else nl):
                    ops.layernorm_bwd_finalize(self._ln_deferred)
                    self._hook_after_layer(li)
                continue
            s_ffm, s_att, s_conv, s_ff, s_fin = st.layers[li]
            if li + 1 == inter:
                dx, _ = self._ln_bwd(deouts_inter.reshape(M, d), st.x_inter, "encoder.norm", st.int_mean, st.int_rstd, dx)
                pre = None
            if self.conformer:
                x, mean, rstd = s_fin
                dx, pre = self._ln_bwd(dx, x, name + ".norm_final", mean, rstd, None, br(li, "ff"))
                if self.rel:
                    dx, pre = self._ffn_bwd(name + ".feed_forward", name + ".norm_ff", s_ff, dx, 0.5, ACT_SWISH, pre=pre,
                                            nxt=br(li, "conv"))
                    dx, pre = self._conv_bwd(name + ".conv", name + ".norm_conv", s_conv, dx, B, T, pre=pre,
                                             nxt=br(li, "att"))
                    dx, pre = self._attn_bwd(name + ".self_attn", name + ".norm_self_attn", s_att, dx, B, T, st.elens,
                                             st.pos_t, pre=pre, nxt=br(li, "ffm"))
                else:
                    dx, pre = self._ffn_bwd(name + ".feed_forward", name + ".norm_ff", s_ff, dx, 0.5, ACT_SWISH, pre=pre,
                                            nxt=br(li, "att"))
                    dx, pre = self._attn_bwd(name + ".self_attn", name + ".norm_self_attn", s_att, dx, B, T, st.elens,
                                             None, pre=pre, nxt=br(li, "conv"))
                    dx, pre = self._conv_bwd(name + ".conv", name + ".norm_conv", s_conv, dx, B, T, pre=pre,
                                             nxt=br(li, "ffm"))
                dx = self._ffn_bwd(name + ".feed_forward_macaron", name + ".norm_ff_macaron", s_ffm, dx, 0.5, ACT_SWISH,
                                   pre=pre)
            else:
                dx, pre = self._ffn_bwd(name + ".feed_forward", name + ".norm2", s_ff, dx, 1.0, ACT_RELU, pre=pre,
                                        nxt=br(li, "att"))
                if li > 0 and li == inter:
                    dx, pre = self._attn_bwd(name + ".self_attn", name + ".norm1", s_att, dx, B, T, st.elens, None,
                                             pre=pre), None
                elif li > 0:
                    dx, pre = self._attn_bwd(name + ".self_attn", name + ".norm1", s_att, dx, B, T, st.elens, None,
                                             pre=pre, nxt=br(li - 1, "ff"))
                else:
                    dx = self._attn_bwd(name + ".self_attn", name + ".norm1", s_att, dx, B, T, st.elens, None, pre=pre)
            self._flush_wgrads()
            if self.grad_hook is not None and li + 1 <= (inter if inter > 0 else nl):
                # (with an intermediate branch, encoder.norm's gradient is final only once layer inter-1 is done)
                ops.layernorm_bwd_finalize(self._ln_deferred)  # this layer's LayerNorm gradients must be final too
                self.grad_hook(self._layer_offset(li))
        if cpp_bwd:
            self._layer_rt.join_wgrads()
            if self.grad_hook is not None and self._layer_rt.wgrad_side:
                self.grad_hook(self._layer_offset(0))
        ops.layernorm_bwd_finalize(self._ln_deferred)
        # ---- positional scaling, Linear, Conv2d x2 -----------------------------------
        if self.embed_in:
            ops.embed_bwd(st.ids, dx, math.sqrt(d), A.g("encoder.embed.weight"), st.p_enc, st.s_pe)
            return
        dlin = ops.scale_dropout(dx, math.sqrt(d), self.p_enc, st.s_pe)
        self._frontend_bwd(dlin, st)

    def _frontend_bwd(self, dlin, st):
        """gradients of the Conv2d front-end (_frontend_fwd) from dlin, the gradient w.r.t. its output [B*T',d]; reads st.xs, y1,
        y2, w2r, wlr, M, F2"""
        A, d = self.arena, self.d
        M = st.M
        pre = "encoder.conv."
        C, F2 = d, st.F2
        dx = dlin
        y2f = st.y2.view(M, F2 * C)
        dwl = torch.zeros(d, F2 * C, device=dx.device, dtype=torch.float32)  # (f, c) order
        ops.gemm_tn(dlin, y2f, out=dwl, accumulate=True, colsum=A.g(pre + "output.bias"))
        gwl = A.g(pre + "output.weight").view(d, C, F2)
        ops.strided_copy(dwl.view(d, F2, C).permute(0, 2, 1), out=gwl, accumulate=True)
        dy2 = ops.gemm_nn(dlin, st.wlr, dact_pre=y2f, dact=ACT_RELU).view(M * F2, C)
        dw2 = torch.zeros(C, 9 * C, device=dx.device, dtype=torch.float32)
        ops.conv2_wgrad(dy2, st.y1, dw2, dbias=A.g(pre + "conv.2.bias"), accumulate=True)
        ops.strided_copy(dw2.view(C, 3, 3, C).permute(0, 3, 1, 2), out=A.g(pre + "conv.2.weight"), accumulate=True)
        if self._implicit_dgrad and dy2.dtype == torch.bfloat16 and C % 256 == 0 and self._conv_big:
            # all four parity classes in one launch of the large-tile kernel; it wants the weight as [c, kh, kw, n]
            wt = ops.strided_copy(A.p(pre + "conv.2.weight").permute(1, 2, 3, 0), out_dtype=dy2.dtype).view(C, 9 * C)
            if self._conv1_fold:   # conv1's weight gradient in the data gradient's epilogue: dy1 never reaches HBM
                ops.conv2_dgrad_w1(dy2, wt, st.y1, st.xs, A.g(pre + "conv.0.weight").view(C, 9), A.g(pre + "conv.0.bias"),
                                   accumulate=True)
                return
            dy1 = ops.conv2_dgrad_kc(dy2, wt, st.y1)
        elif self._implicit_dgrad:
            dy1 = ops.conv2_dgrad(dy2, st.w2r, st.y1)  # four parity-class implicit GEMMs, no im2col buffer
        else:
            dcol = ops.gemm_nn(dy2, st.w2r)
            dy1 = ops.conv2_col2im(dcol, st.y1)
        ops.conv1_wgrad(st.xs, dy1, A.g(pre + "conv.0.weight").view(C, 9), A.g(pre + "conv.0.bias"), accumulate=True)

    def head_backward(self, eouts, dlogits, head="decoder.output"):
        """-> deouts; accumulates the vocabulary head's gradients."""
        self._apply_mode()
        B, T, d = eouts.shape
        V = dlogits.shape[-1]
        self.arena.attach_grads()
        d2 = dlogits.reshape(B * T, V)
        if V % 8 == 0:
            return self._lin_bwd(d2.contiguous(), eouts.reshape(B * T, d), head + ".weight", head + ".bias").view(B, T, d)
        # ragged vocabulary (phone heads): zero-padded copies give the GEMMs their 8-element K / row rule
        A, Vp = self.arena, (V + 7) // 8 * 8
        dpad = torch.zeros(B * T, Vp, device=d2.device, dtype=d2.dtype)
        dpad[:, :V].copy_(d2)
        wpad = torch.zeros(Vp, d, device=d2.device, dtype=d2.dtype)
        wpad[:V].copy_(A.w(head + ".weight"))
        self._wgrad(dpad[:, :V], eouts.reshape(B * T, d), A.g(head + ".weight"), 1.0, A.g(head + ".bias"), 1.0)
        return ops.gemm_nn(dpad, wpad).view(B, T, d)


# =======================================================================================
# Transformer decoder (attention loss with label smoothing, auxiliary CTC)
#   reference: asr/modeling/decoders/transformer.py:82-146, asr/modeling/transformer.py:156-198
# =======================================================================================
class _DecoderMixin:
    def _dec_init(self):
        cfg = self.cfg
        self.dd = cfg.dec_hidden_size
        self.dh = cfg.dec_num_attention_heads
        self.dnl = cfg.dec_num_layers
        self.p_dec = float(_cfg(cfg, "dropout_dec_rate", 0.0))
        self.lsm = float(_cfg(cfg, "lsm_prob", 0.0))
        self.norm_len = bool(_cfg(cfg, "loss_normalize_length", False))
        self.norm_batch = bool(_cfg(cfg, "loss_normalize_batch", True))
        self.mtl_ctc = float(_cfg(cfg, "mtl_ctc_weight", 0.0))
        # the conditional masked LM's head (cmlm_head): the logit-free kernels where their row rule applies (False: always the
        # materialised logits, the tests' comparator); cmlm_last_head names the branch the last loss took
        self.cmlm_fused_head, self.cmlm_last_head = True, None

    def _abs_table(self, L, device, d):
        key = ("abs", d, str(device))
        if key not in self._tables or self._tables[key].shape[0] < L:
            self._tables[key] = sinusoid(torch.arange(max(L, 512)), d, device)
        return self._tables[key]

    def dec_forward(self, eouts, elens_dev, ys_in, ylens_host, training, keep, causal=True, head=True):
        """teacher-forced decoder: -> logits [B, L, V] (compute dtype), stash.  causal=False is the conditional masked LM
        (decoders/transformer.py:102-105): every position attends to the keys below ylens (not ylens + 1).  head=False stops before
        the final LayerNorm: -> hidden rows [B*L, dd], stash (cmlm_head runs the LayerNorm and the vocabulary head on chosen rows)"""
        with self._scope():
            return self._dec_forward(eouts, elens_dev, ys_in, ylens_host, training, keep, causal, head)

    def _dec_forward(self, eouts, elens_dev, ys_in, ylens_host, training, keep, causal=True, head=True):
        A, dd, dh = self.arena, self.dd, self.dh
        self._keep = keep
        B, T, d = eouts.shape
        L = ys_in.shape[1]
        dev = eouts.device
        p = self.p_dec if training else 0.0
        p_att = self.p_att if training else 0.0
        ids = h2d_i32(torch.as_tensor(ys_in).contiguous(), dev)
        kself = h2d_i32([int(y) + (1 if causal else 0) for y in ylens_host], dev)
        s_emb = self._seed(5000)
        x = ops.embed_fwd(ids, A.w("decoder.embed.weight"), self._abs_table(L, dev, dd), math.sqrt(dd), p, s_emb)
        x = x.view(B * L, dd)
        mem2 = eouts.reshape(B * T, d)
        scale = 1.0 / math.sqrt(dd // dh)
        layers = []
        for li in range(self.dnl):
            name = f"decoder.transformers.{li}"
            site = 5100 + li * 20
            x, s_self = self._attn_fwd(name + ".self_attn", x, B, L, kself, None, name + ".norm1", 1e-12, p, p_att, site,
                                       training, dims=(dd, dh), causal=causal)
            # ---- source attention: queries from the decoder, keys/values from the encoder memory
            sa = name + ".src_attn"
            h2, m2, r2 = ops.layernorm_fwd(x, A.p(name + ".norm2.weight"), A.p(name + ".norm2.bias"), 1e-12, keep)
            q2 = ops.gemm_nt(h2, A.w(sa + ".linear_q.weight"), bias=A.p(sa + ".linear_q.bias")).view(B, L, dd)
            wkv = A.w_span(sa + ".linear_k.weight", sa + ".linear_v.weight", (2 * dd, d))
            bkv = A.p_span(sa + ".linear_k.bias", sa + ".linear_v.bias", (2 * dd,))
            kv = ops.gemm_nt(mem2, wkv, bias=bkv).view(B, T, 2 * dd)
            s_att, s_out = self._seed(site + 4), self._seed(site + 5)
            o2, lse2 = ops.attn_fwd(q2, kv[..., :dd], kv[..., dd:], dh, scale, klens=elens_dev, drop_p=p_att, seed=s_att)
            x1 = ops.gemm_nt(o2.view(B * L, dd), A.w(sa + ".linear_out.weight"), bias=A.p(sa + ".linear_out.bias"),
                             residual=x, res_scale=1.0, drop_p=p, seed=s_out)
            s_src = (x, m2, r2, h2, q2, kv, o2, lse2, s_att, s_out)
            x, s_ff = self._ffn_fwd(name + ".feed_forward", x1, 1.0, ACT_RELU, name + ".norm3", 1e-12, p, site + 8, training)
            layers.append((s_self, s_src, s_ff))
        st = None
        if keep:
            st = _Stash()
            st.B, st.L, st.T, st.ids, st.kself, st.elens, st.s_emb = B, L, T, ids, kself, elens_dev, s_emb
            st.layers, st.x_final, st.mem2 = layers, x, mem2
            st.p, st.p_att, st.causal = p, p_att, causal
        if not head:
            return x, st
        y, mean, rstd = ops.layernorm_fwd(x, A.p("decoder.norm.weight"), A.p("decoder.norm.bias"), 1e-12, keep)
        logits = ops.gemm_nt(y, A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
        if keep:
            st.mean, st.rstd, st.y = mean, rstd, y
        return logits.view(B, L, -1), st

    def cmlm_head(self, x, sel, labels, w, keep, want_logits=False):
        """MaskedLMLoss (cross-entropy, mean over the labelled positions) of the conditional masked LM on the labelled rows alone:
        x [B*L, dd] the decoder's last hidden rows, sel int64 [R] the labelled flat rows, labels int32 [R], w f32 [R] (1 / R; one
        row of weight 0 when nothing is labelled) -> (loss 0-dim f32, head stash, logits of ALL rows [B*L, V] | None)"""
        with self._scope():
            A = self.arena
            xr = x.index_select(0, sel)
            y, mean, rstd = ops.layernorm_fwd(xr, A.p("decoder.norm.weight"), A.p("decoder.norm.bias"), 1e-12, keep)
            W, bias = A.w("decoder.output.weight"), A.p("decoder.output.bias")
            if self.cmlm_fused_head and ops.ce_head_ok(y, W):
                rows, _, ctx = ops.ce_head_fwd(y, W, bias, labels, w)
                head = ("fused", ctx)
            else:
                z = self.head_logits(y.view(1, -1, y.shape[1]), "decoder.output")[0]
                rows, _ = ops.lsm_loss(z, labels, w, 0.0)
                head = ("materialised", z)
            self.cmlm_last_head = head[0]
            logits = None
            if want_logits:
                ya, _, _ = ops.layernorm_fwd(x, A.p("decoder.norm.weight"), A.p("decoder.norm.bias"), 1e-12, False)
                logits = self.head_logits(ya.view(1, -1, ya.shape[1]), "decoder.output")[0]
            return rows.sum(), (xr, y, mean, rstd, head, sel, labels, w), logits

    def cmlm_head_backward(self, hst, n_rows, gscale_dev):
        """-> the gradient of the decoder's last hidden rows [n_rows, dd] (zero off the labelled rows); accumulates decoder.norm
        and decoder.output gradients"""
        with self._scope():
            A = self.arena
            A.attach_grads()
            xr, y, mean, rstd, (kind, hctx), sel, labels, w = hst
            wn, bn = "decoder.output.weight", "decoder.output.bias"
            if kind == "fused":
                dy = ops.ce_head_bwd(y, A.w(wn), A.p(bn), hctx, A.g(wn), A.g(bn), 1.0, gscale_dev)
            else:
                _, dz = ops.lsm_loss(hctx, labels, w, 0.0, True, 1.0, gscale_dev)
                dy = self.head_backward(y.view(1, -1, y.shape[1]), dz.view(1, -1, dz.shape[1]), "decoder.output")[0]
            dxr = ops.layernorm_bwd(dy, xr, A.p("decoder.norm.weight"), mean, rstd, None, A.g("decoder.norm.weight"),
                                    A.g("decoder.norm.bias"))
            return torch.zeros(n_rows, xr.shape[1], device=dxr.device, dtype=dxr.dtype).index_copy_(0, sel, dxr)

    def att_loss(self, logits, ys_out, ylens_host, want_grad=False, gscale_dev=None):
        """LabelSmoothingLoss over t < ylens+1 -> (loss 0-dim f32, dlogits | None)"""
        B, L, V = logits.shape
        dev = logits.device
        w = torch.zeros(B, L, dtype=torch.float32)
        for b, yl in enumerate(ylens_host):
            n = int(yl) + 1
            w[b, :n] = (1.0 / B if self.norm_batch else 1.0) / (n if self.norm_len else 1.0)
        w = w.pin_memory().to(dev, non_blocking=True)
        labels = h2d_i32(torch.as_tensor(ys_out)[:, :L].contiguous(), dev)
        rows, grad = ops.lsm_loss(logits.view(B * L, V), labels.view(-1), w.view(-1), self.lsm, want_grad, 1.0, gscale_dev)
        return rows.sum(), (grad.view(B, L, V) if grad is not None else None)

    def att_kd_loss(self, logits, ys_out, ylens_host, soft, scale_soft=None, scale_hard=None):
        """DistillLoss over t < ylens+1 (criteria.py:66-100, decoders/transformer.py:117-126).
        Without scales -> (loss_soft, loss_hard, None); with device scalars scale_soft / scale_hard (the
        incoming gradients of the two sums) -> (None, None, dlogits)."""
        B, L, V = logits.shape
        dev = logits.device
        w = torch.zeros(B, L, dtype=torch.float32)
        for b, yl in enumerate(ylens_host):
            n = int(yl) + 1
            w[b, :n] = (1.0 / B if self.norm_batch else 1.0) / (n if self.norm_len else 1.0)
        w = w.pin_memory().to(dev, non_blocking=True).view(-1)
        labels = h2d_i32(torch.as_tensor(ys_out)[:, :L].contiguous(), dev).view(-1)
        src = torch.arange(B * L, device=dev, dtype=torch.int32)
        z, q = logits.view(B * L, V), soft.view(B * L, V)
        if scale_soft is None:
            rs, _ = ops.soft_ce(z, q, src, None, w, None, self.lsm)
            rh, _ = ops.soft_ce(z, None, None, labels, None, w, self.lsm)
            return rs.sum(), rh.sum(), None
        _, grad = ops.soft_ce(z, q, src, labels, w * scale_soft, w * scale_hard, self.lsm, want_grad=True)
        return None, None, grad.view(B, L, V)

    def dec_backward(self, st, dlogits, dx=None):
        """-> d_eouts [B,T,d]; accumulates decoder parameter gradients.  dx: the gradient of the last hidden rows instead of
        dlogits (the head's own backward has run: cmlm_head_backward)"""
        with self._scope():
            return self._dec_backward(st, dlogits, dx)

    def _dec_backward(self, st, dlogits, dx=None):
        A, dd, dh = self.arena, self.dd, self.dh
        A.attach_grads()
        B, L, T = st.B, st.L, st.T
        p, p_att = st.p, st.p_att
        d = st.mem2.shape[1]
        if dx is None:
            dy = self._lin_bwd(dlogits.reshape(B * L, -1), st.y, "decoder.output.weight", "decoder.output.bias")
            dx = ops.layernorm_bwd(dy, st.x_final, A.p("decoder.norm.weight"), st.mean, st.rstd, None,
                                   A.g("decoder.norm.weight"), A.g("decoder.norm.bias"))
        scale = 1.0 / math.sqrt(dd // dh)
        dmem = None
        for li in reversed(range(self.dnl)):
            name = f"decoder.transformers.{li}"
            s_self, s_src, s_ff = st.layers[li]
            dx = self._ffn_bwd(name + ".feed_forward", name + ".norm3", s_ff, dx, 1.0, ACT_RELU, p=p)
            # ---- source attention
            sa = name + ".src_attn"
            x, m2, r2, h2, q2, kv, o2, lse2, s_att, s_out = s_src
            dyb, alpha = self._branch_grad(dx, 1.0, p, s_out)
            do2 = self._lin_bwd(dyb, o2.view(B * L, dd), sa + ".linear_out.weight", sa + ".linear_out.bias", alpha)
            dq2 = torch.empty_like(q2)
            dkv = torch.empty_like(kv)
            if self.attn_fused and ops.fused_attn_bwd_ok(q2, None, None, None, False):
                ops.attn_bwd(do2.view(B, L, dd), o2, lse2, q2, kv[..., :dd], kv[..., dd:], dh, scale, dq2, dkv[..., :dd],
                             dkv[..., dd:], klens=st.elens, drop_p=p_att, seed=s_att, materialise="fused")
            else:
                scratch = self._scratch_for(B, dh, L, T, q2.dtype, q2.device, False, st.elens, False)
                ops.attn_bwd(do2.view(B, L, dd), o2, lse2, q2, kv[..., :dd], kv[..., dd:], dh, scale, dq2, dkv[..., :dd],
                             dkv[..., dd:], klens=st.elens, drop_p=p_att, seed=s_att, scratch=scratch)
            dh2 = self._lin_bwd(dq2.view(B * L, dd), h2, sa + ".linear_q.weight", sa + ".linear_q.bias")
            dkv2 = dkv.view(B * T, 2 * dd)
            ops.gemm_tn(dkv2, st.mem2, out=A.g_span(sa + ".linear_k.weight", sa + ".linear_v.weight", (2 * dd, d)),
                        accumulate=True, colsum=A.g_span(sa + ".linear_k.bias", sa + ".linear_v.bias", (2 * dd,)))
            wkv = A.w_span(sa + ".linear_k.weight", sa + ".linear_v.weight", (2 * dd, d))
            if dmem is None:
                dmem = ops.gemm_nn(dkv2, wkv)
            else:
                ops.gemm_nn(dkv2, wkv, out=dmem, residual=dmem, res_scale=1.0)
            dx = ops.layernorm_bwd(dh2, x, A.p(name + ".norm2.weight"), m2, r2, dx, A.g(name + ".norm2.weight"),
                                   A.g(name + ".norm2.bias"))
            dx = self._attn_bwd(name + ".self_attn", name + ".norm1", s_self, dx, B, L, st.kself, None, dims=(dd, dh),
                                causal=st.causal, p_res=p, p_att=p_att)
        ops.embed_bwd(st.ids, dx, math.sqrt(dd), A.g("decoder.embed.weight"), p, st.s_emb)
        return dmem.view(B, T, d)


for _n, _f in list(vars(_DecoderMixin).items()):
    if not _n.startswith("__"):
        setattr(CTCEngine, _n, _f)
ASREngine = CTCEngine


# =======================================================================================
# RNN-Transducer decoder: LSTM prediction network, joint network, transducer loss, greedy decode
#   reference: asr/modeling/decoders/rnn_transducer.py:81-240
# =======================================================================================
class _RNNTMixin:
    def _rnnt_init(self):
        cfg = self.cfg
        self.r_emb = cfg.embedding_size
        self.r_H = cfg.dec_hidden_size
        self.r_nl = cfg.dec_num_layers
        self.r_J = cfg.joint_hidden_size
        self.p_emb = float(_cfg(cfg, "dropout_emb_rate", 0.0))
        self.p_dec = float(_cfg(cfg, "dropout_dec_rate", 0.0))
        self.mtl_ctc = float(_cfg(cfg, "mtl_ctc_weight", 0.0))
        # the output layer + transducer loss without the [B,T,U,V] logits (csrc/gemm_big.hip epilogues); EMOASR_RNNT_FUSED=0: the
        # materialised path.  rnnt_chunk: lattice cells per gradient chunk of the backward
        self.rnnt_fused = os.environ.get("EMOASR_RNNT_FUSED", "1") != "0"
        self.rnnt_chunk = int(os.environ.get("EMOASR_RNNT_CHUNK", 65536))

    def _lstm_bias(self, name):
        A = self.arena
        return A.p(name + ".bias_ih_l0") + A.p(name + ".bias_hh_l0")  # tiny f32 add (glue)

    def rnnt_recurrency(self, ids_tm, state, training, keep):
        """prediction network, TIME-MAJOR: ids_tm int32 [U,B] -> douts [U,B,H]; state = (hs, cs) lists of
        per-layer [B,H] tensors (h in compute dtype, c f32) or None."""
        self._apply_mode()
        A, H = self.arena, self.r_H
        U, B = ids_tm.shape
        p_emb = self.p_emb if training else 0.0
        p = self.p_dec if training else 0.0
        s_emb = self._seed(7000)
        x = ops.embed_fwd(ids_tm, A.w("decoder.embed.weight"), None, 1.0, p_emb, s_emb)  # [U,B,E]
        layers, new_h, new_c = [], [], []
        for l in range(self.r_nl):
            name = f"decoder.rnns.{l}"
            w_ih, w_hh = A.w(name + ".weight_ih_l0"), A.w(name + ".weight_hh_l0")
            h_prev = state[0][l] if state is not None else None
            c_prev = state[1][l] if state is not None else None
            # input projection + the recurrence: one cooperative launch or the per-position chain (emoasr_amd/recurrence.py)
            hseq, cseq, gact = lstm_layer_fwd(x, w_ih, w_hh, self._lstm_bias(name), h_prev, c_prev)
            h_prev, c_prev = hseq[U - 1], cseq[U - 1]
            new_h.append(h_prev)
            new_c.append(c_prev)
            s_do = self._seed(7010 + l)
            y = ops.scale_dropout(hseq, 1.0, p, s_do) if p > 0 else hseq
            if keep:
                layers.append((x, hseq, cseq, gact, s_do, state[0][l] if state is not None else None,
                               state[1][l] if state is not None else None))
            x = y
        st = None
        if keep:
            st = _Stash()
            st.ids, st.layers, st.s_emb, st.p, st.p_emb = ids_tm, layers, s_emb, p, p_emb
        return x, (new_h, new_c), st

    def rnnt_recurrency_bwd(self, st, dy):
        """dy [U,B,H] gradient w.r.t. the prediction-network output; accumulates parameter gradients"""
        self._apply_mode()
        A, H = self.arena, self.r_H
        U, B = st.ids.shape
        for l in reversed(range(self.r_nl)):
            name = f"decoder.rnns.{l}"
            x_in, hseq, cseq, gact, s_do, h0, c0 = st.layers[l]
            w_ih, w_hh = A.w(name + ".weight_ih_l0"), A.w(name + ".weight_hh_l0")
            dh_seq = ops.scale_dropout(dy, 1.0, st.p, s_do) if st.p > 0 else dy
            dy = lstm_layer_bwd(dh_seq, x_in, hseq, cseq, gact, h0, c0, w_ih, w_hh, A.g(name + ".weight_ih_l0"),
                                A.g(name + ".weight_hh_l0"), A.g(name + ".bias_ih_l0"), A.g(name + ".bias_hh_l0"))
        ops.embed_bwd(st.ids, dy, 1.0, A.g("decoder.embed.weight"), st.p_emb, st.s_emb)

    def rnnt_prediction_stacked(self, ys_in_list, training):
        """the prediction network of SEVERAL micro-batches in one pass (it reads the labels only): their <sos>-prefixed label
        matrices [B_k, U_k] are padded to the longest and stacked along the batch; the cooperative recurrence takes up to eight
        groups of 64 sequences in one launch (csrc/lstm_coop.hip), so the 2 x layers launches of ~0.3 / 0.5 ms that every
        micro-batch paid are paid once.  Padded positions sit behind every real one of their sequence: they change neither the
        real outputs nor (with a zero output gradient) any parameter gradient.
        -> (douts [U_max, B_tot, H] time-major, stash for rnnt_recurrency_bwd, [(b0, b1, U_k)] per micro-batch)"""
        with self._scope():
            mats = [torch.as_tensor(y).to(torch.int32) for y in ys_in_list]
            Umax, Btot = max(m.shape[1] for m in mats), sum(m.shape[0] for m in mats)
            ids = torch.zeros(Btot, Umax, dtype=torch.int32)
            spans, b0 = [], 0
            for m in mats:
                ids[b0:b0 + m.shape[0], : m.shape[1]] = m
                spans.append((b0, b0 + m.shape[0], m.shape[1]))
                b0 += m.shape[0]
            dev = self.arena.flat.device
            ids_tm = h2d_i32(ids.t().contiguous(), dev)
            douts, _, rst = self.rnnt_recurrency(ids_tm, None, training, True)
            return douts, rst, spans

    def rnnt_prediction_stacked_ok(self, n_seqs):
        """does the stacked prediction network pay?  (only with the cooperative recurrence: bf16, <= 512 sequences)"""
        if os.environ.get("EMOASR_RNNT_PRED_STACKED", "1") == "0":   # (A/B switch)
            return False
        probe = torch.empty(0, device=self.arena.flat.device, dtype=self.dtype)
        return self.dtype == torch.bfloat16 and ops.lstm_seq_supported(probe, n_seqs, self.r_H)

    def rnnt_fused_ok(self, h, w_out):
        """can the output layer run without materialising the logits?  (bf16, V % 8 == 0, J % 64 == 0; EMOASR_RNNT_FUSED=0 or
        engine.rnnt_fused = False select the materialised path)"""
        return (self.rnnt_fused and h.dtype == torch.bfloat16 and w_out.shape[0] % 8 == 0 and w_out.shape[0] >= 64
                and w_out.shape[1] % 64 == 0)

    def rnnt_forward(self, eouts, elens_dev, ys_in, ys_host, ylens_host, blank, training, want_logits=True, pred=None,
                     defer_lattice=False):
        """-> (loss_rnnt 0-dim, logits [B,T,U,V] (None on the fused path: want_logits=False), stash)
        pred: the prediction network's output for this micro-batch, [U, B, H] time-major, when it was computed for several
        micro-batches at once (rnnt_prediction_stacked); rnnt_backward then leaves its gradient in st.ddouts
        defer_lattice (fused output layer only): the lattice runs on a side stream and the first value returned is None; the
        caller does other work of the micro-batch (the auxiliary CTC branch), then calls rnnt_lattice_join(st) -> loss"""
        with self._scope():
            A, J = self.arena, self.r_J
            B, T, d = eouts.shape
            dev = eouts.device
            U = ys_in.shape[1]
            lat_pending = None
            if pred is not None:
                assert tuple(pred.shape) == (U, B, self.r_H) and pred.is_contiguous(), (pred.shape, (U, B, self.r_H))
                douts, rst = pred, None
            else:
                ids_tm = h2d_i32(torch.as_tensor(ys_in).t().contiguous(), dev)  # [U,B]
                douts, _, rst = self.rnnt_recurrency(ids_tm, None, training, True)
            e = ops.gemm_nt(eouts.reshape(B * T, d), A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias")).view(B, T, J)
            g_tm = ops.gemm_nt(douts.view(U * B, self.r_H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
            g = ops.strided_copy(g_tm.view(U, B, J).permute(1, 0, 2))  # [B,U,J]
            h = ops.joint_tanh(e, g)
            labels = torch.as_tensor(ys_host)[:, : max(U - 1, 1)].to(torch.int32)
            if labels.shape[1] < max(U - 1, 1):
                labels = torch.nn.functional.pad(labels, (0, max(U - 1, 1) - labels.shape[1]))
            labels = h2d_i32(labels.contiguous(), dev)
            ylens = h2d_i32([int(v) for v in ylens_host], dev)
            w_out = A.w("decoder.output.weight")
            if want_logits or not self.rnnt_fused_ok(h, w_out):
                logits = ops.gemm_nt(h.view(B * T * U, J), w_out, bias=A.p("decoder.output.bias"))
                logits = logits.view(B, T, U, -1)
                ctx, nll = ops.rnnt_forward(logits, labels, elens_dev, ylens, blank)
            else:
                # the output layer reduced in the GEMM's epilogue (csrc/gemm_big.hip): soft-max partials + the blank / label logits of
                # every lattice cell; the [B,T,U,V] logits (0.9 GB per micro-batch at the L4 sizes) are never formed
                logits = None
                if defer_lattice and os.environ.get("EMOASR_RNNT_LATTICE_SIDE", "1") != "0":
                    if getattr(self, "_lat_stream", None) is None:
                        self._lat_stream = torch.cuda.Stream(device=dev)
                    ctx, nll, ev, keep = ops.rnnt_head_forward(h.view(B * T * U, J), w_out, A.p("decoder.output.bias"), B, T, U,
                                                               labels, elens_dev, ylens, blank, lattice_stream=self._lat_stream)
                    lat_pending = (ev, keep)
                else:
                    ctx, nll = ops.rnnt_head_forward(h.view(B * T * U, J), w_out, A.p("decoder.output.bias"), B, T, U, labels,
                                                     elens_dev, ylens, blank)
            st = _Stash()
            st.rst, st.douts, st.h, st.logits, st.ctx, st.nll = rst, douts, h, logits, ctx, nll
            st.labels, st.elens, st.ylens, st.blank, st.eouts = labels, elens_dev, ylens, blank, eouts
            st.B, st.T, st.U = B, T, U
            if lat_pending is not None:
                st.lat_pending = lat_pending
                return None, logits, st
            return nll.mean(), logits, st

    def rnnt_lattice_join(self, st):
        """the loss of a rnnt_forward(..., defer_lattice=True) call: the calling stream waits for the side stream's lattice"""
        pend = getattr(st, "lat_pending", None)
        if pend is not None:
            torch.cuda.current_stream().wait_event(pend[0])
            st.lat_pending = None
        return st.nll.mean()

    def rnnt_backward(self, st, gscale_dev, extra_dlogits=None):
        """-> d_eouts [B,T,d]; accumulates decoder gradients (the logits buffer is overwritten by its gradient).
        extra_dlogits [B*T*U,V] (or (rows int64 [R], [R,V])): gradient of another loss on the same logits
        (distillation), added in."""
        with self._scope():
            A, J, H = self.arena, self.r_J, self.r_H
            A.attach_grads()
            B, T, U = st.B, st.T, st.U
            if st.logits is None:
                return self._rnnt_backward_fused(st, gscale_dev)
            dz = ops.rnnt_grad(st.logits, st.ctx, st.nll, st.labels, st.elens, st.ylens, st.blank, 1.0 / B, gscale_dev,
                               out=st.logits)
            if isinstance(extra_dlogits, tuple):  # (row indices, a few gradient rows)
                dz.view(-1, dz.shape[-1]).index_add_(0, extra_dlogits[0], extra_dlogits[1])
            elif extra_dlogits is not None:
                ops.strided_copy(extra_dlogits.view(dz.shape), out=dz, accumulate=True)
            V = dz.shape[-1]
            dz2 = dz.view(B * T * U, V)
            h2 = st.h.view(B * T * U, J)
            ops.gemm_tn(dz2, h2, out=A.g("decoder.output.weight"), accumulate=True, colsum=A.g("decoder.output.bias"))
            dpre = ops.gemm_nn(dz2, A.w("decoder.output.weight"), dact_pre=h2, dact=ops.DACT_TANH_OUT)
            de, dg = ops.joint_reduce(dpre.view(B, T, U, J))
            d = st.eouts.shape[2]
            deouts = self._lin_bwd(de.view(B * T, J), st.eouts.reshape(B * T, d), "decoder.w_enc.weight",
                                   "decoder.w_enc.bias").view(B, T, d)
            dg_tm = ops.strided_copy(dg.permute(1, 0, 2)).view(U * B, J)
            ddouts = self._lin_bwd(dg_tm, st.douts.view(U * B, H), "decoder.w_dec.weight", "decoder.w_dec.bias")
            self._rnnt_pred_bwd(st, ddouts.view(U, B, H))
            return deouts

    def _rnnt_pred_bwd(self, st, ddouts):
        """the prediction network's backward -- or, when its forward ran stacked over several micro-batches, the gradient handed
        back to that pass (st.ddouts)"""
        if st.rst is None:
            st.ddouts = ddouts
        else:
            self.rnnt_recurrency_bwd(st.rst, ddouts)

    def _rnnt_backward_fused(self, st, gscale_dev):
        """backward of the fused output layer: the cells are walked in row chunks; per chunk the logits are recomputed and turned
        into their gradient inside the GEMM's epilogue (emoasr_rnnt_head_grad), then consumed by the weight-gradient and the
        data-gradient products.  The chunk buffer (RNNT_CHUNK rows x V, 128 MB at the L4 sizes) is the only [cells, V] storage."""
        A, J, H = self.arena, self.r_J, self.r_H
        B, T, U = st.B, st.T, st.U
        N = B * T * U
        w_out, b_out = A.w("decoder.output.weight"), A.p("decoder.output.bias")
        V = w_out.shape[0]
        coef, ycol = ops.rnnt_coef(st.ctx, st.nll, st.labels, st.elens, st.ylens, 1.0 / B, gscale_dev)
        h2 = st.h.view(N, J)
        dpre = torch.empty(N, J, device=h2.device, dtype=h2.dtype)
        CH = min(N, self.rnnt_chunk)
        # (rows padded to a multiple of 64 columns: with V = 1000 a row is 2000 bytes and every 128-byte store of the gradient tile
        # straddles two lines written by different workgroups)
        Vp = (V + 63) // 64 * 64
        dzp = torch.zeros(CH, Vp, device=h2.device, dtype=h2.dtype)   # (the pad columns stay zero: the kernels write V of them)
        dzc = dzp[:, :V]
        # the data gradient dz . W_out as an NT product over the PADDED columns against W_out^T [J, Vp] (zero pad): a long reduction
        # onto two 256-column tiles, which the large-tile kernel takes (csrc/gemm_big.hip: emo_gemm_nt_big_wants) -- 143 -> ~80 us
        # per 65 536-cell chunk on the 64 x 64 NN kernel
        nt_form = os.environ.get("EMOASR_RNNT_DJOINT_NT", "1") != "0" and J % 256 == 0
        if nt_form:
            w_t = torch.zeros(J, Vp, device=h2.device, dtype=h2.dtype)
            w_t[:, :V].copy_(w_out.t())
        for r0 in range(0, N, CH):
            n = min(CH, N - r0)
            dz = ops.rnnt_head_grad(h2[r0:r0 + n], w_out, b_out, coef[r0:r0 + n], ycol[r0:r0 + n], st.blank, dzc[:n])
            ops.gemm_tn(dz, h2[r0:r0 + n], out=A.g("decoder.output.weight"), accumulate=True, colsum=A.g("decoder.output.bias"))
            if nt_form:
                ops.gemm_nt(dzp[:n], w_t, out=dpre[r0:r0 + n], dact_pre=h2[r0:r0 + n], dact=ops.DACT_TANH_OUT)
            else:
                ops.gemm_nn(dz, w_out, out=dpre[r0:r0 + n], dact_pre=h2[r0:r0 + n], dact=ops.DACT_TANH_OUT)
        de, dg = ops.joint_reduce(dpre.view(B, T, U, J))
        d = st.eouts.shape[2]
        deouts = self._lin_bwd(de.view(B * T, J), st.eouts.reshape(B * T, d), "decoder.w_enc.weight",
                               "decoder.w_enc.bias").view(B, T, d)
        dg_tm = ops.strided_copy(dg.permute(1, 0, 2)).view(U * B, J)
        ddouts = self._lin_bwd(dg_tm, st.douts.view(U * B, H), "decoder.w_dec.weight", "decoder.w_dec.bias")
        self._rnnt_pred_bwd(st, ddouts.view(U, B, H))
        return deouts

    def rnnt_greedy(self, eouts, elens_host, blank, eos, max_seq_len=256, window=64):
        """time-synchronous greedy search (rnn_transducer.py:194-240).  While the arg-max is blank the
        prediction network does not move, so the frames t, t+1, ... can be scored against the SAME decoder
        state in one batched joint + output GEMM: each round scores up to `window` frames, finds the first
        non-blank one on the device and brings (index, token) back with one 8-byte copy -- one host round
        trip per emitted label (plus one per all-blank window) instead of one per frame.  The sequence of
        (frame, token) decisions is exactly the reference's."""
        with self._scope(), torch.no_grad():
            A, J = self.arena, self.r_J
            A.refresh_shadow()
            dev = eouts.device
            hyps, aligns = [], []
            V = A.w("decoder.output.weight").shape[0]
            # the one-launch search per utterance that fits it (model shape, LDS image, step-tag range); the launch chain otherwise
            fits = [bool(ops.lib.size_query("emoasr_rnnt_greedy_fits", ops.dt(eouts), self.r_emb, self.r_H, J, V, self.r_nl,
                                            int(elens_host[b]), max_seq_len)) for b in range(eouts.shape[0])]
            if all(fits):
                return self._rnnt_greedy_device(eouts, elens_host, blank, eos, max_seq_len)
            for b in range(eouts.shape[0]):
                if fits[b]:
                    h1, a1 = self._rnnt_greedy_device(eouts[b:b + 1], [int(elens_host[b])], blank, eos, max_seq_len)
                    hyps += h1
                    aligns += a1
                    continue
                hyp, align = self._rnnt_greedy_chain(eouts[b], int(elens_host[b]), blank, eos, max_seq_len, window)
                hyps.append(hyp)
                aligns.append(align)
            return hyps, aligns

    def _rnnt_greedy_chain(self, eouts_b, T, blank, eos, max_seq_len, window):
        """one utterance through the launch chain: windows of frames scored against the same decoder state, the first non-blank
        frame found on the device, one host round trip per emitted label"""
        A, J = self.arena, self.r_J
        dev = eouts_b.device
        e_all = ops.gemm_nt(eouts_b[:max(T, 1)], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))
        dout, state, _ = self.rnnt_recurrency(h2d_i32([[eos]], dev), None, False, False)
        g = ops.gemm_nt(dout.view(1, self.r_H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
        hyp, align, t = [], [], 0
        while t < T:
            n = min(window, T - t)
            h = ops.joint_tanh(e_all[t:t + n].view(1, n, J), g.view(1, 1, J))
            logits = ops.gemm_nt(h.view(n, J), A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
            k, tok = ops.first_not_equal(ops.argmax_rows(logits), blank).tolist()
            if k < 0:  # every frame of the window is blank
                align += [blank] * n
                t += n
                continue
            align += [blank] * k + [tok]
            t += k  # the label is emitted AT frame t+k: the search stays on that frame
            hyp.append(tok)
            dout, state, _ = self.rnnt_recurrency(h2d_i32([[tok]], dev), state, False, False)
            g = ops.gemm_nt(dout.view(1, self.r_H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
            if len(hyp) > max_seq_len:
                break
        return hyp, align

    def _rnnt_greedy_device(self, eouts, elens_host, blank, eos, max_seq_len):
        """the whole search of an utterance as ONE cooperative launch (csrc/rnnt_greedy.hip): no host round trip per label; the
        utterances of a batch are enqueued one after the other and read back with a single synchronisation"""
        from . import lib
        A, J, H, E = self.arena, self.r_J, self.r_H, self.r_emb
        dev = eouts.device
        w_out = A.w("decoder.output.weight")
        V = w_out.shape[0]
        nbytes = lib.size_query("emoasr_rnnt_greedy_ws_bytes", H, J)
        b_l = [self._lstm_bias(f"decoder.rnns.{l}").contiguous() for l in range(2)]
        outs = []
        for b in range(eouts.shape[0]):
            T = int(elens_host[b])
            e_all = ops.gemm_nt(eouts[b, :max(T, 1)], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            hyp = torch.empty(max_seq_len + 1, device=dev, dtype=torch.int32)
            align = torch.empty(T + max_seq_len + 1, device=dev, dtype=torch.int32)
            lens = torch.zeros(2, device=dev, dtype=torch.int32)
            lib.call("emoasr_rnnt_greedy", ops.dt(eouts), T, E, H, J, V, blank, eos, max_seq_len, ops._p(e_all),
                     ops._p(A.w("decoder.embed.weight")), ops._p(A.w("decoder.rnns.0.weight_ih_l0")),
                     ops._p(A.w("decoder.rnns.0.weight_hh_l0")), ops._p(b_l[0]), ops._p(A.w("decoder.rnns.1.weight_ih_l0")),
                     ops._p(A.w("decoder.rnns.1.weight_hh_l0")), ops._p(b_l[1]), ops._p(A.w("decoder.w_dec.weight")),
                     ops._p(A.p("decoder.w_dec.bias")), ops._p(w_out), ops._p(A.p("decoder.output.bias")), ops._p(ws), nbytes,
                     ops._p(hyp), ops._p(align), ops._p(lens), ops._stream())
            outs.append((e_all, ws, hyp, align, lens))
        hyps, aligns = [], []
        for e_all, ws, hyp, align, lens in outs:
            nh, na = lens.tolist()    # (the first read synchronises)
            err = int(ws[64:68].view(torch.int32).item())
            if err:
                raise RuntimeError("rnnt_greedy: a grid barrier gave up waiting (csrc/rnnt_greedy.hip); "
                                   "emoasr_set_option('rnnt_greedy_coop', 0) selects the launch chain")
            hyps.append(hyp[:nh].tolist())
            aligns.append(align[:na].tolist())
        return hyps, aligns

    def rnnt_beam_search(self, eouts, beam_width, blank, eos, num_expands=3, return_scores=False):
        """alignment-length synchronous beam search for ONE utterance (rnn_transducer.py:242-325,348-359): the expansion round as a
        replayed HIP graph (_rnnt_beam_search_graph) unless EMOASR_RNNT_BEAM_GRAPH=0 or the utterance does not fit its static
        buffers; then the launch chain below.  return_scores: (hyps, float64 scores) instead of hyps (tests compare the two forms)."""
        T = eouts.shape[1]
        if (os.environ.get("EMOASR_RNNT_BEAM_GRAPH", "1") != "0" and beam_width <= 16
                and (T * num_expands + 2) * beam_width + 1 <= self._BEAM_POOL - 16 and T <= self._BEAM_TMAX):
            return self._rnnt_beam_search_graph(eouts, beam_width, blank, eos, num_expands, return_scores)
        return self._rnnt_beam_search_chain(eouts, beam_width, blank, eos, num_expands, return_scores)

    _BEAM_POOL, _BEAM_TMAX = 32768, 4096   # (the pool's last 16 slots are the warm-up's scratch, never a hypothesis's)

    def _rnnt_beam_round_graph(self, beam_width, nb, blank):
        """the device work of ONE expansion round over nb live hypotheses, captured once as a HIP graph over static buffers:
        control words (last labels, source / destination slots of the LSTM states in the pool, frame index) come in through
        `ctl`, (blank log-prob, top-k log-probs, top-k ids) per hypothesis go out through `out`.  The host loop pays one replay
        per round instead of ~12 C-ABI calls, ~16 allocations and the torch glue (246 us per round, host-bound:
        tools/l4_beam_prof.py).  Round 5: the captured body is five launches (csrc/rnnt_beam.hip) that read the control words from
        the PINNED host record and write the result record into pinned host memory -- no upload / download launches: 124 -> 66 us
        per round; EMOASR_RNNT_BEAM_FUSED=0 captures the launch chain with explicit copies as before."""
        st = self.__dict__.setdefault("_beam_static", None)
        A, J, H, nl = self.arena, self.r_J, self.r_H, self.r_nl
        dev = A.flat.device
        if st is None:
            st = self._beam_static = _Stash()
            st.ph = [torch.zeros(self._BEAM_POOL, H, device=dev, dtype=self.dtype) for _ in range(nl)]
            st.pc = [torch.zeros(self._BEAM_POOL, H, device=dev, dtype=torch.float32) for _ in range(nl)]
            st.e = torch.zeros(self._BEAM_TMAX, J, device=dev, dtype=self.dtype)
            st.ctl = torch.zeros(3 * 16 + 1, device=dev, dtype=torch.int64)
            st.ctl_host = torch.zeros(3 * 16 + 1, dtype=torch.int64).pin_memory()
            st.out = torch.zeros(16, 1 + 2 * 16, device=dev, dtype=torch.float32)
            st.out_host = torch.zeros(16, 1 + 2 * 16, dtype=torch.float32).pin_memory()
            st.hj = torch.zeros(16, J, device=dev, dtype=self.dtype)
            st.bias = [self._lstm_bias(f"decoder.rnns.{l}").contiguous() for l in range(nl)]   # (refreshed per search, below)
            st.graphs = {}
        key = (beam_width, nb, blank)
        if key in st.graphs:
            return st, st.graphs[key]

        # the fused round's kernels have LDS plans of their own (csrc/rnnt_beam.hip: a vocabulary row of <= 60 KB in the pick
        # kernel, 16 rows of H floats in the joint kernel, nin + H columns in the f32 LSTM step); a model outside them decodes
        # through the launch chain as before round 5 -- decided here from the same limits, and once more by the warm-up below
        # (an entry point that still refuses turns the round into the chain body instead of failing the search)
        V_ = A.w("decoder.output.weight").shape[0]
        nin_max = max(A.w(f"decoder.rnns.{l}.weight_ih_l0").shape[1] for l in range(nl)) if nl else 0
        fits = V_ * 4 <= 60 * 1024 and 16 * H * 4 <= 64 * 1024 and (self.dtype == torch.bfloat16 or nin_max + H <= 2368)
        mode = {"fused": os.environ.get("EMOASR_RNNT_BEAM_FUSED", "1") != "0" and nl >= 1 and fits}
        st.zero_copy = mode["fused"]

        def body_fused():
            # csrc/rnnt_beam.hip: five launches -- one per LSTM layer (gather, both products, cell, scatter), the joint input, the
            # output layer, the pick (log-softmax + blank + top-k into the result record)
            from . import lib
            with self._scope():
                # zero-copy hand-off: the kernels read the control words straight from the PINNED host record (each word once,
                # through LDS) and the pick kernel writes the result record into pinned host memory -- no upload / download
                # launches (two ~5 us copy kernels + their enqueue per round)
                dtc = ops.dt(st.ph[0])
                words = lambda base: tuple(c_void_p(base.data_ptr() + 8 * o) for o in (0, 16, 32, 48))
                h_ids, h_src, h_dst, _ = words(st.ctl_host)       # the first launch reads the host record (and copies it over) ...
                p_ids, p_src, p_dst, p_t = words(st.ctl)          # ... the later ones its device twin
                emb = A.w("decoder.embed.weight")
                xtab, ldx, xidx = emb, emb.shape[1], h_ids
                for l in range(nl):
                    name = f"decoder.rnns.{l}"
                    w_ih, w_hh = A.w(name + ".weight_ih_l0"), A.w(name + ".weight_hh_l0")
                    first = l == 0
                    lib.call("emoasr_rnnt_beam_lstm", dtc, nb, w_ih.shape[1], H, ops._p(xtab), ldx, xidx, ops._p(w_ih), ops._p(w_hh),
                             ops._p(st.bias[l]), ops._p(st.ph[l]), ops._p(st.pc[l]), h_src if first else p_src,
                             h_dst if first else p_dst, ops._p(st.ctl_host) if first else None, ops._p(st.ctl) if first else None,
                             st.ctl.numel() if first else 0, ops._stream())
                    xtab, ldx, xidx = st.ph[l], H, p_dst
                hj = st.hj[:nb]
                lib.call("emoasr_rnnt_beam_joint", dtc, nb, H, J, self._BEAM_TMAX, ops._p(st.ph[nl - 1]), p_dst,
                         ops._p(A.w("decoder.w_dec.weight")), ops._p(A.p("decoder.w_dec.bias")), ops._p(st.e), p_t, ops._p(hj),
                         ops._stream())
                logits = ops.gemm_nt(hj, A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
                lib.call("emoasr_rnnt_beam_pick", dtc, nb, logits.shape[1], beam_width, blank, ops._p(logits), logits.stride(0),
                         ops._p(st.out_host), st.out_host.stride(0), ops._stream())

        def body():
            if mode["fused"]:
                return body_fused()
            with self._scope():
                ids = st.ctl[:nb].to(torch.int32).view(1, nb)
                src, dst, t = st.ctl[16:16 + nb], st.ctl[32:32 + nb], st.ctl[48:49]
                prev = ([p.index_select(0, src) for p in st.ph], [p.index_select(0, src) for p in st.pc])
                dout, (nh, nc), _ = self.rnnt_recurrency(ids, prev, False, False)
                for l in range(nl):
                    st.ph[l].index_copy_(0, dst, nh[l])
                    st.pc[l].index_copy_(0, dst, nc[l])
                g = ops.gemm_nt(dout.view(nb, H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
                h = ops.joint_tanh(st.e.index_select(0, t).view(1, 1, J), g.view(1, nb, J))
                logits = ops.gemm_nt(h.view(nb, J), A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
                lp = ops.log_softmax(logits)
                vals, idx, _ = ops.topk(lp[:, 1:], beam_width)
                st.out[:nb, 0:1].copy_(lp[:, blank:blank + 1])
                st.out[:nb, 1:1 + beam_width].copy_(vals)
                st.out[:nb, 1 + beam_width:1 + 2 * beam_width].copy_(idx)

        # the warm-up runs the body for real: give it control words of its own -- label 0, the zero state of slot 0 as source and
        # the pool's reserved scratch slots as destination -- so that it never writes a slot a live hypothesis reads (the
        # caller uploads the round's words after this call, before the replay)
        st.ctl_host.zero_()
        st.ctl_host[32:32 + 16] = torch.arange(self._BEAM_POOL - 16, self._BEAM_POOL)
        st.ctl.copy_(st.ctl_host)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        from . import lib
        with torch.cuda.stream(side):
            try:
                body()   # warm-up outside the capture (allocator, lazy initialisation)
            except lib.EmoasrHipError:
                if not mode["fused"]:
                    raise
                mode["fused"] = st.zero_copy = False   # outside a fused kernel's limits: the launch chain's body
                st.ctl.copy_(st.ctl_host)
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_):
            body()
        st.graphs[key] = g_
        return st, g_

    def _rnnt_beam_search_graph(self, eouts, beam_width, blank, eos, num_expands=3, return_scores=False):
        """the search of rnnt_beam_search with every expansion round's device work replayed from a HIP graph; the bookkeeping
        (stable sort by float64 score, merge of equal label sequences by log-add, cut to the beam) stays on the host, as in the
        reference and in _rnnt_beam_search_chain, whose arithmetic and launch order the captured body repeats."""
        import numpy as np
        with self._scope(), torch.no_grad():
            A, J = self.arena, self.r_J
            A.refresh_shadow()
            T = eouts.shape[1]
            e_all = ops.gemm_nt(eouts[0], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))  # [T,J]
            st, _ = self._rnnt_beam_round_graph(beam_width, 1, blank)
            st.e[:T].copy_(e_all)
            for l in range(self.r_nl):   # bias_ih + bias_hh of the current weights, into the buffers the captured launches read
                st.bias[l].copy_(self._lstm_bias(f"decoder.rnns.{l}"))
            for l in range(self.r_nl):   # slot 0: the zero state every search starts from
                st.ph[l][0].zero_()
                st.pc[l][0].zero_()
            ctl, out = st.ctl_host.numpy(), st.out_host.numpy()
            stream = torch.cuda.current_stream()
            nslot = 1
            beams = [([eos], 0.0, 0)]   # (hyp, score, slot of the LSTM state from BEFORE its last label)

            def merge(cands):
                seen = {}
                for hyp, score, slot in cands:
                    key = tuple(hyp)
                    if key in seen:
                        seen[key][1] = float(np.logaddexp(seen[key][1], score))
                    else:
                        seen[key] = [hyp, score, slot]
                return [tuple(c) for c in seen.values()]

            for t in range(T):
                frame_out, live = [], beams
                for v in range(num_expands):
                    nb = len(live)
                    if nb == 0:
                        break
                    _, graph = self._rnnt_beam_round_graph(beam_width, nb, blank)
                    for i, (hyp, _, slot) in enumerate(live):
                        ctl[i], ctl[16 + i], ctl[32 + i] = hyp[-1], slot, nslot + i
                    ctl[48] = t
                    if not st.zero_copy:
                        st.ctl.copy_(st.ctl_host, non_blocking=True)
                    graph.replay()
                    if not st.zero_copy:
                        st.out_host.copy_(st.out, non_blocking=True)
                    stream.synchronize()
                    host = out[:nb].astype(np.float64)
                    last = v == num_expands - 1
                    for i, (hyp, score, slot) in enumerate(live):
                        frame_out.append((hyp, score + float(host[i, 0]), slot))
                    grown = []
                    if not last:
                        for i, (hyp, score, slot) in enumerate(live):
                            for k in range(beam_width):
                                grown.append((hyp + [int(host[i, 1 + beam_width + k]) + 1], score + float(host[i, 1 + k]), nslot + i))
                    nslot += nb
                    grown.sort(key=lambda c: -c[1])
                    live = merge(grown)[:beam_width]
                frame_out.sort(key=lambda c: -c[1])
                beams = merge(frame_out)[:beam_width]
            if return_scores:
                return [hyp for hyp, _, _ in beams], [score for _, score, _ in beams]
            return [hyp for hyp, _, _ in beams]

    def _rnnt_beam_search_chain(self, eouts, beam_width, blank, eos, num_expands=3, return_scores=False):
        """alignment-length synchronous beam search for ONE utterance (rnn_transducer.py:242-325,348-359).

        eouts [1,T,d].  Per frame up to `num_expands` rounds; each round is one batched prediction-network
        step over the live hypotheses (every hypothesis keeps the LSTM state from before its last label, as
        the reference does), one joint + output GEMM, log-softmax and top-k on the device, and ONE D2H of
        (blank score, k scores, k ids) per live hypothesis; bookkeeping (stable sort by float64 score, merge
        of equal label sequences by log-add, cut to the beam) stays on the host like the reference.
        Returns the surviving label sequences best-first, including the leading <sos>."""
        import numpy as np
        with self._scope(), torch.no_grad():
            A, J, H, nl = self.arena, self.r_J, self.r_H, self.r_nl
            A.refresh_shadow()
            dev = eouts.device
            T = eouts.shape[1]
            e_all = ops.gemm_nt(eouts[0], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))  # [T,J]
            cdt = e_all.dtype
            zero = ([torch.zeros(1, H, device=dev, dtype=cdt) for _ in range(nl)],
                    [torch.zeros(1, H, device=dev, dtype=torch.float32) for _ in range(nl)])
            beams = [([eos], 0.0, (zero, 0))]  # (hyp, score, (state tensors, row))

            def merge(cands):
                seen = {}
                for hyp, score, st in cands:
                    key = tuple(hyp)
                    if key in seen:
                        seen[key][1] = float(np.logaddexp(seen[key][1], score))
                    else:
                        seen[key] = [hyp, score, st]
                return [tuple(c) for c in seen.values()]

            def gather(live):
                srcs = {id(st[0]): st[0] for _, _, st in live}
                if len(srcs) == 1:
                    (hs, cs), = srcs.values()
                    rows = [st[1] for _, _, st in live]
                    if rows == list(range(hs[0].shape[0])):
                        return hs, cs
                    ix = torch.tensor(rows, device=dev)
                    return [h.index_select(0, ix) for h in hs], [c.index_select(0, ix) for c in cs]
                hs = [torch.cat([st[0][0][l][st[1]:st[1] + 1] for _, _, st in live]) for l in range(nl)]
                cs = [torch.cat([st[0][1][l][st[1]:st[1] + 1] for _, _, st in live]) for l in range(nl)]
                return hs, cs

            for t in range(T):
                frame_out, live = [], beams
                for v in range(num_expands):
                    nb = len(live)
                    if nb == 0:
                        break
                    prev = gather(live)
                    ids = h2d_i32([[hyp[-1] for hyp, _, _ in live]], dev)  # [1,nb]
                    dout, (nh, nc), _ = self.rnnt_recurrency(ids, prev, False, False)
                    g = ops.gemm_nt(dout.view(nb, H), A.w("decoder.w_dec.weight"), bias=A.p("decoder.w_dec.bias"))
                    h = ops.joint_tanh(e_all[t].view(1, 1, J), g.view(1, nb, J))
                    logits = ops.gemm_nt(h.view(nb, J), A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
                    lp = ops.log_softmax(logits)
                    last = v == num_expands - 1
                    if last:
                        host = lp[:, blank].cpu().double().numpy().reshape(nb, 1)
                    else:
                        vals, idx, _ = ops.topk(lp[:, 1:], beam_width)
                        host = torch.cat([lp[:, blank:blank + 1], vals, idx.to(torch.float32)], 1).cpu().double().numpy()
                    for i, (hyp, score, st) in enumerate(live):
                        frame_out.append((hyp, score + float(host[i, 0]), st))
                    grown = []
                    if not last:
                        after = (nh, nc)
                        for i, (hyp, score, st) in enumerate(live):
                            for k in range(beam_width):
                                grown.append((hyp + [int(host[i, 1 + beam_width + k]) + 1],
                                              score + float(host[i, 1 + k]), (after, i)))
                    grown.sort(key=lambda c: -c[1])
                    live = merge(grown)[:beam_width]
                frame_out.sort(key=lambda c: -c[1])
                beams = merge(frame_out)[:beam_width]
            if return_scores:
                return [hyp for hyp, _, _ in beams], [score for _, score, _ in beams]
            return [hyp for hyp, _, _ in beams]



# =======================================================================================
# RNN encoder: Conv2d front-end (or none) -> bidirectional LSTM layers over packed sequences
#   reference: asr/modeling/encoders/rnn.py:14-81
# =======================================================================================
class _RNNEncMixin:
    """encoder_type "rnn": every layer is nn.LSTM(bidirectional=True, batch_first=True) over pack_padded_sequence(x, elens), the two
    directions' outputs summed (enc_hidden_sum_fwd_bwd) and dropout applied (also after the last layer).  Per layer: the input
    projection of both directions as two GEMMs into one [B*T', 8H] buffer, the recurrence, and the sum / mask / dropout
    epilogue.  The recurrence is one cooperative launch for both directions where emoasr_bilstm_seq_supported says so (bf16,
    B <= 256, H <= 512, option "lstm_coop"), else a per-step chain (the recurrent products through the product kernels, so all
    three compute modes hold; one length-aware cell launch for both directions per step, csrc/bilstm.hip).  T' = max(elens): the output is as long as pad_packed_sequence's."""

    def _rnn_elens(self, xlens_host):
        if _cfg(self.cfg, "input_layer", "conv2d") == "none":
            return list(xlens_host)
        return [((v - 1) // 2 - 1) // 2 for v in xlens_host]

    def _rnn_enc_forward(self, xs, xlens_host, training, stash):
        self.ensure_bound()
        A, dt = self.arena, self.dtype
        A.refresh_shadow()
        stash = training if stash is None else stash
        p = self.p_enc if training else 0.0
        xlens_host = [int(v) for v in xlens_host]
        elens_host = self._rnn_elens(xlens_host)
        assert min(elens_host) >= 1, f"emoasr_amd: RNN encoder needs at least one frame per utterance after subsampling ({elens_host})"
        B, dev = xs.shape[0], xs.device
        # frames past the longest utterance change nothing (pack_padded_sequence drops them): run over max(xlens) only
        xs = xs[:, : max(xlens_host)].contiguous()
        elens = h2d_i32(elens_host, dev)
        st = _Stash() if stash else None
        if _cfg(self.cfg, "input_layer", "conv2d") == "none":
            T2 = xs.shape[1]
            x = ops.strided_copy(xs, out_dtype=dt).view(B * T2, -1) if dt != torch.float32 else xs.view(B * T2, -1)
        else:
            x, y1, y2, w2r, wlr = self._frontend_fwd(xs)
            T2 = y2.shape[1]
            if st is not None:
                st.xs, st.y1, st.y2, st.w2r, st.wlr, st.F2 = xs, y1, y2, w2r, wlr, y2.shape[2]
        assert T2 == max(elens_host), (T2, max(elens_host))
        if st is not None:
            st.B, st.T2, st.M, st.elens, st.p, st.layers = B, T2, B * T2, elens, p, []
        for l in range(self.nl):
            x, ls = self._bilstm_fwd(l, x, B, T2, elens, p, stash)
            if st is not None:
                st.layers.append(ls)
        self.eouts_inter = None
        return x.view(B, T2, self.d), elens_host, elens, st

    def _bilstm_fwd(self, l, x, B, T, elens, p, keep):
        A, H, dt = self.arena, self.d, self.dtype
        name = f"encoder.rnns.{l}"
        dev, M = x.device, B * T
        pre = torch.empty(M, 8 * H, device=dev, dtype=dt)
        for d, sfx in enumerate(("", "_reverse")):
            bias = A.p(name + ".bias_ih_l0" + sfx) + A.p(name + ".bias_hh_l0" + sfx)  # tiny f32 add (glue)
            ops.gemm_nt(x, A.w(name + ".weight_ih_l0" + sfx), out=pre[:, 4 * H * d: 4 * H * (d + 1)], bias=bias)
        hseq = torch.empty(2, B, T, H, device=dev, dtype=dt)
        hprev = torch.empty(2, B, T, H, device=dev, dtype=dt)
        cseq = torch.empty(2, B, T, H, device=dev, dtype=torch.float32)
        gact = torch.empty(2, B, T, 4 * H, device=dev, dtype=dt)
        w_hh = (A.w(name + ".weight_hh_l0"), A.w(name + ".weight_hh_l0_reverse"))
        hstate = torch.empty(2, B, H, device=dev, dtype=dt)
        cstate = torch.empty(2, B, H, device=dev, dtype=torch.float32)
        rec = torch.empty(2, B, 4 * H, device=dev, dtype=dt)
        pre3 = pre.view(B, T, 8 * H)
        if T > 1 and ops.bilstm_seq_supported(pre, B, H):
            # both directions' whole recurrence in one cooperative launch (csrc/lstm_coop.hip; option "lstm_coop" = 0: the chain)
            ops.bilstm_seq_fwd(elens, pre3, w_hh[0], w_hh[1], hseq, hprev, cseq, gact)
        else:
            for s in range(T):
                if s > 0:
                    ops.gemm_nt(hstate[0], w_hh[0], out=rec[0])
                    ops.gemm_nt(hstate[1], w_hh[1], out=rec[1])
                ops.bilstm_cell_fwd(s, elens, pre3, rec if s > 0 else None, hstate, cstate, hseq, hprev, cseq, gact)
        s_do = self._seed(8000 + l)
        y = ops.bilstm_out(elens, hseq[0], hseq[1], p, s_do)
        ls = (x, hprev, cseq, gact, s_do) if keep else None
        return y.view(M, H), ls

    def _rnn_enc_backward(self, st, deouts):
        A, H = self.arena, self.d
        A.attach_grads()
        B, T, M = st.B, st.T2, st.M
        dy = deouts.reshape(B, T, H).contiguous()
        none_in = _cfg(self.cfg, "input_layer", "conv2d") == "none"
        for l in reversed(range(self.nl)):
            dy = self._bilstm_bwd(l, st.layers[l], dy, B, T, st.elens, st.p, need_dx=(l > 0 or not none_in))
            if self.grad_hook is not None:
                self.grad_hook(self._rnn_layer_offset(l))
        if not none_in:
            self._frontend_bwd(dy.view(M, H), st)

    def _bilstm_bwd(self, l, ls, dy, B, T, elens, p, need_dx=True):
        A, H = self.arena, self.d
        x_in, hprev, cseq, gact, s_do = ls
        name = f"encoder.rnns.{l}"
        dev, dt, M = dy.device, dy.dtype, B * T
        dh = ops.bilstm_out(elens, dy, None, p, s_do)   # both directions take the same masked gradient
        dg = torch.empty(2, B, T, 4 * H, device=dev, dtype=dt)
        w_hh = (A.w(name + ".weight_hh_l0"), A.w(name + ".weight_hh_l0_reverse"))
        if T > 1 and ops.bilstm_seq_supported(dh, B, H):
            ops.bilstm_seq_bwd(elens, dh, gact, cseq, w_hh[0], w_hh[1], dg)
        else:
            dgc = torch.empty(2, B, 4 * H, device=dev, dtype=dt)
            dhrec = torch.empty(2, B, H, device=dev, dtype=dt)
            dcstate = torch.empty(2, B, H, device=dev, dtype=torch.float32)
            for s in reversed(range(T)):
                if s < T - 1:
                    ops.gemm_nn(dgc[0], w_hh[0], out=dhrec[0])
                    ops.gemm_nn(dgc[1], w_hh[1], out=dhrec[1])
                ops.bilstm_cell_bwd(s, elens, dh, dhrec if s < T - 1 else None, dcstate, gact, cseq, dg, dgc)
        nin = x_in.shape[-1]
        dx = None
        for d, sfx in enumerate(("", "_reverse")):
            dgd = dg[d].view(M, 4 * H)
            ops.gemm_tn(dgd, x_in.view(M, nin), out=A.g(name + ".weight_ih_l0" + sfx), accumulate=True,
                        colsum=A.g(name + ".bias_ih_l0" + sfx))
            ops.colsum(dgd, out=A.g(name + ".bias_hh_l0" + sfx), accumulate=True)
            # padded frames and each direction's first frame pair a zero gradient / a zero hprev row: no boundary pairing exists
            ops.gemm_tn(dgd, hprev[d].view(M, H), out=A.g(name + ".weight_hh_l0" + sfx), accumulate=True)
            if need_dx:
                w_ih = A.w(name + ".weight_ih_l0" + sfx)
                dx = ops.gemm_nn(dgd, w_ih) if dx is None else ops.gemm_nn(dgd, w_ih, residual=dx, res_scale=1.0)
        return None if dx is None else dx.view(B, T, nin)

    def _rnn_layer_offset(self, l):
        """lowest gradient-arena offset of RNN layer l's parameters"""
        pre = f"encoder.rnns.{l}."
        return min(o for n, o in self.arena.offsets.items() if n.startswith(pre))


for _n, _f in list(vars(_RNNTMixin).items()):
    if not _n.startswith("__"):
        setattr(CTCEngine, _n, _f)

for _n, _f in list(vars(_RNNEncMixin).items()):
    if not _n.startswith("__"):
        setattr(CTCEngine, _n, _f)


# =======================================================================================
# LAS decoder: LSTM cells with location-aware additive attention
#   reference: asr/modeling/decoders/las.py:22-343
# Only layer 0 and the attention are sequential (the attention reads its own previous weights, layer 0 reads the previous
# context).  Per position: one recurrent product of [ctx | h] against [W_ih[:, E:] | W_hh] with the hoisted embedding term as its
# residual, the cell kernel, the query projection, the attention step (csrc/las.hip).  Hoisted: the embedding gather and its input
# product, the key projection, LSTM layers 1.. as whole-sequence layers (recurrence.py), intermed + tanh and the vocabulary head.
# Time-major throughout; the logits are transposed to [B, L, V] at the end.
# =======================================================================================
class _LASMixin:
    def _las_init(self):
        cfg = self.cfg
        self.l_E, self.l_H, self.l_nl = cfg.embedding_size, cfg.dec_hidden_size, cfg.dec_num_layers
        self.l_A, self.l_I = cfg.attn_dim, cfg.dec_intermediate_size
        self.p_dec = float(_cfg(cfg, "dropout_dec_rate", 0.0))
        self.lsm = float(_cfg(cfg, "lsm_prob", 0.0))
        self.norm_len = bool(_cfg(cfg, "loss_normalize_length", False))
        self.norm_batch = bool(_cfg(cfg, "loss_normalize_batch", True))
        self.mtl_ctc = float(_cfg(cfg, "mtl_ctc_weight", 0.0))

    def _las_weights(self):
        A = self.arena
        return ops.LasWeights(A.p("decoder.score.conv.weight"), A.p("decoder.score.w_conv.weight"),
                              A.p("decoder.score.w_conv.bias"), A.p("decoder.score.w_score.weight"))

    def _las_bias(self, l):
        A = self.arena
        return A.p(f"decoder.rnns.{l}.bias_ih") + A.p(f"decoder.rnns.{l}.bias_hh")  # tiny f32 add (glue)

    def _las_cast(self, x):
        """an f32 accumulation buffer as a GEMM operand of the compute dtype"""
        return x if self.dtype == torch.float32 else ops.strided_copy(x, out_dtype=self.dtype)

    def las_forward(self, eouts, elens_dev, ys_in, ylens_host, training, p_attn, keep):
        """teacher-forced decoder: eouts [B,T,D] (compute dtype), ys_in [B,L] -> logits [B,L,V], stash.  Every row runs all L
        positions; those past ylens + 1 of a row reach neither the loss nor a gradient (their dlogits are zero)."""
        with self._scope():
            return self._las_forward(eouts, elens_dev, ys_in, training, p_attn, keep)

    def _las_forward(self, eouts, elens_dev, ys_in, training, p_attn, keep):
        A, E, H, NL, AD, I = self.arena, self.l_E, self.l_H, self.l_nl, self.l_A, self.l_I
        B, T, D = eouts.shape
        L = ys_in.shape[1]
        dev, dt = eouts.device, self.dtype
        p = self.p_dec if training else 0.0
        p_att = float(p_attn) if training else 0.0
        ids_tm = h2d_i32(torch.as_tensor(ys_in).t().contiguous(), dev)   # [L,B]
        s_emb, s_att, s_h0 = self._seed(8000), self._seed(8001), self._seed(8002)
        emb = ops.embed_fwd(ids_tm, A.w("decoder.embed.weight"), None, 1.0, p, s_emb)   # [L,B,E]
        w_ih0, w_hh0 = A.w("decoder.rnns.0.weight_ih"), A.w("decoder.rnns.0.weight_hh")
        pre0 = ops.gemm_nt(emb.view(L * B, E), w_ih0[:, :E], bias=self._las_bias(0)).view(L, B, 4 * H)
        wcat = torch.cat([w_ih0[:, E:], w_hh0], dim=1)   # [4H, D+H]: once per pass (the shadow weights change every step)
        eo2 = eouts.reshape(B * T, D)
        pk = ops.gemm_nt(eo2, A.w("decoder.score.w_key.weight"), bias=A.p("decoder.score.w_key.bias")).view(B, T, AD)
        W = self._las_weights()
        wq, bq = A.w("decoder.score.w_query.weight"), A.p("decoder.score.w_query.bias")
        # xcat[i] = [ctx_{i-1} | h_{i-1}] (row 0: zeros): the recurrent product's input at position i, and the per-position
        # context / undropped layer-0 output the backward needs
        xcat = torch.zeros(L + 1, B, D + H, device=dev, dtype=dt)
        cseq = torch.empty(L, B, H, device=dev, dtype=torch.float32)
        gact = torch.empty(L, B, 4 * H, device=dev, dtype=dt)
        hd0 = torch.empty(L, B, H, device=dev, dtype=dt)      # the DROPPED layer-0 outputs: the queries, and layer 1's input
        pq = torch.empty(L, B, AD, device=dev, dtype=dt)
        aw = torch.empty(L, B, T, device=dev, dtype=torch.float32)
        lse = torch.empty(L, B, device=dev, dtype=torch.float32)
        scores = torch.empty(B, T, device=dev, dtype=torch.float32)
        for i in range(L):
            gates = pre0[i] if i == 0 else ops.gemm_nt(xcat[i], wcat, residual=pre0[i], res_scale=1.0)
            h = xcat[i + 1][:, D:]
            ops.lstm_cell_fwd(gates, cseq[i - 1] if i else None, h, cseq[i], gact[i])
            if p > 0:
                ops.strided_copy(h, out=hd0[i])
                ops.scale_dropout(hd0[i], 1.0, p, s_h0 + 7919 * i, out=hd0[i])
                q = hd0[i]
            else:
                q = h
            ops.gemm_nt(q, wq, bias=bq, out=pq[i])
            ops.las_attend_fwd(W, pk, pq[i], aw[i - 1] if i else None, eouts, elens_dev, p_att, s_att, i, aw=aw[i],
                               ctx=xcat[i + 1][:, :D], lse=lse[i], scores=scores)
        if p <= 0:
            ops.strided_copy(xcat[1:, :, D:], out=hd0)
        layers, x = [], hd0
        for l in range(1, NL):
            name = f"decoder.rnns.{l}"
            hseq, cs, ga = lstm_layer_fwd(x, A.w(name + ".weight_ih"), A.w(name + ".weight_hh"), self._las_bias(l), None, None)
            s_do = self._seed(8010 + l)
            y = ops.scale_dropout(hseq, 1.0, p, s_do) if p > 0 else hseq
            layers.append((x, hseq, cs, ga, s_do))
            x = y
        top = x.view(L * B, H)
        w_i = A.w("decoder.intermed.weight")   # [I, D+H]: columns of the context, then of the top layer
        ctx_rows = xcat[1:].view(L * B, D + H)[:, :D]
        e = ops.gemm_nt(ctx_rows, w_i[:, :D], bias=A.p("decoder.intermed.bias"))
        g = ops.gemm_nt(top, w_i[:, D:])
        hgen = ops.joint_tanh(e.view(L * B, 1, I), g.view(L * B, 1, I)).view(L * B, I)
        logits_tm = ops.gemm_nt(hgen, A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))
        V = logits_tm.shape[1]
        logits = ops.strided_copy(logits_tm.view(L, B, V).permute(1, 0, 2))   # [B,L,V]
        st = None
        if keep:
            st = _Stash()
            st.B, st.T, st.D, st.L, st.V = B, T, D, L, V
            st.ids_tm, st.emb, st.wcat, st.eouts, st.pk, st.W, st.elens = ids_tm, emb, wcat, eouts, pk, W, elens_dev
            st.xcat, st.cseq, st.gact, st.hd0, st.pq, st.aw, st.lse = xcat, cseq, gact, hd0, pq, aw, lse
            st.layers, st.top, st.hgen = layers, top, hgen
            st.p, st.p_att, st.s_emb, st.s_att, st.s_h0 = p, p_att, s_emb, s_att, s_h0
        return logits, st

    def las_backward(self, st, dlogits):
        """-> d_eouts [B,T,D]; accumulates the decoder's parameter gradients.  Walks the positions in reverse with the attention
        backward kernel and the cell backward; the weight gradients of w_key, w_query, intermed, output, the embedding and layer
        0's LSTM are single products over accumulated buffers after the loop.  (score.w_score.bias receives nothing: the soft-max
        is shift-invariant, its gradient is identically zero.)"""
        with self._scope():
            return self._las_backward(st, dlogits)

    def _las_backward(self, st, dlogits):
        A, E, H, NL, AD, I = self.arena, self.l_E, self.l_H, self.l_nl, self.l_A, self.l_I
        A.attach_grads()
        B, T, D, L, V = st.B, st.T, st.D, st.L, st.V
        dev, dt = st.eouts.device, self.dtype
        p = st.p
        xcat, pk, W = st.xcat, st.pk, st.W
        dz = ops.strided_copy(dlogits.view(B, L, V).permute(1, 0, 2)).view(L * B, V)
        ops.gemm_tn(dz, st.hgen, out=A.g("decoder.output.weight"), accumulate=True, colsum=A.g("decoder.output.bias"))
        dpre = ops.gemm_nn(dz, A.w("decoder.output.weight"), dact_pre=st.hgen, dact=ops.DACT_TANH_OUT)   # [LB, I]
        w_i, g_wi = A.w("decoder.intermed.weight"), A.g("decoder.intermed.weight")
        ctx_rows = xcat[1:].view(L * B, D + H)[:, :D]
        ops.gemm_tn(dpre, ctx_rows, out=g_wi[:, :D], accumulate=True, colsum=A.g("decoder.intermed.bias"))
        ops.gemm_tn(dpre, st.top, out=g_wi[:, D:], accumulate=True)
        # res[i] = [d ctx_i from generate | 0]: the residual of the recurrent product's data gradient at position i + 1
        res = torch.zeros(L, B, D + H, device=dev, dtype=dt)
        ops.gemm_nn(dpre, w_i[:, :D], out=res.view(L * B, D + H)[:, :D])
        dy = ops.gemm_nn(dpre, w_i[:, D:]).view(L, B, H)
        for l in reversed(range(1, NL)):
            name = f"decoder.rnns.{l}"
            x_in, hseq, cs, ga, s_do = st.layers[l - 1]
            dh_seq = ops.scale_dropout(dy, 1.0, p, s_do) if p > 0 else dy
            dy = lstm_layer_bwd(dh_seq, x_in, hseq, cs, ga, None, None, A.w(name + ".weight_ih"), A.w(name + ".weight_hh"),
                                A.g(name + ".weight_ih"), A.g(name + ".weight_hh"), A.g(name + ".bias_ih"), A.g(name + ".bias_hh"))
        dhd0 = dy   # gradient of the dropped layer-0 outputs from the layers above (the query path is added per position)
        dpq = torch.zeros(L, B, AD, device=dev, dtype=torch.float32)
        daw = torch.zeros(L, B, T, device=dev, dtype=torch.float32)   # daw[i]: what position i + 1's convolution sends to aw_i
        dpk = torch.zeros(B, T, AD, device=dev, dtype=torch.float32)
        deo = torch.zeros(B, T, D, device=dev, dtype=torch.float32)
        dgp0 = torch.empty(L, B, 4 * H, device=dev, dtype=dt)
        dc = torch.zeros(B, H, device=dev, dtype=torch.float32)
        g_ws, g_wc = A.g("decoder.score.w_score.weight"), A.g("decoder.score.w_conv.weight")
        g_bc, g_filt = A.g("decoder.score.w_conv.bias"), A.g("decoder.score.conv.weight")
        wq = A.w("decoder.score.w_query.weight")
        for i in reversed(range(L)):
            if i == L - 1:
                dctx, dh_rec = res[i][:, :D], None
            else:
                dx = ops.gemm_nn(st.dgp_next, st.wcat, residual=res[i], res_scale=1.0)   # [B, D+H] = [d ctx_i | d h_i]
                dctx, dh_rec = dx[:, :D], dx[:, D:]
            ops.las_attend_bwd(W, pk, st.pq[i], st.aw[i - 1] if i else None, st.eouts, st.elens, st.p_att, st.s_att, i, st.aw[i],
                               xcat[i + 1][:, :D], st.lse[i], dctx, daw[i] if i < L - 1 else None, dpq[i],
                               daw[i - 1] if i else None, dpk, deo, g_ws, g_wc, g_bc, g_filt)
            dhd = ops.gemm_nn(self._las_cast(dpq[i]), wq, residual=dhd0[i], res_scale=1.0)   # query path + the layers above
            if p > 0:
                ops.scale_dropout(dhd, 1.0, p, st.s_h0 + 7919 * i, out=dhd)
            c_prev = st.cseq[i - 1] if i else None
            if dh_rec is None:
                ops.lstm_cell_bwd(dhd, None, dc, st.gact[i], c_prev, st.cseq[i], dgp0[i])
            else:
                ops.lstm_cell_bwd(dh_rec, dhd, dc, st.gact[i], c_prev, st.cseq[i], dgp0[i])
            st.dgp_next = dgp0[i]
        st.dgp_next = None
        dgp2 = dgp0.view(L * B, 4 * H)
        w_ih0, g_ih0 = A.w("decoder.rnns.0.weight_ih"), A.g("decoder.rnns.0.weight_ih")
        ops.gemm_tn(dgp2, st.emb.view(L * B, E), out=g_ih0[:, :E], accumulate=True, colsum=A.g("decoder.rnns.0.bias_ih"))
        ops.colsum(dgp2, out=A.g("decoder.rnns.0.bias_hh"), accumulate=True)
        xin = xcat[:L].view(L * B, D + H)
        ops.gemm_tn(dgp2, xin[:, :D], out=g_ih0[:, E:], accumulate=True)
        ops.gemm_tn(dgp2, xin[:, D:], out=A.g("decoder.rnns.0.weight_hh"), accumulate=True)
        demb = ops.gemm_nn(dgp2, w_ih0[:, :E]).view(L, B, E)
        ops.embed_bwd(st.ids_tm, demb, 1.0, A.g("decoder.embed.weight"), p, st.s_emb)
        ops.gemm_tn(self._las_cast(dpq.view(L * B, AD)), st.hd0.view(L * B, H), out=A.g("decoder.score.w_query.weight"),
                    accumulate=True, colsum=A.g("decoder.score.w_query.bias"))
        dpk_c = self._las_cast(dpk.view(B * T, AD))
        ops.gemm_tn(dpk_c, st.eouts.reshape(B * T, D), out=A.g("decoder.score.w_key.weight"), accumulate=True,
                    colsum=A.g("decoder.score.w_key.bias"))
        deouts = ops.gemm_nn(dpk_c, A.w("decoder.score.w_key.weight"), residual=self._las_cast(deo.view(B * T, D)), res_scale=1.0)
        return deouts.view(B, T, D)

    # ------------------------------------------------------------------ decoding
    def las_step(self, S, ids, parents, first):
        """one token for nb <= beam_width hypotheses of one utterance.  S: the utterance's state (las_beam_search): weights, the key
        projection, and two slot pools per state array -- [ctx | h0], c0, h / c of the layers above, the attention weights -- that
        take turns as source and destination.  ids int32 [nb] (device): the hypotheses' last tokens; parents int64 [nb] (device):
        the source slot of each; the new state of row k goes to slot k of the other pool.
        -> (top log-probabilities f32 [nb, bw], their tokens int32 [nb, bw])"""
        A, E, H, NL, I = self.arena, self.l_E, self.l_H, self.l_nl, self.l_I
        D, nb = S.D, ids.shape[0]
        src, dst = S.pools[S.cur], S.pools[1 - S.cur]
        x_in = src.xc.index_select(0, parents)          # parent -> child copies by slot index
        c_prev = src.c0.index_select(0, parents)
        emb = ops.embed_fwd(ids.view(nb, 1), A.w("decoder.embed.weight"), None, 1.0).view(nb, E)
        gates = ops.gemm_nt(emb, S.w_ih0[:, :E], bias=S.bias[0])
        if not first:
            gates = ops.gemm_nt(x_in, S.wcat, residual=gates, res_scale=1.0)
        xc, c0 = dst.xc[:nb], dst.c0[:nb]
        h = xc[:, D:]
        ops.lstm_cell_fwd(gates, None if first else c_prev, h, c0, S.gact[:nb])
        pq = ops.gemm_nt(h, S.wq, bias=S.bq)
        aw_prev = None if first else src.aw.index_select(0, parents)
        ops.las_attend_fwd(S.W, S.pk, pq, aw_prev, S.eo, None, 0.0, 0, 0, aw=dst.aw[:nb], ctx=xc[:, :D], scores=S.scores)
        x = h
        for l in range(1, NL):
            name = f"decoder.rnns.{l}"
            g = ops.gemm_nt(x, A.w(name + ".weight_ih"), bias=S.bias[l])
            if not first:
                g = ops.gemm_nt(src.hu[l - 1].index_select(0, parents), A.w(name + ".weight_hh"), residual=g, res_scale=1.0)
            ops.lstm_cell_fwd(g, None if first else src.cu[l - 1].index_select(0, parents), dst.hu[l - 1][:nb], dst.cu[l - 1][:nb],
                              S.gact[:nb])
            x = dst.hu[l - 1][:nb]
        w_i = A.w("decoder.intermed.weight")
        e = ops.gemm_nt(xc[:, :D], w_i[:, :D], bias=A.p("decoder.intermed.bias"))
        g = ops.gemm_nt(x, w_i[:, D:])
        hgen = ops.joint_tanh(e.view(nb, 1, I), g.view(nb, 1, I)).view(nb, I)
        logits = ops.gemm_nt(hgen, A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"), out_f32=True)
        vals, idx, _ = ops.topk(ops.log_softmax(logits), S.bw)
        S.cur = 1 - S.cur
        return vals, idx

    def las_beam_search(self, eouts, beam_width, len_weight, eos, max_len):
        """LASDecoder.decode's search (las.py:196-287) for ONE utterance, eouts [1,T,D]: the device advances all live hypotheses by
        one token per las_step call; the host keeps the reference's bookkeeping literally -- every live beam expanded by its top
        beam_width tokens, all expansions sorted (stable), the best beam_width kept, ended beams with an empty stripped hypothesis
        dropped, final score + len_weight * len(hyp) with the leading <eos> counted, stop at beam_width results.
        -> (hyps, scores), both empty when no hypothesis ever ends"""
        with torch.no_grad(), self._scope():
            A, E, H, NL, AD = self.arena, self.l_E, self.l_H, self.l_nl, self.l_A
            bw = int(beam_width)
            dev, dt = eouts.device, self.dtype
            eo = eouts[0].to(dt).contiguous()
            T, D = eo.shape
            S = _Stash()
            S.bw, S.D, S.eo, S.cur = bw, D, eo, 0
            S.pk = ops.gemm_nt(eo, A.w("decoder.score.w_key.weight"), bias=A.p("decoder.score.w_key.bias"))   # once per utterance
            S.W = self._las_weights()
            S.w_ih0 = A.w("decoder.rnns.0.weight_ih")
            S.wcat = torch.cat([S.w_ih0[:, E:], A.w("decoder.rnns.0.weight_hh")], dim=1)
            S.bias = [self._las_bias(l) for l in range(NL)]
            S.wq, S.bq = A.w("decoder.score.w_query.weight"), A.p("decoder.score.w_query.bias")
            S.gact = torch.empty(bw, 4 * H, device=dev, dtype=dt)
            S.scores = torch.empty(bw, T, device=dev, dtype=torch.float32)
            S.pools = []
            for _ in range(2):
                P = _Stash()
                P.xc = torch.zeros(bw, D + H, device=dev, dtype=dt)
                P.c0 = torch.zeros(bw, H, device=dev, dtype=torch.float32)
                P.hu = torch.zeros(max(NL - 1, 1), bw, H, device=dev, dtype=dt)
                P.cu = torch.zeros(max(NL - 1, 1), bw, H, device=dev, dtype=torch.float32)
                P.aw = torch.zeros(bw, T, device=dev, dtype=torch.float32)
                S.pools.append(P)
            beams = [{"hyp": [eos], "score": 0.0, "slot": 0}]
            results = []
            for i in range(max_len):
                ids, parents = h2d_pack([torch.tensor([b["hyp"][-1] for b in beams], dtype=torch.int32),
                                         torch.tensor([b["slot"] for b in beams], dtype=torch.int64)], dev)
                vals, idx = self.las_step(S, ids, parents, i == 0)
                vals, idx = vals.cpu(), idx.cpu()
                new_beams = []
                for k, beam in enumerate(beams):
                    for j in range(bw):
                        new_beams.append({"hyp": beam["hyp"] + [int(idx[k, j])], "score": beam["score"] + float(vals[k, j]),
                                          "slot": k})
                beams = sorted(new_beams, key=lambda x: x["score"], reverse=True)[:bw]
                extend = []
                for beam in beams:
                    if beam["hyp"][-1] == eos:
                        hyp = [t for t in beam["hyp"] if t != eos]
                        if len(hyp) < 1:   # only <eos> is not acceptable
                            continue
                        results.append({"hyp": hyp, "score": beam["score"] + len_weight * len(beam["hyp"])})
                        if len(results) >= bw:
                            break
                    else:
                        extend.append(beam)
                if len(results) >= bw or not extend:
                    break
                beams = extend
            results = sorted(results, key=lambda x: x["score"], reverse=True)
            return [r["hyp"] for r in results], [r["score"] for r in results]


for _n, _f in list(vars(_LASMixin).items()):
    if not _n.startswith("__"):
        setattr(CTCEngine, _n, _f)
