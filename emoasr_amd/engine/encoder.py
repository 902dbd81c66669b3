"""Explicit forward/backward sequencing of the HIP kernels for the CTC models
(Conv2d front-end -> Transformer/Conformer encoder -> CTC head).

There is no autograd graph inside: forward() stashes what backward() needs, backward()
walks the layers in reverse calling the hand-written gradient kernels and accumulates
parameter gradients straight into a flat f32 gradient arena.  torch supplies device
memory and the stream only.

Reference behaviour being reproduced (file:line in the reference):
  encoder      asr/modeling/encoders/transformer.py:84-113, encoders/conv.py:20-28
  conformer    asr/modeling/conformer.py:47-54,77-95,121-143,191-229
  transformer  asr/modeling/transformer.py:43-45,96-99,117-118,143-153
  CTC          asr/modeling/decoders/ctc.py:103-115,176-201
"""
import math
import os

import torch

from .. import ops
from ..ops import ACT_RELU, ACT_SWISH
from .arena import AttnStash, ConvStash, FFNStash, LayerRecord, ParamArena, _Stash, _cfg, h2d_i32, h2d_pack, sinusoid
from .las import LASDecoder
from .rnn_encoder import RNNEncoder
from .rnnt import RNNTDecoder
from .transformer_decoder import TransformerDecoder


class CTCEngine(TransformerDecoder, RNNTDecoder, RNNEncoder, LASDecoder):
    """Forward / backward of encoder + CTC head on HIP kernels."""

    def __init__(self, cfg, module, compute_dtype=torch.bfloat16, bn_buffers=None, f32_split=False, arena=None):
        """arena: an ArenaView over a larger model's arena, under whose key prefix `module` sits (P-ELECTRA's generator); the owner
        of that arena re-homes the parameters and rebuilds this engine.  Default: the engine's own ParamArena over `module`."""
        self.cfg = cfg
        # f32 storage with every product as three bf16 MFMAs over (hi, lo) operand pairs (csrc/gemm.hip SplitCfg): the
        # throughput mode that meets the 1e-3 bar; compute_dtype stays torch.float32
        self.split = bool(f32_split) and compute_dtype == torch.float32
        self.d = cfg.enc_hidden_size
        self.h = _cfg(cfg, "enc_num_attention_heads", 0)   # (an RNN encoder's config has no attention fields)
        self.nl = cfg.enc_num_layers
        self.conformer = cfg.encoder_type == "conformer"
        # bidirectional LSTM stack (encoders/rnn.py; rnn_encoder.py) in place of the Transformer / Conformer layers
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
        from .. import lib as _lib
        self._conv_fused = _lib.get_option("conv_fused") != 0
        self._ffn_save_dact = _lib.get_option("ffn_save_dact") != 0
        self._conv_big = _lib.get_option("conv_big") != 0
        self.p_enc = float(_cfg(cfg, "dropout_enc_rate", 0.0))
        self.p_att = float(_cfg(cfg, "dropout_attn_rate", 0.0))
        self.dtype = compute_dtype
        self.module = module
        self._own_arena = arena is None
        self.arena = ParamArena(module, compute_dtype) if arena is None else arena
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
        # inference only, off by default (the reference never masks padded frames): the convolution module reads zeros at the frames
        # past an utterance's end, so an utterance inside a padded batch gets the output it gets alone.  Every other kernel of the
        # stack is row-wise or masked by the lengths already.  Takes the per-kernel path (the C++ layer call has no such form).
        self.mask_padding = False
        self._conv_lens = None
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
            assert self._own_arena, "emoasr_amd: the parameters left the shared arena; its owner re-binds them and rebuilds this engine"
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
        self._conv_lens = elens if self.mask_padding and not training and not stash else None
        if self._cpp_layers and self.conformer and self.rel and not self.attn_store_scores and self._conv_lens is None:
            # one C-ABI call per layer (csrc/layer.hip); intermediates land in per-layer workspaces and
            # become tensors only when the backward sweep asks for them (layer_rt.LayerStash)
            if self._layer_rt is None:
                from ..layer_rt import ConformerLayerRuntime
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
        self._conv_lens = None
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
        return y, FFNStash(x, mean, rstd, h, u, a, s_in, s_out)

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
        return y, AttnStash(x, mean, rstd, h, qkv, pp, o, lse, s_att, s_out, sts)

    def _conv_fwd(self, name, x, B, T, norm_name, p_enc, site, training):
        A, d = self.arena, self.d
        h, mean, rstd = ops.layernorm_fwd(x, A.p(norm_name + ".weight"), A.p(norm_name + ".bias"), 1e-5, self._keep)
        g = ops.gemm_nt(h, A.w(name + ".pointwise_conv1.weight", (2 * d, d)), bias=A.p(name + ".pointwise_conv1.bias"))
        wd = A.p(name + ".depthwise_conv.weight")
        bn = name + ".batch_norm"
        rm, rv = self._buffers(bn + ".running_mean"), self._buffers(bn + ".running_var")
        wdk, bd = wd.view(d, wd.shape[-1]), A.p(name + ".depthwise_conv.bias")
        fused = self._conv_fused and g.dtype == torch.bfloat16  # GLU inside the convolution's staging pass (convfused.hip)
        if self._conv_lens is not None:      # (mask_padding: the GLU writes zeros past every utterance's end)
            fused, gl = False, ops.glu_fwd_masked(g, B, T, self._conv_lens)
        else:
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
        return y, ConvStash(x, mean, rstd, h, g, gl, c, bmean, bvar, z, s_out)

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
            return y, LayerRecord(s_ffm, s_att, s_conv, s_ff, (x, mean, rstd))
        x, s_att = self._attn_fwd(name + ".self_attn", x, B, T, elens, None, name + ".norm1", 1e-12, p_enc, p_att,
                                  site + 2, training)
        x, s_ff = self._ffn_fwd(name + ".feed_forward", x, 1.0, ACT_RELU, name + ".norm2", 1e-12, p_enc, site + 6, training)
        return x, LayerRecord(None, s_att, None, s_ff, None)

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
        from .. import lib
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
            from ..layer_rt import ConformerLayerRuntime
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
        from ..layer_rt import LayerStash
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

        def br(li, which):  # branch spec of sublayer `which` ("ffm", "att", "conv", "ff") of layer li
            scale = 0.5 if which == "ffm" or (which == "ff" and self.conformer) else 1.0
            return (scale, p, getattr(LayerRecord(*st.layers[li]), which).s_out)

        # the intermediate branch's gradient joins dx where the sweep reaches the output of layer `inter`-1;
        # a dropout-masked branch gradient carried across that point would be stale, so it is not produced
        inter = self.inter_layer if deouts_inter is not None else 0
        first = None if (self.conformer or inter == nl) else br(nl - 1, "ff")
        dx, pre = self._ln_bwd(deouts.reshape(M, d), st.x_final, "encoder.norm", st.fin_mean, st.fin_rstd, None, first)
        cpp_bwd = self._cpp_bwd_ok(st)
        if cpp_bwd:
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


ASREngine = CTCEngine
