"""Transformer decoder (attention loss with label smoothing, auxiliary CTC) and the conditional masked LM's head.
  reference: asr/modeling/decoders/transformer.py:82-146, asr/modeling/transformer.py:156-198"""
import math

import torch

from .. import ops
from ..ops import ACT_RELU
from .arena import _Stash, _cfg, h2d_i32, sinusoid


class TransformerDecoder:
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

    def cmlm_head(self, x, sel, labels, w, keep, want_logits=False, sample_seed=None, sample_fused=True, sample_min_rows=None):
        """MaskedLMLoss (cross-entropy, mean over the labelled positions) of the conditional masked LM on the labelled rows alone:
        x [B*L, dd] the decoder's last hidden rows, sel int64 [R] the labelled flat rows, labels int32 [R], w f32 [R] (1 / R; one
        row of weight 0 when nothing is labelled) -> (loss 0-dim f32, head stash, logits of ALL rows [B*L, V] | None).
        sample_seed (P-ELECTRA's generator): one Gumbel-max sample per labelled row as well, noise row = the index among the labelled
        rows -> (loss, head stash, logits | None, samples int32 [R]).  The samples leave the head product's epilogue
        (ops.ce_head_sample_fwd: no [R, V] logits; cmlm_last_head "fused-sample") where sample_fused and ops.ce_head_sample_ok with
        sample_min_rows hold, else ops.sample_rows reads the materialised logits of the labelled rows."""
        with self._scope():
            A = self.arena
            xr = x.index_select(0, sel)
            y, mean, rstd = ops.layernorm_fwd(xr, A.p("decoder.norm.weight"), A.p("decoder.norm.bias"), 1e-12, keep)
            W, bias = A.w("decoder.output.weight"), A.p("decoder.output.bias")
            samples = None
            if sample_seed is not None:
                if sample_fused and ops.ce_head_sample_ok(y, W, sample_min_rows):
                    rows, _, samples, ctx = ops.ce_head_sample_fwd(y, W, bias, labels, w, sample_seed, 0, sample_min_rows)
                    head = ("fused", ctx)
                else:
                    z = self.head_logits(y.view(1, -1, y.shape[1]), "decoder.output")[0]
                    rows, _ = ops.lsm_loss(z, labels, w, 0.0)
                    _, samples, _ = ops.sample_rows(z, labels, w, sample_seed)
                    head = ("materialised", z)
                self.cmlm_last_head = "fused-sample" if head[0] == "fused" else head[0]
            elif self.cmlm_fused_head and ops.ce_head_ok(y, W):
                rows, _, ctx = ops.ce_head_fwd(y, W, bias, labels, w)
                head = ("fused", ctx)
            else:
                z = self.head_logits(y.view(1, -1, y.shape[1]), "decoder.output")[0]
                rows, _ = ops.lsm_loss(z, labels, w, 0.0)
                head = ("materialised", z)
            if sample_seed is None:
                self.cmlm_last_head = head[0]
            logits = None
            if want_logits:
                ya, _, _ = ops.layernorm_fwd(x, A.p("decoder.norm.weight"), A.p("decoder.norm.bias"), 1e-12, False)
                logits = self.head_logits(ya.view(1, -1, ya.shape[1]), "decoder.output")[0]
            out = (rows.sum(), (xr, y, mean, rstd, head, sel, labels, w), logits)
            return out if sample_seed is None else out + (samples,)

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

    def _att_targets(self, ys_out, ylens_host, B, L, dev):
        """-> (row weights f32 [B*L]: the loss normalisation over t < ylens+1, zero past it; labels int32 [B*L]), on the device"""
        w = torch.zeros(B, L, dtype=torch.float32)
        for b, yl in enumerate(ylens_host):
            n = int(yl) + 1
            w[b, :n] = (1.0 / B if self.norm_batch else 1.0) / (n if self.norm_len else 1.0)
        w = w.pin_memory().to(dev, non_blocking=True).view(-1)
        return w, h2d_i32(torch.as_tensor(ys_out)[:, :L].contiguous(), dev).view(-1)

    def att_loss(self, logits, ys_out, ylens_host, want_grad=False, gscale_dev=None):
        """LabelSmoothingLoss over t < ylens+1 -> (loss 0-dim f32, dlogits | None)"""
        B, L, V = logits.shape
        w, labels = self._att_targets(ys_out, ylens_host, B, L, logits.device)
        rows, grad = ops.lsm_loss(logits.view(B * L, V), labels, w, self.lsm, want_grad, 1.0, gscale_dev)
        return rows.sum(), (grad.view(B, L, V) if grad is not None else None)

    def att_kd_loss(self, logits, ys_out, ylens_host, soft, scale_soft=None, scale_hard=None):
        """DistillLoss over t < ylens+1 (criteria.py:66-100, decoders/transformer.py:117-126).
        Without scales -> (loss_soft, loss_hard, None); with device scalars scale_soft / scale_hard (the
        incoming gradients of the two sums) -> (None, None, dlogits)."""
        B, L, V = logits.shape
        w, labels = self._att_targets(ys_out, ylens_host, B, L, logits.device)
        src = torch.arange(B * L, device=logits.device, dtype=torch.int32)
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
