"""LAS decoder: LSTM cells with location-aware additive attention.
  reference: asr/modeling/decoders/las.py:22-343
Only layer 0 and the attention are sequential (the attention reads its own previous weights, layer 0 reads the previous
context).  Per position: one recurrent product of [ctx | h] against [W_ih[:, E:] | W_hh] with the hoisted embedding term as its
residual, the cell kernel, the query projection, the attention step (csrc/las.hip).  Hoisted: the embedding gather and its input
product, the key projection, LSTM layers 1.. as whole-sequence layers (recurrence.py), intermed + tanh and the vocabulary head.
Time-major throughout; the logits are transposed to [B, L, V] at the end."""
import torch

from .. import ops
from ..recurrence import lstm_stack_bwd, lstm_stack_fwd
from .arena import _Stash, _cfg, h2d_i32, h2d_pack


class LASDecoder:
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
        # (sites 8000 .. 8002 are also the RNN encoder's layers 0 .. 2: rnn_encoder.py, _bilstm_fwd)
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
        upper = ((A.w(f"decoder.rnns.{l}.weight_ih"), A.w(f"decoder.rnns.{l}.weight_hh"), self._las_bias(l), self._seed(8010 + l),
                  None, None) for l in range(1, NL))   # (a generator: each bias sum is launched when the stack reaches its layer)
        x, _, layers = lstm_stack_fwd(hd0, upper, p, True)
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
        grads = [tuple(A.g(f"decoder.rnns.{l}.{n}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(1, NL)]
        dhd0 = lstm_stack_bwd(dy, st.layers, grads, p)   # gradient of the dropped layer-0 outputs from the layers above (the query path is added per position)
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
