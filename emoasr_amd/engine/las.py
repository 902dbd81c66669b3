"""LAS decoder: LSTM cells with location-aware additive attention.
  reference: asr/modeling/decoders/las.py:22-343
Only layer 0 and the attention are sequential (the attention reads its own previous weights, layer 0 reads the previous
context).  Per position: one recurrent product of [ctx | h] against [W_ih[:, E:] | W_hh] with the hoisted embedding term as its
residual, the cell kernel, the query projection, the attention step (csrc/las.hip).  Hoisted: the embedding gather and its input
product, the key projection, LSTM layers 1.. as whole-sequence layers (recurrence.py), intermed + tanh and the vocabulary head.
Time-major throughout; the logits are transposed to [B, L, V] at the end.
The beam searches fuse a next-token LM on request: the host form calls it per step, the batched device form
steps the RNN LM inside its captured chain, and the (lm_weight, len_weight) grid searches every distinct weight once.  A Transformer
LM is stepped there too, over the prefix tree of csrc/lm_tree.hip, under decoder.las_tlm_fusion = "device" (section 33)."""
import ctypes

import numpy as np
import torch

from .. import lib, lockstep, ops
from ..recurrence import lstm_stack_bwd, lstm_stack_fwd
from .arena import _Stash, _cfg, h2d_i32, h2d_pack


LAS_BEAM_MAX_ROWS = 1024            # S * W rows of one chunk of the batched search
LAS_BEAM_POOL_BUDGET_BYTES = 2 << 30    # the two attention-weight pools of one chunk


def las_beam_pool_bytes(nb, Tmax, lm_row_bytes=0):
    """bytes of the attention-weight pools of nb rows: two halves (source / destination of a step), Tmax f32 per row; a fused RNN
    LM adds the two halves of its state pools, lm_row_bytes per row and half (las_lm_row_bytes)"""
    return 2 * nb * (Tmax * 4 + lm_row_bytes)


def las_lm_row_bytes(lm, esz):
    """bytes of one row of one half of a fused RNN LM's state pools: h (compute dtype) and c (f32) of every layer; 0 without one"""
    return 0 if lm is None else lm.L * lm.H * (esz + 4)


def las_tlm_dims(lm, W, max_len):
    """(Lcap, node_cap) of the prefix tree a fused Transformer LM steps over (section 33): lm_tree.las_list_cap / las_node_cap"""
    from .. import lm_tree
    return lm_tree.las_list_cap(max_len, lm.params.max_seq_len), lm_tree.las_node_cap(W, max_len)


def las_tlm_search_bytes(lm, W, max_len, V):
    """bytes of one search's share of a fused Transformer LM's prefix tree (lm_tree.las_search_bytes); 0 without one"""
    if lm is None:
        return 0
    from .. import lm_tree
    P = lm.params
    Lcap, node_cap = las_tlm_dims(lm, W, max_len)
    return lm_tree.las_search_bytes(W, Lcap, node_cap, P.num_layers, P.hidden_size, V, 2 if lm.compute_dtype == torch.bfloat16 else 4)


def las_beam_chunk_capacity(W, Tmax, budget=None, max_rows=None, lm_row_bytes=0, tree_bytes=0):
    """S_max: the most searches of width W one chunk of las_beam_search_batch holds -- S_max * W <= LAS_BEAM_MAX_ROWS rows and
    las_beam_pool_bytes(S_max * W, Tmax, lm_row_bytes) + S_max * tree_bytes <= LAS_BEAM_POOL_BUDGET_BYTES (tree_bytes: a fused
    Transformer LM's prefix tree per search, las_tlm_search_bytes); never below one search"""
    budget = LAS_BEAM_POOL_BUDGET_BYTES if budget is None else budget
    max_rows = LAS_BEAM_MAX_ROWS if max_rows is None else max_rows
    return max(1, min(max_rows // W, budget // (las_beam_pool_bytes(W, Tmax, lm_row_bytes) + tree_bytes)))


def _is_tlm(lm):
    return getattr(lm, "lm_type", None) == "transformer"


def _las_lm_cost(lm, esz, W, max_len, V):
    """las_beam_chunk_capacity's keywords for a fused LM: the RNN LM's state pools per row, a Transformer LM's tree per search"""
    if _is_tlm(lm):
        return dict(tree_bytes=las_tlm_search_bytes(lm, W, max_len, V))
    return dict(lm_row_bytes=las_lm_row_bytes(lm, esz))


LAS_BUFFER_SETS = 4    # buffer sets (each with its captured steps) the batched search keeps: (S, W, LM, grid) configurations


class _LasBeamBuffers(lockstep.BookBuffers):
    """lockstep.BookBuffers of one (S, W, max_len, frame capacities) configuration of the batched search, with the LAS search's own
    pools: the stacked frames and keys, the decoder state and attention weights of two halves, the gathered parents' rows"""

    def __init__(self, dev, dt, S, W, Lmax, E, H, NL, D, AD, rows_cap, Tcap, V=0, rnn=None, grid=False, tlm=None):
        super().__init__(dev, dt, S, W, W, Lmax, V, rnn, grid)      # (rnn = (L, H, E) of a fused RNN LM; section 28)
        nb = S * W
        self.tree = None
        if tlm is not None:      # tlm = (Lcap, node_cap) of a fused Transformer LM's prefix tree (section 33): two halves of nb slots
            from .. import lm_tree
            self.tree = lm_tree.TreeState(S, W, 2 * nb, tlm[0], tlm[1], dev)
            self.lm_logits = torch.zeros(nb, V, device=dev, dtype=torch.float32)     # the LM's log-probabilities, row for row
            self.row_id = torch.arange(nb, device=dev, dtype=torch.int32)
        self.rows_cap, self.Tcap = rows_cap, Tcap
        f32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        cdt = lambda *s: torch.zeros(*s, device=dev, dtype=dt)
        self.pk, self.eo = cdt(rows_cap, AD), cdt(rows_cap, D)
        nu = max(NL - 1, 1)
        self.pools = []
        for _ in range(2):   # take turns as source and destination of a step
            P = _Stash()
            P.xc, P.c0 = cdt(nb, D + H), f32(nb, H)
            P.hu, P.cu = cdt(nu, nb, H), f32(nu, nb, H)
            P.aw = f32(nb, Tcap)
            self.pools.append(P)
        # the parents' rows of the small state arrays, gathered for the step (emoasr_las_state_gather)
        self.g_xc, self.g_c0, self.g_hu, self.g_cu = cdt(nb, D + H), f32(nb, H), cdt(nu, nb, H), f32(nu, nb, H)
        self.gact = cdt(nb, 4 * H)
        self.scores = f32(nb, Tcap)
        self.wcat = cdt(4 * H, D + H)
        self.bias = f32(NL, 4 * H)


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
    def las_step(self, S, ids, parents, first, lm_lp=None, mu=0.0):
        """one token for nb <= beam_width hypotheses of one utterance.  S: the utterance's state (las_beam_search): weights, the key
        projection, and two slot pools per state array -- [ctx | h0], c0, h / c of the layers above, the attention weights -- that
        take turns as source and destination.  ids int32 [nb] (device): the hypotheses' last tokens; parents int64 [nb] (device):
        the source slot of each; the new state of row k goes to slot k of the other pool.
        lm_lp f32 [nb, >= V] with mu > 0: the LM's next-token log-probabilities, the row becomes log_softmax(head) + mu * lm_lp[:, :V].
        -> (top values of the row f32 [nb, bw], their tokens int32 [nb, bw])"""
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
        vals, idx, _ = ops.topk(ops.log_softmax(logits, add=lm_lp, mu=mu), S.bw)   # (the fused row is formed in f32)
        S.cur = 1 - S.cur
        return vals, idx

    def las_beam_search(self, eouts, beam_width, len_weight, eos, max_len, lm=None, lm_weight=0):
        """LASDecoder.decode's search (las.py:196-287) for ONE utterance, eouts [1,T,D]: the device advances all live hypotheses by
        one token per las_step call; the host keeps the reference's bookkeeping literally -- every live beam expanded by its top
        beam_width tokens, all expansions sorted (stable), the best beam_width kept, ended beams with an empty stripped hypothesis
        dropped, final score + len_weight * len(hyp) with the leading <eos> counted, stop at beam_width results.
        lm with lm_weight > 0: any next-token LM, fused as the reference's attention search fuses it
        (decoders/transformer.py:217-226) -- one LM call per step over the live hypotheses, a stateful LM's state kept per
        hypothesis in a slot pool as the host joint search keeps it; a live row is log_softmax(head) + lm_weight * log_softmax(LM).
        Without one the launches and the results are today's.
        -> (hyps, scores), both empty when no hypothesis ever ends"""
        use_lm = lm is not None and lm_weight > 0
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
            beams = [{"hyp": [eos], "score": 0.0, "slot": 0, "lm_slot": -1}]     # (-1: the LM's zero state)
            stateful = use_lm and getattr(lm, "stateful", False)
            if stateful:
                lm_pools = lm.new_pools(2 * bw, bw)

            def lm_rows(i):
                """f32 [nb, >= V]: the LM's next-token log-probabilities after every live hypothesis"""
                nb = len(beams)
                if stateful:      # this step's half of the pool; the beams' slots are in the other one
                    base = (i % 2) * bw
                    ctl = h2d_i32([b["hyp"][-1] for b in beams] + [b["lm_slot"] for b in beams] + [base + m for m in range(nb)], dev)
                    lm.step(lm_pools, nb, ctl[:nb], ctl[nb:2 * nb], ctl[2 * nb:])
                    return lm_pools.logp[:nb]
                ys_in = torch.tensor([b["hyp"] for b in beams], dtype=torch.int64)
                if hasattr(lm, "predict_device"):     # (16 rows per call)
                    rows = [lm.predict_device(ys_in[m:m + 16], [i + 1] * min(16, nb - m)) for m in range(0, nb, 16)]
                    return rows[0] if len(rows) == 1 else torch.cat(rows, 0)
                return lm.predict(ys_in.to(dev), torch.tensor([i + 1] * nb), None)[0].to(torch.float32).contiguous()

            results = []
            for i in range(max_len):
                ids, parents = h2d_pack([torch.tensor([b["hyp"][-1] for b in beams], dtype=torch.int32),
                                         torch.tensor([b["slot"] for b in beams], dtype=torch.int64)], dev)
                if use_lm:
                    vals, idx = self.las_step(S, ids, parents, i == 0, lm_rows(i), float(lm_weight))
                else:
                    vals, idx = self.las_step(S, ids, parents, i == 0)
                vals, idx = vals.cpu(), idx.cpu()
                new_beams = []
                for k, beam in enumerate(beams):
                    for j in range(bw):
                        new_beams.append({"hyp": beam["hyp"] + [int(idx[k, j])], "score": beam["score"] + float(vals[k, j]),
                                          "slot": k, "lm_slot": (i % 2) * bw + k})
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

    # ------------------------------------------------------------------ the same search for S utterances at once
    def _las_batch_step(self, Bf, k, S, W, D, gather, upd, fuse=None):
        """one token for all S * W rows: pool k is the source, pool 1 - k the destination.  A linear chain of launches on the
        current stream, no host round trip: the state gather, the networks on the existing operators, the grouped attention,
        log-softmax + top-W and the batched bookkeeping (emoasr_beam_update_batch, which writes the next step's ids / parents).
        fuse (section 28): the RNN LM's step over all rows (emoasr_rnnlm_step_rows with the search's own ids / parent; half k of
        its pools is the source, half 1 - k the destination) and emoasr_beam_scores_topk in place of log-softmax + top-W -- the
        head's f32 logits as `dec`, the LM's raw logits as `lm`, one weight (fuse.mu) or one per row (fuse.mu_row, the grid);
        fuse.sutt: the searches share utterances (emoasr_las_attend_cells).  Dead rows and finished searches are computed by
        the LM and ignored.
        fuse.tstep (section 33): a Transformer LM instead -- emoasr_lm_tree_advance_beam from the same ids / parent / state,
        emoasr_lm_tree_step on the S W rows, emoasr_log_softmax_rows_to into the f32 rows the score kernel reads; dead rows and
        finished searches take no node and are not computed."""
        A, E, H, NL, I = self.arena, self.l_E, self.l_H, self.l_nl, self.l_I
        nb = S * W
        src, dst = Bf.pools[k], Bf.pools[1 - k]
        lib.call("emoasr_las_state_gather", ctypes.byref(gather[k]), ops._stream())
        emb = ops.embed_fwd(Bf.ids.view(nb, 1), A.w("decoder.embed.weight"), None, 1.0).view(nb, E)
        gates = ops.gemm_nt(emb, A.w("decoder.rnns.0.weight_ih")[:, :E], bias=Bf.bias[0])
        gates = ops.gemm_nt(Bf.g_xc, Bf.wcat, residual=gates, res_scale=1.0)
        h = dst.xc[:, D:]
        ops.lstm_cell_fwd(gates, Bf.g_c0, h, dst.c0, Bf.gact)
        pq = ops.gemm_nt(h, A.w("decoder.score.w_query.weight"), bias=A.p("decoder.score.w_query.bias"))
        if fuse is not None and fuse.sutt is not None:
            ops.las_attend_cells(self._las_weights(), Bf.pk, Bf.eo, Bf.moff[:fuse.U + 1], fuse.sutt, pq, src.aw, Bf.parent, Bf.state,
                                 W, dst.aw, dst.xc[:, :D], Bf.scores)
        else:
            ops.las_attend_group(self._las_weights(), Bf.pk, Bf.eo, Bf.moff, pq, src.aw, Bf.parent, Bf.state, W, dst.aw, dst.xc[:, :D],
                                 Bf.scores)
        x = h
        for l in range(1, NL):
            name = f"decoder.rnns.{l}"
            g = ops.gemm_nt(x, A.w(name + ".weight_ih"), bias=Bf.bias[l])
            g = ops.gemm_nt(Bf.g_hu[l - 1], A.w(name + ".weight_hh"), residual=g, res_scale=1.0)
            ops.lstm_cell_fwd(g, Bf.g_cu[l - 1], dst.hu[l - 1], dst.cu[l - 1], Bf.gact)
            x = dst.hu[l - 1]
        w_i = A.w("decoder.intermed.weight")
        e = ops.gemm_nt(dst.xc[:, :D], w_i[:, :D], bias=A.p("decoder.intermed.bias"))
        g = ops.gemm_nt(x, w_i[:, D:])
        hgen = ops.joint_tanh(e.view(nb, 1, I), g.view(nb, 1, I)).view(nb, I)
        logits = ops.gemm_nt(hgen, A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"), out_f32=True)
        if fuse is None:
            logp = ops.log_softmax(logits)
            V = logp.shape[1]
            lib.call("emoasr_topk", nb, V, W, ops._p(logp), V, None, 0, ops._p(Bf.vals), ops._p(Bf.cands), None, ops._stream())
        else:
            V = logits.shape[1]
            if fuse.tstep is not None:
                # the Transformer LM over the prefix tree (section 33): half k of the slots is the source, half 1 - k the destination;
                # a row without a node keeps its stale (finite) f32 row, which the update never reads
                ops.split_products(fuse.split)
                Bf.tree.advance_beam(Bf.ids, Bf.parent, Bf.state, k * nb, (1 - k) * nb)
                ops.log_softmax_rows_to(fuse.tstep(), nb, Bf.row_id, Bf.lm_logits, V, row_ok=Bf.tree.row_node)
                ops.split_products(self.split)
            else:
                lib.call("emoasr_rnnlm_step_rows", fuse.dt_code, ctypes.byref(fuse.rows[k]), ops._p(Bf.ids), ops._p(Bf.parent),
                         ops._stream())
            if fuse.mu_row is None:
                lib.call("emoasr_beam_scores_topk", lib.F32, nb, V, W, ops._p(logits), V, ops._p(Bf.lm_logits), V, fuse.mu,
                         ops._p(Bf.vals), ops._p(Bf.cands), None, ops._stream())
            else:
                lib.call("emoasr_beam_scores_topk_rows", lib.F32, nb, V, W, ops._p(logits), V, ops._p(Bf.lm_logits), V,
                         ops._p(fuse.mu_row), ops._p(Bf.vals), ops._p(Bf.cands), None, ops._stream())
        lib.call("emoasr_beam_update_batch", ctypes.byref(upd), ops._stream())

    def _las_beam_chunk(self, eouts, elens, W, len_weight, eos, max_len, lm=None, lm_weight=0, grid=None, sort=True, first=0):
        """S = len(elens) searches in lockstep -> (hyps[s], scores[s]): each search's results sorted by score (stable; sort=False:
        in the order the search found them).  lm with lm_weight > 0: the RNN LM fused on the device (section 28), or a Transformer
        LM over the prefix tree (section 33; a search past the tree's limits is a RuntimeError naming it, `first` being the
        chunk's first utterance).
        grid = (sutt, mus): the fusion grid's chunk -- the U = len(elens) utterances' frames, key projection and eouts are stored
        once, search s runs over utterance sutt[s] (consecutive per utterance) with the LM weight mus[s] > 0; lm_weight is not
        read and len_weight must be 0."""
        A, E, H, NL, AD = self.arena, self.l_E, self.l_H, self.l_nl, self.l_A
        dev, dt = eouts.device, self.dtype
        U, D = len(elens), eouts.shape[2]
        S = len(grid[0]) if grid else U
        nb = S * W
        use_lm = lm is not None and (lm_weight > 0 or grid is not None)
        if grid:
            sutt, mus = grid
            assert lm is not None and len(mus) == S and all(m > 0 for m in mus) and len_weight == 0
        V = A.p("decoder.output.bias").numel()
        bstream = getattr(self, "_beam_stream", None)   # its own stream: the legacy default stream cannot be captured
        if bstream is None:
            bstream = self._beam_stream = torch.cuda.Stream(device=dev)
        caller = torch.cuda.current_stream()
        bstream.wait_stream(caller)
        with torch.no_grad(), torch.cuda.stream(bstream), self._scope():
            moff, offs = ops.las_group_offsets(elens, dev)
            total, longest = offs[-1], max(elens)
            rows_cap = (total + 1023) // 1024 * 1024
            Tcap = (longest + 63) // 64 * 64
            rnn = tlm = lm_guard = None
            if use_lm:
                LA = lm._prepare()     # (arena bound, compute-dtype weights and the summed biases current: before the capture)
            if use_lm and _is_tlm(lm):
                P = lm.params
                assert P.vocab_size == V, "las_tlm_why_not decides what the prefix tree can fuse"
                tlm = las_tlm_dims(lm, W, max_len)
                sizes = ("tlm", P.num_layers, P.hidden_size, P.num_attention_heads, P.intermediate_size, P.vocab_size,
                         LA.shadow.dtype) + tlm
                lm_guard = (LA.flat.data_ptr(), LA.shadow.data_ptr(), lm._pe.data_ptr())
            elif use_lm:
                assert lm.V == V and LA.shadow.dtype == dt, "las_rnnlm_why_not decides what the device form can fuse"
                sizes = rnn = (lm.L, lm.H, lm.E)
                lm_guard = (LA.flat.data_ptr(), LA.shadow.data_ptr()) + tuple(b.data_ptr() for b in lm._bias)
            key = (str(dev), dt, S, W, max_len, V, E, H, NL, D, AD) + ((sizes, grid is not None) if use_lm else ())
            # a few sets of buffers (with their captured steps) are kept, least recently used first: a grid alternates between its
            # chunk shapes and the search without the LM, a caller between fused and unfused calls
            sets = getattr(self, "_las_buf_sets", None)
            if sets is None:
                sets = self._las_buf_sets = {}
            Bf = sets.pop(key, None)
            if Bf is None or Bf.rows_cap < rows_cap or Bf.Tcap < Tcap:
                Bf = None       # (drop the smaller set before the larger one is allocated)
                while len(sets) >= LAS_BUFFER_SETS:
                    sets.pop(next(iter(sets)))
                Bf = _LasBeamBuffers(dev, dt, S, W, max_len, E, H, NL, D, AD, rows_cap, Tcap, V, rnn, grid is not None, tlm)
            sets[key] = Bf
            self._las_beam_bufs = (key, Bf)      # the set of the last call
            # ---- this call's inputs, into the buffers the captured steps read ----
            Bf.moff[:U + 1].copy_(moff)
            if grid:
                Bf.sutt.copy_(ops.las_cells_map(sutt, U, dev))
                mu32 = np.asarray(mus, dtype=np.float32)        # rounded as emoasr_beam_scores_topk's one weight is
                Bf.mu_row.copy_(torch.from_numpy(np.repeat(mu32, W)).to(dev))
            mem = torch.cat([eouts[b, :elens[b]] for b in range(U)], 0).to(dt) if U > 1 else eouts[0, :elens[0]].to(dt).contiguous()
            Bf.eo[:total].copy_(mem)
            # the key projection: ONE product over all stacked frames
            ops.gemm_nt(mem, A.w("decoder.score.w_key.weight"), bias=A.p("decoder.score.w_key.bias"), out=Bf.pk[:total])
            Bf.wcat.copy_(torch.cat([A.w("decoder.rnns.0.weight_ih")[:, E:], A.w("decoder.rnns.0.weight_hh")], dim=1))
            for l in range(NL):
                Bf.bias[l].copy_(self._las_bias(l))

            def reset(done):
                lockstep.reset_book(Bf, S, W, eos, done)
                P = Bf.pools[0]   # step 0 reads its parents' rows here: zeros, so the general step is the first step too
                P.xc.zero_(); P.c0.zero_(); P.hu.zero_(); P.cu.zero_(); P.aw.zero_()
                if tlm:      # every slot the empty prefix, no node taken, no bit raised: step 0 reads slot s W of half 0
                    Bf.tree.reset()
                elif use_lm:   # (the warm-up's steps write both halves) step 0 reads half 0 of the LM's pools at the search's row 0
                    Bf.lm_h[:, :nb].zero_(); Bf.lm_c[:, :nb].zero_()

            mu = 0.0 if (grid or not use_lm) else float(np.float32(lm_weight))     # (the grid: the weights are device data)
            gkey = (A.flat.data_ptr(), A.shadow.data_ptr(), float(len_weight), eos, id(Bf), ops.dt(Bf.pk), lm_guard, mu,
                    U if grid else None)
            if Bf.graphs is None or Bf.graphs[0] != gkey:
                ub = lib.BeamUpdateBatch()
                lockstep.fill_beam_update(ub, Bf, S, W, W, eos, max_len, len_weight)     # attention only: psi and lm_at stay NULL
                gather = []
                for k in (0, 1):
                    P = Bf.pools[k]
                    pairs = [(P.xc, Bf.g_xc), (P.c0, Bf.g_c0)]
                    for l in range(NL - 1):
                        pairs += [(P.hu[l], Bf.g_hu[l]), (P.cu[l], Bf.g_cu[l])]
                    gather.append(ops.las_state_gather_args(pairs, Bf.parent, Bf.state, W))
                fuse = None
                if use_lm:
                    fuse = _Stash()
                    fuse.dt_code, fuse.mu, fuse.mu_row = ops.dt(Bf.pk), mu, Bf.mu_row if grid else None
                    fuse.sutt, fuse.U = (Bf.sutt, U) if grid else (None, U)
                    fuse.tstep = None
                    if tlm:      # the step's record holds the parameter addresses of this arena (lm_guard is in the key)
                        from .. import lm_tree
                        fuse.split = lm._split()
                        ops.split_products(fuse.split)
                        fuse.tstep = lm_tree.TreeStep(lm, Bf.tree)
                        ops.split_products(self.split)
                    else:
                        # the even step reads half 0 of the LM's pools and writes half 1, the odd step the reverse
                        fuse.rows, fuse.tabs, fuse.ws = lockstep.rnnlm_rows_pair(lm, LA, Bf, nb, V, fuse.dt_code, even_src=0)
                graphs = lockstep.capture_two_steps(lambda k: self._las_batch_step(Bf, k, S, W, D, gather, ub, fuse), reset)
                Bf.graphs = (gkey, graphs, (ub, gather, fuse))
            reset(0)
            host = lockstep.replay_until_done(Bf.graphs[1], Bf, max_len, S, self, "_las_beam_stats")   # (totals: tools/las_beam_bench.py)
            if tlm:      # a raised bit is an error naming the search and the limit, as the host form's max_seq_len assertion is
                names = ([f"utterance {first + u} at lm_weight {float(m):g}" for u, m in zip(sutt, mus)] if grid
                         else [f"utterance {first + s}" for s in range(S)])
                Bf.tree.raise_for_status("las_beam_search_batch (las_tlm_fusion = 'device')", names, tags=True)
        caller.wait_stream(bstream)
        return lockstep.batch_nbest_from_pack(host, Bf.pack_off, S, W, max_len, sort)

    def las_beam_search_batch(self, eouts, elens, beam_width, len_weight, eos, max_len, lm=None, lm_weight=0, lm_weights=None,
                              len_weights=None):
        """las_beam_search for every utterance of the batch: eouts [B, Tmax, D], utterance b over its own
        elens[b] >= 1 frames (frames past them are never read) -> (hyps, scores) with hyps[b] / scores[b] what las_beam_search
        returns for eouts[b:b+1, :elens[b]].  All searches of a chunk step in lockstep on the device: per step one captured chain
        of launches, no host round trip, one download at the end.  Chunks hold at most las_beam_chunk_capacity searches.
        lm with lm_weight > 0: the RNN LM fused inside the chain (section 28; modeling/functions.py:las_rnnlm_why_not says what it takes).
        lm_weights / len_weights: the shallow-fusion grid instead -- (hyps[b][c], scores[b][c]) for the cells in lm_weight-outer,
        len_weight-inner order; every distinct positive lm_weight of an utterance is searched once at len_weight 0 (the searches of
        an utterance share its frames: emoasr_las_attend_cells), weights <= 0 fold into one search without the LM, and the
        len_weights are expanded on the host in double (beam_search_device.expand_len_weights); len_weight and lm_weight are
        not read."""
        W = int(beam_width)
        elens = [int(n) for n in elens]
        B, T = eouts.shape[0], eouts.shape[1]
        if len(elens) != B or any(n < 1 or n > T for n in elens):
            raise ValueError(f"las_beam_search_batch: every utterance needs 1 <= elens[b] <= {T} frames, got elens {elens}")
        V = self.arena.p("decoder.output.bias").numel()
        assert 1 <= W <= 32 and W <= V, "the batched LAS search handles beams of 1..32 hypotheses, at most the vocabulary"
        Tcap = (max(elens) + 63) // 64 * 64
        esz = 2 if self.dtype == torch.bfloat16 else 4
        if lm_weights is not None:
            return self._las_beam_grid(eouts, elens, W, eos, max_len, lm, lm_weights, len_weights, Tcap, esz, V)
        if lm is None or lm_weight <= 0:
            lm, lm_weight = None, 0
        cap = las_beam_chunk_capacity(W, Tcap, **_las_lm_cost(lm, esz, W, max_len, V))
        hyps, scores = [], []
        for b0 in range(0, B, cap):
            n = elens[b0:b0 + cap]
            if lm is None:
                h, s = self._las_beam_chunk(eouts[b0:b0 + cap, :max(n)], n, W, len_weight, eos, max_len)
            elif _is_tlm(lm):
                h, s = self._las_beam_chunk(eouts[b0:b0 + cap, :max(n)], n, W, len_weight, eos, max_len, lm, lm_weight, first=b0)
            else:
                h, s = self._las_beam_chunk(eouts[b0:b0 + cap, :max(n)], n, W, len_weight, eos, max_len, lm, lm_weight)
            hyps += h
            scores += s
        return hyps, scores

    def _las_beam_grid(self, eouts, elens, W, eos, max_len, lm, lm_weights, len_weights, Tcap, esz, V):
        """las_beam_search_batch's grid: lockstep.run_fusion_grid on the LAS chunks"""
        lm_weights, len_weights = [float(a) for a in lm_weights], [float(b) for b in len_weights]
        B = len(elens)

        def search_plain():      # the search without the LM: the batched search as it is, no LM launches
            cap = las_beam_chunk_capacity(W, Tcap)
            hyps, scores = [], []
            for b0 in range(0, B, cap):
                n = elens[b0:b0 + cap]
                h, s = self._las_beam_chunk(eouts[b0:b0 + cap, :max(n)], n, W, 0, eos, max_len, sort=False)
                hyps += h
                scores += s
            return hyps, scores

        def search_fused(positive, weights, found):
            cap = las_beam_chunk_capacity(W, Tcap, **_las_lm_cost(lm, esz, W, max_len, V))
            for utts, n, sutt, k_local in lockstep.grid_chunks(B, len(positive), cap, elens):
                ks = [positive[j] for j in k_local]
                sub = eouts[utts[0]:utts[-1] + 1, :max(n)]      # (a chunk's utterances are consecutive)
                more = dict(first=utts[0]) if _is_tlm(lm) else {}
                h, s = self._las_beam_chunk(sub, n, W, 0, eos, max_len, lm, 0, grid=(sutt, [weights[k] for k in ks]), sort=False, **more)
                for i, (u, k) in enumerate(zip(sutt, ks)):
                    found[utts[u]][k] = (h[i], s[i])

        return lockstep.run_fusion_grid(B, lm_weights, len_weights, lm is not None, search_plain, search_fused,
                                        lambda f, a: lockstep.expand_len_weights(*f, len_weights))
