"""RNN-Transducer decoder: LSTM prediction network, joint network, transducer loss; the greedy and beam searches are its base class
(engine/rnnt_search.py).
  reference: asr/modeling/decoders/rnn_transducer.py:81-240"""
import os

import torch

from .. import ops
from ..recurrence import lstm_stack_bwd, lstm_stack_fwd
from .arena import _Stash, _cfg, h2d_i32
from .rnnt_search import RNNTSearch


class RNNTDecoder(RNNTSearch):
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
        A = self.arena
        p_emb = self.p_emb if training else 0.0
        p = self.p_dec if training else 0.0
        s_emb = self._seed(7000)
        x = ops.embed_fwd(ids_tm, A.w("decoder.embed.weight"), None, 1.0, p_emb, s_emb)  # [U,B,E]
        # per layer the input projection + the recurrence (one cooperative launch or the per-position chain), then dropout; a
        # generator: each bias sum is launched when the stack reaches its layer
        spec = ((A.w(f"decoder.rnns.{l}.weight_ih_l0"), A.w(f"decoder.rnns.{l}.weight_hh_l0"), self._lstm_bias(f"decoder.rnns.{l}"),
                 self._seed(7010 + l), state[0][l] if state is not None else None, state[1][l] if state is not None else None)
                for l in range(self.r_nl))
        x, new_state, layers = lstm_stack_fwd(x, spec, p, keep)
        st = None
        if keep:
            st = _Stash()
            st.ids, st.layers, st.s_emb, st.p, st.p_emb = ids_tm, layers, s_emb, p, p_emb
        return x, new_state, st

    def rnnt_recurrency_bwd(self, st, dy):
        """dy [U,B,H] gradient w.r.t. the prediction-network output; accumulates parameter gradients"""
        self._apply_mode()
        A = self.arena
        grads = [tuple(A.g(f"decoder.rnns.{l}.{n}_l0") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                 for l in range(self.r_nl)]
        dy = lstm_stack_bwd(dy, st.layers, grads, st.p)
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
            return self._rnnt_joint_bwd(st, dpre)

    def _rnnt_joint_bwd(self, st, dpre):
        """dpre [B*T*U, J]: gradient of the joint network's pre-activation -> d_eouts [B,T,d]; w_enc, w_dec, then the prediction network"""
        J, H, (B, T, U) = self.r_J, self.r_H, (st.B, st.T, st.U)
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
        return self._rnnt_joint_bwd(st, dpre)
