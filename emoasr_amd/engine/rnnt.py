"""RNN-Transducer decoder: LSTM prediction network, joint network, transducer loss, greedy and beam search.
  reference: asr/modeling/decoders/rnn_transducer.py:81-240"""
import os
from ctypes import c_void_p

import torch

from .. import lockstep, ops
from ..recurrence import lstm_stack_bwd, lstm_stack_fwd
from .arena import _Stash, _cfg, h2d_i32


class RNNTDecoder:
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
        from .. import lib
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

    # ---- the batched greedy search in lockstep (csrc/rnnt_greedy_batch.hip) -------------------------------
    # joint rows per step: S K <= 1024, so a chunk holds 1024 // K searches (128 at K = 8).  What the cap implies at the L4 sizes
    # (J = 512, V = 1000, bf16): 1 MB of joint rows, 2 MB of logits, 2 S state slots per layer (0.8 MB for two layers), and the
    # stacked w_enc . eouts + b of the chunk, 1 KB per frame (39 MB for 128 utterances of 300 frames); twice that in f32.
    _GREEDY_BATCH_ROWS = 1024
    # frames_per_step and the steps between two reads of the live counter (once ceil(max(elens) / K) steps have run): the fastest
    # of K = 1 / 2 / 4 / 8 at every batch size and dtype measured, and of blocks of 4 / 8 / 16 / 32
    _GREEDY_BATCH_K = 8
    _GREEDY_BATCH_POLL = 32

    def rnnt_greedy_batch_why_not(self):
        """why the batched greedy search cannot take this model (None: it can): nl >= 1 and the limits of
        emoasr_rnnt_beam_lstm_rows / _joint_rows that rnnt_beam_device_ok checks for width 1 -- 16 rows of H floats in the joint
        kernel's LDS, nin + H columns in the LSTM step's (the MFMA plan's 1904 in bf16, as rnnt_beam_lm_why_not) -- with the
        kernels' vector widths.  rnnt_beam_device_ok's bound on the vocabulary belongs to the pick kernel, which keeps a row in
        LDS; the greedy book kernel reads its rows from global memory, so any vocabulary of two labels or more is taken."""
        A, H, nl = self.arena, self.r_H, self.r_nl
        if self.dtype not in (torch.float32, torch.bfloat16):
            return f"the compute dtype {self.dtype} is neither float32 nor bfloat16"
        if nl < 1:
            return "the prediction network has no LSTM layer"
        V_ = A.w("decoder.output.weight").shape[0]
        if V_ < 2:
            return f"the vocabulary ({V_}) has no label beside blank"
        vec, wide = (8, 1904) if self.dtype == torch.bfloat16 else (4, 2368)
        nins = [A.w(f"decoder.rnns.{l}.weight_ih_l0").shape[1] for l in range(nl)]
        if H % 8 or H % vec or any(n % vec for n in nins) or max(nins) + H > wide or 16 * H * 4 > 64 * 1024:
            return (f"the prediction network's sizes (embedding {self.r_emb}, hidden {H}, layers {nl}) are outside "
                    f"emoasr_rnnt_beam_lstm_rows' limits")
        return None

    def _rnnt_greedy_batch_graph(self, S, K, blank, eos, max_seq_len, total, longest):
        """static buffers of S searches of K frames per step over <= st.rows frames in all, none longer than st.tmax, and ONE STEP
        of all of them (LSTM layers on S rows, joint on S K rows, output product, book) captured as a HIP graph.  The warm-up runs
        the body with every search finished (no frames): every row is inactive, no state is touched."""
        from .. import lib
        tab = self.__dict__.setdefault("_greedy_batch_static", {})
        key = (S, K, blank, eos, max_seq_len)
        st = tab.get(key)
        if st is not None and st.rows >= total and st.tmax >= longest:
            return st
        A, J, H, nl = self.arena, self.r_J, self.r_H, self.r_nl
        dev = A.flat.device
        st = _Stash()
        st.rows, st.tmax = 1024, 512
        while st.rows < total:
            st.rows *= 2
        while st.tmax < longest:
            st.tmax *= 2
        R = st.R = S * K
        st.nslots = 2 * S
        st.ph = [torch.zeros(st.nslots, H, device=dev, dtype=self.dtype) for _ in range(nl)]
        st.pc = [torch.zeros(st.nslots, H, device=dev, dtype=torch.float32) for _ in range(nl)]
        st.e = torch.zeros(st.rows, J, device=dev, dtype=self.dtype)
        st.hj = torch.zeros(R, J, device=dev, dtype=self.dtype)
        st.row_off = torch.zeros(S + 1, device=dev, dtype=torch.int32)
        st.ctl, st.state, st.hyp, st.align, st.lens, st.live = ops.rnnt_greedy_batch_buffers(S, K, max_seq_len, st.tmax, dev)
        st.bias = [self._lstm_bias(f"decoder.rnns.{l}").contiguous() for l in range(nl)]   # (refreshed per search)

        def launches():
            """the step without its bookkeeping -> the logits [S K, V] of the rows of st.ctl"""
            with self._scope():
                dtc = ops.dt(st.ph[0])
                l_lab, l_src, l_dst, l_act = (c_void_p(st.ctl.data_ptr() + 8 * S * i) for i in range(4))
                j_dst, j_act, j_row = (c_void_p(st.ctl.data_ptr() + 8 * (4 * S + R * i)) for i in range(3))
                emb = A.w("decoder.embed.weight")
                xtab, ldx, nx, xidx = emb, emb.shape[1], emb.shape[0], l_lab
                for l in range(nl):
                    w_ih, w_hh = A.w(f"decoder.rnns.{l}.weight_ih_l0"), A.w(f"decoder.rnns.{l}.weight_hh_l0")
                    lib.call("emoasr_rnnt_beam_lstm_rows", dtc, S, w_ih.shape[1], H, ops._p(xtab), ldx, nx, xidx, ops._p(w_ih),
                             ops._p(w_hh), ops._p(st.bias[l]), ops._p(st.ph[l]), ops._p(st.pc[l]), st.nslots, l_src, l_dst, l_act,
                             ops._stream())
                    xtab, ldx, nx, xidx = st.ph[l], H, st.nslots, l_dst
                lib.call("emoasr_rnnt_beam_joint_rows", dtc, R, H, J, st.rows, ops._p(st.ph[nl - 1]), st.nslots, j_dst, j_act,
                         ops._p(A.w("decoder.w_dec.weight")), ops._p(A.p("decoder.w_dec.bias")), ops._p(st.e), j_row,
                         ops._p(st.hj), ops._stream())
                return ops.gemm_nt(st.hj, A.w("decoder.output.weight"), bias=A.p("decoder.output.bias"))

        def body():
            with self._scope():    # (the scope pins the stream the calls go to: the book kernel belongs to the capture as well)
                logits = launches()
                ops.rnnt_greedy_batch_book(st.row_off, K, blank, max_seq_len, logits, st.ctl, st.state, st.hyp, st.align, st.lens,
                                           st.live)

        st.launches = launches     # (tests run the same launches step by step and keep the books on the host)
        ops.rnnt_greedy_batch_start(st.row_off, K, eos, max_seq_len, st.ctl, st.state, st.lens, st.live)   # (row_off all zero)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()   # warm-up outside the capture (allocator, lazy initialisation)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        st.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(st.graph):
            body()
        tab[key] = st
        return st

    def _rnnt_greedy_batch_load(self, eouts, elens, K, blank, eos, max_seq_len):
        """one chunk's searches ready for their first step: the buffers and graph, w_enc . eouts + b stacked, the zero states, the
        control words of step 0"""
        A, nl = self.arena, self.r_nl
        S, total, longest = len(elens), sum(elens), max(elens)
        st = self._rnnt_greedy_batch_graph(S, K, blank, eos, max_seq_len, total, longest)
        offs = [0]
        for b in range(S):
            # w_enc . eouts + b per utterance, as the per-utterance forms compute it (a row's bits then do not depend on the batch)
            if elens[b]:
                st.e[offs[-1]:offs[-1] + elens[b]].copy_(ops.gemm_nt(eouts[b, :elens[b]], A.w("decoder.w_enc.weight"),
                                                                     bias=A.p("decoder.w_enc.bias")))
            offs.append(offs[-1] + elens[b])
        st.row_off.copy_(torch.tensor(offs, dtype=torch.int32))
        for l in range(nl):
            st.bias[l].copy_(self._lstm_bias(f"decoder.rnns.{l}"))
            st.ph[l].view(S, 2, self.r_H)[:, 0].zero_()    # slot 2 s: the zero state search s starts from
            st.pc[l].view(S, 2, self.r_H)[:, 0].zero_()
        ops.rnnt_greedy_batch_start(st.row_off, K, eos, max_seq_len, st.ctl, st.state, st.lens, st.live)
        return st

    @staticmethod
    def _rnnt_greedy_batch_read(st, S):
        lens = st.lens.tolist()
        hyp, align = st.hyp.cpu(), st.align.cpu()
        return [hyp[s, :lens[s][0]].tolist() for s in range(S)], [align[s, :lens[s][1]].tolist() for s in range(S)]

    def rnnt_greedy_batch(self, eouts, elens, blank, eos, max_seq_len=256, frames_per_step=None, poll_block=None):
        """time-synchronous greedy search (rnn_transducer.py:194-240) of a BATCH in lockstep, the bookkeeping on the device
        (csrc/rnnt_greedy_batch.hip): eouts [B, Tmax, d], utterance b is searched over its own elens[b] frames -> (hyps, aligns)
        as rnnt_greedy returns them.  One step -- LSTM layers on S rows, joint and output product on S K rows (K =
        frames_per_step consecutive frames of every live search against its current state), book -- is captured once per (S, K)
        and replayed: ceil(max(elens) / K) times (no search can finish sooner), then in blocks of poll_block steps with one
        4-byte read of the live counter after each, until it is zero; never more than max(elens) + max_seq_len + 1 steps.
        Batches are searched in chunks of _GREEDY_BATCH_ROWS // K utterances.  A model outside the rows kernels' limits is a
        ValueError naming the reason (rnnt_greedy_batch_why_not); rnnt_greedy takes any model.  self.rnnt_greedy_batch_stats:
        the replays and counter reads of the last call."""
        K = self._GREEDY_BATCH_K if frames_per_step is None else int(frames_per_step)
        block = self._GREEDY_BATCH_POLL if poll_block is None else int(poll_block)
        if not 1 <= K <= ops.RNNT_GREEDY_BATCH_MAX_FRAMES:
            raise ValueError(f"rnnt_greedy_batch: frames_per_step {K} is outside 1..{ops.RNNT_GREEDY_BATCH_MAX_FRAMES}")
        if block < 1:
            raise ValueError(f"rnnt_greedy_batch: poll_block {block} is below 1")
        elens = [int(v) for v in elens]
        B = eouts.shape[0]
        assert len(elens) == B and all(0 <= n <= eouts.shape[1] for n in elens), (elens, tuple(eouts.shape))
        why = self.rnnt_greedy_batch_why_not()
        if why is not None:
            raise ValueError(f"rnnt_greedy_batch: {why}")
        stats = self.rnnt_greedy_batch_stats = dict(steps=0, polls=0, bound=0)
        hyps, aligns = [], []
        cap = max(1, self._GREEDY_BATCH_ROWS // K)
        with self._scope(), torch.no_grad():
            self.arena.refresh_shadow()
            for b0 in range(0, B, cap):
                lens = elens[b0:b0 + cap]
                st = self._rnnt_greedy_batch_load(eouts[b0:b0 + cap], lens, K, blank, eos, max_seq_len)
                bound = max(lens) + max_seq_len + 1
                steps, todo = 0, -(-max(lens) // K)
                while True:
                    for _ in range(todo):
                        st.graph.replay()
                    steps += todo
                    live = int(st.live.item())
                    stats["polls"] += 1
                    if live == 0:
                        break
                    todo = min(block, bound - steps)
                    if todo <= 0:
                        raise RuntimeError(f"rnnt_greedy_batch: {live} searches still live after {steps} steps (bound {bound})")
                stats["steps"] += steps
                stats["bound"] += bound
                h, a = self._rnnt_greedy_batch_read(st, len(lens))
                hyps += h
                aligns += a
        return hyps, aligns

    def rnnt_beam_search(self, eouts, beam_width, blank, eos, num_expands=3, return_scores=False, lm=None, lm_weight=0,
                         len_weight=0):
        """alignment-length synchronous beam search for ONE utterance (rnn_transducer.py:242-325,348-359): the expansion round as a
        replayed HIP graph (_rnnt_beam_search_graph) unless EMOASR_RNNT_BEAM_GRAPH=0 or the utterance does not fit its static
        buffers; then the launch chain below.  return_scores: (hyps, float64 scores) instead of hyps (tests compare the two forms).
        lm with lm_weight > 0: shallow fusion through the launch chain, the only host form that fuses;
        without it lm_weight and len_weight are not read."""
        if lm is not None and lm_weight > 0:
            return self._rnnt_beam_search_chain(eouts, beam_width, blank, eos, num_expands, return_scores, lm, lm_weight, len_weight)
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
            from .. import lib
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
        from .. import lib
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

    _BEAM_BATCH_CAP = 64   # searches per launch chain: S W <= 1024 rows, S (E + 1) W state slots per layer (25 MB at H = 512, W = 16)

    _BEAM_POOL_BUDGET = 256 << 20   # bytes of state pools (prediction network + LM) one chunk of fused searches may hold

    def rnnt_beam_lm_why_not(self, lm):
        """why the batched device search cannot fuse this LM (None: it can).  The LM's LSTM layers run through
        emoasr_rnnt_beam_lstm_rows beside the prediction network's and csrc/rnnt_beam_lm.hip ranks the candidates: an RNN LM
        (lm_type == "rnn") of the engine's compute dtype and product mode, its layer sizes inside that kernel's LDS plans, its
        vocabulary at least the model's"""
        if getattr(lm, "lm_type", None) != "rnn":
            return f"lm_type {getattr(lm, 'lm_type', None)!r} is not 'rnn' (no per-hypothesis state the slot pools could hold)"
        V_ = self.arena.w("decoder.output.weight").shape[0]
        if lm.compute_dtype != self.dtype or lm.compute_dtype not in (torch.float32, torch.bfloat16) or bool(lm.f32_split) != bool(self.split):
            return f"the LM computes in {lm.compute_dtype} (split products: {bool(lm.f32_split)}), the model in {self.dtype} ({bool(self.split)})"
        vec, wide = (8, 1904) if self.dtype == torch.bfloat16 else (4, 2368)
        if lm.L < 1 or lm.H % 8 or lm.H % vec or lm.E % vec or max(lm.E, lm.H) + lm.H > wide or 16 * lm.H * 4 > 64 * 1024:
            return f"the LM's sizes (embedding {lm.E}, hidden {lm.H}, layers {lm.L}) are outside emoasr_rnnt_beam_lstm_rows' limits"
        if lm.V < V_:
            return f"the LM's vocabulary ({lm.V}) is smaller than the model's ({V_})"
        return None

    _TLM_POOL_BUDGET = 8 << 30     # bytes of K / V node pools one chunk of Transformer-LM fused searches may hold (the joint search's
                                   # cache budget, not the 256 MB of the LSTM pools: a node is layers x d x 2 values)

    def rnnt_beam_tlm_why_not(self, lm):
        """why the batched device search cannot fuse this LM over the prefix tree (None: it can).  The LM's step
        is emoasr_lm_tree_step (csrc/lm_tree.hip) beside the prediction network's launches: a causal Transformer LM (lm_type ==
        "transformer") of the engine's compute dtype and product mode, its vocabulary at least the model's, its heads and its longest
        prefix inside emoasr_lm_tree_attn's plan.  rnnt_beam_lm_why_not keeps answering for the RNN form."""
        from .. import lm_tree
        if getattr(lm, "lm_type", None) != "transformer":
            return f"lm_type {getattr(lm, 'lm_type', None)!r} is not 'transformer'"
        if not getattr(lm, "causal", False):
            return "there is no causal LM (the prefix tree steps p(next token | prefix))"
        if lm.compute_dtype != self.dtype or lm.compute_dtype not in (torch.float32, torch.bfloat16) or bool(lm.f32_split) != bool(self.split):
            return f"the LM computes in {lm.compute_dtype} (split products: {bool(lm.f32_split)}), the model in {self.dtype} ({bool(self.split)})"
        P = lm.params
        V_ = self.arena.w("decoder.output.weight").shape[0]
        if P.vocab_size < V_:
            return f"the LM's vocabulary ({P.vocab_size}) is smaller than the model's ({V_})"
        if not lm_tree.head_ok(P.hidden_size, P.num_attention_heads):
            return (f"the LM's heads ({P.hidden_size} over {P.num_attention_heads}) are outside emoasr_lm_tree_attn's plan "
                    f"(8 .. 128 wide, a multiple of 8)")
        if lm_tree.attn_lds_bytes(P.max_seq_len) > lm_tree.LDS_BYTES:
            return (f"max_seq_len {P.max_seq_len} needs {lm_tree.attn_lds_bytes(P.max_seq_len)} bytes of LDS in emoasr_lm_tree_attn "
                    f"({lm_tree.LDS_BYTES} at most)")
        return None

    @staticmethod
    def _tlm_frames(longest):
        """the frame capacity the tree's buffers are sized for: the longest utterance, rounded up to 64 frames"""
        return max(64, -(-int(longest) // 64) * 64)

    def rnnt_beam_tlm_chunk_capacity(self, W, E, lm, longest):
        """searches per launch chain with the Transformer LM: _BEAM_BATCH_CAP, and no more than hold their tree -- W (E - 1) frames + 1
        nodes per search (the worst case: every fused round steps W rows) of (K, V) x layers x d values, the lists of its (E + 1) W
        slots and the prediction network's pools -- inside _TLM_POOL_BUDGET; never below one"""
        from .. import lm_tree
        P = lm.params
        esz = 2 if self.dtype == torch.bfloat16 else 4
        frames = self._tlm_frames(longest)
        nodes, Lcap = lm_tree.node_cap(W, E, frames), lm_tree.list_cap(E, frames, P.max_seq_len)
        per_search = (2 * P.num_layers * nodes * P.hidden_size * esz + (E + 1) * W * (Lcap + 1) * 4
                      + (E + 1) * W * (esz + 4) * self.r_nl * self.r_H)
        return max(1, min(self._BEAM_BATCH_CAP, self._TLM_POOL_BUDGET // per_search))

    def rnnt_beam_device_ok(self, beam_width, num_expands=3, lm=None):
        """does the model fit the batched search's round kernels?  (the limits of the fused round, _rnnt_beam_round_graph, and of
        the bookkeeping kernel: beam_width <= 16, beam_width <= V - 1; with an LM to fuse, rnnt_beam_lm_why_not as well)"""
        A, H, nl = self.arena, self.r_H, self.r_nl
        V_ = A.w("decoder.output.weight").shape[0]
        nin_max = max(A.w(f"decoder.rnns.{l}.weight_ih_l0").shape[1] for l in range(nl)) if nl else 0
        fits = V_ * 4 <= 60 * 1024 and 16 * H * 4 <= 64 * 1024 and (self.dtype == torch.bfloat16 or nin_max + H <= 2368)
        if lm is not None and self.rnnt_beam_lm_why_not(lm) is not None:
            return False
        return nl >= 1 and fits and 1 <= beam_width <= min(ops.RNNT_BEAM_MAX_WIDTH, V_ - 1) and 1 <= num_expands <= ops.RNNT_BEAM_MAX_EXPANDS

    def rnnt_beam_chunk_capacity(self, W, E, lm=None):
        """searches per launch chain: _BEAM_BATCH_CAP, and with an LM no more than hold their state pools -- (E + 1) W slots per
        search of (h in the compute dtype, c in f32) per layer of both networks -- inside _BEAM_POOL_BUDGET; never below one"""
        if lm is None:
            return self._BEAM_BATCH_CAP
        esz = 2 if self.dtype == torch.bfloat16 else 4
        per_search = (E + 1) * W * (esz + 4) * (self.r_nl * self.r_H + lm.L * lm.H)
        return max(1, min(self._BEAM_BATCH_CAP, self._BEAM_POOL_BUDGET // per_search))

    @staticmethod
    def rnnt_len_expand(hyps, scores, len_weight):
        """the finish of a fused search: final = score + len_weight * len(hyp) in doubles (the hypothesis with its leading <sos>,
        decoders/transformer.py:274), then a stable descending re-sort"""
        w = float(len_weight)
        sc = [float(s) + w * float(len(h)) for h, s in zip(hyps, scores)]
        order = sorted(range(len(sc)), key=lambda i: -sc[i])
        return [hyps[i] for i in order], [sc[i] for i in order]

    def rnnt_beam_search_batch(self, eouts, elens, beam_width, blank, eos, num_expands=3, lm=None, lm_weights=None, len_weights=None,
                               tlm_fusion="host"):
        """alignment-length synchronous beam search for a BATCH (rnn_transducer.py:242-325 per utterance; the reference asserts a
        batch of one): eouts [B, Tmax, d], utterance b is searched over its own elens[b] frames -> (hyps[b][n], scores[b][n]),
        best first, hypotheses with the leading <sos>, float64 scores.  The bookkeeping runs on the device
        (csrc/rnnt_beam_book.hip): one frame -- num_expands rounds of (LSTM layers, joint, output product, pick, book) over all
        S W rows -- is captured once per (S, W) and replayed max(elens) times without a synchronisation in between.  Batches above
        _BEAM_BATCH_CAP are searched in chunks.  A model outside the round kernels' limits is searched utterance by utterance
        through rnnt_beam_search.

        lm_weights (a list; None: the call above, unchanged): the shallow-fusion GRID ->
        (hyps[b][cell][n], scores[b][cell][n]), cells in lm_weight-outer, len_weight-inner order (len_weights None: [0]).  A search
        is an (utterance, lm_weight) pair: every distinct positive lm_weight of an utterance is searched once with the LM's LSTM
        stepped beside the prediction network's, all weights <= 0 (or no LM) are ONE search on the chain above.  The len_weights
        are a host expansion of a fused search's results (rnnt_len_expand); the search without the LM does not read them.  An LM
        or a width the device form cannot take is searched utterance by utterance through the host form.

        tlm_fusion ("host", the default: everything above, unchanged; or "device"; decoder.rnnt_tlm_fusion): with "device" a
        Transformer LM is fused on the device too, stepped over a prefix tree of K / V nodes in chunks of
        rnnt_beam_tlm_chunk_capacity searches; an LM or a width that form cannot take is then a ValueError naming the reason, and a
        search that outgrows the LM's positions or its node pool a RuntimeError naming the search.  self.rnnt_tlm_stats: the nodes
        every search of the last such call took, and their bound."""
        if tlm_fusion not in ("host", "device"):
            raise ValueError(f"emoasr_amd: rnnt_tlm_fusion is 'host' or 'device', not {tlm_fusion!r}")
        elens = [int(v) for v in elens]
        B = eouts.shape[0]
        assert len(elens) == B and all(0 <= n <= eouts.shape[1] for n in elens), (elens, tuple(eouts.shape))
        with self._scope():
            self.arena.refresh_shadow()
        if lm_weights is not None:
            return self._rnnt_beam_search_grid(eouts, elens, beam_width, blank, eos, num_expands, lm, lm_weights, len_weights,
                                               tlm_fusion)
        hyps, scores = [], []
        if not self.rnnt_beam_device_ok(beam_width, num_expands):
            for b in range(B):
                if elens[b] == 0:
                    h, s = [[eos]], [0.0]
                else:
                    h, s = self.rnnt_beam_search(eouts[b:b + 1, :elens[b]], beam_width, blank, eos, num_expands, return_scores=True)
                hyps.append(h)
                scores.append([float(v) for v in s])
            return hyps, scores
        for b0 in range(0, B, self._BEAM_BATCH_CAP):
            h, s = self._rnnt_beam_search_device(eouts[b0:b0 + self._BEAM_BATCH_CAP], elens[b0:b0 + self._BEAM_BATCH_CAP], beam_width,
                                                 blank, eos, num_expands)
            hyps += h
            scores += s
        return hyps, scores

    def _rnnt_beam_search_grid(self, eouts, elens, W, blank, eos, E, lm, lm_weights, len_weights, tlm_fusion="host"):
        """rnnt_beam_search_batch with lm_weights: lockstep.run_fusion_grid over (utterance, weight) pairs in chunks; the fused
        searches' results are expanded by rnnt_len_expand, the search without the LM does not read the len_weights.  tlm_fusion ==
        "device" sends a Transformer LM through the same chunks over the prefix tree instead of the host chain."""
        from ..modeling.lm import require_next_token_lm
        lm_weights = [float(a) for a in lm_weights]
        len_weights = [0.0] if len_weights is None else [float(v) for v in len_weights]
        require_next_token_lm(lm, max(lockstep.grid_cell_plan(lm_weights, len_weights, lm is not None)[0]))
        B = len(elens)

        tlm = tlm_fusion == "device" and getattr(lm, "lm_type", None) == "transformer"
        if tlm and any(a > 0 for a in lm_weights):      # asked for by name: no quiet detour through the host chain
            why = self.rnnt_beam_tlm_why_not(lm)
            if why is None and not self.rnnt_beam_device_ok(W, E):
                why = f"the model, beam_width {W} or num_expands {E} is outside the batched device search's limits"
            if why is not None:
                raise ValueError(f"emoasr_amd: rnnt_tlm_fusion = 'device' cannot fuse this LM: {why}")

        def search_fused(positive, weights, found):
            if not tlm and not self.rnnt_beam_device_ok(W, E, lm):      # the host chain, utterance by utterance
                for b in range(B):
                    for k in positive:
                        if elens[b] == 0:
                            found[b][k] = ([[eos]], [0.0])
                        else:
                            h, s = self._rnnt_beam_search_chain(eouts[b:b + 1, :elens[b]], W, blank, eos, E, True, lm, weights[k], 0)
                            found[b][k] = (h, [float(v) for v in s])
                return
            pairs = [(b, k) for b in range(B) for k in positive]
            if tlm:
                cap = self.rnnt_beam_tlm_chunk_capacity(W, E, lm, max(elens, default=0))
                self.rnnt_tlm_stats = dict(nodes=[], node_cap=0, lcap=0)
            else:
                cap = self.rnnt_beam_chunk_capacity(W, E, lm)
            for p0 in range(0, len(pairs), cap):
                chunk = pairs[p0:p0 + cap]
                h, s = self._rnnt_beam_search_device(eouts, elens, W, blank, eos, E, lm, [weights[k] for _, k in chunk],
                                                     [b for b, _ in chunk])
                for i, (b, k) in enumerate(chunk):
                    found[b][k] = (h[i], s[i])

        return lockstep.run_fusion_grid(B, lm_weights, len_weights, lm is not None,
                                        lambda: self.rnnt_beam_search_batch(eouts, elens, W, blank, eos, E), search_fused,
                                        lambda f, a: [self.rnnt_len_expand(*f, w) if a > 0 else f for w in len_weights])

    def _rnnt_beam_frame_graph(self, S, W, blank, eos, E, total, lm=None, longest=0):
        """static buffers of S searches of width W over <= st.rows frames in all, and ONE FRAME of all of them (E rounds of
        LSTM layers, joint, output product, pick, book) captured as a HIP graph.  The warm-up runs the body with every search
        finished (no frames): every row is inactive, no state is touched.
        lm (an RNN LM that rnnt_beam_lm_why_not passes, _prepare()d by the caller): the fused frame -- every round but the last runs
        the LM's LSTM layers under the same control words on pools lh / lc beside ph / pc, gathers the top layer's h, forms the LM's
        logits and ranks the candidates with emoasr_rnnt_beam_pick_lm under the per-search weights st.mu; the last round of a frame
        grows no candidate and stays the chain without the LM.  Keyed by the LM's identity, sizes and parameter addresses.
        lm a Transformer LM that rnnt_beam_tlm_why_not passes, longest = the chunk's longest utterance: the
        same fused rounds with emoasr_lm_tree_advance + emoasr_lm_tree_step (csrc/lm_tree.hip) in place of the LSTM layers, gather and
        head product: the tree state st.tree and the node pools of st.tstep beside ph / pc under the same slot numbers, sized for
        st.tmax >= longest frames."""
        from .. import lib
        tab = self.__dict__.setdefault("_beam_batch_static", {})
        key = (S, W, blank, eos, E)
        tlm = lm is not None and getattr(lm, "lm_type", None) == "transformer"
        if tlm:
            LA, P = lm._arena, lm.params
            key += ("tlm", id(lm), P.vocab_size, P.hidden_size, P.num_attention_heads, P.intermediate_size, P.num_layers,
                    P.max_seq_len, LA.flat.data_ptr(), LA.shadow.data_ptr(), lm._pe.data_ptr())
        elif lm is not None:
            LA = lm._arena
            key += (id(lm), lm.V, lm.E, lm.H, lm.L, LA.flat.data_ptr(), LA.shadow.data_ptr(), lm._bias[0].data_ptr())
        st = tab.get(key)
        if st is not None and st.rows >= total and (not tlm or st.tmax >= longest):
            return st
        if st is not None:
            del tab[key], st       # (the pools of the outgrown record are released before the larger ones are taken)
        A, J, H, nl = self.arena, self.r_J, self.r_H, self.r_nl
        dev = A.flat.device
        V_ = A.w("decoder.output.weight").shape[0]
        st = _Stash()
        st.rows = 1024
        while st.rows < total:
            st.rows *= 2
        st.R, st.nslots = S * W, S * (E + 1) * W
        R = st.R
        st.ph = [torch.zeros(st.nslots, H, device=dev, dtype=self.dtype) for _ in range(nl)]
        st.pc = [torch.zeros(st.nslots, H, device=dev, dtype=torch.float32) for _ in range(nl)]
        st.e = torch.zeros(st.rows, J, device=dev, dtype=self.dtype)
        st.ctl = torch.zeros(5, R, device=dev, dtype=torch.int64)
        st.rec = torch.zeros(R, 1 + 2 * W, device=dev, dtype=torch.float32)
        st.hj = torch.zeros(R, J, device=dev, dtype=self.dtype)
        st.row_off = torch.zeros(S + 1, device=dev, dtype=torch.int32)
        st.ws = torch.empty(lib.size_query("emoasr_rnnt_beam_ws_bytes", S, st.rows, W, E), device=dev, dtype=torch.uint8)
        st.status = torch.zeros(1, device=dev, dtype=torch.int32)
        st.bias = [self._lstm_bias(f"decoder.rnns.{l}").contiguous() for l in range(nl)]   # (refreshed per search)
        if tlm:
            from .. import lm_tree
            st.tmax = self._tlm_frames(longest)
            # the node pools of ALL kept records stay inside the budget: the oldest records go first (a chunk of another size,
            # another width or another LM left them behind)
            st.tbytes = (2 * P.num_layers * S * lm_tree.node_cap(W, E, st.tmax) * P.hidden_size
                         * (2 if self.dtype == torch.bfloat16 else 4))
            held = [k for k, v in tab.items() if getattr(v, "tbytes", 0)]
            while held and sum(tab[k].tbytes for k in held) + st.tbytes > self._TLM_POOL_BUDGET:
                del tab[held.pop(0)]
            st.tree = lm_tree.TreeState(S, W, st.nslots, lm_tree.list_cap(E, st.tmax, lm.params.max_seq_len),
                                        lm_tree.node_cap(W, E, st.tmax), dev)
            st.tstep = lm_tree.TreeStep(lm, st.tree, c_void_p(st.ctl.data_ptr()), c_void_p(st.ctl.data_ptr() + 8 * R * 2))
            st.mu = torch.zeros(S, device=dev, dtype=torch.float32)
        elif lm is not None:
            st.lh = [torch.zeros(st.nslots, lm.H, device=dev, dtype=self.dtype) for _ in range(lm.L)]
            st.lc = [torch.zeros(st.nslots, lm.H, device=dev, dtype=torch.float32) for _ in range(lm.L)]
            st.lmh = torch.zeros(R, lm.H, device=dev, dtype=self.dtype)
            st.mu = torch.zeros(S, device=dev, dtype=torch.float32)

        def lstm_layers(dtc, emb, weights, bias, ph, pc, Hl, p_lab, p_src, p_dst, p_act):
            xtab, ldx, nx, xidx = emb, emb.shape[1], emb.shape[0], p_lab
            for l, (w_ih, w_hh) in enumerate(weights):
                lib.call("emoasr_rnnt_beam_lstm_rows", dtc, R, w_ih.shape[1], Hl, ops._p(xtab), ldx, nx, xidx, ops._p(w_ih),
                         ops._p(w_hh), ops._p(bias[l]), ops._p(ph[l]), ops._p(pc[l]), st.nslots, p_src, p_dst, p_act,
                         ops._stream())
                xtab, ldx, nx, xidx = ph[l], Hl, st.nslots, p_dst

        def body():
            with self._scope():
                dtc = ops.dt(st.ph[0])
                p_lab, p_src, p_dst, p_act, p_row = (c_void_p(st.ctl.data_ptr() + 8 * R * i) for i in range(5))
                emb = A.w("decoder.embed.weight")
                w_out, b_out = A.w("decoder.output.weight"), A.p("decoder.output.bias")
                weights = [(A.w(f"decoder.rnns.{l}.weight_ih_l0"), A.w(f"decoder.rnns.{l}.weight_hh_l0")) for l in range(nl)]
                for v in range(E):
                    fuse = lm is not None and v < E - 1
                    lstm_layers(dtc, emb, weights, st.bias, st.ph, st.pc, H, p_lab, p_src, p_dst, p_act)
                    if fuse and tlm:
                        # the lists of the destination slots, a node per live row; like the LSTM rows kernel this relies on the book
                        # kernel's mark and sweep: no live row's source slot is a destination slot of the same round
                        st.tree.advance(p_src, p_dst, p_act)
                        lm_logits = st.tstep()
                    elif fuse:
                        LA = lm._arena
                        lstm_layers(dtc, LA.w("lm.embed.weight"), [lm._w(l) for l in range(lm.L)], lm._bias, st.lh, st.lc, lm.H,
                                    p_lab, p_src, p_dst, p_act)
                    lib.call("emoasr_rnnt_beam_joint_rows", dtc, R, H, J, st.rows, ops._p(st.ph[nl - 1]), st.nslots, p_dst, p_act,
                             ops._p(A.w("decoder.w_dec.weight")), ops._p(A.p("decoder.w_dec.bias")), ops._p(st.e), p_row,
                             ops._p(st.hj), ops._stream())
                    logits = ops.gemm_nt(st.hj, w_out, bias=b_out)
                    if fuse:
                        if not tlm:
                            lib.call("emoasr_rnnt_beam_gather_rows", dtc, R, lm.H, ops._p(st.lh[lm.L - 1]), st.nslots, p_dst, p_act,
                                     ops._p(st.lmh), ops._stream())
                            lm_logits = ops.gemm_nt(st.lmh, LA.w("lm.output.weight"), bias=LA.p("lm.output.bias"))
                        lib.call("emoasr_rnnt_beam_pick_lm", dtc, R, V_, lm_logits.shape[1], W, blank, W, ops._p(logits), logits.stride(0),
                                 ops._p(lm_logits), lm_logits.stride(0), ops._p(st.mu), p_act, ops._p(st.rec), st.rec.stride(0),
                                 ops._stream())
                    else:
                        lib.call("emoasr_rnnt_beam_pick", dtc, R, V_, W, blank, ops._p(logits), logits.stride(0), ops._p(st.rec),
                                 st.rec.stride(0), ops._stream())
                    ops.rnnt_beam_book(st.row_off, W, E, V_, eos, st.rec, st.ctl, st.ws, st.status)

        ops.rnnt_beam_start(st.row_off, W, E, V_, eos, st.ctl, st.ws, st.status)   # (row_off all zero: every search finished)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()   # warm-up outside the capture (allocator, lazy initialisation)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        st.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(st.graph):
            body()
        tab[key] = st
        return st

    def _rnnt_beam_search_device(self, eouts, elens, W, blank, eos, E, lm=None, mus=None, sutt=None):
        """one chunk of rnnt_beam_search_batch: S <= _BEAM_BATCH_CAP searches, one per utterance -- or, with sutt, search s over
        utterance sutt[s] (the same utterance several times in a row: its rows of w_enc . eouts + b are replicated per search, so
        the frame offsets keep rising and the bookkeeping is what it was).  lm, mus: the fused chain with the LM weight mus[s] of
        search s (f32-rounded on the device; 0 ranks by the model alone, through the same launches)."""
        with self._scope(), torch.no_grad():
            A, nl = self.arena, self.r_nl
            sutt = list(range(len(elens))) if sutt is None else list(sutt)
            lens = [elens[b] for b in sutt]
            S, total, longest = len(lens), sum(lens), max(lens)
            V_ = A.w("decoder.output.weight").shape[0]
            tlm = lm is not None and getattr(lm, "lm_type", None) == "transformer"
            if lm is not None:
                assert len(mus) == S and (self.rnnt_beam_tlm_why_not(lm) if tlm else self.rnnt_beam_lm_why_not(lm)) is None
                lm._prepare()      # (compute-dtype weights current, bias_ih + bias_hh / the position table rebuilt in place)
            st = self._rnnt_beam_frame_graph(S, W, blank, eos, E, total, lm, longest)
            offs, rows_of = [0], {}
            for b in sutt:
                # w_enc . eouts + b per utterance, as the single-utterance forms compute it (a row's bits then do not depend on
                # the batch it came in); formed once for the consecutive searches of an utterance
                if elens[b]:
                    if b not in rows_of:
                        rows_of = {b: ops.gemm_nt(eouts[b, :elens[b]], A.w("decoder.w_enc.weight"), bias=A.p("decoder.w_enc.bias"))}
                    st.e[offs[-1]:offs[-1] + elens[b]].copy_(rows_of[b])
                offs.append(offs[-1] + elens[b])
            st.row_off.copy_(torch.tensor(offs, dtype=torch.int32))
            for l in range(nl):
                st.bias[l].copy_(self._lstm_bias(f"decoder.rnns.{l}"))
                st.ph[l].view(S, -1, self.r_H)[:, 0].zero_()    # slot 0 of every search's region: the zero state it starts from
                st.pc[l].view(S, -1, self.r_H)[:, 0].zero_()
            if lm is not None:
                st.mu.copy_(torch.tensor([float(m) for m in mus], dtype=torch.float32))
            if tlm:
                st.tree.reset()    # llen = 0 in every slot (a search's first slot is its zero state), no node taken, no bit raised
            elif lm is not None:
                for l in range(lm.L):
                    st.lh[l].view(S, -1, lm.H)[:, 0].zero_()
                    st.lc[l].view(S, -1, lm.H)[:, 0].zero_()
            st.status.zero_()
            ops.rnnt_beam_start(st.row_off, W, E, V_, eos, st.ctl, st.ws, st.status)
            for _ in range(longest):
                st.graph.replay()
            if tlm:    # a raised bit is an error naming the search and the limit, as the host form's max_seq_len assertion is
                st.tree.raise_for_status("rnnt_beam_search_batch (Transformer-LM fusion)",
                                         [f"search {s} (utterance {b}, lm_weight {float(mus[s]):g})" for s, b in enumerate(sutt)])
                stats = self.rnnt_tlm_stats = getattr(self, "rnnt_tlm_stats", None) or dict(nodes=[], node_cap=0, lcap=0)
                stats["nodes"] += st.tree.nnodes.tolist()
                stats["node_cap"], stats["lcap"] = st.tree.node_cap, st.tree.Lcap
            hyps, scores, _ = ops.rnnt_beam_finish(st.row_off, W, E, V_, eos, longest * (E - 1), st.ws, st.status)
            return hyps, scores

    def _rnnt_lm_rows(self, lm, live, rows, states, V):
        """shallow fusion, host form: the LM's log-probability row (f32 [V] on the device: log_softmax over the LM's vocabulary,
        cut to the model's) of every live hypothesis, from lm.predict -- the stateful one-step call for the RNN LM (the state
        after a label sequence is kept per label tuple; a hypothesis' parent was live one round earlier), the whole prefix for
        the Transformer LM -- cached per label tuple in rows / states -> [nb, V]"""
        todo = []
        for hyp, _, _ in live:
            key = tuple(hyp)
            if key not in rows and key not in todo:
                todo.append(key)
        if todo:
            if getattr(lm, "stateful", False):
                prev = None
                if any(len(k) > 1 for k in todo):
                    zero = lm.zero_states(1, self.arena.flat.device)
                    parts = [states[k[:-1]] if len(k) > 1 else zero for k in todo]
                    prev = (torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1))
                logp, (h, c) = lm.predict(torch.tensor([[k[-1]] for k in todo]), [1] * len(todo), prev)
                for i, k in enumerate(todo):
                    states[k] = (h[:, i:i + 1].clone(), c[:, i:i + 1].clone())
            else:
                n = max(len(k) for k in todo)
                ys = torch.zeros(len(todo), n, dtype=torch.int64)
                for i, k in enumerate(todo):
                    ys[i, :len(k)] = torch.tensor(k)
                logp, _ = lm.predict(ys, [len(k) for k in todo], None)
            assert logp.shape[1] >= V, f"the LM's vocabulary ({logp.shape[1]}) is smaller than the model's ({V})"
            for i, k in enumerate(todo):
                rows[k] = logp[i, :V].to(torch.float32).clone()
        return torch.stack([rows[tuple(hyp)] for hyp, _, _ in live])

    def _rnnt_beam_search_chain(self, eouts, beam_width, blank, eos, num_expands=3, return_scores=False, lm=None, lm_weight=0,
                                len_weight=0):
        """alignment-length synchronous beam search for ONE utterance (rnn_transducer.py:242-325,348-359).

        lm with lm_weight > 0: shallow fusion (the reference's search takes the arguments and never reads
        them).  The non-blank candidates of a live hypothesis are the beam_width best v >= 1 of f = lp + mu * lq in torch f32 (mu
        rounded to f32, product and sum rounded separately), lq the LM's row for the hypothesis' label sequence (_rnnt_lm_rows); the
        blank extension takes no LM term; at the end score + len_weight * len(hyp) and a stable re-sort (rnnt_len_expand).  A
        masked LM is refused.  Without an LM (or lm_weight <= 0) neither weight is read.

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
            fuse = lm is not None and lm_weight > 0
            if fuse:
                from ..modeling.lm import require_next_token_lm
                require_next_token_lm(lm, lm_weight)
                mu = torch.tensor(float(lm_weight), device=dev, dtype=torch.float32)
                lm_rows, lm_states = {}, {}

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
                        cand = lp
                        if fuse:   # two f32 roundings: the product, then the sum (csrc/rnnt_beam_lm.hip does the same)
                            cand = lp + mu * self._rnnt_lm_rows(lm, live, lm_rows, lm_states, lp.shape[1])
                        vals, idx, _ = ops.topk(cand[:, 1:], beam_width)
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
            hyps, scores = [hyp for hyp, _, _ in beams], [score for _, score, _ in beams]
            if fuse:
                hyps, scores = self.rnnt_len_expand(hyps, scores, len_weight)
            if return_scores:
                return hyps, scores
            return hyps
