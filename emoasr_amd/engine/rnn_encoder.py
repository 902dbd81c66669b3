"""RNN encoder: Conv2d front-end (or none) -> bidirectional LSTM layers over packed sequences.
  reference: asr/modeling/encoders/rnn.py:14-81"""
import torch

from .. import ops
from .arena import _Stash, _cfg, h2d_i32


class RNNEncoder:
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
        s_do = self._seed(8000 + l)   # (sites 8000 + l overlap the LAS decoder's 8000 / 8001 / 8002: las.py, _las_forward)
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
