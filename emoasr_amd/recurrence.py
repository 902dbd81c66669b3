"""Unidirectional LSTM layers over a whole sequence, TIME-MAJOR, forward and backward: one layer (lstm_layer_fwd / lstm_layer_bwd) and
the teacher-forced stack of them with dropout after every layer (lstm_stack_fwd / lstm_stack_bwd) -- shared by the transducer's
prediction network (engine/rnnt.py), the RNN LM (modeling/rnnlm.py) and the LAS decoder's layers 1 and up (engine/las.py).  The
embedding in front of the stack, and its gradient, stay with the callers.

The input projection is one product over all positions; the recurrence is one cooperative launch (csrc/lstm_coop.hip) where
ops.lstm_seq_supported says so (bf16, H % 32 == 0, H <= 512, option "lstm_coop"), else the per-position chain: recurrent product
with the stored pre-activation as its residual, then the cell kernel.  Hidden sizes above the cooperative kernel's 512 therefore
run the chain (2 launches per position)."""
from typing import NamedTuple

import torch

from . import ops

# one layer of lstm_stack_fwd for lstm_stack_bwd: input, lstm_layer_fwd's outputs, the output dropout's seed, initial state | None, weights
LSTMRecord = NamedTuple("LSTMRecord", [(f, object) for f in "x hseq cseq gact s_do h0 c0 w_ih w_hh".split()])


def lstm_layer_fwd(x, w_ih, w_hh, bias, h0, c0):
    """x [U,B,nin] (compute dtype), w_ih [4H,nin], w_hh [4H,H], bias f32 [4H] = bias_ih + bias_hh, h0 [B,H] | None, c0 f32 [B,H] | None
    -> (hseq [U,B,H], cseq f32 [U,B,H], gact [U,B,4H] activated i | f | g | o)"""
    U, B, nin = x.shape
    H = w_hh.shape[1]
    dev = x.device
    pre = ops.gemm_nt(x.view(U * B, nin), w_ih, bias=bias).view(U, B, 4 * H)
    hseq = torch.empty(U, B, H, device=dev, dtype=x.dtype)
    cseq = torch.empty(U, B, H, device=dev, dtype=torch.float32)
    gact = torch.empty(U, B, 4 * H, device=dev, dtype=x.dtype)
    if U > 1 and ops.lstm_seq_supported(x, B, H):
        # the whole recurrence in one cooperative launch (csrc/lstm_coop.hip) instead of 2 launches per position
        ops.lstm_seq_fwd(pre, w_hh, h0, c0, hseq, cseq, gact)
    else:
        h_prev, c_prev = h0, c0
        for u in range(U):
            gates = pre[u] if h_prev is None else ops.gemm_nt(h_prev, w_hh, residual=pre[u], res_scale=1.0)
            ops.lstm_cell_fwd(gates, c_prev, hseq[u], cseq[u], gact[u])
            h_prev, c_prev = hseq[u], cseq[u]
    return hseq, cseq, gact


def lstm_layer_bwd(dh_seq, x_in, hseq, cseq, gact, h0, c0, w_ih, w_hh, g_w_ih, g_w_hh, g_b_ih, g_b_hh):
    """dh_seq [U,B,H]: gradient w.r.t. the layer's outputs.  ACCUMULATES the four parameter gradients (f32; both biases receive the
    same column sums; g_b_hh None: the caller copies g_b_ih's) -> dx [U,B,nin]"""
    U, B, H = dh_seq.shape
    dgp = torch.empty(U, B, 4 * H, device=dh_seq.device, dtype=dh_seq.dtype)
    if U > 1 and ops.lstm_seq_supported(dh_seq, B, H):
        # the whole backward recurrence in one cooperative launch (csrc/lstm_coop.hip)
        ops.lstm_seq_bwd(dh_seq.contiguous(), gact, cseq, c0, w_hh, dgp)
    else:
        dc = torch.zeros(B, H, device=dh_seq.device, dtype=torch.float32)
        dh_rec = None
        for u in reversed(range(U)):
            ops.lstm_cell_bwd(dh_seq[u], dh_rec, dc, gact[u], cseq[u - 1] if u > 0 else c0, cseq[u], dgp[u])
            if u > 0:
                dh_rec = ops.gemm_nn(dgp[u], w_hh)
    nin = x_in.shape[-1]
    dgp2 = dgp.view(U * B, 4 * H)
    ops.gemm_tn(dgp2, x_in.reshape(U * B, nin), out=g_w_ih, accumulate=True, colsum=g_b_ih)
    if g_b_hh is not None:
        ops.colsum(dgp2, out=g_b_hh, accumulate=True)
    if U > 1:
        ops.gemm_tn(dgp[1:].reshape((U - 1) * B, 4 * H), hseq[:-1].reshape((U - 1) * B, H), out=g_w_hh, accumulate=True)
    if h0 is not None:
        # position 0's gates contain h0 . W_hh^T
        ops.gemm_tn(dgp[0], h0, out=g_w_hh, accumulate=True)
    return ops.gemm_nn(dgp2, w_ih).view(U, B, nin)


def lstm_stack_fwd(x, layers, p, keep):
    """x [U,B,nin]; layers: per layer (w_ih, w_hh, bias, seed, h0 | None, c0 | None), taken one at a time as the stack reaches the
    layer (a caller whose bias sum is a launch of its own hands in a generator); p: dropout rate on every layer's output
    -> (dropped output of the top layer [U,B,H], ([h_final per layer], [c_final per layer]), [LSTMRecord per layer] if keep else None)"""
    hs, cs, records = [], [], []
    for w_ih, w_hh, bias, seed, h0, c0 in layers:
        hseq, cseq, gact = lstm_layer_fwd(x, w_ih, w_hh, bias, h0, c0)
        hs.append(hseq[-1])
        cs.append(cseq[-1])
        if keep:
            records.append(LSTMRecord(x, hseq, cseq, gact, seed, h0, c0, w_ih, w_hh))
        x = ops.scale_dropout(hseq, 1.0, p, seed) if p > 0 else hseq
    return x, (hs, cs), (records if keep else None)


def lstm_stack_bwd(dy, records, grads, p):
    """dy [U,B,H]: gradient w.r.t. lstm_stack_fwd's output; grads: per layer (g_w_ih, g_w_hh, g_b_ih, g_b_hh | None), accumulated
    into (lstm_layer_bwd) -> gradient w.r.t. the stack's input [U,B,nin]"""
    for r, g in zip(reversed(records), reversed(grads)):
        dh_seq = ops.scale_dropout(dy, 1.0, p, r.s_do) if p > 0 else dy
        dy = lstm_layer_bwd(dh_seq, r.x, r.hseq, r.cseq, r.gact, r.h0, r.c0, r.w_ih, r.w_hh, *g)
    return dy
