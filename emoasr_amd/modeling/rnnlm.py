"""RNN LM (LSTM) for shallow fusion -- module API of lm/modeling/lm.py:22-66 with lm/modeling/rnn.py:13-86 behind it, on HIP kernels:
training, stateful one-step prediction for the beam searches, N-best scoring and the row log-probabilities behind the perplexity.

    lm = LM(params).cuda();  lm.load_state_dict(reference_rnnlm_state_dict)      # params.lm_type == "rnn"
    logits = lm(ys, ylens)                                                     # [B, max(ylens), V] f32
    loss, loss_dict = lm(ys_in, ylens, labels);  loss.backward()               # CrossEntropyLoss(ignore_index=-100), mean
    log_probs, (h, c) = lm.predict(ys [B,N], ylens [B], states=None)           # ONE step: reads ys[b, ylens[b]-1] only; f32 [L,B,H]
    scores = lm.score(ys, ylens)                                               # list: sum_i log p(ys[b,i+1] | ys[b,:i+1])

State-dict keys are the reference's: `lm.embed.weight`, `lm.rnns.{weight_ih,weight_hh,bias_ih,bias_hh}_l{k}`, `lm.output.{weight,bias}`
(`tie_weights` is read and ignored, as the reference does).  No packing: padded positions run through the LSTM; they come after
every real position of their row and never feed a real output.

Training is hand-sequenced (one autograd node, gradients into the parameter arena): embedding -> per layer the input projection
with bias_ih + bias_hh and the recurrence (emoasr_amd/recurrence.py: one cooperative launch per layer, or the per-position chain --
which every hidden size above the cooperative kernel's 512 takes) -> vocabulary head (logit-free where ops.ce_head_ok).  Everything
runs TIME-MAJOR.  Dropout p = dropout_rate in train() mode on the embeddings, between LSTM layers and before the output layer,
seeded per (step, site).

The searches step the LM through slot pools (`new_pools` / `step`): the state of a hypothesis lives in a slot of ph [L, slots, H]
(compute dtype) / pc [L, slots, H] (f32), a step reads the parents' slots and writes fresh ones, log-probability rows go to a row
cache.  One step is csrc/rnnlm.hip (L + 2 launches) or, outside its shape plan and with `step_kernel = False` /
EMOASR_RNNLM_STEP=0, the chain of existing entry points (`_step_chain`).
"""
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import ops
from ..engine import ParamArena, _Stash, h2d_i32
from ..recurrence import lstm_stack_bwd, lstm_stack_fwd
from .blocks import _Holder
from .lm import _LMLossFn, lm_inputs


class RNNLM(_Holder):
    """parameter container with the reference's names (lm/modeling/rnn.py:17-25)"""

    def __init__(self, params):
        super().__init__()
        self.embed = nn.Embedding(params.vocab_size, params.embedding_size)
        self.rnns = nn.LSTM(input_size=params.embedding_size, hidden_size=params.hidden_size, num_layers=params.num_layers,
                            batch_first=True)
        self.output = nn.Linear(params.hidden_size, params.vocab_size)


class RNNLanguageModel(nn.Module):
    stateful = True      # predict() is one step from the caller's (h, c): the searches thread the state

    def __init__(self, params, phase="test", compute_dtype=torch.bfloat16):
        super().__init__()
        self.lm_type = params.lm_type
        assert self.lm_type == "rnn"
        # the fields lm/modeling/rnn.py:17-34 reads; a config written for another LM family (no embedding_size, ...) is not one
        # this model can be built from
        missing = [f for f in ("vocab_size", "embedding_size", "hidden_size", "num_layers", "dropout_rate", "tie_weights")
                   if not hasattr(params, f)]
        if missing:
            raise NotImplementedError(f"emoasr_amd: lm_type='rnn' needs the RNN LM's fields; {missing} are absent from the config")
        self.params = params
        self.f32_split = isinstance(compute_dtype, str) and compute_dtype == "f32x3"
        self.compute_dtype = torch.float32 if self.f32_split else compute_dtype
        self.V, self.E, self.H, self.L = params.vocab_size, params.embedding_size, params.hidden_size, params.num_layers
        self.dropout_rate = float(params.dropout_rate)
        self.tie_weights = bool(params.tie_weights)     # read and ignored (lm/modeling/rnn.py:33-34)
        self.lm = RNNLM(params)
        self._arena = None
        self.fused_head = os.environ.get("EMOASR_CE_HEAD_FUSED", "1") != "0"
        self.last_head = None     # "fused" / "materialised": the path the last loss / score call took
        self.step_kernel = os.environ.get("EMOASR_RNNLM_STEP", "1") != "0"     # A/B switch: csrc/rnnlm.hip or the chain form
        self.last_step = None     # "kernel" / "chain": the form the last step took
        self.seed = 0x5EED
        self.step_count = 0

    def load_state_dict(self, state_dict, strict=True):
        try:
            return super().load_state_dict(state_dict, strict)
        except RuntimeError:
            return self.lm.load_state_dict(state_dict, strict)  # un-prefixed inner dict (lm.py:62-66)

    def zero_states(self, bs, device):
        """(h, c), each [L, bs, H] zeros (lm/modeling/rnn.py:55-60)"""
        return (torch.zeros(self.L, bs, self.H, device=device), torch.zeros(self.L, bs, self.H, device=device))

    # ---------------------------------------------------------------- parameters
    def _seed(self, site):
        return (self.seed * 1000003 + self.step_count * 4099 + site) & 0xFFFFFFFFFFFF

    def _split(self):
        return self.f32_split if self.compute_dtype == torch.float32 else None

    def _prepare(self):
        """arena bound, compute-dtype weights current, bias_ih + bias_hh per layer rebuilt IN PLACE (the parameters move between
        training steps; the step kernel's pointer tables keep reading the same addresses)"""
        if self._arena is None or not self._arena.bound() or self._arena.compute_dtype != self.compute_dtype:
            self._arena = ParamArena(self, self.compute_dtype)
            dev = self._arena.flat.device
            self._bias = [torch.empty(4 * self.H, device=dev, dtype=torch.float32) for _ in range(self.L)]
            self._stepw = None
        A = self._arena
        A.refresh_shadow()
        for l in range(self.L):
            torch.add(A.p(f"lm.rnns.bias_ih_l{l}"), A.p(f"lm.rnns.bias_hh_l{l}"), out=self._bias[l])     # tiny f32 add (glue)
        return A

    def _w(self, l):
        A = self._arena
        return A.w(f"lm.rnns.weight_ih_l{l}"), A.w(f"lm.rnns.weight_hh_l{l}")

    # ---------------------------------------------------------------- sequence forward / backward, time-major
    def _encode(self, ids_tm, p, keep):
        """ids_tm int32 [N,B] on the device -> (dropout(top layer's h) [N*B, H], stash | None)"""
        A = self._arena
        N, B = ids_tm.shape
        s_emb = self._seed(1)
        x = ops.embed_fwd(ids_tm, A.w("lm.embed.weight"), None, 1.0, p, s_emb)     # [N,B,E], dropout fused
        # dropout after layer l: between layers (nn.LSTM(dropout=)), and before `output` after the last
        spec = [(*self._w(l), self._bias[l], self._seed(10 + l), None, None) for l in range(self.L)]
        x, _, layers = lstm_stack_fwd(x, spec, p, keep)
        st = None
        if keep:
            st = _Stash()
            st.ids, st.layers, st.s_emb, st.p = ids_tm, layers, s_emb, p
        return x.view(N * B, self.H), st

    def _head_rows(self, x, labels, w):
        """output layer + soft-max, reduced per row: labels int32 [M] (clamped), w f32 [M] -> (rows f32 [M] = -w[m] log p(labels[m] | row m),
        head stash)"""
        A = self._arena
        rows, head = ops.lm_head_fwd(self.fused_head, x, A.w("lm.output.weight"), A.p("lm.output.bias"), labels, w)
        self.last_head = head[0]
        return rows, head

    def forward(self, ys, ylens=None, labels=None, ps=None, plens=None):
        """lm/modeling/rnn.py:36-53: logits [B, N, V] (f32) without labels, else (loss, {"loss_total": loss})"""
        ys, yl = lm_inputs(ys, ylens, self.V)
        A = self._prepare()
        if labels is None:
            B, N = ys.shape
            if self.training:      # (the reference's logits in train() mode carry its dropout too)
                self.step_count += 1
            p = self.dropout_rate if self.training else 0.0
            with torch.no_grad(), ops.stream_scope(self._split()):
                x, _ = self._encode(h2d_i32(ys.t().contiguous(), A.flat.device), p, False)
                logits = ops.gemm_nt(x, A.w("lm.output.weight"), bias=A.p("lm.output.bias"), out_f32=x.dtype != torch.float32)
            return logits.view(N, B, -1).transpose(0, 1).contiguous()
        labels = (labels.cpu() if torch.is_tensor(labels) else torch.as_tensor(labels)).to(torch.int64)
        if ylens is not None:
            labels = labels[:, : max(yl)]
        loss = _LMLossFn.apply(self, ys, yl, labels.contiguous(), *A.params)
        return loss, {"loss_total": loss}

    def _loss_forward(self, ys, yl, labels, keep):
        A = self._arena
        dev = A.flat.device
        training = self.training
        if training:
            self.step_count += 1
        p = self.dropout_rate if training else 0.0
        valid = labels != -100
        assert labels.shape == ys.shape and int(labels.max()) < self.V, "labels: [B, N] ids below vocab_size or -100"
        w = valid.to(torch.float32) / max(int(valid.sum()), 1)     # mean over the rows with a label (CrossEntropyLoss, ignore_index=-100)
        with ops.stream_scope(self._split()):
            ids = h2d_i32(ys.t().contiguous(), dev)
            lab = h2d_i32(labels.clamp(min=0).t().contiguous().view(-1), dev)
            w_dev = w.t().contiguous().view(-1).pin_memory().to(dev, non_blocking=True)
            x, st = self._encode(ids, p, keep)
            rows, head = self._head_rows(x, lab, w_dev)
            loss = rows.sum()
        if keep:
            st.x, st.head, st.lab, st.w = x, head, lab, w_dev
        return loss, st

    def _loss_backward(self, st, g):
        """g: the incoming gradient of the loss (0-dim, on the device).  Accumulates every parameter gradient into the arena."""
        with ops.stream_scope(self._split()):
            A = self._arena
            A.attach_grads()
            g1 = g.to(torch.float32).reshape(1)
            N, B = st.ids.shape
            wname, bname = "lm.output.weight", "lm.output.bias"
            dy = ops.lm_head_bwd(st.head, st.x, A.w(wname), A.p(bname), st.lab, st.w, A.g(wname), A.g(bname), g1)
            # one set of column sums for both biases: they enter the gates as a sum, their gradients are the same numbers
            db = [torch.zeros(4 * self.H, device=dy.device, dtype=torch.float32) for _ in range(self.L)]
            grads = [(A.g(f"lm.rnns.weight_ih_l{l}"), A.g(f"lm.rnns.weight_hh_l{l}"), db[l], None) for l in range(self.L)]
            dy = lstm_stack_bwd(dy.view(N, B, self.H), st.layers, grads, st.p)
            for l in range(self.L):
                A.g(f"lm.rnns.bias_ih_l{l}").add_(db[l])
                A.g(f"lm.rnns.bias_hh_l{l}").add_(db[l])
            ops.embed_bwd(st.ids, dy, 1.0, A.g("lm.embed.weight"), st.p, st.s_emb)

    # ---------------------------------------------------------------- scoring
    def token_logprobs(self, ys, ylens, labels):
        """log p(labels[b,i] | ys[b,:i+1]) for every position with labels != -100 (zeros elsewhere) -> float64 [B, N] on the HOST
        (the Transformer LM's definition; one device-to-host copy of the row values)"""
        ys, yl = lm_inputs(ys, ylens, self.V)
        labels = (labels.cpu() if torch.is_tensor(labels) else torch.as_tensor(labels)).to(torch.int64)[:, : ys.shape[1]]
        A = self._prepare()
        dev = A.flat.device
        B, N = ys.shape
        valid = labels != -100
        with torch.no_grad(), ops.stream_scope(self._split()):
            ids = h2d_i32(ys.t().contiguous(), dev)
            lab = h2d_i32(labels.clamp(min=0).t().contiguous().view(-1), dev)
            w_dev = valid.to(torch.float32).t().contiguous().view(-1).pin_memory().to(dev, non_blocking=True)
            x, _ = self._encode(ids, 0.0, False)
            rows, _ = self._head_rows(x, lab, w_dev)
        return -rows.cpu().to(torch.float64).view(N, B).t() * valid.to(torch.float64)

    def score(self, ys, ylens, batch_size=100):
        """per row sum_{i < ylens[b]-1} log p(ys[b,i+1] | ys[b,:i+1]) -> Python list of floats, summed on the host in double precision
        (lm/modeling/transformer.py:79-99's definition).  An EXTENSION beyond the reference, whose RNNLM.score is `pass` and returns
        None (lm/modeling/rnn.py:83-86)."""
        ys = (ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys)).to(torch.int64)
        yl = [int(v) for v in (ylens.tolist() if torch.is_tensor(ylens) else ylens)]
        out = []
        batch_size = batch_size or len(yl)
        for b0 in range(0, len(yl), batch_size):
            y, l = ys[b0:b0 + batch_size, : max(yl[b0:b0 + batch_size])], yl[b0:b0 + batch_size]
            labels = torch.full_like(y, -100)
            for b, n in enumerate(l):
                labels[b, : n - 1] = y[b, 1:n]
            out += self.token_logprobs(y, l, labels).sum(dim=1).tolist()
        return out

    # ---------------------------------------------------------------- the stateful step
    def new_pools(self, slots, rows=None):
        """state pools for `slots` hypotheses and a row cache of `rows` log-probability rows (default: one per slot)"""
        A = self._prepare()
        dev = A.flat.device
        return SimpleNamespace(ph=torch.zeros(self.L, slots, self.H, device=dev, dtype=self.compute_dtype),
                               pc=torch.zeros(self.L, slots, self.H, device=dev, dtype=torch.float32),
                               logp=torch.zeros(slots if rows is None else rows, self.V, device=dev, dtype=torch.float32))

    def step(self, pools, nb, ids, src, dst, row_dst=None):
        """one LM step for nb rows: row i consumes token ids[i] from the state in slot src[i] (< 0: the zero state), its new state goes
        to slot dst[i], its log-probability row to pools.logp[row_dst[i]] (None: row i).  All lists int32 on the device; several rows
        may share a src, no dst may equal a src of the same call.  Call _prepare() (new_pools does) after the parameters moved."""
        with torch.no_grad(), ops.stream_scope(self._split()):
            if self.step_kernel and ops.rnnlm_step_supported(pools.ph, min(nb, ops.RNNLM_STEP_MAX), self.L, self.E, self.H):
                if self._stepw is None:
                    A = self._arena
                    ws = [self._w(l) for l in range(self.L)]
                    self._stepw = ops.RnnlmStepWeights(A.w("lm.embed.weight"), [w[0] for w in ws], [w[1] for w in ws], self._bias,
                                                       A.w("lm.output.weight"), A.p("lm.output.bias"))
                if nb > ops.RNNLM_STEP_MAX and row_dst is None:
                    row_dst = torch.arange(nb, device=pools.ph.device, dtype=torch.int32)
                for i0 in range(0, nb, ops.RNNLM_STEP_MAX):     # (chunks are independent: no dst is any row's src)
                    ops.rnnlm_step(self._stepw, min(ops.RNNLM_STEP_MAX, nb - i0), ids[i0:], pools.ph, pools.pc, src[i0:], dst[i0:],
                                   pools.logp, None if row_dst is None else row_dst[i0:])
                self.last_step = "kernel"
            else:
                self._step_chain(pools, nb, ids, src, dst, row_dst)
                self.last_step = "chain"

    def _step_chain(self, pools, nb, ids, src, dst, row_dst):
        """the same step from entry points that predate csrc/rnnlm.hip: embedding, two products and the cell kernel per layer, the
        head's product, log-softmax; slots gathered / scattered by index (2 L + 4 kernels + 4 L + 1 index ops)"""
        A = self._arena
        x = ops.embed_fwd(ids[:nb].view(1, nb), A.w("lm.embed.weight"), None, 1.0).view(nb, self.E)
        s, d = src[:nb].long(), dst[:nb].long()
        live = (s >= 0).view(nb, 1)
        s = s.clamp(min=0)
        for l in range(self.L):
            w_ih, w_hh = self._w(l)
            h_prev = pools.ph[l].index_select(0, s) * live.to(x.dtype)
            c_prev = pools.pc[l].index_select(0, s) * live.to(torch.float32)
            pre = ops.gemm_nt(x, w_ih, bias=self._bias[l])
            gates = ops.gemm_nt(h_prev, w_hh, residual=pre, res_scale=1.0)
            h = torch.empty(nb, self.H, device=x.device, dtype=x.dtype)
            c = torch.empty(nb, self.H, device=x.device, dtype=torch.float32)
            ops.lstm_cell_fwd(gates, c_prev, h, c, torch.empty_like(gates))
            pools.ph[l].index_copy_(0, d, h)
            pools.pc[l].index_copy_(0, d, c)
            x = h
        logits = ops.gemm_nt(x, A.w("lm.output.weight"), bias=A.p("lm.output.bias"), out_f32=x.dtype != torch.float32)
        lp = ops.log_softmax(logits)
        if row_dst is None:
            pools.logp[:nb] = lp
        else:
            pools.logp.index_copy_(0, row_dst[:nb].long(), lp)

    def predict(self, ys, ylens, states=None):
        """lm/modeling/rnn.py:62-81: ONE step.  Reads only ys[b, ylens[b] - 1]; states = (h, c), each [L, B, H] (None: zeros)
        -> (log_probs [B, V] f32, (h', c') each f32 [L, B, H], h' holding compute-dtype values); the prefix is never re-run.  The state tensors can be
        sliced with [:, b:b+1] and joined with torch.cat(dim=1), as the reference's search code does."""
        ys_host = (ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys)).to(torch.int64)
        yl = [int(v) for v in (ylens.tolist() if torch.is_tensor(ylens) else ylens)]
        B = ys_host.shape[0]
        last = [int(ys_host[b, yl[b] - 1]) for b in range(B)]
        assert all(0 <= v < self.V for v in last), "token id outside the vocabulary"
        with torch.no_grad():
            pools = self.new_pools(2 * B, B)     # slots 0 .. B-1: the incoming states, B .. 2B-1: the new ones
            dev = pools.ph.device
            if states is not None:
                assert tuple(states[0].shape) == (self.L, B, self.H) and tuple(states[1].shape) == (self.L, B, self.H)
                pools.ph[:, :B] = states[0].to(device=dev, dtype=self.compute_dtype)
                pools.pc[:, :B] = states[1].to(device=dev, dtype=torch.float32)
            ctl = h2d_i32(last + (list(range(B)) if states is not None else [-1] * B) + list(range(B, 2 * B)), dev)
            self.step(pools, B, ctl[:B], ctl[B:2 * B], ctl[2 * B:])
            return pools.logp, (pools.ph[:, B:].float(), pools.pc[:, B:])
