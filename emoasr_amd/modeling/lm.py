"""Transformer LM for shallow fusion -- module API of lm/modeling/lm.py:22-66 and
lm/modeling/transformer.py:19-77 (a causal BERT, vendored HF v3.0.0 modeling_bert.py:159-554),
on HIP kernels: shallow-fusion inference, training, N-best scoring and the row log-probabilities behind the perplexity.

    lm = LM(params).cuda();  lm.load_state_dict(reference_lm_state_dict)
    log_probs, states = lm.predict(ys [B,N] int64, ylens [B], states=None)     # [B, V], None
    logits = lm(ys, ylens)                                                     # [B, max(ylens), V] f32
    loss, loss_dict = lm(ys_in, ylens, labels);  loss.backward()               # CrossEntropyLoss(ignore_index=-100), mean
    scores = lm.score(ys, ylens)                                               # list: sum_i log p(ys[b,i+1] | ys[b,:i+1])

Training (forward / backward sequencing below, no autograd graph inside): post-LN BERT blocks with a causal + padding key mask,
hidden dropout 0.1 after the embedding LayerNorm / attention.output.dense / output.dense and attention-probability dropout 0.1
(the reference builds its config without dropout arguments, so train() mode always has both: `hidden_dropout_prob`,
`attention_probs_dropout_prob` here, eval() turns them off).  Gradients land in the parameter arena; `bert.pooler.*` is never
read and its .grad stays None.  In bf16 with V % 8 == 0, d % 64 == 0 and at least ops.CE_HEAD_MIN_ROWS rows the vocabulary head
of the loss / score path never writes [rows, V] logits (ops.ce_head_fwd / ce_head_bwd); otherwise (and in f32 / f32x3, and
in forward() without labels, which returns them) the logits are materialised.  token_logprobs / score always run without dropout.

State-dict keys match the reference (`lm.transformer.bert.*`, `lm.transformer.cls.predictions.*`,
output embedding tied to the word embedding).  `LM(params)` with `lm_type == "rnn"` returns the LSTM LM of modeling/rnnlm.py
(same module API, `stateful = True`); every type but these, "bert", "electra" and "electra-disc" is outside the path.

`lm_type == "bert"` is the masked LM of lm/modeling/bert.py:17-92 -- the same stack without the causal mask, keys `lm.bert.bert.*` /
`lm.bert.cls.predictions.*`, `mask_id = params.mask_id` -- on the same code, parametrised by the key prefix and `causal`:

    loss, loss_dict = lm(ys_masked, ylens, labels);  loss.backward()           # labels -100 except at the masked positions
    lp = lm.masked_logprobs(ys, ylens)                                         # f64 [B, N] on the host: log p(ys[b,i] | the rest of ys[b])
    scores = lm.score(ys, ylens)                                               # pseudo-log-likelihood: the row sums

Its transform + vocabulary head run on the gathered labelled rows only (`head_at_labels`), its attention backward takes the
single-pass kernel in bf16, `masked_logprobs` builds the masked copies on the device (ops.mlm_expand) and walks them in chunks of
token rows, and `predict` / `zero_states` raise: a bidirectional LM has no next-token distribution.

`lm_type in ("electra", "electra-disc")` is ELECTRA (lm/modeling/electra.py:33-132): a generator (`lm.gmodel.*`, ElectraForMaskedLM)
and a discriminator (`lm.dmodel.*`, ElectraForPreTraining), two stacks of the same blocks described by a `_Stack` each (key prefix,
embedding / hidden / inner size, heads, layers, `embeddings_project` present), in one parameter arena:

    loss, loss_dict = lm(ys_masked, ylens, labels);  loss.backward()           # loss_gen + electra_disc_weight * loss_disc
    loss, loss_dict = lm.forward_disc(ys, ylens, error_labels)                 # the discriminator alone, BCE over n < ylens[b]
    scores = lm.score(ys, ylens)                                               # one encoder pass: sums of sigmoid(logit), see score()

The generator's replacement tokens are drawn on the device (ops.sample_rows: Gumbel-max, a function of `lm.seed`, `lm.step_count`,
row and column), put in place by ops.electra_corrupt, and the discriminator's binary head runs on the rows n < ylens[b]
(ops.bce_head_fwd / _bwd); `lm.forced_samples`, `lm.last_corruption` and `lm.sample_path` are the hooks.
"""
import math
from types import SimpleNamespace
import os

import torch
import torch.nn as nn

from .. import lockstep, ops
from ..engine import ParamArena, _Stash, h2d_i32
from ..ops import ACT_GELU
from .blocks import _Holder


class _Self(_Holder):
    def __init__(self, d):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)


class _DenseLN(_Holder):
    def __init__(self, din, dout):
        super().__init__()
        self.dense = nn.Linear(din, dout)
        self.LayerNorm = nn.LayerNorm(dout, eps=1e-12)


class _Dense(_Holder):
    def __init__(self, din, dout):
        super().__init__()
        self.dense = nn.Linear(din, dout)


class _Attention(_Holder):
    def __init__(self, d):
        super().__init__()
        self.self = _Self(d)
        self.output = _DenseLN(d, d)


class _Layer(_Holder):
    def __init__(self, d, inner):
        super().__init__()
        self.attention = _Attention(d)
        self.intermediate = _Dense(d, inner)
        self.output = _DenseLN(inner, d)


class _Embeddings(_Holder):
    def __init__(self, vocab, d, max_len):
        super().__init__()
        self.word_embeddings = nn.Embedding(vocab, d, padding_idx=0)
        self.position_embeddings = nn.Embedding(max_len, d)
        self.token_type_embeddings = nn.Embedding(2, d)
        self.LayerNorm = nn.LayerNorm(d, eps=1e-12)


class _Encoder(_Holder):
    def __init__(self, d, inner, n):
        super().__init__()
        self.layer = nn.ModuleList(_Layer(d, inner) for _ in range(n))


class _Bert(_Holder):
    def __init__(self, vocab, d, inner, n, max_len):
        super().__init__()
        self.embeddings = _Embeddings(vocab, d, max_len)
        self.encoder = _Encoder(d, inner, n)
        self.pooler = _Dense(d, d)  # present in reference checkpoints, unused by predict()


class _Predictions(_Holder):
    def __init__(self, vocab, d):
        super().__init__()
        self.transform = _DenseLN(d, d)
        self.decoder = nn.Linear(d, vocab, bias=False)
        self.bias = nn.Parameter(torch.zeros(vocab))
        self.decoder.bias = self.bias


class _Cls(_Holder):
    def __init__(self, vocab, d):
        super().__init__()
        self.predictions = _Predictions(vocab, d)


class _BertForMaskedLM(_Holder):
    def __init__(self, vocab, d, inner, n, max_len):
        super().__init__()
        self.bert = _Bert(vocab, d, inner, n, max_len)
        self.cls = _Cls(vocab, d)
        self.cls.predictions.decoder.weight = self.bert.embeddings.word_embeddings.weight  # tied


class TransformerLM(nn.Module):
    def __init__(self, params):
        super().__init__()
        self.transformer = _BertForMaskedLM(params.vocab_size, params.hidden_size, params.intermediate_size,
                                            params.num_layers, params.max_seq_len)

    def zero_states(self, bs, device):
        return None  # stateless


class BERTMaskedLM(nn.Module):
    """parameter container of the masked LM (lm/modeling/bert.py:17-33): the same stack without the causal mask"""

    def __init__(self, params):
        super().__init__()
        self.bert = _BertForMaskedLM(params.vocab_size, params.hidden_size, params.intermediate_size,
                                     params.num_layers, params.max_seq_len)
        self.mask_id = params.mask_id

    def load_state_dict(self, state_dict, strict=True):
        try:
            return super().load_state_dict(state_dict, strict)
        except RuntimeError:
            return self.bert.load_state_dict(state_dict, strict)  # the bare BertForMaskedLM dict (bert.py:88-92)


class _ElectraEmbeddings(_Holder):
    """modeling_electra.py:114-125: word, position, token-type tables and their LayerNorm at embedding_size"""

    def __init__(self, vocab, e, max_len):
        super().__init__()
        self.word_embeddings = nn.Embedding(vocab, e, padding_idx=0)
        self.position_embeddings = nn.Embedding(max_len, e)
        self.token_type_embeddings = nn.Embedding(2, e)
        self.LayerNorm = nn.LayerNorm(e, eps=1e-12)


class _ElectraModel(_Holder):
    """modeling_electra.py:240-253: no pooler; embeddings_project exists only when embedding_size != hidden_size"""

    def __init__(self, vocab, e, d, inner, n, max_len):
        super().__init__()
        self.embeddings = _ElectraEmbeddings(vocab, e, max_len)
        if e != d:
            self.embeddings_project = nn.Linear(e, d)
        self.encoder = _Encoder(d, inner, n)


class _GeneratorPredictions(_Holder):
    """modeling_electra.py:146-160: dense(hidden -> embedding), GELU, LayerNorm(embedding) built WITHOUT the config's eps (1e-5)"""

    def __init__(self, e, d):
        super().__init__()
        self.LayerNorm = nn.LayerNorm(e)
        self.dense = nn.Linear(d, e)


class _DiscriminatorPredictions(_Holder):
    def __init__(self, d):
        super().__init__()
        self.dense = nn.Linear(d, d)
        self.dense_prediction = nn.Linear(d, 1)


class _ElectraForMaskedLM(_Holder):
    def __init__(self, vocab, e, d, inner, n, max_len):
        super().__init__()
        self.electra = _ElectraModel(vocab, e, d, inner, n, max_len)
        self.generator_predictions = _GeneratorPredictions(e, d)
        self.generator_lm_head = nn.Linear(e, vocab)
        self.generator_lm_head.weight = self.electra.embeddings.word_embeddings.weight  # tied (init_weights -> tie_weights)


class _ElectraForPreTraining(_Holder):
    def __init__(self, vocab, e, d, inner, n, max_len):
        super().__init__()
        self.electra = _ElectraModel(vocab, e, d, inner, n, max_len)
        self.discriminator_predictions = _DiscriminatorPredictions(d)


_ELECTRA_FIELDS = ("mask_id", "electra_disc_weight") + tuple(
    f"{s}_{f}" for s in ("gen", "disc") for f in ("embedding_size", "hidden_size", "num_layers", "num_attention_heads", "intermediate_size"))


class ELECTRAModel(nn.Module):
    """parameter container of lm/modeling/electra.py:33-69: generator (ElectraForMaskedLM) and discriminator (ElectraForPreTraining)"""

    def __init__(self, params):
        super().__init__()
        P = params
        self.gmodel = _ElectraForMaskedLM(P.vocab_size, P.gen_embedding_size, P.gen_hidden_size, P.gen_intermediate_size,
                                          P.gen_num_layers, P.max_seq_len)
        self.dmodel = _ElectraForPreTraining(P.vocab_size, P.disc_embedding_size, P.disc_hidden_size, P.disc_intermediate_size,
                                             P.disc_num_layers, P.max_seq_len)
        self.electra_disc_weight = P.electra_disc_weight
        self.mask_id = P.mask_id

    def load_state_dict(self, state_dict, strict=True):
        try:
            return super().load_state_dict(state_dict, strict)
        except RuntimeError:
            return self.dmodel.load_state_dict(state_dict, strict)  # a bare ElectraForPreTraining dict: the discriminator alone


def lm_inputs(ys, ylens, vocab_size):
    """token rows and their lengths as every LM takes them -> (ys int64 [B, max(ylens)] on the host, [length per row])"""
    ys = (ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys)).to(torch.int64)
    if ylens is None:
        yl = [ys.shape[1]] * ys.shape[0]      # (no mask: every position is a key)
    else:
        yl = [int(v) for v in (ylens.tolist() if torch.is_tensor(ylens) else ylens)]
        ys = ys[:, : max(yl)]      # (lm/modeling/rnn.py:37-39)
    assert len(yl) == ys.shape[0] and min(yl) >= 1, "ylens: one length >= 1 per row"
    assert 0 <= int(ys.min()) and int(ys.max()) < vocab_size, "token id outside the vocabulary"
    return ys.contiguous(), yl


class _Stack:
    """what _encode / _backward_stack need to know of one post-LN BERT stack: the key prefix of its model (`...bert.` /
    `...electra.`), embedding / hidden / inner sizes, heads, layers, the causal mask, whether embeddings_project sits between the
    embedding LayerNorm (+ dropout) and the blocks, the offset of its dropout seed sites and its position + token-type(0) table"""

    def __init__(self, pre, emb, d, inner, heads, layers, causal, project=False, site=0):
        assert d % heads == 0 and d // heads == 64, (
            f"emoasr_amd: {pre!r} has hidden size {d} over {heads} heads = {d / heads:g} per head; the attention kernels need heads 64 wide")
        assert project == (emb != d), "embeddings_project exists exactly when embedding_size != hidden_size"
        self.pre, self.emb, self.d, self.inner, self.heads, self.layers = pre, emb, d, inner, heads, layers
        self.causal, self.project, self.site = causal, project, site
        self.pe = None


_ELECTRA_TYPES = ("electra", "electra-disc")
_NO_PREDICT = ("emoasr_amd: the BERT masked LM (lm_type='bert') has no next-token distribution: predict / zero_states and the "
               "beam searches' shallow fusion need a causal LM (lm_type 'transformer' or 'rnn'); use LM.score for rescoring")


_NO_PREDICT_ELECTRA = ("emoasr_amd: ELECTRA (lm_type 'electra' / 'electra-disc') has no next-token distribution: predict / zero_states "
                       "and the beam searches' shallow fusion need a causal LM (lm_type 'transformer' or 'rnn'); use LM.score for "
                       "rescoring")


_P2W_TYPES = ("pbert", "pctc", "ptransformer")
_NO_PREDICT_P2W = ("emoasr_amd: the phone-to-word models (modeling/p2w.py: lm_type 'pbert' / 'pctc') have no next-token "
                   "distribution: predict / zero_states and the beam searches' shallow fusion need a causal LM (lm_type "
                   "'transformer' or 'rnn'); they correct a CTC hypothesis through emoasr_amd.correct")


_PELECTRA_TYPES = ("pelectra", "pelectra-disc")
_NO_PREDICT_PELECTRA = ("emoasr_amd: P-ELECTRA (modeling/pelectra.py: lm_type 'pelectra' / 'pelectra-disc') has no next-token "
                        "distribution: predict / zero_states and the beam searches' shallow fusion need a causal LM (lm_type "
                        "'transformer' or 'rnn'); use PELECTRA.score for rescoring")


def require_next_token_lm(lm, lm_weight):
    """entry check of the beam searches: shallow fusion needs p(next token | prefix), which a bidirectional LM does not define"""
    if lm is not None and lm_weight > 0 and getattr(lm, "lm_type", None) == "bert":
        raise NotImplementedError(_NO_PREDICT)
    if lm is not None and lm_weight > 0 and getattr(lm, "lm_type", None) in _ELECTRA_TYPES:
        raise NotImplementedError(_NO_PREDICT_ELECTRA)
    if lm is not None and lm_weight > 0 and getattr(lm, "lm_type", None) in _P2W_TYPES:
        raise NotImplementedError(_NO_PREDICT_P2W)
    if lm is not None and lm_weight > 0 and getattr(lm, "lm_type", None) in _PELECTRA_TYPES:
        raise NotImplementedError(_NO_PREDICT_PELECTRA)


class _StackOps:
    """What LM and PELECTRA (modeling/pelectra.py) share: the post-LN BERT stacks (_encode / _backward_stack over a `_Stack` each) and
    ELECTRA's discriminator on top of one (_disc_forward / _disc_backward, replaced_probs, _electra_score).  The host class provides
    `_arena` (a bound ParamArena), `_stack` / `_stacks`, `seed`, `step_count`, `attn_fused`, `params`, `compute_dtype` / `f32_split`
    and, for the discriminator, `_D` (its key prefix), `_disc`, `electra`, `lm_type` and `_prepare()`."""

    def _seed(self, site, S=None):
        site += S.site if S is not None else 0
        return (self.seed * 1000003 + self.step_count * 4099 + site) & 0xFFFFFFFFFFFF

    def _split(self):
        return self.f32_split if self.compute_dtype == torch.float32 else None

    def _inputs(self, ys, ylens):
        P = self.params
        ys, yl = lm_inputs(ys, ylens, P.vocab_size)
        assert ys.shape[1] <= P.max_seq_len, f"sequence length {ys.shape[1]} exceeds max_seq_len {P.max_seq_len}"
        return ys, yl

    def _electra_inputs(self, ys, ylens, target, name):
        ys, yl = self._inputs(ys, ylens)
        if target is None:
            raise ValueError(f"emoasr_amd: lm_type={self.lm_type!r} needs `{name}` (the reference dereferences them unconditionally)")
        target = (target.cpu() if torch.is_tensor(target) else torch.as_tensor(target)).to(torch.int64)[:, : ys.shape[1]].contiguous()
        assert target.shape == ys.shape, f"{name}: [B, N] like ys"
        return ys, yl, target

    def _refresh_pe(self):
        A = self._arena
        for S in self._stacks:
            emb = S.pre + "embeddings."
            pos, typ = A.p(emb + "position_embeddings.weight"), A.p(emb + "token_type_embeddings.weight")
            ops.strided_copy(pos, out=S.pe)
            ops.strided_copy(typ[0].expand(pos.shape[0], pos.shape[1]), out=S.pe, accumulate=True)
        self._pe_stale = False

    def _encode(self, ids, klens, B, N, p_h, p_att, keep, S=None):
        """ids int32 [B,N], klens int32 [B] on the device -> (hidden [B*N, d], stash | None): embeddings (+ embeddings_project) + the
        post-LN blocks of stack S (modeling_bert.py:159-436, modeling_electra.py:324-337), dropout by the seeded sites"""
        A, S = self._arena, S or self._stack
        d, H, nl, causal = S.d, S.heads, S.layers, S.causal
        pre = S.pre
        e = ops.embed_fwd(ids, A.w(pre + "embeddings.word_embeddings.weight"), S.pe, 1.0).view(B * N, S.emb)
        x, m0, r0 = ops.layernorm_fwd(e, A.p(pre + "embeddings.LayerNorm.weight"), A.p(pre + "embeddings.LayerNorm.bias"),
                                      1e-12, keep)
        s_emb = self._seed(1, S)
        if p_h > 0:
            x = ops.scale_dropout(x, 1.0, p_h, s_emb)
        xe = x
        if S.project:
            x = ops.gemm_nt(xe, A.w(pre + "embeddings_project.weight"), bias=A.p(pre + "embeddings_project.bias"))
        scale = 1.0 / math.sqrt(d // H)
        layers = []
        for i in range(nl):
            lay = f"{pre}encoder.layer.{i}."
            s_att, s_o, s_f = self._seed(100 + 10 * i, S), self._seed(101 + 10 * i, S), self._seed(102 + 10 * i, S)
            wqkv = A.w_span(lay + "attention.self.query.weight", lay + "attention.self.value.weight", (3 * d, d))
            bqkv = A.p_span(lay + "attention.self.query.bias", lay + "attention.self.value.bias", (3 * d,))
            qkv = ops.gemm_nt(x, wqkv, bias=bqkv).view(B, N, 3 * d)
            o, lse = ops.attn_fwd(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], H, scale, klens=klens, causal=causal,
                                  drop_p=p_att, seed=s_att)
            y = ops.gemm_nt(o.view(B * N, d), A.w(lay + "attention.output.dense.weight"),
                            bias=A.p(lay + "attention.output.dense.bias"), residual=x, res_scale=1.0, drop_p=p_h, seed=s_o)
            x1, m1, r1 = ops.layernorm_fwd(y, A.p(lay + "attention.output.LayerNorm.weight"),
                                           A.p(lay + "attention.output.LayerNorm.bias"), 1e-12, keep)
            u = torch.empty(B * N, S.inner, device=x.device, dtype=x.dtype) if keep else None
            a = ops.gemm_nt(x1, A.w(lay + "intermediate.dense.weight"), bias=A.p(lay + "intermediate.dense.bias"),
                            act=ACT_GELU, pre_out=u)
            y2 = ops.gemm_nt(a, A.w(lay + "output.dense.weight"), bias=A.p(lay + "output.dense.bias"), residual=x1,
                             res_scale=1.0, drop_p=p_h, seed=s_f)
            x2, m2, r2 = ops.layernorm_fwd(y2, A.p(lay + "output.LayerNorm.weight"), A.p(lay + "output.LayerNorm.bias"),
                                           1e-12, keep)
            if keep:
                layers.append((x, qkv, o, lse, y, m1, r1, x1, u, a, y2, m2, r2, s_att, s_o, s_f))
            x = x2
        if not keep:
            return x, None
        st = _Stash()
        st.B, st.N, st.ids, st.klens, st.p_h, st.p_att = B, N, ids, klens, p_h, p_att
        st.e, st.m0, st.r0, st.s_emb, st.layers, st.xe = e, m0, r0, s_emb, layers, xe
        return x, st

    def _lin_bwd(self, dy, x_in, wname, bname, **epi):   # gradients of y = x_in W^T + b; -> dy W with the epilogue
        A = self._arena
        w = A.w(wname)
        ops.gemm_tn(dy, x_in, out=A.g(wname), accumulate=True, colsum=A.g(bname))
        return ops.gemm_nn(dy, w, **epi)

    def _ln_bwd(self, dy, x_in, name, mean, rstd):
        A = self._arena
        return ops.layernorm_bwd(dy, x_in, A.p(name + ".weight"), mean, rstd, None, A.g(name + ".weight"), A.g(name + ".bias"))

    def _backward_stack(self, st, dx, S):
        """dx [B*N, d]: the gradient of stack S's last hidden state -> every gradient of its blocks and embeddings, accumulated"""
        A = self._arena
        d, H, nl, causal = S.d, S.heads, S.layers, S.causal
        B, N, p_h, p_att = st.B, st.N, st.p_h, st.p_att
        pre = S.pre
        word = pre + "embeddings.word_embeddings.weight"
        lin_bwd, ln_bwd = self._lin_bwd, self._ln_bwd
        drop = lambda t, seed: ops.scale_dropout(t, 1.0, p_h, seed) if p_h > 0 else t
        # ---- blocks, last to first.  Post-LN: LayerNorm backward first, then the branch and the residual together
        scale = 1.0 / math.sqrt(d // H)
        scratch = None
        for i in reversed(range(nl)):
            lay = f"{pre}encoder.layer.{i}."
            xin, qkv, o, lse, y, m1, r1, x1, u, a, y2, m2, r2, s_att, s_o, s_f = st.layers[i]
            dy2 = ln_bwd(dx, y2, lay + "output.LayerNorm", m2, r2)
            du = lin_bwd(drop(dy2, s_f), a, lay + "output.dense.weight", lay + "output.dense.bias", dact_pre=u, dact=ACT_GELU)
            dx1 = lin_bwd(du, x1, lay + "intermediate.dense.weight", lay + "intermediate.dense.bias", residual=dy2, res_scale=1.0)
            dy = ln_bwd(dx1, y, lay + "attention.output.LayerNorm", m1, r1)
            do = lin_bwd(drop(dy, s_o), o.view(B * N, d), lay + "attention.output.dense.weight", lay + "attention.output.dense.bias")
            dqkv = torch.empty_like(qkv)
            q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
            dq, dk, dv = dqkv[..., :d], dqkv[..., d:2 * d], dqkv[..., 2 * d:]
            # (the single-pass attention backward has no causal mask: the masked LM takes it in bf16, the causal LM the
            # materialised path, as the ASR decoder's self-attention)
            if self.attn_fused and ops.fused_attn_bwd_ok(q, None, None, None, causal):
                ops.attn_bwd(do.view(B, N, d), o, lse, q, k, v, H, scale, dq, dk, dv, klens=st.klens, drop_p=p_att, seed=s_att,
                             materialise="fused")
            else:
                if scratch is None:   # (zeroed once: every layer of the step masks the same entries)
                    scratch = ops.AttnScratch(B, H, N, N, qkv.dtype, qkv.device, False)
                ops.attn_bwd(do.view(B, N, d), o, lse, q, k, v, H, scale, dq, dk, dv, klens=st.klens, causal=causal,
                             drop_p=p_att, seed=s_att, scratch=scratch)
            dqkv2 = dqkv.view(B * N, 3 * d)
            qn, vn = lay + "attention.self.query.", lay + "attention.self.value."
            ops.gemm_tn(dqkv2, xin, out=A.g_span(qn + "weight", vn + "weight", (3 * d, d)), accumulate=True,
                        colsum=A.g_span(qn + "bias", vn + "bias", (3 * d,)))
            dx = ops.gemm_nn(dqkv2, A.w_span(qn + "weight", vn + "weight", (3 * d, d)), residual=dy, res_scale=1.0)
        # ---- embeddings (modeling_bert.py:159-201): word rows scattered, positions summed over the batch, token type 0 over all rows
        emb, E = pre + "embeddings.", S.emb
        if S.project:     # (modeling_electra.py:328-329: after the embedding dropout)
            dx = lin_bwd(dx, st.xe, pre + "embeddings_project.weight", pre + "embeddings_project.bias")
        de = ln_bwd(drop(dx, st.s_emb), st.e, emb + "LayerNorm", st.m0, st.r0)
        ops.embed_bwd(st.ids, de.view(B, N, E), 1.0, A.g(word))
        ops.colsum(de.view(B, N * E), out=A.g(emb + "position_embeddings.weight").view(-1)[: N * E], accumulate=True)
        ops.colsum(de, out=A.g(emb + "token_type_embeddings.weight")[0], accumulate=True)

    def _active_rows(self, yl, B, N, dev):
        """flat rows b * N + n with n < ylens[b] -> (int64 device tensor | None when every row is active, their number)"""
        if min(yl) >= N:
            return None, B * N
        rows = torch.cat([torch.arange(b * N, b * N + n, dtype=torch.int32) for b, n in enumerate(yl)])
        return h2d_i32(rows, dev).long(), rows.numel()

    def _disc_forward(self, d_ids, klens, yl, y_all, B, N, p_h, p_att, keep):
        """the discriminator on ids d_ids: encoder, dense + GELU, binary head on the rows n < ylens[b] against y_all f32 [B*N]
        -> (loss_disc 0-dim, stash | None)"""
        A, dev = self._arena, d_ids.device
        x, dst = self._encode(d_ids, klens, B, N, p_h, p_att, keep, self._disc)
        act, n_act = self._active_rows(yl, B, N, dev)
        xa, ya = (x, y_all) if act is None else (x.index_select(0, act), y_all.index_select(0, act))
        wa = torch.full((n_act,), 1.0 / n_act, device=dev, dtype=torch.float32)
        dp = self._D + "discriminator_predictions."
        hu = torch.empty_like(xa) if keep else None
        hh = ops.gemm_nt(xa, A.w(dp + "dense.weight"), bias=A.p(dp + "dense.bias"), act=ACT_GELU, pre_out=hu)
        z, lrows, _ = ops.bce_head_fwd(hh, A.w(dp + "dense_prediction.weight").view(-1), A.p(dp + "dense_prediction.bias"), ya, wa)
        if not keep:
            return lrows.sum(), None
        st = _Stash()
        st.dst, st.xa, st.ya, st.wa, st.hu, st.hh, st.z, st.act = dst, xa, ya, wa, hu, hh, z, act
        return lrows.sum(), st

    def _disc_backward(self, st, wd, g1):
        """gradients of wd * g1 * loss_disc of _disc_forward's stash, accumulated into the arena"""
        A = self._arena
        B, N = st.dst.B, st.dst.N
        dp = self._D + "discriminator_predictions."
        dhh = ops.bce_head_bwd(st.hh, A.w(dp + "dense_prediction.weight").view(-1), st.z, st.ya, st.wa,
                               A.g(dp + "dense_prediction.weight").view(-1), A.g(dp + "dense_prediction.bias"), wd, g1)
        dxa = self._lin_bwd(ops.act_bwd(dhh, st.hu, ACT_GELU), st.xa, dp + "dense.weight", dp + "dense.bias")
        if st.act is not None:
            dxa = torch.zeros(B * N, self._disc.d, device=g1.device, dtype=dxa.dtype).index_copy_(0, st.act, dxa)
        self._backward_stack(st.dst, dxa, self._disc)

    def replaced_probs(self, ys, ylens):
        """ELECTRA only.  sigmoid of the discriminator's logit at every position of `ys` as given (padding included; keys at
        n >= ylens[b] are masked) -> float64 [B, N] on the HOST: one encoder pass, ONE device-to-host copy"""
        assert self.electra, "replaced_probs is ELECTRA's discriminator (lm_type 'electra' / 'electra-disc')"
        ys, _ = self._inputs(ys, None)
        yl = [int(v) for v in (ylens.tolist() if torch.is_tensor(ylens) else ylens)]
        B, N = ys.shape
        assert len(yl) == B and 1 <= min(yl) and max(yl) <= N, "ylens: one length in 1..N per row"
        A = self._prepare()
        dev = A.flat.device
        D = self._D + "discriminator_predictions."
        with torch.no_grad(), ops.stream_scope(self._split()):
            x, _ = self._encode(h2d_i32(ys, dev), h2d_i32(yl, dev), B, N, 0.0, 0.0, False, self._disc)
            hh = ops.gemm_nt(x, A.w(D + "dense.weight"), bias=A.p(D + "dense.bias"), act=ACT_GELU)
            _, _, sig = ops.bce_head_fwd(hh, A.w(D + "dense_prediction.weight").view(-1), A.p(D + "dense_prediction.bias"),
                                         want_sigmoid=True)
        return sig.cpu().to(torch.float64).view(B, N)

    def _electra_score(self, ys, ylens):
        probs = self.replaced_probs(ys, ylens)
        if probs.shape[0] == 1:
            return [float(probs[0].sum())]
        return [-float(probs[b, : int(n)].sum()) for b, n in enumerate(ylens)]


class LM(_StackOps, nn.Module):
    stateful = False     # predict() carries no state between calls: the searches re-run the prefix (RNN LM: modeling/rnnlm.py)

    def __new__(cls, params=None, phase="test", compute_dtype=torch.bfloat16):     # (params=None: copy / pickle re-create the object bare)
        if cls is LM and params is not None and params.lm_type == "rnn":
            from .rnnlm import RNNLanguageModel
            return RNNLanguageModel(params, phase, compute_dtype)     # (not an LM instance: __init__ below is not run on it)
        return super().__new__(cls)

    def __init__(self, params, phase="test", compute_dtype=torch.bfloat16):
        super().__init__()
        self.lm_type = params.lm_type
        if self.lm_type not in ("transformer", "bert") + _ELECTRA_TYPES:
            raise NotImplementedError(f"emoasr_amd: lm_type={self.lm_type!r} is outside the HIP hot path")
        self.params = params
        # "f32x3" (f32 storage, split-bf16 products: modeling/asr.py) -> float32 + the library's split switch asserted per call
        self.f32_split = isinstance(compute_dtype, str) and compute_dtype == "f32x3"
        self.compute_dtype = torch.float32 if self.f32_split else compute_dtype
        # one stack, two LMs: the key prefix and the causal mask are all that differ (the reference's TransformerLM is its
        # BertForMaskedLM run with causal=True)
        self.causal = self.lm_type == "transformer"
        self.electra = self.lm_type in _ELECTRA_TYPES
        if self.electra:
            self._init_electra(params)
            return
        root = "lm.transformer." if self.causal else "lm.bert."
        self._PRE, self._CP = root + "bert.", root + "cls.predictions."
        self._NO_GRAD = (self._PRE + "pooler.dense.weight", self._PRE + "pooler.dense.bias")
        self._stack = _Stack(self._PRE, params.hidden_size, params.hidden_size, params.intermediate_size,
                             params.num_attention_heads, params.num_layers, self.causal)
        self._stacks = (self._stack,)
        if self.causal:
            self.lm = TransformerLM(params)
        else:
            if not hasattr(params, "mask_id"):
                raise NotImplementedError("emoasr_amd: lm_type='bert' needs the masked LM's fields; ['mask_id'] is absent from the config")
            self.lm = BERTMaskedLM(params)
            self.mask_id = params.mask_id
        # masked-LM labels cover a fraction of the positions: transform + vocabulary head run on the gathered labelled rows only
        # (a causal LM labels nearly every row and keeps the all-rows head with row weights)
        self.head_at_labels = not self.causal
        self._init_common()

    def _init_common(self):
        self.attn_fused = True     # A/B switch of the single-pass attention backward (bf16, non-causal only)
        self._arena = None
        # the reference's TransformersConfig defaults (lm/modeling/transformer.py:22-29 passes neither): active in train() mode
        self.hidden_dropout_prob = 0.1
        self.attention_probs_dropout_prob = 0.1
        self.fused_head = os.environ.get("EMOASR_CE_HEAD_FUSED", "1") != "0"   # A/B switch of the logit-free head
        self.last_head = None     # "fused" / "materialised": the path the last loss / score call took
        self.seed = 0x5EED
        self.step_count = 0

    def _init_electra(self, params):
        missing = [f for f in _ELECTRA_FIELDS if not hasattr(params, f)]
        if missing:
            raise NotImplementedError(f"emoasr_amd: lm_type={self.lm_type!r} needs ELECTRA's fields; {missing} are absent from the config")
        P = params
        self.lm = ELECTRAModel(params)
        self.mask_id = P.mask_id
        self.electra_disc_weight = float(P.electra_disc_weight)
        self._G, self._D = "lm.gmodel.", "lm.dmodel."
        # dropout seed sites: the generator keeps the sites of the other LMs, the discriminator's are offset past any layer count
        self._gen = _Stack(self._G + "electra.", P.gen_embedding_size, P.gen_hidden_size, P.gen_intermediate_size,
                           P.gen_num_attention_heads, P.gen_num_layers, False, P.gen_embedding_size != P.gen_hidden_size, site=0)
        self._disc = _Stack(self._D + "electra.", P.disc_embedding_size, P.disc_hidden_size, P.disc_intermediate_size,
                            P.disc_num_attention_heads, P.disc_num_layers, False, P.disc_embedding_size != P.disc_hidden_size,
                            site=1 << 20)
        assert max(P.gen_num_layers, P.disc_num_layers) * 10 + 102 < 1 << 20, "dropout seed sites of the two stacks would collide"
        self._stack, self._stacks = self._disc, (self._gen, self._disc)
        self._NO_GRAD = ()
        self.head_at_labels = True
        self.sample_path = "hip"       # "torch": comparator of tools/lm_bench.py (softmax + multinomial + indexed assignment)
        self.forced_samples = None     # int64 [B, N]: replaces the drawn samples at the masked positions (tests, replaying a run)
        self.last_corruption = None    # (generated_ids int32 [B, N], labels_replaced f32 [B, N]) of the last forward, on the device
        self._init_common()

    def load_state_dict(self, state_dict, strict=True):
        try:
            return super().load_state_dict(state_dict, strict)
        except RuntimeError:
            return self.lm.load_state_dict(state_dict, strict)  # un-prefixed inner dict (lm.py:62-66)

    def zero_states(self, bs, device):
        if not self.causal:
            raise NotImplementedError(_NO_PREDICT_ELECTRA if self.electra else _NO_PREDICT)
        return self.lm.zero_states(bs, device)

    # ---------------------------------------------------------------- HIP forward
    def _bind(self):
        if self._arena is None or not self._arena.bound() or self._arena.compute_dtype != self.compute_dtype:
            self._arena = ParamArena(self, self.compute_dtype)
            A = self._arena
            for S in self._stacks:     # position + token-type(0) rows folded into one additive table per stack (modeling_bert.py:196-201)
                emb = S.pre + "embeddings."
                S.pe = (A.p(emb + "position_embeddings.weight") + A.p(emb + "token_type_embeddings.weight")[0]).contiguous()
        return self._arena

    @property
    def _pe(self):
        return self._stack.pe

    def _forward_rows(self, ids, klens, idx, B, N):
        """ids int32 [B,N], klens int32 [B], idx [B] (flat position b * N + ylens[b] - 1 of every row's last token), all on the
        device -> f32 log-probs [B, V]"""
        A = self._arena
        P = self.params
        d, H, nl = P.hidden_size, P.num_attention_heads, P.num_layers
        pre = "lm.transformer.bert."
        x = ops.embed_fwd(ids, A.w(pre + "embeddings.word_embeddings.weight"), self._pe, 1.0).view(B * N, d)
        x, _, _ = ops.layernorm_fwd(x, A.p(pre + "embeddings.LayerNorm.weight"), A.p(pre + "embeddings.LayerNorm.bias"),
                                    1e-12, False)
        scale = 1.0 / math.sqrt(d // H)
        for i in range(nl):
            lay = f"{pre}encoder.layer.{i}."
            wqkv = A.w_span(lay + "attention.self.query.weight", lay + "attention.self.value.weight", (3 * d, d))
            bqkv = A.p_span(lay + "attention.self.query.bias", lay + "attention.self.value.bias", (3 * d,))
            qkv = ops.gemm_nt(x, wqkv, bias=bqkv).view(B, N, 3 * d)
            o, _ = ops.attn_fwd(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], H, scale, klens=klens, causal=True)
            y = ops.gemm_nt(o.view(B * N, d), A.w(lay + "attention.output.dense.weight"),
                            bias=A.p(lay + "attention.output.dense.bias"), residual=x, res_scale=1.0)
            x1, _, _ = ops.layernorm_fwd(y, A.p(lay + "attention.output.LayerNorm.weight"),
                                         A.p(lay + "attention.output.LayerNorm.bias"), 1e-12, False)
            u = ops.gemm_nt(x1, A.w(lay + "intermediate.dense.weight"), bias=A.p(lay + "intermediate.dense.bias"),
                            act=ACT_GELU)
            y2 = ops.gemm_nt(u, A.w(lay + "output.dense.weight"), bias=A.p(lay + "output.dense.bias"), residual=x1,
                             res_scale=1.0)
            x, _, _ = ops.layernorm_fwd(y2, A.p(lay + "output.LayerNorm.weight"), A.p(lay + "output.LayerNorm.bias"),
                                        1e-12, False)
        rows = x.index_select(0, idx)
        cp = "lm.transformer.cls.predictions."
        t = ops.gemm_nt(rows, A.w(cp + "transform.dense.weight"), bias=A.p(cp + "transform.dense.bias"), act=ACT_GELU)
        t, _, _ = ops.layernorm_fwd(t, A.p(cp + "transform.LayerNorm.weight"), A.p(cp + "transform.LayerNorm.bias"),
                                    1e-12, False)
        logits = ops.gemm_nt(t, A.w(pre + "embeddings.word_embeddings.weight"), bias=A.p(cp + "bias"), out_f32=True)
        return ops.log_softmax(logits)

    def predict_device(self, ys, ylens):
        """ys CPU int64 [B,N]; ylens list -> f32 log-probs [B, V] on the device (row ylens[b]-1).

        Up to 16 rows (what the beam searches ask for, one call per output step or per frame): the ~90 launches of the forward
        are replayed from a HIP graph over static buffers, one graph per (rows padded to 4 / 16, length padded to a multiple of
        8) -- the call was host-bound (1.5 ms of launch sequencing for ~0.4 ms of kernels).  Padding rows / positions are masked
        by their key lengths and never read back; the real rows' arithmetic is the eager call's.  EMOASR_LM_GRAPH=0: eager."""
        if not self.causal:
            raise NotImplementedError(_NO_PREDICT_ELECTRA if self.electra else _NO_PREDICT)
        arena_before = self._arena
        A = self._bind()
        if A is not arena_before:
            self._graphs = {}     # (captured launches hold the old arena's addresses)
        A.refresh_shadow()
        if getattr(self, "_pe_stale", False):   # a training step has moved the embeddings since the table was built
            self._refresh_pe()
        ys = torch.as_tensor(ys)
        B, N = ys.shape
        dev = A.flat.device
        yl = [int(v) for v in ylens]
        split = self.f32_split if self.compute_dtype == torch.float32 else None
        if B <= 16 and dev.type == "cuda" and os.environ.get("EMOASR_LM_GRAPH", "1") != "0" and not torch.cuda.is_current_stream_capturing():
            return self._predict_graph(ys, yl, B, N, dev, split)
        with ops.stream_scope(split):
            ids = h2d_i32(ys.contiguous(), dev)
            klens = h2d_i32(yl, dev)
            idx = h2d_i32([b * N + v - 1 for b, v in enumerate(yl)], dev)
            return self._forward_rows(ids, klens, idx, B, N)

    def _predict_graph(self, ys, yl, B, N, dev, split):
        Bp, Np = (4 if B <= 4 else 16), (N + 7) // 8 * 8
        graphs = self.__dict__.setdefault("_graphs", {})
        g = graphs.get((Bp, Np))
        if g is None:
            g = SimpleNamespace()
            n_ids = Bp * Np
            g.host = torch.zeros(n_ids + 2 * Bp, dtype=torch.int32).pin_memory()
            g.dev = torch.zeros(n_ids + 2 * Bp, dtype=torch.int32, device=dev)
            g.ids, g.klens, g.idx = g.dev[:n_ids].view(Bp, Np), g.dev[n_ids:n_ids + Bp], g.dev[n_ids + Bp:]
            g.host[n_ids:n_ids + Bp] = 1     # (a valid state for the warm-up run: every row one token long)
            g.host[n_ids + Bp:] = torch.arange(Bp, dtype=torch.int32) * Np
            g.dev.copy_(g.host)

            def body():
                with ops.stream_scope(split):
                    return self._forward_rows(g.ids, g.klens, g.idx, Bp, Np)

            g.graph, g.out = lockstep.capture_after_warmup(body, dev)
            graphs[(Bp, Np)] = g
        n_ids = Bp * Np
        h = g.host
        if getattr(g, "ev", None) is not None:
            g.ev.synchronize()   # (the previous call's upload has left the pinned record)
        h[:n_ids + Bp] = 0
        h[:n_ids].view(Bp, Np)[:B, :N] = ys.to(torch.int32)
        h[n_ids:n_ids + Bp] = 1
        h[n_ids:n_ids + B] = torch.tensor(yl, dtype=torch.int32)
        h[n_ids + Bp:] = torch.arange(Bp, dtype=torch.int32) * Np
        h[n_ids + Bp:n_ids + Bp + B] += torch.tensor(yl, dtype=torch.int32) - 1
        g.dev.copy_(h, non_blocking=True)
        g.ev = torch.cuda.Event()
        g.ev.record()
        g.graph.replay()
        return g.out[:B].clone()

    def predict(self, ys, ylens, states=None):
        if not self.causal:
            raise NotImplementedError(_NO_PREDICT_ELECTRA if self.electra else _NO_PREDICT)
        with torch.no_grad():
            ys_host = ys.cpu() if torch.is_tensor(ys) else torch.as_tensor(ys)
            yl = ylens.tolist() if torch.is_tensor(ylens) else list(ylens)
            return self.predict_device(ys_host, yl), states

    # ---------------------------------------------------------------- training, scoring
    MAX_TOKEN_ROWS = 16384     # masked_logprobs: token rows (copies x padded length) per encoder run

    def _prepare(self):
        """arena bound, compute-dtype weights and the additive position + token-type(0) table current (the parameters move
        between training steps; the table is rebuilt IN PLACE, so captured predict graphs keep reading the right address)"""
        arena_before = self._arena
        A = self._bind()
        if A is not arena_before:
            self._graphs = {}
        A.refresh_shadow()
        self._refresh_pe()
        return A

    def _transform(self, x, keep):
        """cls.predictions.transform (modeling_bert.py:537-554): dense + GELU + LayerNorm -> (t2, stash)"""
        A, cp = self._arena, self._CP
        tu = torch.empty_like(x) if keep else None
        t = ops.gemm_nt(x, A.w(cp + "transform.dense.weight"), bias=A.p(cp + "transform.dense.bias"), act=ACT_GELU, pre_out=tu)
        t2, mt, rt = ops.layernorm_fwd(t, A.p(cp + "transform.LayerNorm.weight"), A.p(cp + "transform.LayerNorm.bias"),
                                       1e-12, keep)
        return t2, (x, tu, t, mt, rt)

    def _head_rows(self, t2, labels, w):
        """the tied output projection + soft-max, reduced per row: labels int32 [M] (clamped), w f32 [M]
        -> (rows f32 [M] = -w[m] * log p(labels[m] | row m), head stash)"""
        A = self._arena
        rows, head = ops.lm_head_fwd(self.fused_head, t2, A.w(self._PRE + "embeddings.word_embeddings.weight"),
                                     A.p(self._CP + "bias"), labels, w)
        self.last_head = head[0]
        return rows, head

    def forward(self, ys, ylens=None, labels=None, ps=None, plens=None):
        """lm/modeling/lm.py:45-46, transformer.py:35-56: logits [B, N, V] (f32) without labels, else (loss, {"loss_total": loss});
        ELECTRA (electra.py:71-100): (loss, {loss_gen, loss_disc, num_replaced, num_masked}), labels required"""
        if self.electra:
            return self._electra_forward(ys, ylens, labels)
        ys, yl = self._inputs(ys, ylens)
        A = self._prepare()
        if labels is None:
            B, N = ys.shape
            if self.training:      # (the reference's logits in train() mode carry its dropout too)
                self.step_count += 1
            p_h = float(self.hidden_dropout_prob) if self.training else 0.0
            p_att = float(self.attention_probs_dropout_prob) if self.training else 0.0
            with torch.no_grad(), ops.stream_scope(self._split()):
                dev = A.flat.device
                x, _ = self._encode(h2d_i32(ys, dev), h2d_i32(yl, dev), B, N, p_h, p_att, False)
                t2, _ = self._transform(x, False)
                W = A.w(self._PRE + "embeddings.word_embeddings.weight")
                logits = ops.gemm_nt(t2, W, bias=A.p(self._CP + "bias"), out_f32=t2.dtype != torch.float32)
            return logits.view(B, N, -1)
        labels = (labels.cpu() if torch.is_tensor(labels) else torch.as_tensor(labels)).to(torch.int64)
        if ylens is not None:
            labels = labels[:, : max(yl)]
        loss = _LMLossFn.apply(self, ys, yl, labels.contiguous(), *A.params)
        return loss, {"loss_total": loss}

    def logits_at(self, ys, ylens, rows):
        """masked LM (lm_type "bert"), inputs that already lie on the device: ys int [S, Lw] (device), ylens [S] (host, each >= 1),
        rows int [n] (device): flat positions s * Lw + j of ys -> logits [n, V] (f32) of those positions.  The
        stack runs on all tokens, in chunks of MAX_TOKEN_ROWS token rows (sequences x padded length); the transform and the
        vocabulary product run on the n gathered rows alone.  Nothing is copied to the host."""
        assert not self.causal and not self.electra, "logits_at is the masked LM's (lm_type='bert')"
        P = self.params
        A = self._prepare()
        dev = A.flat.device
        assert ys.is_cuda and rows.is_cuda and ys.dim() == 2, "logits_at takes device tensors (forward takes host ids)"
        S, Lw = ys.shape
        yl = [int(v) for v in (ylens.tolist() if torch.is_tensor(ylens) else ylens)]
        assert len(yl) == S and min(yl) >= 1 and max(yl) <= min(Lw, P.max_seq_len), f"ylens in [1, {min(Lw, P.max_seq_len)}]"
        Lp = min((max(yl) + 7) // 8 * 8, Lw, P.max_seq_len)     # (the padding is masked by the key lengths)
        n = rows.numel()
        with torch.no_grad(), ops.stream_scope(self._split()):
            W = A.w(self._PRE + "embeddings.word_embeddings.weight")
            if n == 0:
                return torch.empty(0, W.shape[0], device=dev, dtype=torch.float32)
            ids = ys[:, :Lp].to(torch.int32).contiguous()
            r = rows.to(torch.int64)
            r = (r // Lw) * Lp + r % Lw
            klens = h2d_i32(yl, dev)
            chunk = max(1, self.MAX_TOKEN_ROWS // Lp)
            h = None
            for s0 in range(0, S, chunk):
                s1 = min(s0 + chunk, S)
                x, _ = self._encode(ids[s0:s1], klens[s0:s1], s1 - s0, Lp, 0.0, 0.0, False)
                g = x.index_select(0, (r - s0 * Lp).clamp_(0, (s1 - s0) * Lp - 1))
                h = g if h is None else torch.where(((r >= s0 * Lp) & (r < s1 * Lp)).unsqueeze(1), g, h)
            t2, _ = self._transform(h, False)
            return ops.gemm_nt(t2, W, bias=A.p(self._CP + "bias"), out_f32=t2.dtype != torch.float32)

    def _loss_forward(self, ys, yl, labels, keep):
        A = self._arena
        dev = A.flat.device
        B, N = ys.shape
        training = self.training
        if training:
            self.step_count += 1
        p_h = float(self.hidden_dropout_prob) if training else 0.0
        p_att = float(self.attention_probs_dropout_prob) if training else 0.0
        valid = labels != -100
        assert labels.shape == ys.shape and int(labels.max()) < self.params.vocab_size, "labels: [B, N] ids below vocab_size or -100"
        count = int(valid.sum())
        sel = None
        if self.head_at_labels:     # the M labelled rows only (no label at all: one row of weight 0)
            rows_host = valid.view(-1).nonzero().view(-1) if count else torch.zeros(1, dtype=torch.int64)
            lab_host = labels.view(-1)[rows_host].clamp(min=0)
            w = torch.full((rows_host.numel(),), 1.0 / count if count else 0.0)
        else:
            lab_host = labels.clamp(min=0).view(-1)
            w = valid.to(torch.float32) / max(count, 1)     # mean over the rows with a label (CrossEntropyLoss, ignore_index=-100)
        with ops.stream_scope(self._split()):
            ids, klens, lab = h2d_i32(ys, dev), h2d_i32(yl, dev), h2d_i32(lab_host, dev)
            w_dev = w.view(-1).pin_memory().to(dev, non_blocking=True)
            x, st = self._encode(ids, klens, B, N, p_h, p_att, keep)
            if self.head_at_labels:
                sel = rows_host.pin_memory().to(dev, non_blocking=True)
                x = x.index_select(0, sel)
            t2, tst = self._transform(x, keep)
            rows, head = self._head_rows(t2, lab, w_dev)
            loss = rows.sum()
        if keep:
            self._pe_stale = True     # (an update follows: predict() rebuilds the position table before its next use)
            st.t2, st.tst, st.head, st.lab, st.w, st.sel = t2, tst, head, lab, w_dev, sel
        return loss, st

    def _loss_backward(self, st, g):
        """g: the incoming gradient of the loss (0-dim, on the device).  Accumulates every parameter gradient into the arena."""
        with ops.stream_scope(self._split()):
            self._backward(st, g.to(torch.float32).reshape(1))

    def _backward(self, st, g1):
        A = self._arena
        A.attach_grads()
        S = self._stack
        d = S.d
        B, N = st.B, st.N
        pre, cp = self._PRE, self._CP
        word = pre + "embeddings.word_embeddings.weight"
        lin_bwd, ln_bwd = self._lin_bwd, self._ln_bwd
        # ---- vocabulary head (tied to the word embedding: its weight gradient lands in the embedding's slot)
        dt2 = ops.lm_head_bwd(st.head, st.t2, A.w(word), A.p(cp + "bias"), st.lab, st.w, A.g(word), A.g(cp + "bias"), g1)
        x, tu, t, mt, rt = st.tst
        dpre = ops.act_bwd(ln_bwd(dt2, t, cp + "transform.LayerNorm", mt, rt), tu, ACT_GELU)
        dx = lin_bwd(dpre, x, cp + "transform.dense.weight", cp + "transform.dense.bias")
        if st.sel is not None:     # the head ran on gathered rows: their gradient goes back to its rows, every other row has none
            dx = torch.zeros(B * N, d, device=dx.device, dtype=dx.dtype).index_copy_(0, st.sel, dx)
        self._backward_stack(st, dx, S)
        for n in self._NO_GRAD:      # never read by the LM: .grad stays None as in the reference (AdamW then leaves them alone)
            A.params[A.names.index(n)].grad = None

    def token_logprobs(self, ys, ylens, labels):
        """log p(labels[b,i] | ys[b,:i+1]) for every position with labels != -100 (zeros elsewhere) -> float64 [B, N] on the HOST:
        the logit-free head forward (label logit minus log-sum-exp), ONE device-to-host copy of the row values"""
        assert not self.electra, "token_logprobs is a next-token or masked LM's; ELECTRA scores with replaced_probs"
        ys, yl = self._inputs(ys, ylens)
        labels = (labels.cpu() if torch.is_tensor(labels) else torch.as_tensor(labels)).to(torch.int64)[:, : ys.shape[1]]
        A = self._prepare()
        dev = A.flat.device
        B, N = ys.shape
        valid = labels != -100
        with torch.no_grad(), ops.stream_scope(self._split()):
            ids, klens, lab = h2d_i32(ys, dev), h2d_i32(yl, dev), h2d_i32(labels.clamp(min=0).contiguous().view(-1), dev)
            w_dev = valid.to(torch.float32).contiguous().view(-1).pin_memory().to(dev, non_blocking=True)
            x, _ = self._encode(ids, klens, B, N, 0.0, 0.0, False)
            t2, _ = self._transform(x, False)
            rows, _ = self._head_rows(t2, lab, w_dev)
        return -rows.cpu().to(torch.float64).view(B, N) * valid.to(torch.float64)

    def masked_logprobs(self, ys, ylens, max_token_rows=None):
        """masked LM only.  Entry (b, i), i < ylens[b]: log p(ys[b,i] | ys[b] with position i replaced by mask_id); zeros elsewhere
        -> float64 [B, N] on the HOST.  The R = sum(ylens) masked copies are built on the device (ops.mlm_expand) and walked in
        chunks of at most max_token_rows token rows (copies x padded length; a chunk may begin and end inside a sequence); of every
        copy only its masked row goes through transform + head, and the R row values come back in ONE device-to-host copy."""
        assert not self.causal and not self.electra, "masked_logprobs is the masked LM's (lm_type='bert'); a causal LM has token_logprobs"
        assert ylens is not None
        ys, yl = self._inputs(ys, ylens)
        A = self._prepare()
        dev = A.flat.device
        B, N = ys.shape
        Np = min((N + 7) // 8 * 8, self.params.max_seq_len)     # (whole 32-byte id rows; the padding is masked by the key lengths)
        row0 = [0]
        for n in yl:
            row0.append(row0[-1] + n)
        R = row0[-1]
        chunk = max(1, int(max_token_rows or self.MAX_TOKEN_ROWS) // Np)
        with torch.no_grad(), ops.stream_scope(self._split()):
            ys_dev, yl_dev, row0_dev = h2d_i32(ys, dev), h2d_i32(yl, dev), h2d_i32(row0, dev)
            ones = torch.ones(min(chunk, R), device=dev, dtype=torch.float32)
            out = torch.empty(R, device=dev, dtype=torch.float32)
            for r0 in range(0, R, chunk):
                rc = min(chunk, R - r0)
                ids, klens, idx, lab = ops.mlm_expand(ys_dev, yl_dev, row0_dev, r0, rc, Np, int(self.mask_id), 0, total=R)
                x, _ = self._encode(ids, klens, rc, Np, 0.0, 0.0, False)
                t2, _ = self._transform(x.index_select(0, idx), False)
                rows, _ = self._head_rows(t2, lab, ones[:rc])
                out[r0:r0 + rc] = rows
        flat = -out.cpu().to(torch.float64)
        res = torch.zeros(B, N, dtype=torch.float64)
        for b, n in enumerate(yl):
            res[b, :n] = flat[row0[b]:row0[b + 1]]
        return res

    def score(self, ys, ylens, batch_size=100):
        """causal LM (lm/modeling/transformer.py:79-99): per row sum_{i < ylens[b]-1} log p(ys[b,i+1] | ys[b,:i+1]); masked LM
        (lm/modeling/bert.py:54-86): the pseudo-log-likelihood, the row sums of masked_logprobs (all copies of a call are stacked and
        chunked by token rows there, so `batch_size` -- copies per run in the reference -- changes nothing) -> Python list of floats
        (summed on the host in double precision, as the reference sums Python floats).
        ELECTRA (lm/modeling/electra.py:116-132): one discriminator pass, p = sigmoid(logit) = the probability that a token was
        replaced, one device-to-host copy of the [B, N] probabilities, `batch_size` unused as in the reference.  The reference's
        SIGN QUIRK is kept: a call with B > 1 rows returns -sum(p[b, :ylens[b]]) per row (higher = fewer suspected errors), a call
        with ONE row returns +sum(p[0, :]) over ALL N positions of `ys` as given, padding included -- the two are not comparable."""
        if self.electra:
            return self._electra_score(ys, ylens)
        if not self.causal:
            return self.masked_logprobs(ys, ylens).sum(dim=1).tolist()
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

    # ---------------------------------------------------------------- ELECTRA (lm/modeling/electra.py:33-132)
    SITE_SAMPLE = 7      # seed site of the generator's samples (the dropout sites are 1 and 100 + 10 * layer + {0, 1, 2})

    def _electra_forward(self, ys, ylens, labels):
        """electra.py:71-100 -> (loss_gen + electra_disc_weight * loss_disc, {loss_gen, loss_disc, num_replaced, num_masked}): one
        autograd node; the sample is discrete, so no gradient flows from the discriminator into the generator"""
        ys, yl, labels = self._electra_inputs(ys, ylens, labels, "labels")
        A = self._prepare()
        loss = _ElectraLossFn.apply(self, "both", ys, yl, labels, *A.params)
        aux = self._aux
        B = ys.shape[0]
        return loss, {"loss_gen": aux["loss_gen"], "loss_disc": aux["loss_disc"], "num_replaced": aux["counters"][0] / B,
                      "num_masked": aux["counters"][1] / B}

    def forward_disc(self, ys, ylens=None, error_labels=None):
        """electra.py:102-114: the discriminator alone on `ys`, BCE against error_labels (0 / 1, -100 where n >= ylens[b]) over the
        positions n < ylens[b] -> (loss, {"loss_total": loss}).  The generator is not run and its parameters' .grad is None after the
        backward (do not mix forward and forward_disc inside one gradient-accumulation window)."""
        if not self.electra:
            raise NotImplementedError(f"emoasr_amd: forward_disc is ELECTRA's; lm_type={self.lm_type!r} has no discriminator")
        ys, yl, err = self._electra_inputs(ys, ylens, error_labels, "error_labels")
        A = self._prepare()
        loss = _ElectraLossFn.apply(self, "disc", ys, yl, err, *A.params)
        return loss, {"loss_total": loss}

    def _electra_loss_forward(self, mode, ys, yl, target, keep):
        A = self._arena
        dev = A.flat.device
        B, N = ys.shape
        training = self.training
        if training:
            self.step_count += 1
        p_h = float(self.hidden_dropout_prob) if training else 0.0
        p_att = float(self.attention_probs_dropout_prob) if training else 0.0
        G = self._G
        st = _Stash()
        st.mode = mode
        with ops.stream_scope(self._split()):
            ids, klens = h2d_i32(ys, dev), h2d_i32(yl, dev)
            if mode == "both":
                labels = target
                valid = labels != -100
                assert int(labels.max()) < self.params.vocab_size, "labels: [B, N] ids below vocab_size or -100"
                count = int(valid.sum())
                rows_host = valid.view(-1).nonzero().view(-1) if count else torch.zeros(1, dtype=torch.int64)     # (no label: one row of weight 0)
                lab = h2d_i32(labels.view(-1)[rows_host].clamp(min=0), dev)
                sel = h2d_i32(rows_host, dev)
                w = torch.full((rows_host.numel(),), 1.0 / count if count else 0.0).pin_memory().to(dev, non_blocking=True)
                # ---- generator: encoder, transform + vocabulary head on the labelled rows, loss rows and one sample per row
                x, gst = self._encode(ids, klens, B, N, p_h, p_att, keep, self._gen)
                sel64 = sel.long()
                xs = x.index_select(0, sel64)
                tu = torch.empty(xs.shape[0], self._gen.emb, device=dev, dtype=xs.dtype) if keep else None
                gp = G + "generator_predictions."
                t = ops.gemm_nt(xs, A.w(gp + "dense.weight"), bias=A.p(gp + "dense.bias"), act=ACT_GELU, pre_out=tu)
                t2, mt, rt = ops.layernorm_fwd(t, A.p(gp + "LayerNorm.weight"), A.p(gp + "LayerNorm.bias"), 1e-5, keep)
                # [M, V] logits in rows padded to a multiple of 8 columns: the shipped V = 9 798 is none, and the gradient
                # products read dz with that row stride
                W = A.w(G + "electra.embeddings.word_embeddings.weight")
                V = W.shape[0]
                logits = torch.empty(xs.shape[0], (V + 7) // 8 * 8, device=dev, dtype=t2.dtype)[:, :V]
                ops.gemm_nt(t2, W, out=logits, bias=A.p(G + "generator_lm_head.bias"))
                if self.sample_path == "torch":     # comparator: what the reference does, on the gathered rows
                    rows, _ = ops.lsm_loss(logits, lab, w, 0.0)
                    samples = torch.softmax(logits.float(), dim=1).multinomial(1).view(-1).to(torch.int32)
                else:
                    rows, samples, _ = ops.sample_rows(logits, lab, w, self._seed(self.SITE_SAMPLE))
                if self.forced_samples is not None:
                    forced = torch.as_tensor(self.forced_samples).to(torch.int64)[:, :N].contiguous()
                    assert forced.shape == ys.shape, "forced_samples: int64 [B, N]"
                    forced = forced.view(-1)[rows_host]
                    assert 0 <= int(forced.min()) and int(forced.max()) < V, "forced_samples: token id outside the vocabulary"
                    samples = h2d_i32(forced, dev)
                loss_gen = rows.sum()
                m = slice(0, rows_host.numel() if count else 0)
                if self.sample_path == "torch":
                    generated = ids.clone()
                    original = ids.clone()
                    generated.view(-1)[sel64[m]] = samples[m]
                    original.view(-1)[sel64[m]] = lab[m]
                    replaced = (generated != original).to(torch.float32)
                    counters = torch.stack([replaced.sum(), torch.full((), float(count), device=dev)]).to(torch.int32)
                else:
                    generated, replaced, counters = ops.electra_corrupt(ids, sel[m], lab[m], samples[m])
                self.last_corruption = (generated, replaced)
                st.gst, st.xs, st.tu, st.t, st.mt, st.rt, st.t2 = gst, xs, tu, t, mt, rt, t2
                st.logits, st.lab, st.w, st.sel = logits, lab, w, sel64
                d_ids, y_all = generated, replaced.view(-1)
            else:
                err = target
                mask = torch.arange(N)[None, :] < torch.tensor(yl)[:, None]
                assert bool(((err == 0) | (err == 1))[mask].all()), "error_labels: 0 / 1 at every position n < ylens[b]"
                d_ids = ids
                y_all = err.clamp(min=0).to(torch.float32).view(-1).pin_memory().to(dev, non_blocking=True)
                loss_gen = counters = None
            # ---- discriminator: encoder, dense + GELU, binary head on the rows n < ylens[b]
            loss_disc, dstash = self._disc_forward(d_ids, klens, yl, y_all, B, N, p_h, p_att, keep)
            loss = loss_disc if mode == "disc" else loss_gen + self.electra_disc_weight * loss_disc
        self._aux = {"loss_gen": loss_gen, "loss_disc": loss_disc, "counters": counters}
        if not keep:
            return loss, None
        self._pe_stale = True
        st.disc = dstash
        return loss, st

    def _padded_word(self, W):
        """the generator's word embedding [V, E] with zero rows up to a multiple of 8 (the inner dimension of dz . W): W itself
        where V already is one, else a copy refreshed here, once per backward"""
        V, E = W.shape
        Vp = (V + 7) // 8 * 8
        if Vp == V:
            return W
        buf = self.__dict__.get("_wpad")
        if buf is None or buf.shape != (Vp, E) or buf.dtype != W.dtype or buf.device != W.device:
            buf = self.__dict__["_wpad"] = torch.zeros(Vp, E, device=W.device, dtype=W.dtype)
        ops.strided_copy(W, out=buf[:V])
        return buf

    def _electra_loss_backward(self, st, g):
        A = self._arena
        G = self._G
        lin_bwd, ln_bwd = self._lin_bwd, self._ln_bwd
        with ops.stream_scope(self._split()):
            g1 = g.to(torch.float32).reshape(1)
            A.attach_grads()
            B, N = st.disc.dst.B, st.disc.dst.N
            dev = g1.device
            self._disc_backward(st.disc, 1.0 if st.mode == "disc" else self.electra_disc_weight, g1)
            if st.mode == "disc":
                # the generator was not run: its .grad is None, as in the reference (AdamW then leaves it bit-identical).  A
                # discriminator-only step therefore does not share an accumulation window with a generator step.
                for n, p in zip(A.names, A.params):
                    if n.startswith(G):
                        p.grad = None
                return
            # ---- generator: vocabulary head (tied to its word embedding), transform, the labelled rows scattered back
            gp, word = G + "generator_predictions.", G + "electra.embeddings.word_embeddings.weight"
            M, V = st.logits.shape
            Wp = self._padded_word(A.w(word))
            dzp = torch.zeros(M, Wp.shape[0], device=dev, dtype=st.logits.dtype)     # (the padding columns stay 0)
            dz = dzp[:, :V]
            ops.lsm_loss(st.logits, st.lab, st.w, 0.0, True, 1.0, g1, grad=dz)
            ops.gemm_tn(dz, st.t2, out=A.g(word), accumulate=True, colsum=A.g(G + "generator_lm_head.bias"))
            dt2 = ops.gemm_nn(dzp, Wp)
            dpre = ops.act_bwd(ln_bwd(dt2, st.t, gp + "LayerNorm", st.mt, st.rt), st.tu, ACT_GELU)
            dxs = lin_bwd(dpre, st.xs, gp + "dense.weight", gp + "dense.bias")
            dx = torch.zeros(B * N, self._gen.d, device=dev, dtype=dxs.dtype).index_copy_(0, st.sel, dxs)
            self._backward_stack(st.gst, dx, self._gen)

class _ElectraLossFn(torch.autograd.Function):
    """ELECTRA's training loss (mode "both": generator + weighted discriminator; "disc": the discriminator alone) as ONE autograd node"""

    @staticmethod
    def forward(ctx, lm, mode, ys, yl, target, *params):
        keep = any(ctx.needs_input_grad)
        loss, st = lm._electra_loss_forward(mode, ys, yl, target, keep)
        ctx.lm, ctx.st = lm, st
        return loss

    @staticmethod
    def backward(ctx, g):
        ctx.lm._electra_loss_backward(ctx.st, g)
        ctx.st = None
        return (None, None, None, None, None) + (None,) * len(ctx.lm._arena.params)


class _LMLossFn(torch.autograd.Function):
    """the LM training loss as ONE autograd node over the parameters: backward() runs the hand-written gradient kernels"""

    @staticmethod
    def forward(ctx, lm, ys, yl, labels, *params):
        keep = any(ctx.needs_input_grad)     # (False under torch.no_grad(): nothing is stashed)
        loss, st = lm._loss_forward(ys, yl, labels, keep)
        ctx.lm, ctx.st = lm, st
        return loss

    @staticmethod
    def backward(ctx, g):
        ctx.lm._loss_backward(ctx.st, g)
        ctx.st = None
        return (None, None, None, None) + (None,) * len(ctx.lm._arena.params)
