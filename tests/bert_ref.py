"""A small torch restatement of the BERT masked LM (and, with causal=True, of the Transformer LM: the same stack), written from its
behaviour: post-LN BERT blocks over word + position + token-type(0) embeddings, the `cls.predictions` transform and the output
projection tied to the word embedding.  The state-dict keys are the model's (`lm.bert.bert.*`, `lm.bert.cls.predictions.*`; pass
root="lm.transformer." for the causal LM), any float dtype (f64 for references), autograd for the gradients.  No dropout: the
fixtures and the tests run without it.

`round_to` simulates a low-precision run on the CPU: every activation that the HIP path stores in the compute dtype (embedding sum,
projections, attention output, GELU, LayerNorm outputs) is rounded to that dtype; the weights are the caller's to round.  Summation
order, the f32 soft-max statistics and the roundings inside fused epilogues are NOT simulated."""
import math

import torch
import torch.nn.functional as F

ROOT = "lm.bert."


def _rnd(x, round_to):
    return x if round_to is None else x.to(round_to).to(x.dtype)


def _ln(sd, name, x, round_to):
    return _rnd(F.layer_norm(x, x.shape[-1:], sd[name + ".weight"], sd[name + ".bias"], 1e-12), round_to)


def _lin(sd, name, x, round_to=None):
    return _rnd(x @ sd[name + ".weight"].t() + sd[name + ".bias"], round_to)


def num_layers(sd, root=ROOT):
    return sum(1 for k in sd if k.startswith(root + "bert.encoder.layer.") and k.endswith("attention.self.query.weight"))


def hidden(sd, ys, ylens=None, heads=2, causal=False, round_to=None, root=ROOT):
    """ys int64 [B, N] (already trimmed) -> last hidden state [B, N, d]; keys at positions >= ylens[b] are masked"""
    pre = root + "bert."
    B, N = ys.shape
    emb = pre + "embeddings."
    x = sd[emb + "word_embeddings.weight"][ys] + sd[emb + "position_embeddings.weight"][:N] + sd[emb + "token_type_embeddings.weight"][0]
    x = _ln(sd, emb + "LayerNorm", _rnd(x, round_to), round_to)
    d = x.shape[-1]
    dk = d // heads
    allowed = torch.ones(B, 1, N, N, dtype=torch.bool)
    if ylens is not None:
        allowed = allowed & (torch.arange(N)[None, :] < torch.as_tensor(ylens)[:, None])[:, None, None, :]
    if causal:
        allowed = allowed & torch.tril(torch.ones(N, N, dtype=torch.bool))
    for i in range(num_layers(sd, root)):
        lay = f"{pre}encoder.layer.{i}."
        q, k, v = (_lin(sd, lay + "attention.self." + n, x, round_to).view(B, N, heads, dk).transpose(1, 2)
                   for n in ("query", "key", "value"))
        s = (q @ k.transpose(-1, -2)) / math.sqrt(dk)
        p = torch.softmax(s.masked_fill(~allowed, float("-inf")), dim=-1)
        o = _rnd((p @ v).transpose(1, 2).reshape(B, N, d), round_to)
        x = _ln(sd, lay + "attention.output.LayerNorm", _lin(sd, lay + "attention.output.dense", o) + x, round_to)
        u = _rnd(F.gelu(_lin(sd, lay + "intermediate.dense", x)), round_to)
        x = _ln(sd, lay + "output.LayerNorm", _lin(sd, lay + "output.dense", u) + x, round_to)
    return x


def head(sd, x, round_to=None, root=ROOT):
    """cls.predictions: dense + GELU + LayerNorm, then the tied projection + bias -> logits [..., V]"""
    cp = root + "cls.predictions."
    t = _ln(sd, cp + "transform.LayerNorm", _rnd(F.gelu(_lin(sd, cp + "transform.dense", x)), round_to), round_to)
    return t @ sd[root + "bert.embeddings.word_embeddings.weight"].t() + sd[cp + "bias"]


def logits(sd, ys, ylens=None, heads=2, causal=False, round_to=None, root=ROOT):
    """ys int64 [B, N] -> [B, max(ylens), V]; ylens None: no mask, every position is a key"""
    if ylens is not None:
        ys = ys[:, : int(max(ylens))]
    return head(sd, hidden(sd, ys, ylens, heads, causal, round_to, root), round_to, root)


def loss(sd, ys, ylens, labels, heads=2, causal=False, round_to=None, root=ROOT):
    """mean cross-entropy over labels != -100"""
    lg = logits(sd, ys, ylens, heads, causal, round_to, root)
    labels = labels[:, : lg.shape[1]]
    return F.cross_entropy(lg.reshape(-1, lg.shape[-1]), labels.reshape(-1), ignore_index=-100)


def masked_logprobs(sd, ys, ylens, mask_id, heads=2, round_to=None, root=ROOT):
    """[B, N]: entry (b, i), i < ylens[b], is log p(ys[b, i] | ys[b, :ylens[b]] with position i replaced by mask_id); zeros elsewhere.
    Every sequence's copies run unpadded and unmasked, as the reference's score does."""
    out = torch.zeros(ys.shape, dtype=sd[root + "cls.predictions.bias"].dtype)
    for b, n in enumerate(int(v) for v in ylens):
        copies = ys[b, :n].repeat(n, 1)
        copies[torch.arange(n), torch.arange(n)] = mask_id
        rows = hidden(sd, copies, None, heads, False, round_to, root)[torch.arange(n), torch.arange(n)]
        lp = torch.log_softmax(head(sd, rows, round_to, root), dim=-1)
        out[b, :n] = lp[torch.arange(n), ys[b, :n]]
    return out


def score(sd, ys, ylens, mask_id, heads=2, round_to=None, root=ROOT):
    """pseudo-log-likelihood per row"""
    return masked_logprobs(sd, ys, ylens, mask_id, heads, round_to, root).sum(dim=1).tolist()
