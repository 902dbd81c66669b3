"""A small torch restatement of ELECTRA (lm_type="electra"), written from its behaviour: two post-LN BERT stacks over word +
position + token-type(0) embeddings held at embedding_size, a Linear embedding_size -> hidden_size after them where the two sizes
differ, no pooler.  Generator head: dense(hidden -> embedding), GELU, LayerNorm(eps 1e-5), projection tied to the generator's word
embedding + its own bias; cross-entropy (mean) over labels != -100.  Discriminator head: dense(hidden -> hidden), GELU,
dense_prediction(hidden -> 1); BCE-with-logits (mean) over the positions n < ylens[b].  The state-dict keys are the model's
(`lm.gmodel.*`, `lm.dmodel.*`), any float dtype (f64 for references), autograd for the gradients.  No dropout, and no sampling: the
generated ids are an argument.

`round_to` simulates a low-precision run on the CPU as tests/bert_ref.py does: every activation the HIP path stores in the compute
dtype is rounded to it; the weights are the caller's to round."""
import math

import torch
import torch.nn.functional as F

from tests.bert_ref import _lin, _rnd

G, D = "lm.gmodel.", "lm.dmodel."


def _ln(sd, name, x, round_to, eps=1e-12):
    return _rnd(F.layer_norm(x, x.shape[-1:], sd[name + ".weight"], sd[name + ".bias"], eps), round_to)


def hidden(sd, root, ys, ylens, heads, round_to=None):
    """ys int64 [B, N] (already trimmed) -> last hidden state [B, N, hidden] of the stack under `root` (G or D)"""
    pre = root + "electra."
    B, N = ys.shape
    emb = pre + "embeddings."
    x = sd[emb + "word_embeddings.weight"][ys] + sd[emb + "position_embeddings.weight"][:N] + sd[emb + "token_type_embeddings.weight"][0]
    x = _ln(sd, emb + "LayerNorm", _rnd(x, round_to), round_to)
    if pre + "embeddings_project.weight" in sd:
        x = _lin(sd, pre + "embeddings_project", x, round_to)
    d = x.shape[-1]
    dk = d // heads
    allowed = torch.ones(B, 1, N, N, dtype=torch.bool)
    if ylens is not None:
        allowed = allowed & (torch.arange(N)[None, :] < torch.as_tensor(ylens)[:, None])[:, None, None, :]
    n_layers = sum(1 for k in sd if k.startswith(pre + "encoder.layer.") and k.endswith("attention.self.query.weight"))
    for i in range(n_layers):
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


def gen_logits(sd, ys, ylens, heads=1, round_to=None):
    x = hidden(sd, G, ys, ylens, heads, round_to)
    t = _rnd(F.gelu(_lin(sd, G + "generator_predictions.dense", x)), round_to)
    t = _ln(sd, G + "generator_predictions.LayerNorm", t, round_to, 1e-5)
    return t @ sd[G + "electra.embeddings.word_embeddings.weight"].t() + sd[G + "generator_lm_head.bias"]


def gen_loss(sd, ys, ylens, labels, heads=1, round_to=None):
    lg = gen_logits(sd, ys, ylens, heads, round_to)
    return F.cross_entropy(lg.reshape(-1, lg.shape[-1]), labels.reshape(-1), ignore_index=-100)


def disc_logits(sd, ys, ylens, heads=2, round_to=None):
    """[B, N] logits of "this token was replaced" """
    x = hidden(sd, D, ys, ylens, heads, round_to)
    h = _rnd(F.gelu(_lin(sd, D + "discriminator_predictions.dense", x)), round_to)
    return _lin(sd, D + "discriminator_predictions.dense_prediction", h).squeeze(-1)


def disc_loss(sd, ys, ylens, targets, heads=2, round_to=None):
    """BCE-with-logits, mean over n < ylens[b] (every position without ylens); targets [B, N], anything where n >= ylens[b]"""
    z = disc_logits(sd, ys, ylens, heads, round_to)
    active = torch.ones_like(ys, dtype=torch.bool) if ylens is None else torch.arange(ys.shape[1])[None, :] < torch.as_tensor(ylens)[:, None]
    return F.binary_cross_entropy_with_logits(z[active], targets[active].to(z.dtype))


def corrupt(ys_in, labels, sample_ids):
    """-> (generated ids, labels_replaced int64): samples at the masked positions; replaced <=> not the token the mask hid"""
    masked = labels != -100
    generated, original = ys_in.clone(), ys_in.clone()
    original[masked] = labels[masked]
    generated[masked] = sample_ids[masked]
    return generated, (generated != original).long()


def loss(sd, ys_in, ylens, labels, sample_ids, disc_weight, gen_heads=1, disc_heads=2, round_to=None):
    """-> (total, loss_gen, loss_disc, num_replaced / B, num_masked / B) with the given samples"""
    n = ys_in.shape[1] if ylens is None else int(max(ylens))
    ys_in, labels, sample_ids = ys_in[:, :n], labels[:, :n], sample_ids[:, :n]
    lg = gen_loss(sd, ys_in, ylens, labels, gen_heads, round_to)
    generated, replaced = corrupt(ys_in, labels, sample_ids)
    ld = disc_loss(sd, generated, ylens, replaced, disc_heads, round_to)
    B = ys_in.shape[0]
    return lg + disc_weight * ld, lg, ld, replaced.sum().item() / B, (labels != -100).sum().item() / B


def token_probs(sd, ys, ylens, heads=2, round_to=None):
    """sigmoid of the discriminator's logits [B, N]"""
    return torch.sigmoid(disc_logits(sd, ys, ylens, heads, round_to))


def score(sd, ys, ylens, heads=2, round_to=None):
    """the reference's N-best score with its sign quirk: one row -> [+sum over all N], several -> -sum over n < ylens[b] per row"""
    p = token_probs(sd, ys, ylens, heads, round_to)
    if ys.shape[0] == 1:
        return [p.sum().item()]
    return [-p[b, : int(n)].sum().item() for b, n in enumerate(ylens)]
