"""A small torch restatement of the RNN LM (embedding -> stacked LSTM, gate order i | f | g | o -> linear head), written from its
behaviour: the same state-dict keys as the model (`lm.embed.weight`, `lm.rnns.{weight,bias}_{ih,hh}_l{k}`, `lm.output.{weight,bias}`),
any float dtype (f64 for the kernel sweeps), autograd for the gradients.  No dropout: the fixtures and the tests run without it.

`round_to` simulates a low-precision run on the CPU: h is rounded to that dtype after every cell (the weights are the caller's to
round).  Summation order and the rounding of the gate pre-activations are NOT simulated."""
import torch


def _rnd(x, round_to):
    return x if round_to is None else x.to(round_to).to(x.dtype)


def num_layers(sd):
    return sum(1 for k in sd if k.startswith("lm.rnns.weight_ih_l"))


def lstm_stack(sd, x, states=None, round_to=None):
    """x [B, N, E]; states (h, c) each [L, B, H] or None -> (top layer's h [B, N, H], (h', c') after the last position)"""
    B, N, _ = x.shape
    L = num_layers(sd)
    hs, cs = [], []
    for l in range(L):
        w_ih, w_hh = sd[f"lm.rnns.weight_ih_l{l}"], sd[f"lm.rnns.weight_hh_l{l}"]
        b = sd[f"lm.rnns.bias_ih_l{l}"] + sd[f"lm.rnns.bias_hh_l{l}"]
        H = w_hh.shape[1]
        h = x.new_zeros(B, H) if states is None else states[0][l].to(x.dtype)
        c = x.new_zeros(B, H) if states is None else states[1][l].to(x.dtype)
        outs = []
        for n in range(N):
            i, f, g, o = (x[:, n] @ w_ih.t() + h @ w_hh.t() + b).chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = _rnd(torch.sigmoid(o) * torch.tanh(c), round_to)
            outs.append(h)
        x = torch.stack(outs, dim=1)
        hs.append(h)
        cs.append(c)
    return x, (torch.stack(hs), torch.stack(cs))


def logits(sd, ys, ylens=None, round_to=None):
    """ys int64 [B, N] -> [B, max(ylens), V]"""
    if ylens is not None:
        ys = ys[:, : int(max(ylens))]
    out, _ = lstm_stack(sd, sd["lm.embed.weight"][ys], None, round_to)
    return out @ sd["lm.output.weight"].t() + sd["lm.output.bias"]


def loss(sd, ys, ylens, labels, round_to=None):
    """mean cross-entropy over labels != -100"""
    lg = logits(sd, ys, ylens, round_to)
    if ylens is not None:
        labels = labels[:, : int(max(ylens))]
    return torch.nn.functional.cross_entropy(lg.reshape(-1, lg.shape[-1]), labels.reshape(-1), ignore_index=-100)


def predict(sd, ys, ylens, states=None):
    """one step: reads ys[b, ylens[b] - 1] only -> (log-probabilities [B, V], (h', c'))"""
    last = torch.stack([ys[b, int(n) - 1] for b, n in enumerate(ylens)])
    out, states = lstm_stack(sd, sd["lm.embed.weight"][last].unsqueeze(1), states)
    lg = out[:, 0] @ sd["lm.output.weight"].t() + sd["lm.output.bias"]
    return torch.log_softmax(lg, dim=-1), states


def token_logprobs(sd, ys, ylens, labels, round_to=None):
    """log p(labels[b, i] | ys[b, :i+1]) where labels != -100, zeros elsewhere -> [B, N]"""
    lp = torch.log_softmax(logits(sd, ys, ylens, round_to), dim=-1)
    labels = labels[:, : lp.shape[1]]
    valid = labels != -100
    return lp.gather(2, labels.clamp(min=0).unsqueeze(2)).squeeze(2) * valid


def score(sd, ys, ylens):
    """per row sum_{i < ylens[b] - 1} log p(ys[b, i+1] | ys[b, :i+1])"""
    labels = torch.full_like(ys, -100)
    for b, n in enumerate(ylens):
        labels[b, : int(n) - 1] = ys[b, 1:int(n)]
    return token_logprobs(sd, ys, ylens, labels).sum(dim=1).tolist()


def random_state(V, E, H, L, seed, dtype=torch.float64, out_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    sd = {"lm.embed.weight": torch.randn(V, E, generator=g, dtype=dtype)}
    for l in range(L):
        nin = E if l == 0 else H
        sd[f"lm.rnns.weight_ih_l{l}"] = torch.randn(4 * H, nin, generator=g, dtype=dtype) / nin ** 0.5
        sd[f"lm.rnns.weight_hh_l{l}"] = torch.randn(4 * H, H, generator=g, dtype=dtype) / H ** 0.5
        sd[f"lm.rnns.bias_ih_l{l}"] = 0.1 * torch.randn(4 * H, generator=g, dtype=dtype)
        sd[f"lm.rnns.bias_hh_l{l}"] = 0.1 * torch.randn(4 * H, generator=g, dtype=dtype)
    sd["lm.output.weight"] = out_scale * torch.randn(V, H, generator=g, dtype=dtype) / H ** 0.5
    sd["lm.output.bias"] = 0.1 * torch.randn(V, generator=g, dtype=dtype)
    return sd
