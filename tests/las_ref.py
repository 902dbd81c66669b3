"""The LAS decoder restated in plain torch, float64 by default (asr/modeling/decoders/las.py:22-343 is the model).

`attend_step` is ONE position of the location-aware attention with the keep mask of the weight dropout as an INPUT (the device
derives it from a counter hash; ops.las_dropmask exports it), `attend_step_grads` its gradients by autograd.  `decoder_forward` is
the whole teacher-forced decoder with the losses.  tests/test_las_cpu.py holds all of it to the reference's goldens; the kernel,
dropout and bf16 tests use it as their yardstick.  `rnd` (decoder_forward) rounds what the device keeps in its compute dtype, to
simulate bf16 storage on the CPU.
"""
import torch
import torch.nn.functional as F

from oracle.decoder import label_smoothing_loss
from oracle.distill import distill_loss
from oracle.model import ctc_loss

CONV_CHANNELS, CONV_WIDTH = 10, 201


def location_features(aw_prev, filt):
    """Conv1d(1, 10, 201, padding 100, no bias) as a cross-correlation: aw_prev [B,T], filt [10,1,201] -> [B,T,10]"""
    half = (CONV_WIDTH - 1) // 2
    win = F.pad(aw_prev, (half, half)).unfold(1, CONV_WIDTH, 1)       # [B,T,201]: win[b,t,k] = aw_prev[b, t + k - 100]
    return win @ filt.reshape(CONV_CHANNELS, CONV_WIDTH).t()


def attend_step(pk, pq, aw_prev, eouts, elens, filt, w_conv, b_conv, w_score, keep=None, p=0.0):
    """pk [B,T,A] = W_key eouts + b, pq [B,A] = W_query q + b, aw_prev [B,T] | None, elens [B] | None, keep [B,T] (0 / 1) | None
    -> (awd [B,T] the dropped weights, ctx [B,D])"""
    B, T, _ = pk.shape
    if aw_prev is None:
        aw_prev = pk.new_zeros(B, T)
    feat = location_features(aw_prev, filt)
    e = torch.tanh(pk + pq[:, None, :] + feat @ w_conv.t() + b_conv) @ w_score.reshape(-1)
    if elens is not None:
        pad = torch.arange(T)[None, :] >= torch.as_tensor(elens)[:, None]
        e = e.masked_fill(pad, torch.finfo(e.dtype).min)
    aw = torch.softmax(e, dim=1)
    awd = aw if keep is None else aw * keep.to(aw.dtype) / (1.0 - p)
    return awd, (awd[:, :, None] * eouts).sum(1)


STEP_INPUTS = ("pk", "pq", "aw_prev", "eouts", "filt", "w_conv", "b_conv", "w_score")


def attend_step_grads(t, elens, dctx, daw, keep=None, p=0.0):
    """t: dict of STEP_INPUTS (aw_prev may be None); the gradients of sum(ctx * dctx) + sum(awd * daw) w.r.t. every input
    -> (awd, ctx, {name: gradient})"""
    leaf = {k: (None if v is None else v.detach().clone().requires_grad_(True)) for k, v in t.items()}
    awd, ctx = attend_step(leaf["pk"], leaf["pq"], leaf["aw_prev"], leaf["eouts"], elens, leaf["filt"], leaf["w_conv"],
                           leaf["b_conv"], leaf["w_score"], keep, p)
    obj = (ctx * dctx).sum()
    if daw is not None:
        obj = obj + (awd * daw).sum()
    obj.backward()
    return awd.detach(), ctx.detach(), {k: v.grad for k, v in leaf.items() if v is not None}


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    i, f, g, o = (x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh).chunk(4, dim=-1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def decoder_forward(sd, cfg, eouts, elens, ys, ylens, ys_in, ys_out, soft=None, keeps=None, p_attn=0.0, rnd=None,
                    prefix="decoder"):
    """LASDecoder.forward with dropout_dec_rate = 0.  keeps: [L][B,T] keep masks of the attention weights | None.
    rnd: callable rounding a tensor to the device's storage dtype | None.  -> dict(loss_total, loss_att, loss_ctc[, loss_kd], logits)"""
    r = (lambda x: x) if rnd is None else rnd
    P = lambda n: sd[prefix + "." + n]
    Wm = lambda n: r(P(n))       # matrices are read from the compute-dtype shadow; biases and the attention's small tensors from f32
    B, T, D = eouts.shape
    L = ys_in.shape[1]
    H, NL = cfg.dec_hidden_size, cfg.dec_num_layers
    eouts = r(eouts)
    emb = r(Wm("embed.weight")[ys_in])                                         # [B,L,E]
    pk = r(eouts @ Wm("score.w_key.weight").t() + P("score.w_key.bias"))
    h = [eouts.new_zeros(B, H) for _ in range(NL)]
    c = [eouts.new_zeros(B, H) for _ in range(NL)]
    ctx, aw, gen = eouts.new_zeros(B, D), None, []
    for i in range(L):
        x = torch.cat([emb[:, i], ctx], dim=-1)
        for l in range(NL):
            h[l], c[l] = lstm_cell(x, h[l], c[l], Wm(f"rnns.{l}.weight_ih"), Wm(f"rnns.{l}.weight_hh"), P(f"rnns.{l}.bias_ih"),
                                   P(f"rnns.{l}.bias_hh"))
            h[l] = r(h[l])
            x = h[l]
        pq = r(h[0] @ Wm("score.w_query.weight").t() + P("score.w_query.bias"))
        aw, ctx = attend_step(pk, pq, aw, eouts, elens, P("score.conv.weight"), P("score.w_conv.weight"), P("score.w_conv.bias"),
                              P("score.w_score.weight"), None if keeps is None else keeps[i], p_attn)
        ctx = r(ctx)
        gen.append(r(torch.tanh(torch.cat([ctx, h[NL - 1]], dim=-1) @ Wm("intermed.weight").t() + P("intermed.bias"))))
    logits = r(torch.stack(gen, dim=1) @ Wm("output.weight").t() + P("output.bias"))
    out = {"logits": logits}
    n1 = torch.as_tensor(ylens) + 1
    args = dict(normalize_length=cfg.loss_normalize_length, normalize_batch=cfg.loss_normalize_batch)
    if soft is not None and cfg.kd_weight > 0:
        loss, out["loss_kd"], out["loss_att"] = distill_loss(logits, ys_out, soft, n1, cfg.kd_weight, cfg.lsm_prob, **args)
    else:
        loss = out["loss_att"] = label_smoothing_loss(logits, ys_out, n1, cfg.vocab_size, cfg.lsm_prob, **args)
    if cfg.mtl_ctc_weight > 0:
        ctc_logits = eouts @ Wm("ctc.output.weight").t() + P("ctc.output.bias")
        out["loss_ctc"] = ctc_loss(ctc_logits, ys, torch.as_tensor(elens), torch.as_tensor(ylens), cfg.blank_id)
        loss = loss + cfg.mtl_ctc_weight * out["loss_ctc"]
    out["loss_total"] = loss
    return out


def valid_positions(ylens, L):
    """bool [B,L]: the positions below ylens + 1 (where the logits are specified)"""
    return torch.arange(L)[None, :] < (torch.as_tensor(ylens) + 1)[:, None]


# ---- the fixture and the seeded cases the CPU and GPU tests share -------------------------------------------------------------
def load_las_golden():
    """tests/golden/las_tiny*.npz -> (decoder config dict, state dict {"decoder.*"}, all arrays as tensors)"""
    import json

    from tests.util import golden_npz
    z = golden_npz("las_tiny")
    cfg = json.loads(bytes(z.pop("config")).decode())
    g = {k: torch.from_numpy(v) for k, v in z.items()}
    return cfg, {k[3:]: v for k, v in g.items() if k.startswith("sd/")}, g


def las_asr_config(cfg):
    """the l3_tiny encoder under the fixture's LAS decoder"""
    from tests.util import CONFIGS
    return dict(CONFIGS["l3_tiny"], **cfg, decoder_type="las")


KERNEL_T = (1, 37, 211)
KERNEL_B, KERNEL_A, KERNEL_D = 3, 80, 128


def kernel_case(T, ragged, dtype=torch.float64):
    """seeded operands of one attention step at B=3, A=80, D=128 -> (dict of STEP_INPUTS, elens | None, dctx, daw)"""
    g = torch.Generator().manual_seed(1000 + T + (7 if ragged else 0))
    B, A, D = KERNEL_B, KERNEL_A, KERNEL_D
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    t = dict(pk=rn(B, T, A), pq=rn(B, A), aw_prev=torch.softmax(2.0 * rn(B, T), dim=1), eouts=rn(B, T, D),
             filt=0.3 * rn(CONV_CHANNELS, 1, CONV_WIDTH), w_conv=0.5 * rn(A, CONV_CHANNELS), b_conv=0.1 * rn(A), w_score=rn(1, A))
    elens = None
    if ragged:
        elens = torch.tensor([T, max(1, T // 2), max(1, (2 * T) // 3)])
        for b in range(B):   # the previous weights of a padded row live on its frames only
            t["aw_prev"][b, elens[b]:] = 0.0
            t["aw_prev"][b] /= t["aw_prev"][b].sum()
    return {k: v.to(dtype) for k, v in t.items()}, elens, rn(B, D).to(dtype), 0.5 * rn(B, T).to(dtype)


GRAD_OF = {"dpk": "pk", "dpq": "pq", "daw_prev": "aw_prev", "deouts": "eouts", "dfilt": "filt", "dw_conv": "w_conv", "db_conv": "b_conv",
           "dw_score": "w_score"}


def step_errors(got, want):
    """largest |difference| of every tensor in units of the case's largest reference magnitude over ALL outputs and gradients
    -> {name: error}.  (One scale per case, not one per tensor: at T = 1 the soft-max is constant, every gradient behind it
    vanishes identically, and what a device computes there is the rounding of two sums that cancel -- an error that has the
    scale of the step's other gradients and none of its own.)"""
    gmax = max(w.abs().max().item() for w in want.values())
    return {k: ((got[k].double().reshape(-1) - w.double().reshape(-1)).abs().max() / gmax).item() for k, w in want.items()}


def step_in_dtype(T, ragged, dtype, keep=None, p=0.0):
    """the restatement's own step (outputs and all gradients) computed in `dtype` on the CPU -> {name: tensor}"""
    t, elens, dctx, daw = kernel_case(T, ragged, dtype)
    awd, ctx, grads = attend_step_grads(t, elens, dctx, daw, keep, p)
    out = {"aw": awd, "ctx": ctx}
    out.update({k: grads[v] for k, v in GRAD_OF.items()})
    return out
