"""The RNN LM (lm_type="rnn") on the HIP path: training, the stateful step and scoring, against the reference's outputs
(tests/golden/rnnlm_tiny, rnnlm_tiny_trace: tests/golden/make_golden_rnnlm.py; the reference ran with every dropout at 0) and
against the f64 restatement tests/rnnlm_ref.py.

Bars of the golden cases are those of tests/test_lm_train_gpu.py: logits 1e-3 / 6e-2 of range, loss 1e-3 / 2e-2 relative, f32
gradients 5e-3 in the max-error form and per-tensor cosine >= 0.9999, bf16 cosine > 0.98, trace parameters 2e-3 of range.
Bars of the shape sweeps: f32 1e-4 of range for the step (summation order only; the issue's bar for step = sequence), for bf16 the
suite's output bar 6e-2 of range (tests/test_rnn_encoder_gpu.py:180); sequence path: loss 1e-3 / 2e-2 (test_rnn_encoder_gpu.py:160),
f32 gradients 1e-3 in the max-error form with the 1e-4 floor (test_rnn_encoder_gpu.py:172-173), bf16 gradients cosine > 0.98
above that floor (test_rnn_encoder_gpu.py:175); fused against materialised head 2e-2 (tests/test_ce_head_gpu.py:127)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnnlm_ref as ref
from tests.rnnlm_util import (PREDICT_STEPS, PREDICT_YLENS, RNNLM_CFG, RNNLM_TRAIN_CFG, TRACE_TOTAL_STEPS, rnnlm_golden,
                              rnnlm_state)

pytestmark = pytest.mark.gpu
L_ = RNNLM_CFG["num_layers"]


def _build(dtype, dev, train=False, dropout=0.0, cfg=RNNLM_CFG, sd=None):
    from emoasr_amd.modeling.lm import LM
    lm = LM(SimpleNamespace(**cfg), compute_dtype=dtype)
    lm.load_state_dict(rnnlm_state(rnnlm_golden()) if sd is None else {k: v.float() for k, v in sd.items()})
    lm = lm.to(dev)
    lm.dropout_rate = dropout
    return lm.train() if train else lm.eval()


def _rel(a, b):
    return ((a.double().cpu() - b.double()).abs().max() / (b.double().abs().max() + 1e-12)).item()


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten().double().cpu(), b.flatten().double(), dim=0).item()


# ---- 1. the golden: logits, loss and gradients, the three-step trace ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_logits(dev, dtype):
    g = rnnlm_golden()
    lm = _build(dtype, dev)
    logits = lm(g["ys_in"], g["ylens"])
    assert logits.shape == g["eval/logits"].shape and logits.dtype == torch.float32
    err = _rel(logits, g["eval/logits"])
    print(f"logits {dtype}: {err:.3e} of range")
    assert err < (1e-3 if dtype == torch.float32 else 6e-2), err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, "f32x3"], ids=["f32", "bf16", "f32x3"])
def test_train_loss_and_grads(dev, dtype):
    g = rnnlm_golden()
    lm = _build(dtype, dev, train=True)
    loss, ld = lm(g["ys_in"], g["ylens"], g["labels"])
    assert set(ld) == {"loss_total"} and ld["loss_total"] is loss
    loss.backward()
    ref_loss = g["train/loss"].item()
    ltol = 2e-2 if dtype == torch.bfloat16 else 1e-3
    print(f"loss {dtype}: {loss.item():.6f} against {ref_loss:.6f}")
    assert abs(loss.item() - ref_loss) < ltol * abs(ref_loss), (loss.item(), ref_loss)
    grads = dict(lm.named_parameters())
    for l in range(L_):
        assert torch.equal(grads[f"lm.rnns.bias_ih_l{l}"].grad, grads[f"lm.rnns.bias_hh_l{l}"].grad), l
    gmax = max(g[k].abs().max().item() for k in g if k.startswith("grad/"))
    worst, worst_name, cos_min, cos_name = 0.0, None, 1.0, None
    for n, p in grads.items():
        want, got = g["grad/" + n], p.grad.float().cpu()
        assert torch.isfinite(got).all(), n
        err = ((got - want).abs().max() / max(want.abs().max().item(), 1e-2 * gmax)).item()
        if err > worst:
            worst, worst_name = err, n
        cos = _cos(got, want)
        if cos < cos_min:
            cos_min, cos_name = cos, n
    print(f"grads {dtype}: worst max-error {worst:.3e} ({worst_name}), min cosine {cos_min:.8f} ({cos_name})")
    if dtype == torch.bfloat16:
        assert cos_min > 0.98, (cos_min, cos_name, worst, worst_name)
    elif dtype == torch.float32:
        assert worst < 5e-3, (worst, worst_name)
        assert cos_min >= 0.9999, (cos_min, cos_name)
    else:
        assert math.isfinite(worst) and math.isfinite(cos_min)      # "f32x3" must run; its accuracy is not under test here


def test_three_step_trace(dev):
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    g, t = rnnlm_golden(), rnnlm_golden("rnnlm_tiny_trace")
    params = SimpleNamespace(**RNNLM_TRAIN_CFG)
    lm = _build(torch.float32, dev, train=True)
    groups = get_optimizer_params_nodecay(list(lm.named_parameters()), weight_decay=params.weight_decay)
    name_of = {id(p): n for n, p in lm.named_parameters()}
    assert [name_of[id(p)] for p in groups[0]["params"]] == g["nodecay/decay"].tolist()
    assert [name_of[id(p)] for p in groups[1]["params"]] == g["nodecay/nodecay"].tolist()
    opt = ScheduledOptimizer(AdamW(groups, lr=0, weight_decay=params.weight_decay), params, num_total_steps=TRACE_TOTAL_STEPS)
    losses, lrs = [], []
    for k in range(3):
        batch = {"ys_in": t[f"ys_in{k}"], "ylens": t["ylens"], "labels": t[f"labels{k}"]}
        losses.append(train_step(lm, opt, batch, params, dev)["loss_total"])
        lrs.append(opt._lr)
    assert t["grad_norms"].min().item() > params.clip_grad_norm      # the clip bit at every step of the reference's run
    assert np.allclose(lrs, t["lrs"].numpy(), rtol=1e-12, atol=0), lrs
    rel = np.abs(np.array(losses) - t["losses"].numpy()) / t["losses"].numpy()
    print("trace losses", losses, "relative error", rel)
    assert rel.max() < 1e-3, rel
    worst = 0.0
    for n, p in lm.named_parameters():
        want = t["param/" + n]
        err = (p.detach().cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        worst = max(worst, err)
        assert err < 2e-3, (n, err)
    print(f"trace final parameters: worst {worst:.3e} of range")


# ---- 2. dropout ---------------------------------------------------------------------------------------------------------------------
def test_dropout_defaults_and_eval(dev):
    from emoasr_amd.modeling.lm import LM
    g = rnnlm_golden()
    lm = LM(SimpleNamespace(**RNNLM_CFG), compute_dtype=torch.float32)
    lm.load_state_dict(rnnlm_state(g))
    lm = lm.to(dev).train()
    assert lm.dropout_rate == RNNLM_CFG["dropout_rate"] == 0.1
    want = g["train/loss"].item()
    with torch.no_grad():
        a = lm(g["ys_in"], g["ylens"], g["labels"])[0].item()
        b = lm(g["ys_in"], g["ylens"], g["labels"])[0].item()
    assert a != b and abs(a - want) > 1e-4 * want and abs(a - want) < 0.5 * want, (a, b, want)
    loss, _ = lm(g["ys_in"], g["ylens"], g["labels"])
    loss.backward()
    assert all(torch.isfinite(p.grad).all() for p in lm.parameters())
    lm.eval()
    with torch.no_grad():
        c = lm(g["ys_in"], g["ylens"], g["labels"])[0].item()
        d = lm(g["ys_in"], g["ylens"], g["labels"])[0].item()
    assert c == d and abs(c - want) < 1e-3 * want, (c, d, want)


def test_dropout_backward_uses_the_forward_masks(dev):
    """f32, dropout 0.1 at all sites, the step counter pinned: the central difference of the loss along the normalised gradient equals
    the gradient's norm (bar and reasoning of tests/test_lm_train_gpu.py::test_dropout_backward_uses_the_forward_masks)"""
    g = rnnlm_golden()
    lm = _build(torch.float32, dev, train=True, dropout=0.1)

    def loss_at():
        lm.step_count = 7
        return lm(g["ys_in"], g["ylens"], g["labels"])[0]

    loss_at().backward()
    A = lm._arena
    direction = A.grad.clone()
    norm = direction.norm().item()
    assert norm >= 0.05, norm
    direction /= norm
    eps = 1e-2
    with torch.no_grad():
        A.flat.add_(direction, alpha=eps)
        up = loss_at().item()
        A.flat.add_(direction, alpha=-2 * eps)
        down = loss_at().item()
        A.flat.add_(direction, alpha=eps)
    fd = (up - down) / (2 * eps)
    print(f"dropout 0.1: |g| {norm:.6f}, central difference {fd:.6f}")
    assert abs(fd - norm) < 1e-2 * norm, (fd, norm)


# ---- 3. the predict chain of the golden ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [True, False], ids=["kernel", "chain"])
def test_predict_chain(dev, kernel):
    g = rnnlm_golden()
    lm = _build(torch.float32, dev)
    lm.step_kernel = kernel
    ys = g["predict/ys"]
    states = None
    for k in range(PREDICT_STEPS):
        lp, states = lm.predict(ys, PREDICT_YLENS[k], states)
        assert lm.last_step == ("kernel" if kernel else "chain")
        assert lp.dtype == torch.float32 and tuple(lp.shape) == (3, RNNLM_CFG["vocab_size"])
        errs = (_rel(lp, g[f"predict/{k}/logp"]), _rel(states[0], g[f"predict/{k}/h"]), _rel(states[1], g[f"predict/{k}/c"]))
        print(f"predict step {k}: log-probs / h / c {errs} of range")
        assert max(errs) < 1e-3, (k, errs)
        # the state tensors slice and join as the reference's search code does
        states = tuple(torch.cat([s[:, b:b + 1] for b in range(3)], dim=1) for s in states)
    # states=None is the zero state; only ys[b, ylens[b] - 1] is read
    a, sa = lm.predict(ys, PREDICT_YLENS[2])
    b, sb = lm.predict(ys, PREDICT_YLENS[2], lm.zero_states(3, dev))
    assert torch.equal(a, b) and torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1])
    other = ys.clone()
    for r, n in enumerate(PREDICT_YLENS[2]):
        other[r, : n - 1] = (other[r, : n - 1] + 5) % 37 + 3
        other[r, n:] = 3
    c, sc = lm.predict(other, PREDICT_YLENS[2])
    assert torch.equal(a, c) and torch.equal(sa[0], sc[0]) and torch.equal(sa[1], sc[1])


# ---- 4. N chained steps reproduce forward() -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [True, False], ids=["kernel", "chain"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_steps_equal_the_sequence(dev, dtype, kernel):
    g = rnnlm_golden()
    lm = _build(dtype, dev)
    lm.step_kernel = kernel
    N = 9
    ys = g["ys_in"][:3, :N]
    want = torch.log_softmax(lm(ys, [N] * 3).cpu(), dim=-1)
    states = None
    rng = want.abs().max().item()
    for n in range(N):
        lp, states = lm.predict(ys, [n + 1] * 3, states)
        err = (lp.cpu() - want[:, n]).abs().max().item() / rng
        if dtype == torch.float32:
            assert err < 1e-4, (n, err)
        else:
            assert err < 6e-2, (n, err)
            assert torch.equal(lp.cpu().argmax(dim=-1), want[:, n].argmax(dim=-1)), n
    print(f"step = sequence {dtype} {'kernel' if kernel else 'chain'}: last position {err:.3e} of range")


# ---- 5. the step, edge shapes and index lists, against f64 on the CPU ---------------------------------------------------------------
STEP_SHAPES = [(1, 1, 32, 32, 40), (5, 2, 48, 64, 40), (16, 2, 64, 96, 40), (17, 3, 40, 64, 1000), (32, 2, 64, 64, 40)]


@pytest.mark.parametrize("kernel", [True, False], ids=["kernel", "chain"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=["x".join(map(str, s)) for s in STEP_SHAPES])
def test_step_edges(dev, shape, dtype, kernel):
    nb, L, E, H, V = shape
    cfg = dict(RNNLM_CFG, vocab_size=V, embedding_size=E, hidden_size=H, num_layers=L)
    sd64 = ref.random_state(V, E, H, L, seed=nb + H, out_scale=4.0)
    lm = _build(dtype, dev, cfg=cfg, sd=sd64)
    lm.step_kernel = kernel
    slots, rows = 2 * nb + 3, nb + 4
    pools = lm.new_pools(slots, rows)
    gen = torch.Generator().manual_seed(nb)
    pools.ph.copy_(torch.randn(L, slots, H, generator=gen).mul(0.5))
    pools.pc.copy_(torch.randn(L, slots, H, generator=gen))
    pools.logp.copy_(torch.randn(rows, V, generator=gen))
    ph0, pc0, lp0 = pools.ph.clone(), pools.pc.clone(), pools.logp.clone()
    # sources among the first nb + 1 slots (duplicates: children of one parent; some rows start from the zero state), destinations a
    # permutation of the upper slots, rows scattered into the larger cache
    src = torch.randint(0, nb + 1, (nb,), generator=gen)
    src[:: 3] = src[0]
    if nb > 2:
        src[1::4] = -1
    dst = (nb + 1 + torch.randperm(nb + 2, generator=gen)[:nb])
    row_dst = torch.randperm(rows, generator=gen)[:nb]
    ids = torch.randint(0, V, (nb,), generator=gen)
    to_dev = lambda t: t.to(torch.int32).to(dev)
    lm.step(pools, nb, to_dev(ids), to_dev(src), to_dev(dst), to_dev(row_dst))
    assert lm.last_step == ("kernel" if kernel else "chain")
    # f64 on the CPU from what the device holds: compute-dtype weights and states
    A = lm._arena
    sdr = {n: (A.p(n) if "bias" in n else A.w(n)).detach().double().cpu() for n in sd64}
    live = (src >= 0).double().view(1, nb, 1)
    h_in = ph0.double().cpu()[:, src.clamp(min=0)] * live
    c_in = pc0.double().cpu()[:, src.clamp(min=0)] * live
    want_lp, (want_h, want_c) = ref.predict(sdr, ids.view(nb, 1), [1] * nb, (h_in, c_in))
    tol = 1e-4 if dtype == torch.float32 else 6e-2
    errs = (_rel(pools.logp[row_dst.to(dev)], want_lp), _rel(pools.ph[:, dst.to(dev)], want_h), _rel(pools.pc[:, dst.to(dev)], want_c))
    print(f"step {shape} {dtype} {'kernel' if kernel else 'chain'}: log-probs / h / c {errs} of range")
    assert max(errs) < tol, errs
    # what the call did not address is bit-unchanged
    keep = torch.ones(slots, dtype=torch.bool)
    keep[dst] = False
    assert torch.equal(pools.ph[:, keep.to(dev)], ph0[:, keep.to(dev)]) and torch.equal(pools.pc[:, keep.to(dev)], pc0[:, keep.to(dev)])
    keep = torch.ones(rows, dtype=torch.bool)
    keep[row_dst] = False
    assert torch.equal(pools.logp[keep.to(dev)], lp0[keep.to(dev)])
    # without row_dst row i goes to row i, the rows beyond nb stay
    pools.logp.copy_(lp0)
    pools.ph.copy_(ph0)
    pools.pc.copy_(pc0)
    lm.step(pools, nb, to_dev(ids), to_dev(src), to_dev(dst))
    assert _rel(pools.logp[:nb], want_lp) < tol and torch.equal(pools.logp[nb:], lp0[nb:])


def test_step_kernel_takes_the_shapes_it_should(dev):
    from emoasr_amd import ops
    bf, f32 = torch.empty(0, device=dev, dtype=torch.bfloat16), torch.empty(0, device=dev)
    assert ops.rnnlm_step_supported(bf, 32, 2, 512, 512) and ops.rnnlm_step_supported(f32, 32, 2, 512, 512)
    assert not ops.rnnlm_step_supported(bf, 33, 2, 512, 512) and not ops.rnnlm_step_supported(bf, 0, 2, 512, 512)
    assert not ops.rnnlm_step_supported(bf, 4, 2, 36, 64) and not ops.rnnlm_step_supported(f32, 4, 2, 64, 36)


def test_more_than_32_rows_run_in_chunks(dev):
    g = rnnlm_golden()
    lm = _build(torch.float32, dev)
    ys = torch.randint(3, 40, (40, 1), generator=torch.Generator().manual_seed(3))
    lm.step_kernel = True
    a, sa = lm.predict(ys, [1] * 40)
    assert lm.last_step == "kernel"
    want, (wh, wc) = ref.predict({k: v.double() for k, v in rnnlm_state(g).items()}, ys, [1] * 40)
    assert _rel(a, want) < 1e-4 and _rel(sa[0], wh) < 1e-4 and _rel(sa[1], wc) < 1e-4


# ---- 6. the sequence path in the LM's layout ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N", [1, 2, 17])
@pytest.mark.parametrize("B", [1, 6, 65])
def test_sequence_loss_and_gradients(dev, B, N, dtype):
    """two 64-sequence groups (B = 65), the U = 1 chain (N = 1), the cooperative launch (bf16, N > 1); ragged labels"""
    V, E, H, L = 40, 32, 64, 2
    cfg = dict(RNNLM_CFG, vocab_size=V, embedding_size=E, hidden_size=H, num_layers=L)
    sd64 = ref.random_state(V, E, H, L, seed=100 * B + N, out_scale=4.0)
    lm = _build(dtype, dev, train=True, cfg=cfg, sd=sd64)
    gen = torch.Generator().manual_seed(B + N)
    ylens = torch.randint(1, N + 1, (B,), generator=gen)
    ylens[0] = N
    ys = torch.randint(0, V, (B, N), generator=gen)
    labels = torch.randint(0, V, (B, N), generator=gen)
    for b, n in enumerate(ylens.tolist()):
        labels[b, n:] = -100
    if N > 2:
        labels[0, 1] = -100
    loss, _ = lm(ys, ylens, labels)
    loss.backward()
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    want = ref.loss(sdr, ys, ylens, labels)
    want.backward()
    ltol = 1e-3 if dtype == torch.float32 else 2e-2
    assert abs(loss.item() - want.item()) < ltol * abs(want.item()), (loss.item(), want.item())
    gmax = max(p.grad.abs().max().item() for p in sdr.values())
    worst, cos_min = 0.0, 1.0
    for n, p in lm.named_parameters():
        w = sdr[n].grad
        if dtype == torch.float32:
            worst = max(worst, (p.grad.double().cpu() - w).abs().max().item() / max(w.abs().max().item(), 1e-4 * gmax))
        elif w.abs().max().item() >= 1e-4 * gmax:
            cos_min = min(cos_min, _cos(p.grad, w))
    print(f"sequence B={B} N={N} {dtype}: loss {loss.item():.6f} / {want.item():.6f}, worst {worst:.3e}, min cosine {cos_min:.6f}")
    assert worst < 1e-3 and cos_min > 0.98, (worst, cos_min)


# ---- 7. scoring ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_score_token_logprobs_and_perplexity(dev, dtype, tmp_path):
    from torch.utils.data import DataLoader
    from emoasr_amd.datasets import LMDataset
    from emoasr_amd.train_lm import ppl_lm
    g = rnnlm_golden()
    sd64 = {k: v.double() for k, v in rnnlm_state(g).items()}
    lm = _build(dtype, dev)
    tol = 1e-3 if dtype == torch.float32 else 6e-2      # per token, of the log-probabilities' range
    lp = lm.token_logprobs(g["ys_in"], g["ylens"], g["labels"])
    want = ref.token_logprobs(sd64, g["ys_in"], g["ylens"], g["labels"])
    assert lp.dtype == torch.float64 and lp.shape == want.shape and not lp[g["labels"] == -100].any()
    assert _rel(lp, want) < tol
    scores = lm.score(g["ys_in"], g["ylens"])
    wscores = ref.score(sd64, g["ys_in"], g["ylens"])
    assert isinstance(scores, list) and len(scores) == 6 and all(isinstance(s, float) for s in scores) and scores[-1] == 0.0
    ntok = sum(int(n) - 1 for n in g["ylens"])
    assert sum(abs(a - b) for a, b in zip(scores, wscores)) / ntok < tol * want.abs().max().item()
    assert lm.score(g["ys_in"], g["ylens"], batch_size=4) == pytest.approx(scores, abs=1e-4)
    path = tmp_path / "lm.tsv"
    path.write_text(str(g["tsv"]))
    for flag in (False, True):
        ds = LMDataset(SimpleNamespace(**dict(RNNLM_CFG, bucket_shuffle=False, add_sos_eos=flag, eos_id=2)), str(path), phase="test")
        cnt, ppl = ppl_lm(DataLoader(ds, batch_size=1, shuffle=False, collate_fn=ds.collate_fn), lm, dev, add_sos_eos=flag)
        total, n = 0.0, 0
        for i in range(len(ds)):
            y = ds[i][1].view(1, -1)
            lab = y[:, 1:].clone()
            if flag:
                lab[:, 0] = lab[:, -1] = -100
            total -= ref.token_logprobs(sd64, y[:, :-1], [y.shape[1] - 1], lab).sum().item()
            n += int((lab != -100).sum())
        wppl = math.exp(total / n)
        print(f"ppl {dtype} add_sos_eos={flag}: {cnt} tokens, {ppl:.5f} against {wppl:.5f}")
        assert cnt == n and abs(math.log(ppl) - math.log(wppl)) < tol * want.abs().max().item()


def test_fused_and_materialised_head_agree(dev):
    V, E, H, L, B, N = 256, 64, 64, 1, 64, 16
    cfg = dict(RNNLM_CFG, vocab_size=V, embedding_size=E, hidden_size=H, num_layers=L)
    lm = _build(torch.bfloat16, dev, train=True, cfg=cfg, sd=ref.random_state(V, E, H, L, seed=5, out_scale=4.0))
    gen = torch.Generator().manual_seed(9)
    ys, labels = torch.randint(0, V, (B, N), generator=gen), torch.randint(0, V, (B, N), generator=gen)
    out = {}
    for fused in (True, False):
        lm.fused_head = fused
        lm.zero_grad()
        loss, _ = lm(ys, [N] * B, labels)
        loss.backward()
        assert lm.last_head == ("fused" if fused else "materialised")
        out[fused] = (loss.item(), lm._arena.grad.clone())
    assert abs(out[True][0] - out[False][0]) < 2e-2 * abs(out[False][0])
    assert _cos(out[True][1], out[False][1].cpu()) > 0.98
