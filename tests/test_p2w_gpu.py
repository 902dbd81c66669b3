"""The phone-to-word models (emoasr_amd/modeling/p2w.py: lm_type "pbert" / "pctc") on the HIP engine against the reference's values
(tests/golden/p2w_tiny*.npz, written by tests/golden/make_golden_p2w.py).

Bars are those of tests/test_bert_gpu.py / tests/test_electra_gpu.py: loss 1e-3 (f32) / 2e-2 (bf16) relative, f32 gradients 5e-3 in the
max-error form with cosine >= 0.9999 per tensor, bf16 gradients cosine > 0.98 over the tensors above 1e-2 of the largest, f32 logits
1e-3 of their range, bf16 logits 4 x the CPU-simulated bf16 error (PBERT_LOGITS_BF16_SIM below)."""
from types import SimpleNamespace

import pytest
import torch

from tests.util import golden_npz

pytestmark = pytest.mark.gpu

P2W_CFG = dict(lm_type="pbert", input_layer="embed", enc_hidden_size=128, enc_num_attention_heads=2, enc_num_layers=2,
               enc_intermediate_size=256, dec_hidden_size=128, dec_num_attention_heads=2, dec_num_layers=2,
               dec_intermediate_size=256, dropout_enc_rate=0.0, dropout_dec_rate=0.0, dropout_attn_rate=0.0, mtl_ctc_weight=0,
               lsm_prob=0, kd_weight=0, max_decode_ylen=64, vocab_size=40, src_vocab_size=12, max_seq_len=64, eos_id=2, mask_id=39,
               phone_eos_id=2, phone_mask_id=11, blank_id=0, add_sos_eos=False)
# bf16 logits: tests/p2w_ref.py with weights and stored activations rounded to bf16 against itself in f32 on the fixture's batch differs
# by at most 6.765e-3 of the logits' range over the valid rows (tests/test_p2w_cpu.py::test_bf16_logit_error_constant recomputes
# it); the bar is 4 x that, as for ELECTRA's token probabilities
PBERT_LOGITS_BF16_SIM = 6.765e-3
_DT = [torch.float32, torch.bfloat16]
_DT_IDS = ["f32", "bf16"]


@pytest.fixture(scope="module")
def g():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" else v) for k, v in golden_npz("p2w_tiny").items()}


def _build(g, kind, dtype, dev, train=False, **kw):
    from emoasr_amd.modeling.p2w import P2W
    lm = P2W(SimpleNamespace(**dict(P2W_CFG, lm_type=kind)), compute_dtype=dtype, **kw)
    lm.load_state_dict({k[len(kind) + 4:]: v for k, v in g.items() if k.startswith(kind + "/sd/")})
    lm = lm.to(dev)
    return lm.train() if train else lm.eval()


def _check_loss_and_grads(lm, g, kind, dtype, loss):
    ref_loss = g[kind + "/loss"].item()
    ref_grads = {k[len(kind) + 6:]: v for k, v in g.items() if k.startswith(kind + "/grad/")}
    ltol = 2e-2 if dtype == torch.bfloat16 else 1e-3
    print(f"{kind} loss {dtype}: {loss.item():.6f} against {ref_loss:.6f}")
    assert abs(loss.item() - ref_loss) < ltol * abs(ref_loss), (loss.item(), ref_loss)
    absent = {n for n, p in lm.named_parameters() if p.grad is None}
    assert absent == {str(n) for n in g[kind + "/grad_absent"]}, absent
    gmax = max(v.abs().max().item() for v in ref_grads.values())
    worst, worst_name, cos_min, cos_name, big = 0.0, None, 1.0, None, 0
    for n, p in lm.named_parameters():
        if p.grad is None:
            continue
        ref, got = ref_grads[n].float(), p.grad.float().cpu()
        assert torch.isfinite(got).all(), n
        err = ((got - ref).abs().max() / max(ref.abs().max().item(), 1e-2 * gmax)).item()
        if err > worst:
            worst, worst_name = err, n
        if ref.abs().max() > (1e-2 if dtype == torch.bfloat16 else 1e-6) * gmax:
            big += 1
            cos = torch.nn.functional.cosine_similarity(got.flatten().double(), ref.flatten().double(), dim=0).item()
            if cos < cos_min:
                cos_min, cos_name = cos, n
    print(f"{kind} grads {dtype}: worst max-error {worst:.3e} ({worst_name}), min cosine {cos_min:.8f} ({cos_name}) over {big} tensors")
    # rows of the phone embedding for phones absent from the batch (0, 1, 10, the mask 11; 2 only pads) are exactly zero
    eg = dict(lm.named_parameters())["encoder.embed.weight"].grad.cpu()
    used = set(torch.cat([g["ps"][b, :int(n)] for b, n in enumerate(g["plens"])]).tolist())
    unused = [v for v in range(P2W_CFG["src_vocab_size"]) if v not in used]
    assert unused and not eg[unused].any() and eg[sorted(used)].any()
    if dtype == torch.bfloat16:
        # (the comparison is not vacuous: 15 of the fixture's pbert tensors and more of its pctc tensors are above the threshold)
        assert big >= 10 and cos_min > 0.98, (big, cos_min, cos_name, worst, worst_name)
        return
    assert worst < 5e-3, (worst, worst_name)
    assert cos_min >= 0.9999, (cos_min, cos_name)


@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_pbert_loss_and_grads(dev, g, dtype):
    lm = _build(g, "pbert", dtype, dev, train=True)
    loss, ld = lm(g["ys_in"], g["ylens"], g["labels"], g["ps"], g["plens"])
    assert set(ld) == {"loss_att", "loss_total"} and ld["loss_total"] is loss
    loss.backward()
    _check_loss_and_grads(lm, g, "pbert", dtype, loss)


@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_pctc_loss_and_grads(dev, g, dtype):
    lm = _build(g, "pctc", dtype, dev, train=True)
    loss, ld = lm(g["ys"], g["ylens"], None, g["ps"], g["plens"])
    assert "loss_total" in ld
    loss.backward()
    _check_loss_and_grads(lm, g, "pctc", dtype, loss)


def test_pbert_logits_f32(dev, g):
    lm = _build(g, "pbert", torch.float32, dev)
    logits = lm(g["ys_in"], g["ylens"], None, g["ps"], g["plens"])
    ref = g["pbert/logits"]
    assert logits.shape == ref.shape
    worst = 0.0
    for b, n in enumerate(g["ylens"].tolist()):     # (rows past ylens are padding on both sides)
        worst = max(worst, ((logits[b, :n].float().cpu() - ref[b, :n]).abs().max() / ref.abs().max()).item())
    print(f"pbert logits f32: {worst:.3e} of range")
    assert worst < 1e-3, worst
    # return_logits=True: the loss path hands back the same logits
    lm2 = _build(g, "pbert", torch.float32, dev, train=True, return_logits=True)
    loss, _, lg = lm2(g["ys_in"], g["ylens"], g["labels"], g["ps"], g["plens"])
    assert lg.shape == ref.shape and abs(loss.item() - g["pbert/loss"].item()) < 1e-3 * g["pbert/loss"].item()
    n = int(g["ylens"][5])
    assert ((lg[5, :n].float().cpu() - ref[5, :n]).abs().max() / ref.abs().max()).item() < 1e-3
    lm3 = _build(g, "pbert", torch.float32, dev, train=True)
    assert len(lm3(g["ys_in"], g["ylens"], g["labels"], g["ps"], g["plens"])) == 2


def test_pbert_logits_bf16(dev, g):
    lm = _build(g, "pbert", torch.bfloat16, dev)
    logits = lm(g["ys_in"], g["ylens"], None, g["ps"], g["plens"])
    ref = g["pbert/logits"]
    worst = max(((logits[b, :n].float().cpu() - ref[b, :n]).abs().max() / ref.abs().max()).item()
                for b, n in enumerate(g["ylens"].tolist()))
    print(f"pbert logits bf16: {worst:.3e} of range (bar {4 * PBERT_LOGITS_BF16_SIM:.3e})")
    assert worst <= 4 * PBERT_LOGITS_BF16_SIM, worst


def test_pctc_greedy_f32(dev, g):
    lm = _build(g, "pctc", torch.float32, dev)
    hyps = lm.decode(g["ps"], g["plens"])
    want, o = [], 0
    for n in g["pctc/hyp_lens"].tolist():
        want.append(g["pctc/hyps"][o:o + n].tolist())
        o += n
    assert hyps == want, (hyps, want)


@pytest.mark.parametrize("kind", ["pbert", "pctc"])
def test_padding_does_not_change_the_loss(dev, g, kind):
    """wider ys / ps with garbage past the lengths: same loss (the f32 loss bar)"""
    lm = _build(g, kind, torch.float32, dev, train=True)
    gen = torch.Generator().manual_seed(1)
    B = g["ys"].shape[0]
    ys = torch.randint(3, 39, (B, g["ys"].shape[1] + 5), generator=gen)
    ps = torch.randint(3, 10, (B, g["ps"].shape[1] + 6), generator=gen)
    labels = torch.randint(3, 39, ys.shape, generator=gen)      # labels past ylens are garbage too: they are cut with ys
    src = g["ys_in"] if kind == "pbert" else g["ys"]
    for b in range(B):
        ys[b, :int(g["ylens"][b])] = src[b, :int(g["ylens"][b])]
        ps[b, :int(g["plens"][b])] = g["ps"][b, :int(g["plens"][b])]
    labels[:, :g["labels"].shape[1]] = g["labels"]
    loss, _ = lm(ys, g["ylens"], labels if kind == "pbert" else None, ps, g["plens"])
    ref = g[kind + "/loss"].item()
    print(f"{kind} padded loss {loss.item():.6f} against {ref:.6f}")
    assert abs(loss.item() - ref) < 1e-3 * abs(ref)


@pytest.mark.parametrize("kind", ["pbert", "pctc"])
def test_train_step_moves_every_parameter(dev, g, kind):
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    params = SimpleNamespace(**dict(P2W_CFG, lm_type=kind, learning_rate=2e-3, lr_schedule_type="lindecay", num_warmup_steps=2,
                                    weight_decay=0.01, clip_grad_norm=0.5, accum_grad=1, log_step=1))
    lm = _build(g, kind, torch.float32, dev, train=True)
    groups = get_optimizer_params_nodecay(list(lm.named_parameters()), weight_decay=params.weight_decay)
    opt = ScheduledOptimizer(AdamW(groups, lr=0, weight_decay=params.weight_decay), params, num_total_steps=10)
    before = {n: p.detach().cpu().clone() for n, p in lm.named_parameters()}
    data = {"ys_in": g["ys_in"] if kind == "pbert" else g["ys"], "ylens": g["ylens"], "ps": g["ps"], "plens": g["plens"],
            "labels": g["labels"] if kind == "pbert" else None}
    out = train_step(lm, opt, data, params, dev)
    assert abs(out["loss_total"] - g[kind + "/loss"].item()) < 1e-3 * g[kind + "/loss"].item()
    for n, p in lm.named_parameters():
        assert torch.isfinite(p).all(), n
        assert not torch.equal(p.detach().cpu(), before[n]), n


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()


def test_pbert_takes_the_fused_head(dev):
    """bf16, V % 8 == 0, V >= 256, d % 64 == 0 and at least 1024 labelled rows: the loss takes the logit-free head kernels, and its
    loss / gradients agree with the materialised branch on the same weights (the bars of tests/test_ce_head_gpu.py for the LM)"""
    from emoasr_amd.modeling.p2w import P2W
    V = 512
    torch.manual_seed(3)
    lm = P2W(SimpleNamespace(**dict(P2W_CFG, vocab_size=V, mask_id=V - 1, max_seq_len=128)), compute_dtype=torch.bfloat16).to(dev).train()
    B, N, P = 24, 64, 90
    ylens = [N - (b % 5) * 7 for b in range(B)]
    plens = [P - (b % 7) * 5 for b in range(B)]
    ys, ps = torch.randint(3, V - 1, (B, N)), torch.randint(3, 11, (B, P))
    labels = torch.randint(3, V - 1, (B, N))
    for b, n in enumerate(ylens):
        labels[b, n:] = -100
    assert int((labels != -100).sum()) >= 1024
    out = {}
    for fused in (True, False):
        eng = lm.engine()
        eng.cmlm_fused_head = fused
        lm.zero_grad()
        loss, _ = lm(ys, ylens, labels, ps, plens)
        loss.backward()
        assert eng.cmlm_last_head == ("fused" if fused else "materialised")
        out[fused] = (loss.item(), {n: p.grad.detach().clone() for n, p in lm.named_parameters() if p.grad is not None})
    (lf, gf), (lm_, gm) = out[True], out[False]
    print(f"pbert loss: fused {lf:.5f}, materialised {lm_:.5f}")
    assert abs(lf - lm_) < 2e-2 * abs(lm_)
    assert set(gf) == set(gm)
    gmax = max(v.abs().max().item() for v in gm.values())
    big = [n for n in gm if gm[n].abs().max() > 1e-2 * gmax]
    assert len(big) >= 10
    for n in big:
        assert _cos(gf[n], gm[n]) > 0.98, (n, _cos(gf[n], gm[n]))


def test_ppl_masked_lm_takes_a_p2w(dev, g, tmp_path):
    """train_lm.ppl_masked_lm over P2WDataset batches of one utterance: every word masked in turn, conditioned on the phones -- against
    the f64 restatement (1e-3 relative, the f32 bar of the BERT LM's perplexity test)"""
    import math
    from emoasr_amd.datasets import P2WDataset
    from emoasr_amd.train_lm import ppl_masked_lm
    from tests import p2w_ref
    path = tmp_path / "p2w.tsv"
    path.write_text(str(g["tsv"]))
    ds = P2WDataset(SimpleNamespace(**dict(P2W_CFG, bucket_shuffle=False, text_augment=False, mask_proportion=0.3,
                                           random_num_to_mask=False)), str(path), phase="test")
    loader = [ds.collate_fn([ds[i]]) for i in range(len(ds))]
    lm = _build(g, "pbert", torch.float32, dev)
    cnt, ppl = ppl_masked_lm(loader, lm, dev, P2W_CFG["mask_id"], P2W_CFG["max_seq_len"])
    sd = {k[9:]: v.double() for k, v in g.items() if k.startswith("pbert/sd/")}
    total, words = 0.0, 0
    for data in loader:
        ys, ps = data["ys_in"], data["ps"]
        n = ys.shape[1]
        copies = ys.repeat(n, 1)
        copies[torch.arange(n), torch.arange(n)] = P2W_CFG["mask_id"]
        lg = p2w_ref.pbert_logits(sd, copies, [n] * n, ps.repeat(n, 1), [ps.shape[1]] * n)
        total -= float(torch.log_softmax(lg, -1)[torch.arange(n), torch.arange(n), ys[0]].sum())
        words += n
    want = math.exp(total / words)
    print(f"P2W masked perplexity {ppl:.4f} against {want:.4f} over {cnt} words")
    assert cnt == words == 24 and abs(ppl - want) < 1e-3 * want
