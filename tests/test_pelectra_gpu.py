"""P-ELECTRA (emoasr_amd/modeling/pelectra.py) on the HIP path against the reference's outputs (tests/golden/pelectra_tiny*.npz:
tests/golden/make_golden_pelectra.py; the reference ran with every dropout at 0 and its samples were recorded).

Bars are the ones tests/test_electra_gpu.py and tests/test_p2w_gpu.py hold for the same sub-models: f32 gradients 5e-3 in the max-error
form with cosine >= 0.9999 per tensor, bf16 losses 2e-2 relative and gradient cosine > 0.98 over the tensors above 1e-2 of the
sub-model's largest, f32 scores 1e-4 per token, bf16 token probabilities ELECTRA's SCORE_BF16_BAR (the same discriminator
architecture).  The f32 losses of the materialised head are held to six digits (1e-6 relative) and the counters exactly.  The fused
sampling head is compared with the materialised one on a random model (V = 256) at the bars of test_p2w_gpu's fused-head test."""
from types import SimpleNamespace

import pytest
import torch

from tests import electra_ref
from tests.test_electra_gpu import SCORE_BF16_BAR
from tests.test_pelectra_cpu import DISC_CFG, PELECTRA_CFG
from tests.util import golden_npz

pytestmark = pytest.mark.gpu
_DT = [torch.float32, torch.bfloat16]
_DT_IDS = ["f32", "bf16"]
SUBS = ("lm.gmodel.", "lm.dmodel.")


@pytest.fixture(scope="module")
def g():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" else v) for k, v in golden_npz("pelectra_tiny").items()}


def _state(g, dtype=torch.float32):
    return {k[3:]: v.to(dtype) for k, v in g.items() if k.startswith("sd/")}


def _build(g, dtype, dev, train=False, cfg=PELECTRA_CFG):
    from emoasr_amd.modeling.pelectra import PELECTRA
    lm = PELECTRA(SimpleNamespace(**cfg), compute_dtype=dtype)
    lm.load_state_dict(_state(g))
    lm = lm.to(dev)
    lm.hidden_dropout_prob = lm.attention_probs_dropout_prob = 0.0
    return lm.train() if train else lm.eval()


def _close(got, ref, tol, what):
    got, ref = float(got), float(ref)
    print(f"{what}: {got:.7f} against {ref:.7f} (relative {abs(got - ref) / abs(ref):.2e}, bar {tol:.0e})")
    assert abs(got - ref) <= tol * abs(ref), (what, got, ref)


def _grads_of(g, key):
    return {k[len(key) + 1:]: v for k, v in g.items() if k.startswith(key + "/")}


def _check_grads(lm, dtype, ref_grads, absent):
    named = dict(lm.named_parameters())
    assert sorted(n for n, p in named.items() if p.grad is None) == sorted(absent)
    for sub in SUBS:
        names = [n for n in named if n.startswith(sub) and n not in absent]
        if not names:
            continue
        gmax = max(ref_grads[n].abs().max().item() for n in names)
        worst, worst_name, cos_min, cos_name, big = 0.0, None, 1.0, None, 0
        for n in names:
            ref, got = ref_grads[n].float(), named[n].grad.float().cpu()
            assert torch.isfinite(got).all(), n
            err = ((got - ref).abs().max() / max(ref.abs().max().item(), 1e-2 * gmax)).item()
            if err > worst:
                worst, worst_name = err, n
            if ref.abs().max() > (1e-2 if dtype == torch.bfloat16 else 1e-6) * gmax:
                big += 1
                cos = torch.nn.functional.cosine_similarity(got.flatten().double(), ref.flatten().double(), dim=0).item()
                if cos < cos_min:
                    cos_min, cos_name = cos, n
        print(f"grads {sub} {dtype}: worst max-error {worst:.3e} ({worst_name}), min cosine {cos_min:.8f} ({cos_name}) over {big} tensors")
        if dtype == torch.bfloat16:
            assert big >= 5 and cos_min > 0.98, (sub, big, cos_min, cos_name, worst, worst_name)
            continue
        assert worst < 5e-3, (sub, worst, worst_name)
        assert cos_min >= 0.9999, (sub, cos_min, cos_name)


def _corrupt(ys_in, labels, samples):
    masked = labels != -100
    generated, original = ys_in.clone(), ys_in.clone()
    generated[masked], original[masked] = samples[masked], labels[masked]
    return generated, (generated != original).long()


# ---------------------------------------------------------------- 1. the reference's step, with its samples
@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
def test_train_loss_and_grads_with_the_recorded_samples(dev, g, dtype):
    from emoasr_amd.engine import arena_of
    lm = _build(g, dtype, dev, train=True)
    lm.forced_samples = g["sample_ids"]
    ys_in, ylens, labels = g["data/ys_in"], g["data/ylens"], g["data/labels"]
    loss, ld = lm(ys_in, ylens, labels, g["data/ps"], g["data/plens"])
    assert set(ld) == {"loss_gen", "loss_disc", "num_replaced", "num_masked"}
    assert all(v.dim() == 0 and v.is_cuda for v in ld.values()) and loss.dim() == 0 and loss.is_cuda
    assert lm.last_head == "materialised"     # (f32, and in bf16 too few rows and V = 40)
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-6
    _close(ld["loss_gen"], g["train/loss_gen"], tol, f"loss_gen {dtype}")
    _close(ld["loss_disc"], g["train/loss_disc"], tol, f"loss_disc {dtype}")
    _close(loss, g["train/loss"], tol, f"loss {dtype}")
    assert ld["num_replaced"].item() == g["train/num_replaced"].item() and ld["num_masked"].item() == g["train/num_masked"].item()
    generated, replaced = lm.last_corruption
    want_gen, want_rep = _corrupt(ys_in, labels, g["sample_ids"])
    assert torch.equal(generated.cpu().long(), want_gen) and torch.equal(replaced.cpu().long(), want_rep)
    # ONE arena holds both sub-models, and the generator's engine works on a view of it
    arena = arena_of(lm.parameters())
    assert arena is lm._arena and lm.engine().arena.arena is arena
    lo, hi = arena.flat.data_ptr(), arena.flat.data_ptr() + 4 * arena.size
    assert all(lo <= p.data_ptr() < hi for p in lm.parameters()) and sorted(arena.names) == sorted(n for n, _ in lm.named_parameters())
    loss.backward()
    assert [str(n) for n in g["grad_absent"]] == []
    _check_grads(lm, dtype, _grads_of(g, "grad"), [])


@pytest.mark.parametrize("dtype", _DT, ids=_DT_IDS)
@pytest.mark.parametrize("cfg", [PELECTRA_CFG, DISC_CFG], ids=["pelectra", "pelectra-disc"])
def test_forward_disc(dev, g, dtype, cfg):
    lm = _build(g, dtype, dev, train=True, cfg=cfg)
    loss, ld = lm.forward_disc(g["discset/ys_in"], g["discset/ylens"], g["discset/error_labels"])
    assert set(ld) == {"loss_total"} and ld["loss_total"] is loss
    _close(loss, g["disc/loss"], 2e-2 if dtype == torch.bfloat16 else 1e-3, f"forward_disc loss {dtype}")
    loss.backward()
    absent = [str(n) for n in g["disc_grad_absent"]]
    assert len(absent) == 92 and all(n.startswith("lm.gmodel.") for n in absent)
    for n, p in lm.named_parameters():
        assert (p.grad is None) == n.startswith("lm.gmodel."), n
    _check_grads(lm, dtype, _grads_of(g, "disc_grad"), absent)


def test_score_f32(dev, g):
    lm = _build(g, torch.float32, dev)
    ys, ylens = g["score/ys"], g["score/ylens"]
    scores = lm.score(ys, ylens)
    assert isinstance(scores, list) and len(scores) == 4 and all(isinstance(s, float) for s in scores)
    for a, b, n in zip(scores, g["score/values"].tolist(), ylens.tolist()):
        assert a < 0 and abs(a - b) <= 1e-4 * n, (a, b, n)
    n1 = int(ylens[1])
    one = lm.score(ys[1:2, :n1], ylens[1:2])
    assert len(one) == 1 and one[0] > 0 and abs(one[0] - g["score/single"].item()) <= 1e-4 * n1, one
    assert abs(one[0] + scores[1]) <= 2e-4 * n1     # the sign quirk: the same row, alone and in a batch


def test_score_bf16(dev, g):
    lm = _build(g, torch.bfloat16, dev)
    ys, ylens = g["score/ys"], g["score/ylens"]
    probs = lm.replaced_probs(ys, ylens)
    assert probs.dtype == torch.float64 and probs.shape == ys.shape and probs.device.type == "cpu"
    with torch.no_grad():
        ref = electra_ref.token_probs(_state(g, torch.float64), ys, ylens)
    mask = torch.arange(ys.shape[1])[None, :] < ylens[:, None]
    err = (probs - ref).abs()[mask].mean().item()
    print(f"score bf16: mean |error| per token {err:.3e} (bar {SCORE_BF16_BAR:.3e})")
    assert err <= SCORE_BF16_BAR, err
    for a, b, n in zip(lm.score(ys, ylens), g["score/values"].tolist(), ylens.tolist()):
        assert abs(a - b) <= SCORE_BF16_BAR * n, (a, b, n)


# ---------------------------------------------------------------- 2. the fused sampling head, end to end
# (the decoder's source attention takes keys of its own width: the encoder is 64 wide too)
FUSED_CFG = dict(PELECTRA_CFG, vocab_size=256, mask_id=255, dec_hidden_size=64, dec_num_attention_heads=1, dec_intermediate_size=128,
                 enc_hidden_size=64, enc_num_attention_heads=1, enc_intermediate_size=128)


def _fused_model(dev):
    from emoasr_amd.modeling.pelectra import PELECTRA
    torch.manual_seed(11)
    lm = PELECTRA(SimpleNamespace(**FUSED_CFG), compute_dtype=torch.bfloat16).to(dev).train()
    lm.hidden_dropout_prob = lm.attention_probs_dropout_prob = 0.0
    lm.sample_head, lm.sample_head_min_rows = "fused", 1
    gen = torch.Generator().manual_seed(12)
    B, N, P = 12, 33, 41
    ylens = [N - (b % 5) * 3 for b in range(B)]
    plens = [P - (b % 7) * 4 for b in range(B)]
    ys, ps = torch.randint(3, 255, (B, N), generator=gen), torch.randint(3, 11, (B, P), generator=gen)
    labels = torch.full((B, N), -100)
    ys_in = ys.clone()
    for b, n in enumerate(ylens):
        pos = torch.randperm(n, generator=gen)[: max(1, n // 3)]
        labels[b, pos], ys_in[b, pos] = ys[b, pos], 255
    return lm, (ys_in, ylens, labels, ps, plens)


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()


def test_fused_sampling_head_end_to_end(dev):
    lm, batch = _fused_model(dev)
    ys_in, ylens, labels = batch[:3]
    masked = labels != -100
    # ---- drawn samples: structure, determinism in (seed, step_count)
    lm.seed, lm.step_count = 77, 4
    loss, ld = lm(*batch)
    assert lm.last_head == "fused-sample" and lm.step_count == 5
    generated, replaced = (t.cpu().long() for t in lm.last_corruption)
    assert torch.equal(generated[~masked], ys_in[~masked]) and ((generated >= 0) & (generated < 256)).all()
    want_gen, want_rep = _corrupt(ys_in, labels, generated)
    assert torch.equal(generated, want_gen) and torch.equal(replaced, want_rep)
    B = ys_in.shape[0]
    assert ld["num_replaced"].item() == pytest.approx(replaced.sum().item() / B) and ld["num_masked"].item() == pytest.approx(masked.sum().item() / B)
    assert 0 < replaced.sum().item()
    lm.step_count = 4
    lm(*batch)
    assert torch.equal(lm.last_corruption[0].cpu().long(), generated)
    lm(*batch)
    assert lm.step_count == 6 and not torch.equal(lm.last_corruption[0].cpu().long(), generated)
    # ---- forced samples: the fused head against the materialised one
    lm.forced_samples = generated
    out = {}
    for head in ("fused", "materialised"):
        lm.sample_head = head
        lm.zero_grad()
        loss, ld = lm(*batch)
        loss.backward()
        assert lm.last_head == ("fused-sample" if head == "fused" else "materialised")
        out[head] = (loss.item(), ld["loss_gen"].item(), {n: p.grad.detach().clone() for n, p in lm.named_parameters() if p.grad is not None})
    (lf, gf_loss, gf), (lm_, gm_loss, gm) = out["fused"], out["materialised"]
    print(f"pelectra loss: fused {lf:.5f} (generator {gf_loss:.5f}), materialised {lm_:.5f} (generator {gm_loss:.5f})")
    assert abs(lf - lm_) < 2e-2 * abs(lm_) and abs(gf_loss - gm_loss) < 2e-2 * abs(gm_loss)
    assert set(gf) == set(gm) == {n for n, _ in lm.named_parameters()}
    gen_names = [n for n in gm if n.startswith("lm.gmodel.")]
    gmax = max(gm[n].abs().max().item() for n in gen_names)
    big = [n for n in gen_names if gm[n].abs().max() > 1e-2 * gmax]
    assert len(big) >= 10
    for n in big:
        assert _cos(gf[n], gm[n]) > 0.98, (n, _cos(gf[n], gm[n]))


# ---------------------------------------------------------------- 3. training steps
def _optimizer(lm, cfg):
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    params = SimpleNamespace(**dict(cfg, learning_rate=2e-3, lr_schedule_type="lindecay", num_warmup_steps=2, weight_decay=0.01,
                                    clip_grad_norm=0.5, accum_grad=1, log_step=1))
    groups = get_optimizer_params_nodecay(list(lm.named_parameters()), weight_decay=params.weight_decay)
    return params, ScheduledOptimizer(AdamW(groups, lr=0, weight_decay=params.weight_decay), params, num_total_steps=10)


def test_train_step_moves_every_parameter(dev, g):
    from emoasr_amd.train_lm import train_step
    lm = _build(g, torch.float32, dev, train=True)
    lm.forced_samples = g["sample_ids"]
    params, opt = _optimizer(lm, PELECTRA_CFG)
    before = {n: p.detach().cpu().clone() for n, p in lm.named_parameters()}
    data = {k: g["data/" + k] for k in ("ys_in", "ylens", "labels", "ps", "plens")}
    out = train_step(lm, opt, data, params, dev)
    assert set(out) == {"loss_gen", "loss_disc", "num_replaced", "num_masked"} and all(isinstance(v, float) for v in out.values())
    assert abs(out["loss_gen"] - g["train/loss_gen"].item()) < 1e-3 * g["train/loss_gen"].item()
    for n, p in lm.named_parameters():
        assert torch.isfinite(p).all(), n
        assert not torch.equal(p.detach().cpu(), before[n]), n


def test_train_step_of_the_discriminator_leaves_the_generator(dev, g):
    from emoasr_amd.train_lm import train_step
    lm = _build(g, torch.float32, dev, train=True, cfg=DISC_CFG)
    params, opt = _optimizer(lm, DISC_CFG)
    before = {n: p.detach().cpu().clone() for n, p in lm.named_parameters()}
    data = {"ys_in": g["discset/ys_in"], "ylens": g["discset/ylens"], "error_labels": g["discset/error_labels"]}
    out = train_step(lm, opt, data, params, dev)
    assert set(out) == {"loss_total"} and abs(out["loss_total"] - g["disc/loss"].item()) < 1e-3 * g["disc/loss"].item()
    for n, p in lm.named_parameters():
        assert torch.equal(p.detach().cpu(), before[n]) == n.startswith("lm.gmodel."), n
