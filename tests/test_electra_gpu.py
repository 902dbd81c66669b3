"""ELECTRA (lm_type="electra" / "electra-disc") on the HIP path against the reference's outputs (tests/golden/electra_tiny:
tests/golden/make_golden_electra.py; the reference ran with every dropout at 0 and its samples were recorded) and, where the fixture
holds no value, against the f64 restatement tests/electra_ref.py on the fixture's weights (itself held to the fixture at 1e-5 by
tests/test_electra_cpu.py).

Bars are those of tests/test_bert_gpu.py: losses 1e-3 / 2e-2 relative, f32 gradients 5e-3 in the max-error form with cosine >= 0.9999
per tensor, bf16 gradients cosine > 0.98 over the tensors above 1e-2 of the largest -- "largest" taken per sub-model, so that the
discriminator (its loss carries electra_disc_weight) does not hide the generator's tensors."""
from types import SimpleNamespace

import pytest
import torch

from tests import electra_ref
from tests.test_electra_cpu import ALIAS, DISC_CFG, ELECTRA_CFG, TIED, grads_of
from tests.util import golden_npz

pytestmark = pytest.mark.gpu

# bf16 bar of the token probabilities, measured on the CPU: tests/electra_ref.py with weights and activations rounded to bf16
# (round_to) against the same code in f32 on the fixture's batch (46 tokens) -- mean |error| of sigmoid(logit), times 4 for
# summation order and the roundings the simulation omits.  (The fixture's discriminator is freshly initialised: its logits are
# small, so the probabilities sit near 0.5 and move little.)
SCORE_BF16_SIM, SCORE_BF16_BAR = 2.208e-5, 8.83e-5
W = ELECTRA_CFG["electra_disc_weight"]


@pytest.fixture(scope="module")
def g():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" else v) for k, v in golden_npz("electra_tiny").items()}


def _state(g, dtype=torch.float32):
    return {k[3:]: v.to(dtype) for k, v in g.items() if k.startswith("sd/")}


def _build(g, dtype, dev, train=False, cfg=ELECTRA_CFG):
    from emoasr_amd.modeling.lm import LM
    lm = LM(SimpleNamespace(**cfg), compute_dtype=dtype)
    lm.load_state_dict(_state(g))
    lm = lm.to(dev)
    lm.hidden_dropout_prob = lm.attention_probs_dropout_prob = 0.0
    return lm.train() if train else lm.eval()


def _close(got, ref, dtype, what):
    tol = 2e-2 if dtype == torch.bfloat16 else 1e-3
    got, ref = (v.detach() if torch.is_tensor(v) else v for v in (got, ref))
    print(f"{what} {dtype}: {float(got):.6f} against {float(ref):.6f}")
    assert abs(float(got) - float(ref)) < tol * abs(float(ref)), (what, float(got), float(ref))


def _check_grads(lm, dtype, ref_grads, absent, n_rows, key_bias_only=True):
    """per sub-model: max-error form and cosine per tensor (f32), cosine over the large tensors (bf16)"""
    named = dict(lm.named_parameters())
    assert ALIAS not in named and sorted(n for n, p in named.items() if p.grad is None) == sorted(absent)
    for sub in ("lm.gmodel.", "lm.dmodel."):
        names = [n for n in named if n.startswith(sub) and n not in absent]
        if not names:
            continue
        gmax = max(ref_grads[n].abs().max().item() for n in names)
        worst, worst_name, cos_min, cos_name, below, big = 0.0, None, 1.0, None, [], 0
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
            else:
                below.append(n)
        print(f"grads {sub} {dtype}: worst max-error {worst:.3e} ({worst_name}), min cosine {cos_min:.8f} ({cos_name}) over {big} tensors")
        pos = named[sub + "electra.embeddings.position_embeddings.weight"].grad
        assert not pos[n_rows:].any() and pos[:n_rows].any()     # positions past the batch's length were never read
        if dtype == torch.bfloat16:
            assert big >= 5 and cos_min > 0.98, (sub, big, cos_min, cos_name, worst, worst_name)
            continue
        # the key biases have an analytically zero gradient (a constant added to every score of a soft-max row) -- and nothing else
        assert not key_bias_only or sorted(below) == sorted(n for n in names if n.endswith("attention.self.key.bias")), below
        assert worst < 5e-3, (sub, worst, worst_name)
        assert cos_min >= 0.9999, (sub, cos_min, cos_name)


# ---------------------------------------------------------------- 1. the reference's step, with its samples
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_train_loss_and_grads_with_the_recorded_samples(dev, g, dtype):
    lm = _build(g, dtype, dev, train=True)
    lm.forced_samples = g["sample_ids"]
    loss, ld = lm(g["ys_in"], g["ylens"], g["labels"])
    assert set(ld) == {"loss_gen", "loss_disc", "num_replaced", "num_masked"}
    assert all(v.dim() == 0 and v.is_cuda for v in ld.values()) and loss.dim() == 0 and loss.is_cuda
    _close(ld["loss_gen"], g["train/loss_gen"], dtype, "loss_gen")
    _close(ld["loss_disc"], g["train/loss_disc"], dtype, "loss_disc")
    _close(loss, g["train/loss"], dtype, "loss")
    assert ld["num_replaced"].item() == pytest.approx(g["train/num_replaced"].item(), abs=1e-6)
    assert ld["num_masked"].item() == pytest.approx(g["train/num_masked"].item(), abs=1e-6)
    generated, replaced = lm.last_corruption
    want_gen, want_rep = electra_ref.corrupt(g["ys_in"], g["labels"], g["sample_ids"])
    assert torch.equal(generated.cpu().long(), want_gen) and torch.equal(replaced.cpu().long(), want_rep)
    loss.backward()
    absent = [str(n) for n in g["grad_absent"]]
    assert absent == []
    ref_grads = grads_of(g, "grad")
    _check_grads(lm, dtype, ref_grads, absent, 17)
    if dtype == torch.float32:     # the tied weight: the vocabulary head's weight gradient + the embedding scatter, both in the reference
        assert lm.lm.gmodel.generator_lm_head.weight is lm.lm.gmodel.electra.embeddings.word_embeddings.weight
        got, ref = dict(lm.named_parameters())[TIED].grad.cpu(), ref_grads[TIED]
        assert ((got - ref).abs().max() / ref.abs().max()).item() < 5e-3
        masked_ids = set(g["labels"][g["labels"] != -100].tolist())
        never_input = [v for v in range(40) if v not in set(g["ys_in"].flatten().tolist()) | masked_ids]
        assert never_input and got[never_input].abs().max() > 0     # rows no token reads still get the head's soft-max gradient


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cfg", [ELECTRA_CFG, DISC_CFG], ids=["electra", "electra-disc"])
def test_forward_disc(dev, g, dtype, cfg):
    lm = _build(g, dtype, dev, train=True, cfg=cfg)
    loss, ld = lm.forward_disc(g["ys"], g["ylens"], g["disc/error_labels"])
    assert set(ld) == {"loss_total"} and ld["loss_total"] is loss
    _close(loss, g["disc/loss"], dtype, "forward_disc loss")
    loss.backward()
    absent = [str(n) for n in g["disc_grad_absent"]]
    assert len(absent) == 44 and all(n.startswith("lm.gmodel.") for n in absent)
    for n, p in lm.named_parameters():
        assert (p.grad is None) == n.startswith("lm.gmodel."), n
    _check_grads(lm, dtype, grads_of(g, "disc_grad"), absent, 17)


def test_no_label_and_no_lengths(dev, g):
    """a batch without a single label: loss_gen 0 from one row of weight zero, nothing replaced, the discriminator still trains;
    without ylens every position is a key and counts in the discriminator's mean"""
    lm = _build(g, torch.float32, dev, train=True)
    labels = torch.full_like(g["labels"], -100)
    loss, ld = lm(g["ys"], g["ylens"], labels)
    assert ld["loss_gen"].item() == 0.0 and ld["num_masked"].item() == 0.0 and ld["num_replaced"].item() == 0.0
    sd = _state(g, torch.float64)
    with torch.no_grad():
        ref = electra_ref.disc_loss(sd, g["ys"], g["ylens"], torch.zeros_like(g["ys"]))
    _close(ld["loss_disc"], ref, torch.float32, "loss_disc without labels")
    loss.backward()
    n = 9
    lm.forced_samples = g["sample_ids"][:3, :n]
    loss, ld = lm(g["ys_in"][:3, :n], None, g["labels"][:3, :n])
    with torch.no_grad():
        _, lg, ldisc, n_rep, n_mask = electra_ref.loss(sd, g["ys_in"][:3, :n], None, g["labels"][:3, :n], g["sample_ids"][:3, :n], W)
    _close(ld["loss_gen"], lg, torch.float32, "loss_gen without ylens")
    _close(ld["loss_disc"], ldisc, torch.float32, "loss_disc without ylens")
    assert ld["num_replaced"].item() == pytest.approx(n_rep) and ld["num_masked"].item() == pytest.approx(n_mask)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_vocabulary_that_is_no_multiple_of_8(dev, g, dtype):
    """V = 45 (the recipe's 9 798 is no multiple of 8 either): the logits and their gradient live in rows padded to 48 columns and
    the product dz . W runs over a zero-padded copy of the word table.  Freshly initialised weights, the fixture's batch with labels
    and samples drawn from the larger vocabulary; the reference values are the f64 restatement's."""
    from emoasr_amd.modeling.lm import LM
    V = 45
    cfg = dict(ELECTRA_CFG, vocab_size=V, mask_id=V - 1)
    torch.manual_seed(3)
    lm = LM(SimpleNamespace(**cfg), compute_dtype=dtype)
    with torch.no_grad():
        for n, p in lm.named_parameters():     # (weights large enough for every tensor's gradient to clear the noise floor)
            p.copy_(torch.randn(p.shape) * (0.2 if p.dim() > 1 else 0.1) + (1.0 if n.endswith("LayerNorm.weight") else 0.0))
    sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in lm.state_dict().items()}
    lm = lm.to(dev).train()
    lm.hidden_dropout_prob = lm.attention_probs_dropout_prob = 0.0
    gen = torch.Generator().manual_seed(9)
    ys_in, ylens = g["ys_in"].clone(), g["ylens"]
    masked = g["labels"] != -100
    ys_in[masked] = V - 1
    labels = torch.where(masked, torch.randint(3, V, masked.shape, generator=gen), torch.full_like(g["labels"], -100))
    samples = torch.randint(0, V, masked.shape, generator=gen)
    samples[masked] = torch.where(torch.rand(int(masked.sum()), generator=gen) < 0.3, labels[masked], samples[masked])
    total, lg, ld_ref, n_rep, n_mask = electra_ref.loss(sd, ys_in, ylens, labels, samples, W)
    total.backward()
    ref_grads = {k: v.grad.float() for k, v in sd.items() if v.grad is not None}
    lm.forced_samples = samples
    loss, ld = lm(ys_in, ylens, labels)
    _close(ld["loss_gen"], lg, dtype, "loss_gen V=45")
    _close(ld["loss_disc"], ld_ref, dtype, "loss_disc V=45")
    assert ld["num_replaced"].item() == pytest.approx(n_rep) and 0 < n_rep < n_mask == pytest.approx(ld["num_masked"].item())
    loss.backward()
    _check_grads(lm, dtype, ref_grads, [], 17)


# ---------------------------------------------------------------- 2. scores
def test_score_f32(dev, g):
    lm = _build(g, torch.float32, dev)
    ys, ylens = g["ys"], g["ylens"]
    scores = lm.score(ys, ylens)
    assert isinstance(scores, list) and len(scores) == 6 and all(isinstance(s, float) for s in scores)
    want = g["score/values"].tolist()
    print(f"score f32: {scores} against {want}")
    for a, b, n in zip(scores, want, ylens.tolist()):
        assert a < 0 and abs(a - b) <= 1e-4 * n, (a, b, n)
    n1 = int(ylens[1])
    one = lm.score(ys[1:2, :n1], ylens[1:2])
    assert len(one) == 1 and one[0] > 0 and abs(one[0] - g["score/single"].item()) <= 1e-4 * n1, one
    probs = lm.replaced_probs(ys, ylens)
    assert probs.dtype == torch.float64 and probs.shape == ys.shape and probs.device.type == "cpu"
    with torch.no_grad():
        ref = electra_ref.token_probs(_state(g, torch.float64), ys, ylens)
    mask = torch.arange(ys.shape[1])[None, :] < ylens[:, None]
    assert (probs - ref).abs()[mask].max() <= 1e-4


def test_score_bf16(dev, g):
    """bar: mean |error| per token probability <= 8.83e-5 = 4 x 2.208e-5, the error of the bf16-rounded restatement against the f32
    one on this batch (46 tokens), measured on the CPU; the 4 x margin covers summation order and the roundings the simulation omits"""
    lm = _build(g, torch.bfloat16, dev)
    ys, ylens = g["ys"], g["ylens"]
    probs = lm.replaced_probs(ys, ylens)
    with torch.no_grad():
        ref = electra_ref.token_probs(_state(g, torch.float64), ys, ylens)
    mask = torch.arange(ys.shape[1])[None, :] < ylens[:, None]
    err = (probs - ref).abs()[mask].mean().item()
    print(f"score bf16: mean |error| per token {err:.3e} (simulated {SCORE_BF16_SIM:.3e}, bar {SCORE_BF16_BAR:.3e})")
    assert err <= SCORE_BF16_BAR, err
    for a, b, n in zip(lm.score(ys, ylens), g["score/values"].tolist(), ylens.tolist()):
        assert abs(a - b) <= SCORE_BF16_BAR * n, (a, b, n)


# ---------------------------------------------------------------- 3. drawn samples
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_drawn_samples(dev, g, dtype):
    lm = _build(g, dtype, dev, train=True)
    ys_in, ylens, labels = g["ys_in"], g["ylens"], g["labels"]
    masked = labels != -100
    lm.seed, lm.step_count = 77, 4
    loss, ld = lm(ys_in, ylens, labels)
    assert lm.step_count == 5
    generated, replaced = (t.cpu().long() for t in lm.last_corruption)
    assert generated.shape == ys_in.shape and torch.equal(generated[~masked], ys_in[~masked])
    assert ((generated >= 0) & (generated < 40)).all()
    original = ys_in.clone()
    original[masked] = labels[masked]
    assert torch.equal(replaced, (generated != original).long())
    B = ys_in.shape[0]
    assert ld["num_replaced"].item() == pytest.approx(replaced.sum().item() / B) and ld["num_masked"].item() == pytest.approx(masked.sum().item() / B)
    with torch.no_grad():
        sd = _state(g, torch.float64)
        ref_disc = electra_ref.disc_loss(sd, generated, ylens, replaced)
        ref_gen = electra_ref.gen_loss(sd, ys_in, ylens, labels)
    _close(ld["loss_disc"], ref_disc, dtype, "loss_disc on the drawn ids")
    _close(ld["loss_gen"], ref_gen, dtype, "loss_gen")
    _close(loss, ref_gen + W * ref_disc, dtype, "loss")
    # the same (seed, step_count): the same samples; the next step: others
    lm.step_count = 4
    lm(ys_in, ylens, labels)
    assert torch.equal(lm.last_corruption[0].cpu().long(), generated)
    lm(ys_in, ylens, labels)
    assert lm.step_count == 6 and not torch.equal(lm.last_corruption[0].cpu().long(), generated)
    lm.seed, lm.step_count = 78, 4
    lm(ys_in, ylens, labels)
    assert not torch.equal(lm.last_corruption[0].cpu().long(), generated)
    # the comparator path draws with torch: same structure, not the same samples
    lm.sample_path = "torch"
    loss_t, ld_t = lm(ys_in, ylens, labels)
    gen_t, rep_t = (t.cpu().long() for t in lm.last_corruption)
    assert torch.equal(gen_t[~masked], ys_in[~masked]) and torch.equal(rep_t, (gen_t != original).long())
    assert ld_t["num_masked"].item() == pytest.approx(masked.sum().item() / B)
    _close(ld_t["loss_gen"], ref_gen, dtype, "loss_gen (torch sampler)")


# ---------------------------------------------------------------- 4. training step, search guard
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
    params, opt = _optimizer(lm, ELECTRA_CFG)
    before = {n: p.detach().cpu().clone() for n, p in lm.named_parameters()}
    out = train_step(lm, opt, {"ys_in": g["ys_in"], "ylens": g["ylens"], "labels": g["labels"]}, params, dev)
    assert set(out) == {"loss_gen", "loss_disc", "num_replaced", "num_masked"} and all(isinstance(v, float) for v in out.values())
    assert abs(out["loss_gen"] - g["train/loss_gen"].item()) < 1e-3 * g["train/loss_gen"].item()
    assert out["num_masked"] == pytest.approx(g["train/num_masked"].item(), abs=1e-6)
    for n, p in lm.named_parameters():
        assert not torch.equal(p.detach().cpu(), before[n]), n


def test_train_step_of_the_discriminator_leaves_the_generator(dev, g):
    from emoasr_amd.train_lm import train_step
    lm = _build(g, torch.float32, dev, train=True, cfg=DISC_CFG)
    params, opt = _optimizer(lm, DISC_CFG)
    before = {n: p.detach().cpu().clone() for n, p in lm.named_parameters()}
    out = train_step(lm, opt, {"ys_in": g["ys"], "ylens": g["ylens"], "error_labels": g["disc/error_labels"]}, params, dev)
    assert set(out) == {"loss_total"} and abs(out["loss_total"] - g["disc/loss"].item()) < 1e-3 * g["disc/loss"].item()
    for n, p in lm.named_parameters():
        assert torch.equal(p.detach().cpu(), before[n]) == n.startswith("lm.gmodel."), n


def test_beam_searches_refuse_electra(g):
    """at their entry, before the decoder or the encoder output is touched (both None here): nothing is launched"""
    from emoasr_amd.modeling.beam_search import joint_beam_search
    from emoasr_amd.modeling.beam_search_device import joint_beam_search_device
    from emoasr_amd.modeling.ctc_beam_search import ctc_prefix_beam_search
    from emoasr_amd.modeling.lm import LM, require_next_token_lm
    for cfg in (ELECTRA_CFG, DISC_CFG):
        lm = LM(SimpleNamespace(**cfg))
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            require_next_token_lm(lm, 0.3)
        for search in (joint_beam_search, joint_beam_search_device, ctc_prefix_beam_search):
            with pytest.raises(NotImplementedError, match="no next-token distribution"):
                search(None, None, None, 4, lm=lm, lm_weight=0.3)
