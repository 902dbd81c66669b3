"""The BERT masked LM (lm_type="bert") on the HIP path against the reference's outputs (tests/golden/bert_tiny:
tests/golden/make_golden_bert.py; the reference ran with every dropout at 0) and, where the fixture holds no value, against the f64
restatement tests/bert_ref.py on the fixture's weights (itself held to the fixture at 1e-5 by tests/test_bert_cpu.py).

Bars are those of tests/test_lm_train_gpu.py: logits 1e-3 / 6e-2 of range, loss 1e-3 / 2e-2 relative, f32 gradients 5e-3 in the
max-error form with cosine >= 0.9999 per tensor, bf16 gradients cosine > 0.98 over the tensors above 1e-2 of the largest."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bert_ref
from tests.test_bert_cpu import BERT_CFG, KD_VARIANTS, TEMP, TOPK, golden_labels, tsv_rows
from tests.util import LM_CFG, golden_npz, load_golden, lm_state

pytestmark = pytest.mark.gpu

POOLER = ("lm.bert.bert.pooler.dense.weight", "lm.bert.bert.pooler.dense.bias")
TIED = "lm.bert.bert.embeddings.word_embeddings.weight"
# bf16 bars, measured on the CPU: tests/bert_ref.py with weights and activations rounded to bf16 (round_to) against the same code in
# f32 -- mean |error| of a masked token's log-probability, times 4 for summation order and the roundings the simulation omits
SCORE_BF16_SIM, SCORE_BF16_BAR = 1.178e-3, 4.71e-3            # the fixture's batch: 46 tokens
PPL_BF16_SIM = {False: 0.988e-3, True: 1.021e-3}              # the four-row TSV: 24 / 32 tokens
PPL_BF16_BAR = {k: 4 * v for k, v in PPL_BF16_SIM.items()}


@pytest.fixture(scope="module")
def g():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" else v) for k, v in golden_npz("bert_tiny").items()}


def _state(g, dtype=torch.float32):
    return {k[3:]: v.to(dtype) for k, v in g.items() if k.startswith("sd/")}


def _build(g, dtype, dev, train=False):
    from emoasr_amd.modeling.lm import LM
    lm = LM(SimpleNamespace(**BERT_CFG), compute_dtype=dtype)
    lm.load_state_dict(_state(g))
    lm = lm.to(dev)
    lm.hidden_dropout_prob = lm.attention_probs_dropout_prob = 0.0
    return lm.train() if train else lm.eval()


def _rel(a, b):
    return ((a.float().cpu() - b).abs().max() / (b.abs().max() + 1e-12)).item()


@pytest.fixture(scope="module")
def ref_tokens(g):
    """f64 restatement: the masked log-probability of every token of the fixture's batch [B, N]"""
    with torch.no_grad():
        return bert_ref.masked_logprobs(_state(g, torch.float64), g["ys"], g["ylens"], BERT_CFG["mask_id"])


# ---------------------------------------------------------------- 1. logits
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_logits(dev, g, dtype):
    lm = _build(g, dtype, dev)
    logits = lm(g["ys_in"], g["ylens"])
    assert logits.shape == g["eval/logits"].shape and logits.dtype == torch.float32
    err = _rel(logits, g["eval/logits"])
    print(f"logits {dtype}: {err:.3e} of range")
    assert err < (1e-3 if dtype == torch.float32 else 6e-2), err
    if dtype == torch.float32:     # no ylens: no mask, every position is a key -- an unpadded row equals itself inside the padded batch
        n = int(g["ylens"][1])
        alone = lm(g["ys_in"][1:2, :n])
        assert alone.shape == (1, n, BERT_CFG["vocab_size"])
        d = (alone[0] - logits[1, :n]).abs().max().item() / g["eval/logits"].abs().max().item()
        print(f"unpadded row against the batch: {d:.3e} of range")
        assert d <= 1e-5, d


# ---------------------------------------------------------------- 2. loss and gradients
def _check_loss_and_grads(lm, dtype, loss, ref_loss, ref_grads, n_rows):
    ltol = 2e-2 if dtype == torch.bfloat16 else 1e-3
    print(f"loss {dtype}: {loss.item():.6f} against {ref_loss:.6f}")
    assert abs(loss.item() - ref_loss) < ltol * abs(ref_loss), (loss.item(), ref_loss)
    gmax = max(v.abs().max().item() for v in ref_grads.values())
    worst, worst_name, cos_min, cos_name, below, big = 0.0, None, 1.0, None, [], 0
    for n, p in lm.named_parameters():
        if n in POOLER:     # never read: no gradient, as in the reference (AdamW then leaves it bit-identical)
            assert p.grad is None, n
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
        else:
            below.append(n)
    print(f"grads {dtype}: worst max-error {worst:.3e} ({worst_name}), min cosine {cos_min:.8f} ({cos_name}) over {big} tensors")
    grads = dict(lm.named_parameters())
    pos = grads["lm.bert.bert.embeddings.position_embeddings.weight"].grad
    assert not pos[n_rows:].any() and pos[:n_rows].any()     # positions past the batch's length were never read
    if dtype == torch.bfloat16:
        assert big >= 20 and cos_min > 0.98, (big, cos_min, cos_name, worst, worst_name)
        return
    # the key biases have an analytically zero gradient (a constant added to every score of a soft-max row) -- and nothing else
    assert sorted(below) == sorted(f"lm.bert.bert.encoder.layer.{i}.attention.self.key.bias" for i in range(BERT_CFG["num_layers"])), below
    assert worst < 5e-3, (worst, worst_name)
    assert cos_min >= 0.9999, (cos_min, cos_name)
    # the tied weight: the output projection's weight gradient (labelled rows only) + the embedding scatter, both in the reference
    assert lm.lm.bert.cls.predictions.decoder.weight is lm.lm.bert.bert.embeddings.word_embeddings.weight
    assert _rel(grads[TIED].grad, ref_grads[TIED].float()) < 5e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_train_loss_and_grads(dev, g, dtype):
    """~30 % of the positions labelled: transform + head run on the M = 13 gathered rows, their dX is scattered back"""
    lm = _build(g, dtype, dev, train=True)
    loss, ld = lm(g["ys_in"], g["ylens"], g["labels"])
    assert set(ld) == {"loss_total"} and ld["loss_total"] is loss
    loss.backward()
    assert {str(n) for n in g["grad_absent"]} == set(POOLER)
    _check_loss_and_grads(lm, dtype, loss, g["train/loss"].item(), {k[5:]: v for k, v in g.items() if k.startswith("grad/")}, 17)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_train_every_position_labelled(dev, g, dtype):
    """M = every row of every sequence (and the padded rows none); the reference values are the f64 restatement's"""
    ys_in, ylens = g["ys_in"], g["ylens"]
    labels = torch.full_like(ys_in, -100)
    for b, n in enumerate(ylens.tolist()):
        labels[b, :n] = g["ys"][b, :n]
    sd = {k: v.requires_grad_(True) for k, v in _state(g, torch.float64).items()}
    ref_loss = bert_ref.loss(sd, ys_in, ylens, labels)
    ref_loss.backward()
    ref_grads = {k: v.grad for k, v in sd.items() if v.grad is not None}
    lm = _build(g, dtype, dev, train=True)
    loss, _ = lm(ys_in, ylens, labels)
    loss.backward()
    _check_loss_and_grads(lm, dtype, loss, ref_loss.item(), ref_grads, 17)


# ---------------------------------------------------------------- 3. the masked copies
def test_mlm_expand_exact(dev):
    from emoasr_amd import ops
    lens, N, Np, mask_id, pad_id, sentinel = [1, 2, 7, 8, 9], 9, 16, 39, 0, -7
    gen = torch.Generator().manual_seed(3)
    ys = torch.randint(3, 39, (len(lens), N), generator=gen, dtype=torch.int32)
    row0 = [0]
    for n in lens:
        row0.append(row0[-1] + n)
    R = row0[-1]
    assert R == 27
    want = []     # host construction of all R copies
    for b, n in enumerate(lens):
        for pos in range(n):
            ids = ys[b, :n].tolist() + [pad_id] * (Np - n)
            ids[pos] = mask_id
            want.append((ids, n, pos, int(ys[b, pos])))
    ys_d, len_d, row0_d = ys.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), torch.tensor(row0, dtype=torch.int32, device=dev)
    for r_begin, r_count in ((0, 27), (3, 8), (26, 1)):     # (3, 8): the third sequence's copies and the fourth's first
        bufs = (torch.full((r_count + 2, Np), sentinel, dtype=torch.int32, device=dev),) + tuple(
            torch.full((r_count + 2,), sentinel, dtype=torch.int32, device=dev) for _ in range(3))
        ids, klens, idx, labels = ops.mlm_expand(ys_d, len_d, row0_d, r_begin, r_count, Np, mask_id, pad_id, total=R, out=bufs)
        torch.cuda.synchronize()
        part = want[r_begin:r_begin + r_count]
        assert ids.cpu().tolist() == [w[0] for w in part]
        assert klens.cpu().tolist() == [w[1] for w in part]
        assert idx.cpu().tolist() == [j * Np + w[2] for j, w in enumerate(part)]
        assert labels.cpu().tolist() == [w[3] for w in part]
        for buf in bufs:
            assert (buf[r_count:] == sentinel).all()
    # out of range: refused on the host, nothing launched
    with pytest.raises(AssertionError):
        ops.mlm_expand(ys_d, len_d, row0_d, 20, 8, Np, mask_id, pad_id, total=R)
    from emoasr_amd import lib
    with pytest.raises(lib.EmoasrHipError):
        ops.mlm_expand(ys_d, len_d, row0_d, 0, 4, Np, -1, pad_id, total=R)


# ---------------------------------------------------------------- 4. pseudo-log-likelihood
def test_score_f32(dev, g, ref_tokens):
    lm = _build(g, torch.float32, dev)
    ys, ylens = g["ys"], g["ylens"]
    scores = lm.score(ys, ylens)
    assert isinstance(scores, list) and len(scores) == 6 and all(isinstance(s, float) for s in scores)
    want = g["score/values"].tolist()
    print(f"score f32: {scores} against {want}")
    for a, b, n in zip(scores, want, ylens.tolist()):
        assert abs(a - b) <= 1e-4 * n, (a, b, n)
    lp = lm.masked_logprobs(ys, ylens)
    assert lp.dtype == torch.float64 and lp.shape == ys.shape and lp.device.type == "cpu"
    for b, n in enumerate(ylens.tolist()):
        assert not lp[b, n:].any() and (lp[b, :n] < 0).all()
    assert (lp - ref_tokens).abs().max() <= 1e-4
    # one copy (Np = 24 token rows) per chunk: chunks begin and end inside sequences; the result must not move
    forced = lm.masked_logprobs(ys, ylens, max_token_rows=32)
    for b, n in enumerate(ylens.tolist()):
        assert (forced[b] - lp[b]).abs().sum() <= 1e-5 * n, b
    for bs in (1, 4):
        for a, b, n in zip(lm.score(ys, ylens, batch_size=bs), scores, ylens.tolist()):
            assert abs(a - b) <= 1e-5 * n


def test_score_bf16(dev, g, ref_tokens):
    """bar: mean |error| per token <= 4.71e-3 = 4 x 1.178e-3, the error of the bf16-rounded restatement against the f32 one on this
    batch (46 tokens), measured on the CPU; the 4 x margin covers summation order and the roundings the simulation omits"""
    lm = _build(g, torch.bfloat16, dev)
    lp = lm.masked_logprobs(g["ys"], g["ylens"])
    ntok = int(g["ylens"].sum())
    err = (lp - ref_tokens).abs().sum().item() / ntok
    print(f"score bf16: mean |error| per token {err:.3e} (simulated {SCORE_BF16_SIM:.3e}, bar {SCORE_BF16_BAR:.3e})")
    assert err <= SCORE_BF16_BAR, err
    forced = lm.masked_logprobs(g["ys"], g["ylens"], max_token_rows=32)
    assert (forced - ref_tokens).abs().sum().item() / ntok <= SCORE_BF16_BAR


# ---------------------------------------------------------------- 5. masked perplexity
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ppl_masked_lm(dev, g, dtype, tmp_path):
    """f32: 1e-3 relative.  bf16: |log ppl - log ref| <= 4 x the simulated mean |error| per token on these utterances (0.988e-3 without,
    1.021e-3 with the <eos> wrappers; the mean of the errors is at most the mean of their magnitudes)"""
    from torch.utils.data import DataLoader
    from emoasr_amd.datasets import LMDataset
    from emoasr_amd.train_lm import ppl_masked_lm
    lm = _build(g, dtype, dev)
    path = tmp_path / "lm.tsv"
    path.write_text(str(g["tsv"]))
    for flag in (False, True):
        cfg = dict(BERT_CFG, bucket_shuffle=False, add_sos_eos=flag, eos_id=2, num_to_mask=1, random_num_to_mask=False)
        ds = LMDataset(SimpleNamespace(**cfg), str(path), phase="test")
        loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=ds.collate_fn)
        cnt, ppl = ppl_masked_lm(loader, lm, dev, mask_id=39, max_seq_len=BERT_CFG["max_seq_len"])
        ref = g[f"ppl/value{int(flag)}"].item()
        print(f"ppl {dtype} add_sos_eos={flag}: {cnt} tokens, {ppl:.5f} against {ref:.5f}")
        assert cnt == int(g[f"ppl/cnt{int(flag)}"])
        if dtype == torch.float32:
            assert abs(ppl - ref) < 1e-3 * ref, (ppl, ref)
        else:
            assert abs(math.log(ppl) - math.log(ref)) <= PPL_BF16_BAR[flag], (ppl, ref)
    cnt, _ = ppl_masked_lm(loader, lm, dev, max_seq_len=10)     # the 11-token utterance (9 + the wrappers) is skipped
    assert cnt == 32 - 11


# ---------------------------------------------------------------- 6. soft labels
def _teacher(g, name, dev):
    if name == "bert":
        return _build(g, torch.float32, dev)
    from emoasr_amd.modeling.lm import LM
    _, _, g3 = load_golden("l3_tiny")
    lm = LM(SimpleNamespace(**LM_CFG), compute_dtype=torch.float32)
    lm.load_state_dict(lm_state(g3))
    return lm.to(dev).eval()


@pytest.mark.parametrize("teacher", ["bert", "lm"])
def test_soft_labels(dev, g, teacher):
    from emoasr_amd import distill
    model = _teacher(g, teacher, dev)
    rows = tsv_rows(g[f"kd/{teacher}_rows"])
    make = distill.make_bert_label if teacher == "bert" else distill.make_lm_label
    for variant, (flag, msl) in KD_VARIANTS[teacher].items():
        key = f"kd/{teacher}/{variant}"
        seqs, plan = (distill.plan_bert if teacher == "bert" else distill.plan_lm)(rows, flag, 2, msl)
        ids, probs, dev_logits = distill.teacher_topk(model, seqs, plan, TOPK, TEMP, want_logits=True)
        ref = g[key + "/logits"]
        assert ids.shape == probs.shape == (ref.shape[0], TOPK) and dev_logits.shape == tuple(ref.shape)
        # exact: a stable descending sort of the SAME logits the top-k was taken of (ties to the lowest index)
        order = torch.sort(torch.from_numpy(dev_logits), dim=1, descending=True, stable=True).indices[:, :TOPK]
        assert np.array_equal(ids, order.numpy())
        # tie-robust, against the reference's logits: no row left out
        rng = ref.abs().max().item()
        ref_sorted = torch.sort(ref, dim=1, descending=True).values
        ref_probs = torch.softmax(ref_sorted[:, :TOPK] / TEMP, dim=1)
        for m in range(ref.shape[0]):
            assert len(set(ids[m].tolist())) == TOPK, (m, ids[m])
            assert (ref[m, torch.from_numpy(ids[m])] >= ref_sorted[m, TOPK - 1] - 1e-3 * rng).all(), (m, ids[m])
            assert (torch.from_numpy(np.sort(probs[m])[::-1].copy()) - ref_probs[m]).abs().max() <= 2e-3, (m, probs[m], ref_probs[m])
        # the dict: structure, hard labels and the <eos> drop as the reference's
        got, want = make(rows, model, None, TOPK, TEMP, flag, 2, msl, batch_size=3), golden_labels(g, key)
        assert list(got) == list(want)
        for utt_id in want:
            assert [len(lab) for lab in got[utt_id]] == [len(lab) for lab in want[utt_id]], (variant, utt_id)
            for a, b in zip(got[utt_id], want[utt_id]):
                assert all(isinstance(v, int) and isinstance(p, float) for v, p in a)
                assert not flag or all(v != 2 for v, _ in a)
                if len(b) == 1 and b[0][1] == 1.0:
                    assert a == b     # the hard label
    import pickle
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        got = make(rows, model, tmp + "/labels.pkl", topk=TOPK)
        with open(tmp + "/labels.pkl", "rb") as f:
            assert pickle.load(f) == got


# ---------------------------------------------------------------- 7. training step, search guard
def test_train_step_moves_everything_but_the_pooler(dev, g):
    from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
    from emoasr_amd.train_lm import train_step
    params = SimpleNamespace(**dict(BERT_CFG, learning_rate=2e-3, lr_schedule_type="lindecay", num_warmup_steps=2, weight_decay=0.01,
                                    clip_grad_norm=0.5, accum_grad=1, log_step=1))
    lm = _build(g, torch.float32, dev, train=True)
    groups = get_optimizer_params_nodecay(list(lm.named_parameters()), weight_decay=params.weight_decay)
    opt = ScheduledOptimizer(AdamW(groups, lr=0, weight_decay=params.weight_decay), params, num_total_steps=10)
    before = {n: p.detach().cpu().clone() for n, p in lm.named_parameters()}
    out = train_step(lm, opt, {"ys_in": g["ys_in"], "ylens": g["ylens"], "labels": g["labels"]}, params, dev)
    assert abs(out["loss_total"] - g["train/loss"].item()) < 1e-3 * g["train/loss"].item()
    for n, p in lm.named_parameters():
        assert torch.equal(p.detach().cpu(), before[n]) == (n in POOLER), n


def test_beam_searches_refuse_a_masked_lm(g):
    """at their entry, before the decoder or the encoder output is touched (both None here): nothing is launched"""
    from emoasr_amd.modeling.beam_search import joint_beam_search
    from emoasr_amd.modeling.beam_search_device import joint_beam_search_device
    from emoasr_amd.modeling.ctc_beam_search import ctc_prefix_beam_search
    from emoasr_amd.modeling.lm import LM
    lm = LM(SimpleNamespace(**BERT_CFG))
    for search in (joint_beam_search, joint_beam_search_device, ctc_prefix_beam_search):
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            search(None, None, None, 4, lm=lm, lm_weight=0.3)
