"""CPU checks of the BERT masked LM (lm_type="bert") against the reference's outputs (tests/golden/bert_tiny:
tests/golden/make_golden_bert.py): the restatement tests/bert_ref.py that the GPU tests and the bf16 bars lean on, the module's
construction and state-dict forms, the dataset's masking and the host part of the soft-label generator."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bert_ref
from tests.util import LM_CFG, golden_npz, load_golden, lm_state

BERT_CFG = dict(LM_CFG, lm_type="bert", mask_id=39)
TOPK, TEMP = 4, 3.0
MASK_CONFIGS = {"num2": (dict(num_to_mask=2, random_num_to_mask=False), False),
                "prop": (dict(mask_proportion=0.3, random_num_to_mask=False), True),
                "rand": (dict(mask_proportion=0.5, random_num_to_mask=True), False)}
KD_VARIANTS = {"bert": {"plain": (False, 256), "eos": (True, 256), "ctx": (True, 10)},
               "lm": {"plain": (False, 256), "eos": (True, 256), "ctx": (True, 8)}}


@pytest.fixture(scope="module")
def g():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" else v) for k, v in golden_npz("bert_tiny").items()}


def state(g, dtype=torch.float64):
    return {k[3:]: v.to(dtype) for k, v in g.items() if k.startswith("sd/")}


def golden_labels(g, key):
    """the arrays of make_golden_bert.pack_labels -> {utt_id: [[(v, p), ...], ...]}"""
    out, o = {}, 0
    ids, probs = g[key + "/ids"].tolist(), g[key + "/probs"].tolist()
    for utt_id, n in zip(g[key + "/utt_ids"].tolist(), g[key + "/lens"].tolist()):
        out.setdefault(str(utt_id), []).append(list(zip(ids[o:o + n], probs[o:o + n])))
        o += n
    return out


def tsv_rows(text):
    lines = str(text).strip().split("\n")
    cols = lines[0].split("\t")
    return [dict(zip(cols, line.split("\t"))) for line in lines[1:]]


def assert_labels_equal(got, want, ptol):
    assert list(got) == list(want)
    for utt_id in want:
        assert len(got[utt_id]) == len(want[utt_id]), utt_id
        for a, b in zip(got[utt_id], want[utt_id]):
            assert [v for v, _ in a] == [v for v, _ in b], (utt_id, a, b)
            assert all(abs(p - q) <= ptol for (_, p), (_, q) in zip(a, b)), (utt_id, a, b)


# ---------------------------------------------------------------- the restatement
def test_restatement_matches_the_reference(g):
    """f64 restatement on the reference's f32 weights against its f32 outputs: 1e-5 of each quantity's range"""
    sd = {k: v.requires_grad_(True) for k, v in state(g).items()}
    with torch.no_grad():
        lg = bert_ref.logits(sd, g["ys_in"], g["ylens"])
    ref = g["eval/logits"].double()
    assert lg.shape == ref.shape
    assert (lg - ref).abs().max() <= 1e-5 * ref.abs().max()
    loss = bert_ref.loss(sd, g["ys_in"], g["ylens"], g["labels"])
    assert abs(loss.item() - g["train/loss"].item()) <= 1e-5 * abs(g["train/loss"].item())
    loss.backward()
    absent = {str(n) for n in g["grad_absent"]}
    assert absent == {"lm.bert.bert.pooler.dense.weight", "lm.bert.bert.pooler.dense.bias"}
    gmax = max(g[k].abs().max().item() for k in g if k.startswith("grad/"))
    aliases = {"lm.bert.cls.predictions.decoder.weight", "lm.bert.cls.predictions.decoder.bias"}     # the tied weight, the head's bias
    n_checked = 0
    for k, p in sd.items():
        if k in absent or k in aliases:
            assert p.grad is None and "grad/" + k not in g, k
            continue
        assert (p.grad - g["grad/" + k].double()).abs().max() <= 1e-5 * gmax, k
        n_checked += 1
    assert n_checked == 46 - 4
    with torch.no_grad():
        sc = bert_ref.score(sd, g["ys"], g["ylens"], BERT_CFG["mask_id"])
    for a, b, n in zip(sc, g["score/values"].tolist(), g["ylens"].tolist()):
        assert abs(a - b) <= 1e-5 * n, (a, b)


def test_restatement_covers_the_causal_lm():
    """the same code with causal=True and the Transformer LM's keys reproduces that LM's golden logits (what it is parametrised for)"""
    _, _, g3 = load_golden("l3_tiny")
    gl = golden_npz("lm_train_tiny")
    sd = {k: v.double() for k, v in lm_state(g3).items()}
    lg = bert_ref.logits(sd, torch.from_numpy(gl["ys_in"]), torch.from_numpy(gl["ylens"]), causal=True, root="lm.transformer.")
    ref = torch.from_numpy(gl["eval/logits"]).double()
    assert (lg - ref).abs().max() <= 1e-5 * ref.abs().max()


# ---------------------------------------------------------------- construction
def test_construction_and_state_dict_forms(g):
    from emoasr_amd.modeling.lm import LM, BERTMaskedLM
    sd = state(g, torch.float32)
    lm = LM(SimpleNamespace(**BERT_CFG))
    assert isinstance(lm.lm, BERTMaskedLM) and lm.mask_id == 39 and lm.lm.mask_id == 39 and not lm.stateful
    mine = lm.state_dict()
    assert list(mine) == list(sd) and len(mine) == 46
    for k in sd:
        assert tuple(mine[k].shape) == tuple(sd[k].shape), k
    assert lm.lm.bert.cls.predictions.decoder.weight is lm.lm.bert.bert.embeddings.word_embeddings.weight
    forms = {"full": sd, "inner": {k[len("lm."):]: v for k, v in sd.items()}, "bare": {k[len("lm.bert."):]: v for k, v in sd.items()}}
    for name, form in forms.items():
        fresh = LM(SimpleNamespace(**BERT_CFG))
        fresh.load_state_dict(form)
        for k, v in fresh.state_dict().items():
            assert torch.equal(v, sd[k]), (name, k)
    with pytest.raises(RuntimeError):
        LM(SimpleNamespace(**BERT_CFG)).load_state_dict({"lm.bert.bert.nothing": torch.zeros(1)})


def test_no_next_token_distribution():
    from emoasr_amd.modeling.lm import LM
    lm = LM(SimpleNamespace(**BERT_CFG))
    with pytest.raises(NotImplementedError, match="no next-token distribution"):
        lm.predict(torch.tensor([[3, 4]]), [2])
    with pytest.raises(NotImplementedError, match="no next-token distribution"):
        lm.zero_states(1, "cpu")
    with pytest.raises(AssertionError):     # and the causal LM has no masked scores
        LM(SimpleNamespace(**LM_CFG)).masked_logprobs(torch.tensor([[3, 4]]), [2])


# ---------------------------------------------------------------- dataset
@pytest.mark.parametrize("name", list(MASK_CONFIGS))
def test_dataset_masks_as_the_reference(g, name, tmp_path):
    from emoasr_amd.datasets import LMDataset
    path = tmp_path / "lm.tsv"
    path.write_text(str(g["tsv"]))
    mask_cfg, flag = MASK_CONFIGS[name]
    ds = LMDataset(SimpleNamespace(**dict(BERT_CFG, bucket_shuffle=False, add_sos_eos=flag, eos_id=2, **mask_cfg)), str(path), phase="train")
    random.seed(0)
    items = [ds[i] for i in range(len(ds))]
    assert all(it[3].dtype == torch.int64 for it in items)
    batch = ds.collate_fn(items)
    for k in ("ys_in", "ylens", "labels"):
        assert torch.equal(batch[k], g[f"mask/{name}/{k}"]), (k, batch[k], g[f"mask/{name}/{k}"])
    masked = batch["labels"] != -100
    assert (batch["ys_in"][masked] == 39).all() and masked.any(dim=1).all()
    test = LMDataset(SimpleNamespace(**dict(BERT_CFG, bucket_shuffle=False, add_sos_eos=flag, eos_id=2, **mask_cfg)), str(path), phase="test")
    utt, y_in, ylen, label = test[0]
    assert label is None and y_in.tolist() == ([2] if flag else []) + [5, 9, 12, 7, 30, 31, 4] + ([2] if flag else [])


def test_dataset_needs_exactly_one_mask_setting(g, tmp_path):
    from emoasr_amd.datasets import LMDataset
    path = tmp_path / "lm.tsv"
    path.write_text(str(g["tsv"]))
    base = dict(BERT_CFG, bucket_shuffle=False, add_sos_eos=False, eos_id=2, random_num_to_mask=False)
    for extra in ({}, dict(num_to_mask=2, mask_proportion=0.3)):
        with pytest.raises(AssertionError):
            LMDataset(SimpleNamespace(**dict(base, **extra)), str(path))


# ---------------------------------------------------------------- label generator, host part
@pytest.mark.parametrize("teacher", ["bert", "lm"])
@pytest.mark.parametrize("variant", ["plain", "eos", "ctx"])
def test_label_assembly_reproduces_the_reference(g, teacher, variant):
    """the reference's logits rows through torch's sort / soft-max, then our offsets, <eos> filter and dict assembly"""
    from emoasr_amd import distill
    flag, msl = KD_VARIANTS[teacher][variant]
    rows = tsv_rows(g[f"kd/{teacher}_rows"])
    seqs, plan = (distill.plan_bert if teacher == "bert" else distill.plan_lm)(rows, flag, 2, msl)
    key = f"kd/{teacher}/{variant}"
    logits = g[key + "/logits"]
    assert logits.shape[0] == sum(1 for p in plan if p[2] is not None)
    o_sorted, v_sorted = torch.sort(logits, dim=1, descending=True)
    ids, probs = v_sorted[:, :TOPK].numpy(), torch.softmax(o_sorted[:, :TOPK] / TEMP, dim=1).numpy()
    got = distill.assemble({}, plan, ids, probs, flag, 2)
    want = golden_labels(g, key)
    assert_labels_equal(got, want, 1e-6)
    lens = [len(lab) for per in got.values() for lab in per]
    if teacher == "lm":
        assert len(got["utt-a"]) == 5 and (variant != "plain" or got["utt-a"][0] == [(5, 1.0)])
        if variant == "ctx":     # the 7- and 9-token rows kept their positions and lost their ends: the hard label is <eos>, dropped
            assert got["utt-a"][0] == [] and got["utt-d"][0] == [] and seqs[4] == [2, 14, 33, 10, 19, 22, 28, 36, 2]
    else:
        assert len(got["utt-a"]) == 2
        if variant == "ctx":
            assert seqs[4] == [2, 14, 33, 10, 39, 22, 28, 36, 2] and plan[4][2] == 4 and plan[0][2] == 3
    if flag:
        assert min(lens) < TOPK     # an <eos> entry was dropped, and the rest was not renormalised
        short = [lab for per in got.values() for lab in per if 0 < len(lab) < TOPK]
        assert short and all(sum(p for _, p in lab) < 1.0 - 1e-3 for lab in short)
    else:
        assert all(n == TOPK or n == 1 for n in lens)
