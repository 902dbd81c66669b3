"""Host side of Transformer-LM training against the reference's outputs (tests/golden/lm_train_tiny, written by
tests/golden/make_golden_lm.py): the LM dataset and its collate function, the optimizer's two parameter groups, and the AdamW
front end accepting them.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from emoasr_amd.datasets import LMDataset
from emoasr_amd.optimizers import AdamW, ScheduledOptimizer, get_optimizer_params_nodecay
from tests.util import LM_CFG, golden_npz


@pytest.fixture(scope="module")
def g():
    return golden_npz("lm_train_tiny")


@pytest.fixture()
def tsv(g, tmp_path):
    path = tmp_path / "lm.tsv"
    path.write_text(str(g["tsv"]))
    return str(path)


def _lm():
    from emoasr_amd.modeling.lm import LM
    return LM(SimpleNamespace(**LM_CFG))


@pytest.mark.parametrize("add_sos_eos", [False, True])
def test_dataset_and_collate_equal_the_reference(g, tsv, add_sos_eos):
    params = SimpleNamespace(**dict(LM_CFG, bucket_shuffle=False, add_sos_eos=add_sos_eos, eos_id=2))
    ds = LMDataset(params, tsv, phase="train")
    assert len(ds) == 4
    batch = ds.collate_fn([ds[i] for i in range(len(ds))])
    k = f"collate{int(add_sos_eos)}/"
    assert batch["utt_ids"] == [str(u) for u in g[k + "utt_ids"]]
    for name in ("ys_in", "ylens", "labels"):
        assert batch[name].dtype == torch.int64
        assert np.array_equal(batch[name].numpy(), g[k + name]), name
    # any other phase: the whole sequence as input, no labels (what ppl_lm reads)
    item = LMDataset(params, tsv, phase="test")[1]
    assert item[3] is None and item[2] == (3 + 2 * int(add_sos_eos))
    assert "labels" not in LMDataset(params, tsv, phase="test").collate_fn([item])


def test_dataset_rejects_other_lm_types(tsv):
    with pytest.raises(NotImplementedError):
        LMDataset(SimpleNamespace(**dict(LM_CFG, lm_type="bert", add_sos_eos=False, eos_id=2)), tsv)


def test_nodecay_groups_equal_the_reference(g):
    lm = _lm()
    groups = get_optimizer_params_nodecay(list(lm.named_parameters()), weight_decay=0.01)
    name_of = {id(p): n for n, p in lm.named_parameters()}
    assert [name_of[id(p)] for p in groups[0]["params"]] == [str(n) for n in g["nodecay/decay"]]
    assert [name_of[id(p)] for p in groups[1]["params"]] == [str(n) for n in g["nodecay/nodecay"]]
    assert groups[0]["weight_decay"] == 0.01 and groups[1]["weight_decay"] == 0.0


def test_adamw_accepts_two_groups_and_speaks_torch_layout():
    lm = _lm()
    groups = get_optimizer_params_nodecay(list(lm.named_parameters()), weight_decay=0.01)
    opt = AdamW(groups, lr=0, weight_decay=0.01)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0]
    sd = opt.state_dict()       # before the model is on a device: empty state, torch's group layout
    n0, n1 = len(groups[0]["params"]), len(groups[1]["params"])
    assert sd["state"] == {} and [g["params"] for g in sd["param_groups"]] == [list(range(n0)), list(range(n0, n0 + n1))]
    ref = torch.optim.AdamW(get_optimizer_params_nodecay(list(lm.named_parameters()), weight_decay=0.01), lr=0, weight_decay=0.01)
    ref.load_state_dict(sd)
    sched = ScheduledOptimizer(opt, SimpleNamespace(lr_schedule_type="lindecay", learning_rate=2e-3, num_warmup_steps=2),
                               num_total_steps=10)
    sched._step = 3
    sched._publish(sched.rate(3))
    assert [g["lr"] for g in opt.param_groups] == [2e-3 * 7 / 8] * 2


def test_lm_still_rejects_other_types_and_exposes_dropout():
    from emoasr_amd.modeling.lm import LM
    with pytest.raises(NotImplementedError):
        LM(SimpleNamespace(**dict(LM_CFG, lm_type="rnn")))
    lm = _lm()
    assert lm.hidden_dropout_prob == 0.1 and lm.attention_probs_dropout_prob == 0.1
    assert hasattr(lm, "score") and hasattr(lm, "forward")
