"""The torch restatement of the RNN LM (tests/rnnlm_ref.py) against the reference's outputs (tests/golden/rnnlm_tiny.npz) at 1e-5,
and what of the feature can be checked without a GPU: LM(params) with lm_type="rnn" constructs with the reference's state-dict
layout, LMDataset collates for it as the reference does."""
from types import SimpleNamespace

import torch

from tests import rnnlm_ref as ref
from tests.rnnlm_util import PREDICT_STEPS, PREDICT_YLENS, RNNLM_CFG, rnnlm_golden, rnnlm_state


def _close(a, b, tol=1e-5):
    return (a.double() - b.double()).abs().max().item() <= tol * max(b.double().abs().max().item(), 1.0)


def test_restatement_logits_loss_and_gradients():
    g = rnnlm_golden()
    sd = {k: v.clone().requires_grad_(True) for k, v in rnnlm_state(g).items()}
    with torch.no_grad():
        lg = ref.logits(sd, g["ys_in"], g["ylens"])
    assert lg.shape == g["eval/logits"].shape and _close(lg, g["eval/logits"])
    loss = ref.loss(sd, g["ys_in"], g["ylens"], g["labels"])
    assert abs(loss.item() - g["train/loss"].item()) < 1e-5
    loss.backward()
    assert set(sd) == {k[5:] for k in g if k.startswith("grad/")}
    for k, p in sd.items():
        assert _close(p.grad, g["grad/" + k]), k
    for l in range(RNNLM_CFG["num_layers"]):
        assert torch.equal(g[f"grad/lm.rnns.bias_ih_l{l}"], g[f"grad/lm.rnns.bias_hh_l{l}"])


def test_restatement_predict_chain():
    g = rnnlm_golden()
    sd = rnnlm_state(g)
    states = None
    for k in range(PREDICT_STEPS):
        lp, states = ref.predict(sd, g["predict/ys"], PREDICT_YLENS[k], states)
        assert _close(lp, g[f"predict/{k}/logp"]), k
        assert _close(states[0], g[f"predict/{k}/h"]) and _close(states[1], g[f"predict/{k}/c"]), k


def test_lm_constructs_with_the_reference_layout():
    from emoasr_amd.modeling.lm import LM
    g = rnnlm_golden()
    lm = LM(SimpleNamespace(**RNNLM_CFG))
    assert lm.stateful is True and LM.stateful is False and lm.lm_type == "rnn"
    mine, want = lm.state_dict(), rnnlm_state(g)
    assert list(mine) == list(want)
    for k in want:
        assert tuple(mine[k].shape) == tuple(want[k].shape), k
    lm.load_state_dict(want)
    lm.load_state_dict({k[3:]: v for k, v in want.items()})      # the un-prefixed inner dict loads too
    h, c = lm.zero_states(3, "cpu")
    assert h.shape == c.shape == (RNNLM_CFG["num_layers"], 3, RNNLM_CFG["hidden_size"]) and not h.any() and not c.any()
    assert torch.equal(lm.state_dict()["lm.output.weight"], want["lm.output.weight"])


def test_lm_dataset_collates_for_the_rnn_lm(tmp_path):
    from emoasr_amd.datasets import LMDataset
    g = rnnlm_golden()
    path = tmp_path / "lm.tsv"
    path.write_text(str(g["tsv"]))
    for flag in (False, True):
        ds = LMDataset(SimpleNamespace(**dict(RNNLM_CFG, bucket_shuffle=False, add_sos_eos=flag, eos_id=2)), str(path), phase="train")
        batch = ds.collate_fn([ds[i] for i in range(len(ds))])
        assert batch["utt_ids"] == g[f"collate{int(flag)}/utt_ids"].tolist()
        for k in ("ys_in", "ylens", "labels"):
            assert torch.equal(batch[k], g[f"collate{int(flag)}/{k}"]), (flag, k)
