"""CPU checks of ELECTRA (lm_type="electra" / "electra-disc") against the reference's outputs (tests/golden/electra_tiny:
tests/golden/make_golden_electra.py): the restatement tests/electra_ref.py that the GPU tests and the bf16 bars lean on, the module's
construction and state-dict forms, and the dataset's batches."""
import random
from types import SimpleNamespace

import pytest
import torch

from tests import electra_ref
from tests.util import LM_CFG, golden_npz

ELECTRA_CFG = dict(lm_type="electra", vocab_size=LM_CFG["vocab_size"], max_seq_len=LM_CFG["max_seq_len"], mask_id=39,
                   electra_disc_weight=2.0,
                   gen_embedding_size=128, gen_hidden_size=64, gen_num_layers=2, gen_num_attention_heads=1, gen_intermediate_size=128,
                   disc_embedding_size=128, disc_hidden_size=128, disc_num_layers=2, disc_num_attention_heads=2,
                   disc_intermediate_size=256)
DISC_CFG = dict(ELECTRA_CFG, lm_type="electra-disc")
MASK_CONFIGS = {"num2": (dict(num_to_mask=2, random_num_to_mask=False), False),
                "prop": (dict(mask_proportion=0.3, random_num_to_mask=False), True)}
TIED = "lm.gmodel.electra.embeddings.word_embeddings.weight"
ALIAS = "lm.gmodel.generator_lm_head.weight"     # the tied weight's second name: in the state dict, not among the parameters


@pytest.fixture(scope="module")
def g():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" else v) for k, v in golden_npz("electra_tiny").items()}


def state(g, dtype=torch.float64):
    return {k[3:]: v.to(dtype) for k, v in g.items() if k.startswith("sd/")}


def grads_of(g, key):
    return {k[len(key) + 1:]: v for k, v in g.items() if k.startswith(key + "/")}


# ---------------------------------------------------------------- the restatement
def test_restatement_matches_the_reference(g):
    """f64 restatement on the reference's f32 weights against its f32 outputs, with the samples the reference drew: 1e-5 relative
    for the losses, 1e-5 of the largest gradient entry for every gradient"""
    sd = {k: v.requires_grad_(True) for k, v in state(g).items()}
    total, lg, ld, n_rep, n_mask = electra_ref.loss(sd, g["ys_in"], g["ylens"], g["labels"], g["sample_ids"],
                                                    ELECTRA_CFG["electra_disc_weight"])
    for got, key in ((total, "loss"), (lg, "loss_gen"), (ld, "loss_disc")):
        ref = g["train/" + key].item()
        assert abs(got.item() - ref) <= 1e-5 * abs(ref), (key, got.item(), ref)
    assert abs(n_rep - g["train/num_replaced"].item()) < 1e-6 and abs(n_mask - g["train/num_masked"].item()) < 1e-6
    total.backward()
    ref_grads = grads_of(g, "grad")
    assert [str(n) for n in g["grad_absent"]] == []
    gmax = max(v.abs().max().item() for v in ref_grads.values())
    n_checked = 0
    for k, p in sd.items():
        if k == ALIAS:
            assert p.grad is None and k not in ref_grads
            continue
        assert (p.grad - ref_grads[k].double()).abs().max() <= 1e-5 * gmax, k
        n_checked += 1
    assert n_checked == len(ref_grads) == 85
    # the discriminator alone
    sd = {k: v.requires_grad_(True) for k, v in state(g).items()}
    loss = electra_ref.disc_loss(sd, g["ys"], g["ylens"], g["disc/error_labels"])
    assert abs(loss.item() - g["disc/loss"].item()) <= 1e-5 * g["disc/loss"].item()
    loss.backward()
    ref_grads = grads_of(g, "disc_grad")
    absent = {str(n) for n in g["disc_grad_absent"]}
    assert absent == {k for k in sd if k.startswith("lm.gmodel.") and k != ALIAS}
    gmax = max(v.abs().max().item() for v in ref_grads.values())
    for k, p in sd.items():
        if k in absent or k == ALIAS:
            assert p.grad is None, k
        else:
            assert (p.grad - ref_grads[k].double()).abs().max() <= 1e-5 * gmax, k
    with torch.no_grad():
        sd = state(g)
        many = electra_ref.score(sd, g["ys"], g["ylens"])
        n1 = int(g["ylens"][1])
        one = electra_ref.score(sd, g["ys"][1:2, :n1], g["ylens"][1:2])
    for a, b, n in zip(many, g["score/values"].tolist(), g["ylens"].tolist()):
        assert a < 0 and abs(a - b) <= 1e-5 * n, (a, b)
    assert one[0] > 0 and abs(one[0] - g["score/single"].item()) <= 1e-5 * n1
    assert abs(one[0] + many[1]) <= 1e-5 * n1     # the sign quirk: the same row, alone and in a batch


# ---------------------------------------------------------------- construction
@pytest.mark.parametrize("cfg", [ELECTRA_CFG, DISC_CFG], ids=["electra", "electra-disc"])
def test_construction_and_state_dict_forms(g, cfg):
    from emoasr_amd.modeling.lm import LM, ELECTRAModel
    sd = state(g, torch.float32)
    lm = LM(SimpleNamespace(**cfg))
    assert isinstance(lm.lm, ELECTRAModel) and lm.mask_id == 39 and lm.electra_disc_weight == 2.0 and not lm.stateful
    mine = lm.state_dict()
    assert list(mine) == list(sd) and len(mine) == 86
    for k in sd:
        assert tuple(mine[k].shape) == tuple(sd[k].shape), k
    assert lm.lm.gmodel.generator_lm_head.weight is lm.lm.gmodel.electra.embeddings.word_embeddings.weight
    assert hasattr(lm.lm.gmodel.electra, "embeddings_project") and not hasattr(lm.lm.dmodel.electra, "embeddings_project")
    assert lm.lm.gmodel.generator_predictions.LayerNorm.eps == 1e-5 and lm.lm.gmodel.electra.embeddings.LayerNorm.eps == 1e-12
    assert not any("pooler" in k for k in mine)
    forms = {"full": sd, "inner": {k[len("lm."):]: v for k, v in sd.items()}}
    for name, form in forms.items():
        fresh = LM(SimpleNamespace(**cfg))
        fresh.load_state_dict(form)
        for k, v in fresh.state_dict().items():
            assert torch.equal(v, sd[k]), (name, k)
    # the discriminator's own dict (an ElectraForPreTraining checkpoint): the discriminator is loaded, the generator left alone
    fresh = LM(SimpleNamespace(**cfg))
    before = {k: v.clone() for k, v in fresh.state_dict().items()}
    fresh.load_state_dict({k[len("lm.dmodel."):]: v for k, v in sd.items() if k.startswith("lm.dmodel.")})
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k] if k.startswith("lm.dmodel.") else before[k]), k
    with pytest.raises(RuntimeError):
        LM(SimpleNamespace(**cfg)).load_state_dict({"lm.gmodel.electra.nothing": torch.zeros(1)})


def test_heads_must_be_64_wide():
    from emoasr_amd.modeling.lm import LM
    with pytest.raises(AssertionError, match="heads 64 wide"):
        LM(SimpleNamespace(**dict(ELECTRA_CFG, gen_num_attention_heads=2)))


def test_no_next_token_distribution_and_labels_needed():
    from emoasr_amd.modeling.lm import LM, require_next_token_lm
    for cfg in (ELECTRA_CFG, DISC_CFG):
        lm = LM(SimpleNamespace(**cfg))
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            lm.predict(torch.tensor([[3, 4]]), [2])
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            lm.predict_device(torch.tensor([[3, 4]]), [2])
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            lm.zero_states(1, "cpu")
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            require_next_token_lm(lm, 0.3)
        require_next_token_lm(lm, 0.0)
        with pytest.raises(ValueError, match="labels"):
            lm(torch.tensor([[3, 4]]), [2])
        with pytest.raises(ValueError, match="error_labels"):
            lm.forward_disc(torch.tensor([[3, 4]]), [2])


def test_other_families_stay_refused():
    from emoasr_amd.datasets import LMDataset
    from emoasr_amd.modeling.lm import LM
    for t in ("pelectra", "pelectra-disc", "pbert", "ptransformer", "pctc"):
        with pytest.raises(NotImplementedError, match="outside the HIP hot path"):
            LM(SimpleNamespace(**dict(ELECTRA_CFG, lm_type=t)))
        with pytest.raises(NotImplementedError, match="outside the HIP hot path"):
            LMDataset(SimpleNamespace(**dict(ELECTRA_CFG, lm_type=t)), "nowhere.tsv")
    with pytest.raises(NotImplementedError, match="absent from the config"):
        LM(SimpleNamespace(**{k: v for k, v in ELECTRA_CFG.items() if k != "gen_embedding_size"}))


# ---------------------------------------------------------------- dataset
@pytest.mark.parametrize("name", list(MASK_CONFIGS))
def test_dataset_masks_as_the_reference(g, name, tmp_path):
    from emoasr_amd.datasets import LMDataset
    path = tmp_path / "lm.tsv"
    path.write_text(str(g["tsv"]))
    mask_cfg, flag = MASK_CONFIGS[name]
    ds = LMDataset(SimpleNamespace(**dict(ELECTRA_CFG, bucket_shuffle=False, add_sos_eos=flag, eos_id=2, **mask_cfg)), str(path), phase="train")
    random.seed(0)
    batch = ds.collate_fn([ds[i] for i in range(len(ds))])
    assert set(batch) == {"utt_ids", "ys_in", "ylens", "labels"}
    for k in ("ys_in", "ylens", "labels"):
        assert torch.equal(batch[k], g[f"mask/{name}/{k}"]), (k, batch[k], g[f"mask/{name}/{k}"])
    masked = batch["labels"] != -100
    assert (batch["ys_in"][masked] == 39).all() and masked.any(dim=1).all()


def test_dataset_error_labels(g, tmp_path):
    from emoasr_amd.datasets import LMDataset
    path = tmp_path / "disc.tsv"
    path.write_text(str(g["disc_tsv"]))
    ds = LMDataset(SimpleNamespace(**dict(DISC_CFG, bucket_shuffle=False, add_sos_eos=False, eos_id=2)), str(path), phase="train")
    batch = ds.collate_fn([ds[i] for i in range(len(ds))])
    assert set(batch) == {"utt_ids", "ys_in", "ylens", "error_labels"}
    for k in ("ys_in", "ylens", "error_labels"):
        assert torch.equal(batch[k], g[f"discset/{k}"]) and batch[k].dtype == g[f"discset/{k}"].dtype, k
    err = batch["error_labels"]
    assert err[0].tolist()[:7] == [0, 0, 1, 0, 0, 1, 0] and (err[1, 3:] == -100).all() and err[2, :5].sum() == 0
