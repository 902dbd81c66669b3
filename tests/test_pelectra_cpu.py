"""CPU checks of P-ELECTRA (emoasr_amd/modeling/pelectra.py: lm_type "pelectra" / "pelectra-disc") against the reference's outputs
(tests/golden/pelectra_tiny*.npz, written by tests/golden/make_golden_pelectra.py): module layout and state-dict forms, the datasets'
batches, the optimizer's decay groups, the prefix view the generator's engine sees the shared arena through, and the refusals.  (The
arena itself lives on the device: that the whole model is bound to ONE is asserted in tests/test_pelectra_gpu.py.)"""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_electra_cpu import ELECTRA_CFG
from tests.test_p2w_cpu import P2W_CFG
from tests.util import golden_npz

PELECTRA_CFG = dict(P2W_CFG, lm_type="pelectra", electra_disc_weight=2.0,
                    **{k: v for k, v in ELECTRA_CFG.items() if k.startswith("disc_")})
DISC_CFG = dict(PELECTRA_CFG, lm_type="pelectra-disc")
MASK = dict(mask_proportion=0.3, random_num_to_mask=False, text_augment=False)


@pytest.fixture(scope="module")
def g():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" else v) for k, v in golden_npz("pelectra_tiny").items()}


def state(g, dtype=torch.float32):
    return {k[3:]: v.to(dtype) for k, v in g.items() if k.startswith("sd/")}


@pytest.mark.parametrize("cfg", [PELECTRA_CFG, DISC_CFG], ids=["pelectra", "pelectra-disc"])
def test_construction_and_state_dict_forms(g, cfg):
    from emoasr_amd.modeling.pelectra import PELECTRA, PELECTRAModel
    sd = state(g)
    lm = PELECTRA(SimpleNamespace(**cfg))
    assert isinstance(lm.lm, PELECTRAModel) and lm.electra_disc_weight == 2.0 and not lm.stateful and not hasattr(lm, "predict")
    assert lm.sample_head == "materialised" and lm.last_head is None and lm.forced_samples is None
    mine = lm.state_dict()
    assert set(mine) == set(sd) and len(mine) == 133
    for k in sd:
        assert tuple(mine[k].shape) == tuple(sd[k].shape), k
    subs = {k.split(".")[2] for k in mine if k.startswith("lm.gmodel.")}
    assert subs == {"encoder", "decoder"} and all(k.startswith(("lm.gmodel.", "lm.dmodel.")) for k in mine)
    forms = {"full": sd, "inner": {k[len("lm."):]: v for k, v in sd.items()}}
    for name, form in forms.items():
        fresh = PELECTRA(SimpleNamespace(**cfg))
        fresh.load_state_dict(form)
        for k, v in fresh.state_dict().items():
            assert torch.equal(v, sd[k]), (name, k)
    # the discriminator's own dict (an ElectraForPreTraining checkpoint): the discriminator is loaded, the generator left alone
    fresh = PELECTRA(SimpleNamespace(**cfg))
    before = {k: v.clone() for k, v in fresh.state_dict().items()}
    fresh.load_state_dict({k[len("lm.dmodel."):]: v for k, v in sd.items() if k.startswith("lm.dmodel.")})
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k] if k.startswith("lm.dmodel.") else before[k]), k
    with pytest.raises(RuntimeError):
        PELECTRA(SimpleNamespace(**cfg)).load_state_dict({"lm.gmodel.encoder.nothing": torch.zeros(1)})


def test_p2w_dataset_makes_pberts_batches_for_pelectra(g, tmp_path):
    from emoasr_amd.datasets import P2WDataset
    path = tmp_path / "p2w.tsv"
    path.write_text(str(g["tsv"]))
    batches = {}
    for kind in ("pelectra", "pbert"):
        ds = P2WDataset(SimpleNamespace(**dict(PELECTRA_CFG, lm_type=kind, bucket_shuffle=False, **MASK)), str(path), phase="train")
        random.seed(0)
        np.random.seed(0)
        batches[kind] = ds.collate_fn([ds[i] for i in range(len(ds))])
    batch = batches["pelectra"]
    assert list(batch) == ["utt_ids", "ps", "plens", "ys_in", "ylens", "labels"]
    for k in ("ps", "plens", "ys_in", "ylens", "labels"):
        assert torch.equal(batch[k], g[f"data/{k}"]), k
        assert torch.equal(batch[k], batches["pbert"][k]), k
    with pytest.raises(NotImplementedError, match="outside the HIP hot path"):
        P2WDataset(SimpleNamespace(**dict(PELECTRA_CFG, lm_type="pelectra-disc", bucket_shuffle=False, **MASK)), str(path))


def test_disc_dataset_makes_the_error_label_batches(g, tmp_path):
    from emoasr_amd.modeling.pelectra import disc_dataset
    path = tmp_path / "disc.tsv"
    path.write_text(str(g["disc_tsv"]))
    params = SimpleNamespace(**dict(DISC_CFG, bucket_shuffle=False))
    ds = disc_dataset(params, str(path), phase="train")
    assert params.lm_type == "pelectra-disc"     # (the caller's parameters are not touched)
    batch = ds.collate_fn([ds[i] for i in range(len(ds))])
    assert "labels" not in batch
    for k in ("ys_in", "ylens", "error_labels"):
        assert np.array_equal(batch[k].numpy(), g[f"discset/{k}"].numpy()), k


def test_adamw_decay_groups_follow_the_reference_names(g):
    """asr/optimizers.py:128-146 on the reference's names (the fixture's keys): no decay where the name contains "bias" or a
    `LayerNorm.weight`.  The rule goes by substring, so the generator's `norm*.weight` (no "LayerNorm" in the name) decay, as they do
    in the reference."""
    from emoasr_amd.modeling.pelectra import PELECTRA
    from emoasr_amd.optimizers import get_optimizer_params_nodecay
    lm = PELECTRA(SimpleNamespace(**PELECTRA_CFG))
    named = list(lm.named_parameters())
    assert {n for n, _ in named} == set(state(g))     # (nothing tied in this model: every key is a parameter)
    groups = get_optimizer_params_nodecay(named, weight_decay=0.01)
    ids = [{id(p) for p in grp["params"]} for grp in groups]
    want_nodecay = {n for n in state(g) if any(s in n for s in ("bias", "LayerNorm.bias", "LayerNorm.weight"))}
    by_id = {id(p): n for n, p in named}
    assert {by_id[i] for i in ids[1]} == want_nodecay and {by_id[i] for i in ids[0]} == set(state(g)) - want_nodecay
    assert groups[0]["weight_decay"] == 0.01 and groups[1]["weight_decay"] == 0.0
    assert any(n.startswith("lm.gmodel.") for n in want_nodecay) and any(n.startswith("lm.dmodel.") for n in want_nodecay)
    assert "lm.gmodel.decoder.norm.weight" not in want_nodecay and "lm.dmodel.electra.embeddings.LayerNorm.weight" in want_nodecay


class _FakeArena:
    """what ArenaView reads of a ParamArena, recording the names it is asked for"""

    def __init__(self, names):
        self.names = list(names)
        self.params = [torch.zeros(1) for _ in names]
        self.offsets = {n: 64 * i for i, n in enumerate(names)}
        self.pviews = {n: p for n, p in zip(names, self.params)}
        self.gviews = {n: torch.ones(1) for n in names}
        self.flat, self.grad, self.shadow, self.size, self.compute_dtype = "flat", "grad", "shadow", 64 * len(names), torch.bfloat16
        self.asked = []

    def _rec(self, *a):
        self.asked.append(a)
        return a

    w = lambda self, name, shape=None: self._rec("w", name, shape)
    g = lambda self, name, shape=None: self._rec("g", name, shape)
    w_span = lambda self, a, b, shape: self._rec("w_span", a, b, shape)
    p_span = lambda self, a, b, shape: self._rec("p_span", a, b, shape)
    g_span = lambda self, a, b, shape: self._rec("g_span", a, b, shape)
    transposed = lambda self, a, b=None, shape=None: self._rec("transposed", a, b, shape)
    attach_grads = lambda self: self._rec("attach_grads")
    refresh_shadow = lambda self: self._rec("refresh_shadow")
    bound = lambda self: True


def test_arena_view_addresses_the_prefixed_parameters():
    from emoasr_amd.engine import ArenaView
    names = ["lm.gmodel.encoder.embed.weight", "lm.gmodel.decoder.output.weight", "lm.gmodel.decoder.output.bias",
             "lm.dmodel.electra.embeddings.word_embeddings.weight"]
    A = _FakeArena(names)
    V = ArenaView(A, "lm.gmodel.")
    assert V.names == ["encoder.embed.weight", "decoder.output.weight", "decoder.output.bias"] and V.params == A.params[:3]
    assert V.offsets == {"encoder.embed.weight": 0, "decoder.output.weight": 64, "decoder.output.bias": 128}
    assert (V.flat, V.grad, V.shadow, V.size, V.compute_dtype) == ("flat", "grad", "shadow", 256, torch.bfloat16) and V.bound()
    assert V.p("decoder.output.bias") is A.params[2]
    assert V.w("decoder.output.weight") == ("w", "lm.gmodel.decoder.output.weight", None)
    assert V.g("decoder.output.bias", (1,)) == ("g", "lm.gmodel.decoder.output.bias", (1,))
    assert V.w_span("a", "b", (2, 2)) == ("w_span", "lm.gmodel.a", "lm.gmodel.b", (2, 2))
    assert V.p_span("a", "b", (2,)) == ("p_span", "lm.gmodel.a", "lm.gmodel.b", (2,))
    assert V.g_span("a", "b", (2,)) == ("g_span", "lm.gmodel.a", "lm.gmodel.b", (2,))
    assert V.transposed("a") == ("transposed", "lm.gmodel.a", None, None)
    V.attach_grads(), V.refresh_shadow()
    assert A.asked[-2:] == [("attach_grads",), ("refresh_shadow",)]


def test_refusals(g):
    from emoasr_amd.modeling.beam_search import joint_beam_search
    from emoasr_amd.modeling.ctc_beam_search import ctc_prefix_beam_search
    from emoasr_amd.modeling.lm import LM, require_next_token_lm
    from emoasr_amd.modeling.pelectra import PELECTRA
    for cfg in (PELECTRA_CFG, DISC_CFG):
        with pytest.raises(NotImplementedError, match="outside the HIP hot path"):
            LM(SimpleNamespace(**cfg))
        lm = PELECTRA(SimpleNamespace(**cfg))
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            require_next_token_lm(lm, 0.3)
        require_next_token_lm(lm, 0.0)
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            lm.zero_states(1, "cpu")
        for search in (joint_beam_search, ctc_prefix_beam_search):
            with pytest.raises(NotImplementedError, match="no next-token distribution"):
                search(None, None, None, 4, lm=lm, lm_weight=0.3)
        with pytest.raises(ValueError, match="ps"):
            lm(torch.tensor([[3, 4]]), [2], torch.tensor([[3, -100]]))
        with pytest.raises(ValueError, match="error_labels"):
            lm.forward_disc(torch.tensor([[3, 4]]), [2])
    with pytest.raises(NotImplementedError, match="PELECTRA is lm_type"):
        PELECTRA(SimpleNamespace(**dict(PELECTRA_CFG, lm_type="pbert")))
    with pytest.raises(NotImplementedError, match="absent from the config"):
        PELECTRA(SimpleNamespace(**{k: v for k, v in PELECTRA_CFG.items() if k != "disc_hidden_size"}))
