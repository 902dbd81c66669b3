"""CPU checks of the phone-to-word family: module layout, data pipeline and refusals against tests/golden/p2w_tiny*.npz (written by
tests/golden/make_golden_p2w.py from the reference), and the pure-python restatement of the token confidences."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.correct_ref import collapse_runs, fuse_ref, softmax64, token_conf_ref
from tests.util import CONFIGS, golden_npz

P2W_CFG = dict(lm_type="pbert", input_layer="embed", enc_hidden_size=128, enc_num_attention_heads=2, enc_num_layers=2,
               enc_intermediate_size=256, dec_hidden_size=128, dec_num_attention_heads=2, dec_num_layers=2,
               dec_intermediate_size=256, dropout_enc_rate=0.0, dropout_dec_rate=0.0, dropout_attn_rate=0.0, mtl_ctc_weight=0,
               lsm_prob=0, kd_weight=0, max_decode_ylen=64, vocab_size=40, src_vocab_size=12, max_seq_len=64, eos_id=2, mask_id=39,
               phone_eos_id=2, phone_mask_id=11, blank_id=0, add_sos_eos=False)
DATA_CASES = {"mask": dict(mask_proportion=0.3, random_num_to_mask=False, text_augment=False),
              "insert": dict(mask_proportion=0.3, random_num_to_mask=False, text_augment=False, mask_insert_poisson_lam=0.2),
              "aug0": dict(mask_proportion=0.3, random_num_to_mask=False, text_augment=True, textaug_max_mask_prob=0.4,
                           textaug_max_replace_prob=0),
              "aug2": dict(mask_proportion=0.3, random_num_to_mask=False, text_augment=True, textaug_max_mask_prob=0.4,
                           textaug_max_replace_prob=0.2)}


@pytest.fixture(scope="module")
def g():
    return golden_npz("p2w_tiny")


@pytest.mark.parametrize("kind", ["pbert", "pctc"])
def test_state_dict_layout_matches_reference(g, kind):
    from emoasr_amd.modeling.p2w import P2W
    lm = P2W(SimpleNamespace(**dict(P2W_CFG, lm_type=kind)))
    want = {k[len(kind) + 4:]: v.shape for k, v in g.items() if k.startswith(kind + "/sd/")}
    mine = lm.state_dict()
    assert set(mine) == set(want) and "encoder.embed.weight" in mine and not any(k.startswith("encoder.conv") for k in mine)
    for k, shape in want.items():
        assert tuple(mine[k].shape) == tuple(shape), k
    lm.load_state_dict({k: torch.from_numpy(g[f"{kind}/sd/{k}"]) for k in want})
    assert not hasattr(lm, "predict") and not hasattr(lm, "zero_states")


@pytest.mark.parametrize("name", sorted(DATA_CASES))
def test_dataset_batches_equal_the_reference(g, name, tmp_path):
    from emoasr_amd.datasets import P2WDataset
    path = tmp_path / "p2w.tsv"
    path.write_text(str(g["tsv"]))
    ds = P2WDataset(SimpleNamespace(**dict(P2W_CFG, bucket_shuffle=False, **DATA_CASES[name])), str(path), phase="train")
    random.seed(0)
    np.random.seed(0)
    batch = ds.collate_fn([ds[i] for i in range(len(ds))])
    assert list(batch) == ["utt_ids", "ps", "plens", "ys_in", "ylens", "labels"]
    for k in ("ps", "plens", "ys_in", "ylens", "labels"):
        assert batch[k].dtype == torch.int64
        assert np.array_equal(batch[k].numpy(), g[f"data/{name}/{k}"]), (name, k)
    test = P2WDataset(SimpleNamespace(**dict(P2W_CFG, bucket_shuffle=False, **DATA_CASES[name])), str(path), phase="test")
    assert "labels" not in test.collate_fn([test[0], test[1]])


def test_pctc_dataset_labels_are_the_phones(g, tmp_path):
    from emoasr_amd.datasets import P2WDataset
    path = tmp_path / "p2w.tsv"
    path.write_text(str(g["tsv"]))
    ds = P2WDataset(SimpleNamespace(**dict(P2W_CFG, lm_type="pctc", bucket_shuffle=False, text_augment=False)), str(path))
    batch = ds.collate_fn([ds[i] for i in range(len(ds))])
    assert torch.equal(batch["labels"].clamp(min=0), batch["ps"] * (batch["labels"] != -100))


def test_text_replace_fails_where_the_reference_does():
    """more replacements asked for than candidates (every position but one is <eos>): the index and value shapes differ"""
    from emoasr_amd.datasets import TextAugment
    aug = TextAugment(SimpleNamespace(textaug_max_mask_prob=0.0, textaug_max_replace_prob=1.0, src_vocab_size=12, phone_eos_id=2,
                                      phone_mask_id=11))
    x = torch.tensor([2, 2, 2, 2, 2, 2, 5, 2])
    failed = 0
    for seed in range(8):     # randint(0, 8) draws more than one replacement at most of these seeds
        random.seed(seed)
        try:
            aug(x)
        except (RuntimeError, IndexError, ValueError):
            failed += 1
    assert failed >= 4


def test_batch_sampler_respects_the_phone_budget():
    import pandas as pd
    from emoasr_amd.datasets import LMBatchSampler
    data = pd.DataFrame({"ylen": [3, 3, 3, 3, 3, 3], "plen": [10, 10, 10, 25, 5, 5]})
    params = SimpleNamespace(max_plens_batch=30, max_ylens_batch=100, batch_size=4)
    s = LMBatchSampler(SimpleNamespace(data=data), params)
    assert sorted(s.indices_batches) == [[0, 1, 2], [3, 4], [5]] and len(s) == 3
    assert sorted(sum(list(s), [])) == list(range(6))
    s = LMBatchSampler(SimpleNamespace(data=data[["ylen"]]), SimpleNamespace(max_ylens_batch=7, batch_size=4))
    assert sorted(s.indices_batches) == [[0, 1], [2, 3], [4, 5]]


def test_out_of_scope_variants_raise():
    from emoasr_amd.datasets import P2WDataset
    from emoasr_amd.modeling.asr import ASR
    from emoasr_amd.modeling.encoders.transformer import TransformerEncoder
    from emoasr_amd.modeling.p2w import P2W
    with pytest.raises(NotImplementedError, match="outside the HIP hot path"):
        P2W(SimpleNamespace(**dict(P2W_CFG, lm_type="ptransformer")))
    with pytest.raises(NotImplementedError, match="outside the HIP hot path"):
        P2WDataset(SimpleNamespace(**dict(P2W_CFG, lm_type="ptransformer")), "nowhere.tsv")
    with pytest.raises(NotImplementedError):
        TransformerEncoder(SimpleNamespace(**P2W_CFG), is_conformer=True)
    with pytest.raises(NotImplementedError):
        TransformerEncoder(SimpleNamespace(**dict(P2W_CFG, input_layer="linear", feat_dim=40, num_framestacks=1)))
    with pytest.raises(NotImplementedError, match="intermediate or phone CTC"):
        TransformerEncoder(SimpleNamespace(**dict(P2W_CFG, mtl_inter_ctc_weight=0.3, inter_ctc_layer_id=1)))
    with pytest.raises(NotImplementedError):
        ASR(SimpleNamespace(**dict(CONFIGS["l2_tiny"], encoder_type="rnn", input_layer="embed", src_vocab_size=12)))


def test_beam_searches_refuse_a_p2w():
    from emoasr_amd.modeling.beam_search import joint_beam_search
    from emoasr_amd.modeling.beam_search_device import joint_beam_search_device
    from emoasr_amd.modeling.ctc_beam_search import ctc_prefix_beam_search
    from emoasr_amd.modeling.lm import require_next_token_lm
    from emoasr_amd.modeling.p2w import P2W
    for kind in ("pbert", "pctc"):
        lm = P2W(SimpleNamespace(**dict(P2W_CFG, lm_type=kind)))
        with pytest.raises(NotImplementedError, match="no next-token distribution"):
            require_next_token_lm(lm, 0.3)
        for search in (joint_beam_search, joint_beam_search_device, ctc_prefix_beam_search):
            with pytest.raises(NotImplementedError, match="no next-token distribution"):
                search(None, None, None, 4, lm=lm, lm_weight=0.3)
        require_next_token_lm(lm, 0)


def test_phone_beam_search_stays_refused():
    from emoasr_amd.modeling.decoders.ctc import CTCDecoder
    dec = CTCDecoder(SimpleNamespace(**dict(CONFIGS["l2_tiny"], mtl_phone_ctc_weight=0.3, hie_mtl_phone=True, phone_vocab_size=12,
                                            inter_ctc_layer_id=1)))
    assert dec.phone_output.weight.shape == (12, CONFIGS["l2_tiny"]["enc_hidden_size"])
    with pytest.raises(NotImplementedError, match="greedy only"):
        dec.decode(None, None, None, beam_width=4, decode_phone=True)


def test_token_confidence_restatement():
    """the pure-python collapse + segment arg-max the kernel tests compare against, on a hand-made path"""
    probs = softmax64(np.log(np.array([[.1, .8, .1], [.2, .7, .1], [.9, .05, .05], [.1, .6, .3], [.1, .6, .3], [.1, .2, .7]])))
    path = [1, 1, 0, 1, 1, 2, 2, 2]      # length 6: the last two frames are padding
    assert collapse_runs(path, 6, 0) == [(1, [0, 1]), (1, [3, 4]), (2, [5])]
    ids, frames, confs, gaps = token_conf_ref(probs, path, 6, 0)
    assert ids == [1, 1, 2] and frames == [0, 3, 5]      # (the tie of frames 3 and 4 goes to the earlier one)
    np.testing.assert_allclose(confs, [0.8, 0.6, 0.7], rtol=1e-12)
    assert gaps[1] == 0.0 and gaps[2] == float("inf")
    assert token_conf_ref(probs, [0] * 6, 6, 0)[0] == [] and collapse_runs(path, 0, 0) == []
    ids, val, margin = fuse_ref(np.log(probs[:2]), np.log(probs[4:6]), 0.5, 3)
    assert ids.tolist() == [1, 1] and np.allclose(val, [0.7, 0.45]) and np.allclose(margin, [0.5, 0.05])


# ---- the f64 restatement (tests/p2w_ref.py) against the reference's values -----------------------------------------------------------
def _sd(g, kind, dtype=torch.float64, grad=False):
    return {k[len(kind) + 4:]: torch.from_numpy(v).to(dtype).requires_grad_(grad) for k, v in g.items() if k.startswith(kind + "/sd/")}


def test_restatement_agrees_with_the_reference(g):
    """losses, logits and gradients to 1e-5 (gradients: of the largest gradient entry of the model)"""
    from tests import p2w_ref
    t = {k: torch.from_numpy(g[k]) for k in ("ys", "ys_in", "labels", "ps")}
    yl, pl = g["ylens"].tolist(), g["plens"].tolist()
    sd = _sd(g, "pbert", grad=True)
    lg = p2w_ref.pbert_logits(sd, t["ys_in"], yl, t["ps"], pl)
    ref = torch.from_numpy(g["pbert/logits"]).double()
    for b, n in enumerate(yl):
        assert ((lg[b, :n].detach() - ref[b, :n]).abs().max() / ref.abs().max()).item() <= 1e-5
    loss = p2w_ref.pbert_loss(sd, t["ys_in"], yl, t["labels"], t["ps"], pl)
    assert abs(loss.item() - float(g["pbert/loss"])) <= 1e-5 * float(g["pbert/loss"])
    loss.backward()
    sdc = _sd(g, "pctc", grad=True)
    lossc = p2w_ref.pctc_loss(sdc, t["ys"], yl, t["ps"], pl)
    assert abs(lossc.item() - float(g["pctc/loss"])) <= 1e-5 * float(g["pctc/loss"])
    lossc.backward()
    for kind, params in (("pbert", sd), ("pctc", sdc)):
        assert len(g[kind + "/grad_absent"]) == 0
        gmax = max(np.abs(v).max() for k, v in g.items() if k.startswith(kind + "/grad/"))
        for k, p in params.items():
            err = (p.grad - torch.from_numpy(g[f"{kind}/grad/{k}"]).double()).abs().max().item() / gmax
            assert err <= 1e-5, (kind, k, err)
    hyps = p2w_ref.greedy(p2w_ref.pctc_logits(sdc, t["ps"], pl).detach(), pl)
    assert sum(hyps, []) == g["pctc/hyps"].tolist() and [len(h) for h in hyps] == g["pctc/hyp_lens"].tolist()


def test_bf16_logit_error_constant(g):
    """tests/test_p2w_gpu.py holds the bf16 logits to 4 x the error of this simulation: the restatement with weights and stored
    activations rounded to bf16 against itself in f32, largest |difference| over the valid rows, of the f32 logits' range"""
    from tests import p2w_ref
    from tests.test_p2w_gpu import PBERT_LOGITS_BF16_SIM
    ys_in, ps = torch.from_numpy(g["ys_in"]), torch.from_numpy(g["ps"])
    yl, pl = g["ylens"].tolist(), g["plens"].tolist()
    sd32 = _sd(g, "pbert", torch.float32)
    sdb = {k: v.to(torch.bfloat16).float() for k, v in sd32.items()}
    a = p2w_ref.pbert_logits(sd32, ys_in, yl, ps, pl)
    b = p2w_ref.pbert_logits(sdb, ys_in, yl, ps, pl, round_to=torch.bfloat16)
    sim = max(((a[i, :n] - b[i, :n]).abs().max() / a.abs().max()).item() for i, n in enumerate(yl))
    assert abs(sim - PBERT_LOGITS_BF16_SIM) <= 0.02 * PBERT_LOGITS_BF16_SIM, sim


def test_confidence_restatement_agrees_with_the_reference():
    """tests/correct_ref.py's collapse + segment arg-max -- the oracle of every ctc_token_conf GPU test -- on the recogniser logits
    and greedy paths the fixture records, against the token_probs_v of the reference's aggregate_logits (f32 soft-max: 1e-6)"""
    c = golden_npz("p2w_tiny_correct")
    for u in range(3):
        logits, aligns = c[f"u{u}/logits"], c[f"u{u}/aligns"]
        assert logits.shape == (len(aligns), 40)
        ids, frames, confs, _ = token_conf_ref(softmax64(logits), aligns, len(aligns), 0)
        assert ids == c[f"u{u}/hyp"].tolist()
        np.testing.assert_allclose(confs, c[f"u{u}/token_probs_v"], rtol=1e-6)
        assert all(aligns[t] == v for t, v in zip(frames, ids))
        masked = np.asarray(confs) < float(c["mask_th"])
        assert (np.where(masked, 39, ids) == c[f"u{u}/hyp_masked"]).all() and masked.any() and not masked.all()
