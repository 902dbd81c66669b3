"""CPU checks of the batched CTC prefix beam search's references and interface (no GPU): the instrumented restatement of
tests/ctc_beam_ref.py equals the oracle on every case the GPU tests use, the cases really contain the events they are meant to
cover (folds of both kinds, re-formed prefixes with a live child, exact ties, <eos>-ending prefixes, gaps above 1e-7), and the
kernel's organisation of the search (node ids instead of a table over label sequences) gives the same result bit for bit."""
import numpy as np
import pytest

from oracle import ctc_beam as ob
from tests import ctc_beam_ref as R


def _run(case):
    V, W, T, scale, lw, seed, tie = case
    lp, top = R.make_rows(seed, T, V, scale, W, tie)
    return lp, top, R.search(lp, top, W, lw)


@pytest.mark.parametrize("case", R.expand(R.ALL_CASES), ids=lambda c: "V%d-W%d-T%d-s%d" % (c[0], c[1], c[2], c[5]))
def test_restatement_equals_the_oracle(case):
    V, W, T, scale, lw, seed, tie = case
    lp, top, (hyps, scores, ev) = _run(case)
    want_h, want_s = ob.ctc_prefix_beam_search(lp.astype(np.float64), R.BLANK, R.EOS, W, lw)
    assert hyps == want_h
    np.testing.assert_allclose(scores, want_s, rtol=0, atol=1e-12)
    assert len(hyps) == min(W, len(hyps)) and all(h[0] == R.EOS for h in hyps)
    # exact order is only demanded where the reference itself is unambiguous
    print(f"folds {ev.folds} (extension first {ev.folds_ext_first}) re-formed {ev.reformed} ties {ev.ties} "
          f"eos {ev.eos_new} min gap {ev.min_gap:.3g}")
    assert ev.min_gap > 1e-7


@pytest.mark.parametrize("case", R.expand(R.ALL_CASES), ids=lambda c: "V%d-W%d-T%d-s%d" % (c[0], c[1], c[2], c[5]))
def test_node_id_merge_equals_the_label_table(case):
    """the merge argument of csrc/ctc_beam.hip: with canonical node ids, `q.parent == p.id and q.last == v` finds every pair of
    candidates the host's table over label vectors folds, and W rounds of arg-max with ties to the lower position are the stable
    sort -- same hypotheses, same order, identical doubles"""
    V, W, T, scale, lw, seed, tie = case
    lp, top, (hyps, scores, _) = _run(case)
    got_h, got_s = R.search_by_ids(lp, top, W, lw)
    assert got_h == hyps and got_s == scores


def test_fold_cases_hold_their_events():
    ext_first = stay_first = 0
    for case in R.expand(R.FOLD_CASES):
        _, _, (_, _, ev) = _run(case)
        assert ev.reformed >= 1, case          # a plain counter for prefix ids would fail on each of these seeds
        assert ev.eos_new >= 1, case
        ext_first += ev.folds_ext_first
        stay_first += ev.folds - ev.folds_ext_first
    assert ext_first >= 100 and stay_first >= 100, (ext_first, stay_first)


def test_tie_cases_hold_exact_ties():
    for case in R.expand(R.TIE_CASES):
        _, _, (_, _, ev) = _run(case)
        assert ev.ties >= 24, (case, ev.ties)                  # dozens per seed
        assert ev.min_gap > 1e-7


def test_small_vocabulary_cannot_fill_the_beam():
    lp, top, (hyps, scores, _) = _run(R.expand(R.SIZE_CASES)[2])
    assert len(hyps) == 5 < 8      # (<eos>), and <eos> + one of the four labels that are not the blank
    hyps0, scores0, _ = R.search(lp[:0], top[:0], 8)
    assert hyps0 == [[R.EOS]] and scores0 == [0.0]


def test_entry_points_are_declared_and_sized():
    from emoasr_amd import lib, ops
    h = lib.load()
    for name in ("emoasr_ctc_beam_batch", "emoasr_ctc_beam_batch_ws_bytes"):
        assert hasattr(h, name)
    assert len(lib.SIGNATURES["emoasr_ctc_beam_batch"]) == 20
    q = lambda *a: lib.size_query("emoasr_ctc_beam_batch_ws_bytes", *a)
    assert q(3, 100, 10) == 32 * (10 * 100 + 3) and q(1, 0, 1) == 32
    assert q(1, 10, 33) == -1 and q(1, 10, 0) == -1 and ops.CTC_BEAM_MAX_WIDTH == 32


def test_decoder_routing_without_a_gpu():
    """the routing decisions that need no device: an LM with a batch is refused, the switch takes two values only"""
    from types import SimpleNamespace

    import torch

    from emoasr_amd.modeling.decoders.ctc import CTCDecoder
    dec = CTCDecoder(SimpleNamespace(blank_id=0, eos_id=2, vocab_size=8, enc_hidden_size=4, kd_weight=0))
    assert dec.ctc_beam_impl == "host"
    eouts = torch.zeros(2, 3, 4)
    with pytest.raises(NotImplementedError, match="one utterance at a time"):
        dec.decode(eouts, [3, 3], beam_width=4, lm=object(), lm_weight=0.3)
    dec.ctc_beam_impl = "gpu"
    with pytest.raises(ValueError):
        dec.decode(eouts, [3, 3], beam_width=4)
    assert "ctc_beam_impl" not in dec.state_dict()
