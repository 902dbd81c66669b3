"""CPU checks of the transducer beam search with the bookkeeping on the device (no GPU): the restatement of tests/rnnt_beam_ref.py
returns the reference's golden hypotheses with the oracle's network as scorer, the kernel's organisation of the search (node ids,
W rounds of arg-max, recycled state slots) equals it bit for bit on synthetic scorers that really hold merges, re-formed prefixes
and exact ties, no destination slot is ever one that is still referenced, and the interface is declared, sized and routed."""
import os

import numpy as np
import pytest
import torch

from tests import rnnt_beam_ref as R


def _oracle_scorer(sd, cfg, eouts, W):
    from oracle import rnnt as orn
    cache = {}

    def scorer(seq, t):
        if seq not in cache:
            douts, _ = orn.recurrency(sd, cfg, torch.tensor([list(seq)]), None)
            cache[seq] = douts[:, -1:]
        lp = torch.log_softmax(orn.joint(sd, eouts[:, t:t + 1], cache[seq])[0, 0, 0], -1)
        top, idx = torch.topk(lp[1:], W)
        return np.float32(lp[cfg.blank_id].item()), top.numpy().astype(np.float32), idx.numpy()
    return scorer


def test_restatement_returns_the_golden_hypotheses():
    from oracle import model as om
    from tests.util import RNNT_BEAM_WIDTHS, load_golden, load_rnnt_beam_golden
    cfg, sd, g = load_golden("l4_tiny")
    assert (cfg.blank_id, cfg.eos_id) == (R.BLANK, R.EOS)
    want = load_rnnt_beam_golden()
    with torch.no_grad():
        for b in range(g["xs"].shape[0]):
            n = int(g["xlens"][b])
            eouts, _ = om.encoder_forward(sd, cfg, g["xs"][b:b + 1, :n], g["xlens"][b:b + 1])
            for bw in RNNT_BEAM_WIDTHS:
                hyps, scores, _ = R.search(_oracle_scorer(sd, cfg, eouts, bw), eouts.shape[1], bw)
                assert hyps == want[bw][b], (b, bw)
                assert len(scores) == len(hyps)


_RESULTS = {}


def _both(case):
    if case not in _RESULTS:
        seed, V, W, T, E, tie = case
        _RESULTS[case] = (R.search(R.scorer_of(case), T, W, E), R.search_by_ids(R.scorer_of(case), T, W, E))
    return _RESULTS[case]


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_node_id_organisation_equals_the_label_tuples(case):
    (hyps, scores, ev), (got_h, got_s, rounds) = _both(case)
    seed, V, W, T, E, tie = case
    assert got_h == hyps and got_s == scores          # identical doubles: both are Python
    assert len(rounds) == T * E and all(h[0] == R.EOS for h in hyps)
    if T == 0:
        assert hyps == [[R.EOS]] and scores == [0.0]
    print(f"merges {ev.merges} re-formed {ev.reformed} ties {ev.ties} min gap {ev.min_gap:.3g}")
    if not tie:
        assert ev.min_gap > 1e-7


def test_cases_hold_their_events():
    merges = reformed = 0
    for case in R.ALL_CASES:
        ev = _both(case)[0][2]
        merges += ev.merges
        reformed += ev.reformed
    assert merges >= 50 and reformed >= 5, (merges, reformed)
    ties = sum(_both(case)[0][2].ties for case in R.TIE_CASES)
    assert ties >= 20, ties


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_slot_safety(case):
    seed, V, W, T, E, tie = case
    rounds = _both(case)[1][2]
    for r in rounds:
        rows = [c for c in r["ctl"] if c[3]]
        dsts = [c[2] for c in rows]
        assert len(set(dsts)) == len(dsts)
        assert not set(dsts) & r["refs"], r                  # no destination is a slot that live, frame list or beams reference
        assert {c[1] for c in rows} <= r["refs"]             # (the sources are among them)
        assert all(0 <= c[1] < (E + 1) * W and 0 <= c[2] < (E + 1) * W for c in rows)


def test_entry_points_are_declared_and_sized():
    from emoasr_amd import lib
    h = lib.load()
    names = ("emoasr_rnnt_beam_lstm_rows", "emoasr_rnnt_beam_joint_rows", "emoasr_rnnt_beam_start", "emoasr_rnnt_beam_book",
             "emoasr_rnnt_beam_finish")
    for name in names + ("emoasr_rnnt_beam_ws_bytes",):
        assert hasattr(h, name), name
    for name in names:
        assert name in lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "emoasr_hip.h")).read()
    for name in names + ("emoasr_rnnt_beam_ws_bytes",):
        assert name + "(" in header, name
    q = lambda *a: lib.size_query("emoasr_rnnt_beam_ws_bytes", *a)
    STATE = 8736          # EMOASR_RNNT_BEAM_STATE_BYTES: 32 + (16 + 16 + 15 * 16) hypotheses of 32 bytes
    assert "#define EMOASR_RNNT_BEAM_STATE_BYTES %d" % STATE in header
    assert q(3, 100, 10, 3) == 3 * STATE + 32 * (10 * 100 * 2 + 3)
    assert q(1, 0, 1, 3) == STATE + 32 and q(2, 50, 16, 1) == 2 * STATE + 64 and q(0, 0, 4, 3) == 0
    assert q(1, 10, 17, 3) == -1 and q(1, 10, 0, 3) == -1 and q(-1, 10, 4, 3) == -1 and q(1, -1, 4, 3) == -1
    assert q(1, 10, 4, 0) == -1 and q(1, 10, 4, 16) == -1


def test_decoder_routing_without_a_gpu():
    from types import SimpleNamespace

    from emoasr_amd.modeling.decoders.rnn_transducer import RNNTDecoder
    dec = RNNTDecoder(SimpleNamespace(blank_id=0, eos_id=2, vocab_size=8, enc_hidden_size=4, kd_weight=0, dec_num_layers=1,
                                      dec_hidden_size=8, embedding_size=8, joint_hidden_size=8, mtl_ctc_weight=0))
    assert dec.rnnt_beam_impl == "host"
    dec.rnnt_beam_impl = "gpu"
    with pytest.raises(ValueError, match="rnnt_beam_impl"):
        dec.decode(torch.zeros(2, 3, 4), [3, 3], beam_width=4)
    with pytest.raises(ValueError, match="rnnt_beam_impl"):
        dec.decode(torch.zeros(1, 3, 4), [3], beam_width=4)
    assert "rnnt_beam_impl" not in dec.state_dict()
