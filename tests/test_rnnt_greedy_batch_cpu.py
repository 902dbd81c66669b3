"""The lockstep greedy search's reference bookkeeping (tests/rnnt_greedy_ref.py) before any kernel is involved: driven by the oracle's
prediction and joint networks on the l4_tiny golden model it reproduces the reference's hypotheses and alignments for every window
size, and the edge cases of the rule (no frames, one frame, all blank, the max_seq_len cut) come out as the reference's loop gives
them."""
import numpy as np
import pytest
import torch

from oracle import model as om
from oracle import rnnt as orn
from tests import rnnt_greedy_ref as G
from tests.util import load_golden, split_ragged


@pytest.fixture(scope="module")
def l4():
    """the golden model, its encoder outputs, and ONE memo of the oracle scorer shared by every window size"""
    cfg, sd, g = load_golden("l4_tiny")
    with torch.no_grad():
        eouts, elens = om.encoder_forward(sd, cfg, g["xs"], g["xlens"])
    douts, picks = {}, {}

    def dout_of(seq):
        """(output, state) of the prediction network after the label sequence, stepped label by label as the reference does"""
        if seq not in douts:
            prev = dout_of(seq[:-1])[1] if len(seq) > 1 else None
            douts[seq] = orn.recurrency(sd, cfg, torch.tensor([[seq[-1]]]), prev)
        return douts[seq]

    def scorer(s, seq, t):
        if (s, seq, t) not in picks:
            with torch.no_grad():
                picks[(s, seq, t)] = int(orn.joint(sd, eouts[s:s + 1, t:t + 1], dout_of(seq)[0]).squeeze(2).argmax(-1)[0])
        return picks[(s, seq, t)]

    return cfg, g, [int(n) for n in elens], scorer


@pytest.mark.parametrize("K", [1, 3, 4, 16])
def test_lockstep_reproduces_the_golden_search(l4, K):
    cfg, g, elens, scorer = l4
    hyps, aligns, steps = G.search(scorer, elens, K, cfg.blank_id, cfg.eos_id)
    assert hyps == split_ragged(g["eval/hyps"], g["eval/hyp_lens"])
    assert aligns == split_ragged(g["eval/aligns"], g["eval/align_lens"])
    assert any(len(h) for h in hyps) and len(steps) - 1 <= max(elens) + 256 + 1
    # the words: step 0 consumes <eos> from slot 0 into slot 1 and reads slot 1; every later LSTM row goes to the slot its search's
    # joint rows of the step before did NOT read; the last entry is all inactive
    assert all(w == (cfg.eos_id, 0, 1, 1) for w in steps[0]["lstm"]) and steps[0]["live"] == len(elens)
    for a, b in zip(steps, steps[1:]):
        for s, (lab, src, dst, on) in enumerate(b["lstm"]):
            if on:
                read = {slot for slot, act, _ in a["joint"][s] if act}
                assert read == {src} and dst == 1 - src and lab != cfg.blank_id
                assert {slot for slot, act, _ in b["joint"][s] if act} == {dst}
    assert steps[-1]["live"] == 0 and not steps[-1]["ctl"].any()


def test_window_one_is_the_reference_loop(l4):
    """K = 1: one joint evaluation per step, so a search takes len(align) steps"""
    cfg, g, elens, scorer = l4
    _, aligns, steps = G.search(scorer, elens, 1, cfg.blank_id, cfg.eos_id)
    assert len(steps) - 1 == max(len(a) for a in aligns)


@pytest.mark.parametrize("K", [1, 3, 4, 16])
def test_edges_of_the_rule(K):
    blank = G.BLANK

    def scorer(s, seq, t):     # no frames, one frame (blank / a label then blank), all blank
        if s == 2:
            return 5 if len(seq) == 1 else blank       # one label at its only frame, then blank
        return blank
    hyps, aligns, steps = G.search(scorer, [0, 1, 1, 7], K)
    assert hyps == [[], [], [5], []] and aligns == [[], [blank], [5, blank], [blank] * 7]
    assert steps[0]["lstm"][0] == (0, 0, 0, 0) and steps[0]["joint"][0] == [(0, 0, 0)] * K and steps[0]["live"] == 3
    assert len(steps) - 1 == max(2, -(-7 // K))
    assert steps[0]["joint"][3] == [(1, 1, i) if i < 7 else (0, 0, 0) for i in range(K)]
    # a scorer that never emits blank, max_seq_len = 2: three labels, then the search stops -- on frame 0
    hyps, aligns, steps = G.search(lambda s, seq, t: 3 + len(seq), [4, 0], K, max_seq_len=2)
    assert hyps == [[4, 5, 6], []] and aligns == [[4, 5, 6], []] and len(steps) - 1 == 3
    assert [st["lstm"][0] for st in steps] == [(G.EOS, 0, 1, 1), (4, 1, 0, 1), (5, 0, 1, 1), (0, 0, 0, 0)]
    assert steps[-1]["live"] == 0 and not steps[-1]["ctl"].any()


def test_control_word_layout():
    """ctl(): [4][S] then [3][S K], global slots 2 s + slot, rows offs[s] + t"""
    L = G.Lockstep([3, 0, 2], 2)
    w = L.ctl([0, 3, 3])
    assert w[:12].reshape(4, 3).tolist() == [[G.EOS, 0, G.EOS], [0, 0, 4], [1, 0, 5], [1, 0, 1]]
    assert w[12:].reshape(3, 6).tolist() == [[1, 1, 0, 0, 5, 5], [1, 1, 0, 0, 1, 1], [0, 1, 0, 0, 3, 4]]
    L.advance(lambda s, i: 7 if (s, i) == (0, 1) else G.BLANK)    # search 0: blank, then 7 at frame 1; search 2: two blanks, done
    assert L.hyps == [[7], [], []] and L.aligns == [[G.BLANK, 7], [], [G.BLANK] * 2] and L.done == [False, True, True]
    w = L.ctl([0, 3, 3])
    assert w[:12].reshape(4, 3).tolist() == [[7, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0]]
    assert w[12:].reshape(3, 6).tolist() == [[0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0]]
    assert np.array_equal(w, L.ctl(np.array([0, 3, 3])))
