"""CPU checks of the transducer's search module (emoasr_amd/engine/rnnt_search.py; no GPU): the one host loop of
the two host-bookkeeping beam searches against tests/rnnt_beam_ref.search, the admission predicates over a table of sizes against the
answers recorded before the limits were gathered into one table, and rnnt_len_expand against its earlier three lines."""
import itertools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnnt_beam_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the host loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_host_loop_is_the_reference_search(case):
    """hypotheses, order and doubles of rnnt_beam_ref.search, the tie cases included (they pin the stable sort and the merge order).
    The synthetic round forms the record [blank | vals | ids] in f32 and widens it to float64, as the real rounds do."""
    from emoasr_amd.engine.rnnt_search import beam_host_loop
    seed, V, W, T, E, tie = case
    scorer = R.scorer_of(case)
    rounds = []

    def round_(live, t, v, last):
        rec = np.zeros((len(live), 1 + 2 * W), dtype=np.float32)
        for i, (hyp, _, state) in enumerate(live):
            assert state == ("state", tuple(hyp[:-1]))          # the state from BEFORE the hypothesis' last label
            blank, vals, ids = scorer(tuple(hyp), t)
            rec[i, 0], rec[i, 1:1 + W], rec[i, 1 + W:] = blank, vals, ids
        rounds.append((t, v, last))
        if last:          # only column 0 is read on a frame's last round
            rec[:, 1:] = np.nan
        return rec.astype(np.float64), lambda i: ("state", tuple(live[i][0]))

    want_h, want_s, _ = R.search(scorer, T, W, E)
    got_h, got_s = beam_host_loop(round_, T, W, E, R.EOS, ("state", ()), True)
    assert got_h == want_h and got_s == want_s          # doubles, no tolerance
    assert beam_host_loop(round_, T, W, E, R.EOS, ("state", ()), False) == want_h
    assert all(last == (v == E - 1) for _, v, last in rounds)
    # the fused tail: score + len_weight * len(hyp), stably re-sorted
    from emoasr_amd.engine.rnnt import RNNTDecoder
    assert beam_host_loop(round_, T, W, E, R.EOS, ("state", ()), True, 0.7) == RNNTDecoder.rnnt_len_expand(want_h, want_s, 0.7)


# ---- the limits table -----------------------------------------------------------------------------------------------------------------
AXES = dict(dtype=["f32", "bf16"], embedding=[8, 12, 512], H=[8, 12, 64, 952, 1032, 1184], layers=[0, 1, 2],
            V=[1, 2, 3, 15360, 15361], W=[1, 3, 16, 17], E=[1, 3, 15, 16])
_DTYPES = dict(f32=torch.float32, bf16=torch.bfloat16)


def _engine(dtype, emb, H, nl, V):
    """what the admission predicates read of an engine: sizes, dtype and the shapes of the arena's weights"""
    def w(name):
        if name == "decoder.output.weight":
            return SimpleNamespace(shape=(V, 8))
        l = int(name.split(".")[2])
        assert name == f"decoder.rnns.{l}.weight_ih_l0" and l < nl, name
        return SimpleNamespace(shape=(4 * H, emb if l == 0 else H))
    return SimpleNamespace(dtype=_DTYPES[dtype], split=False, r_emb=emb, r_H=H, r_nl=nl, arena=SimpleNamespace(w=w))


def _answers(Eng):
    """the three predicates over every combination of AXES, as strings of 0 / 1 in itertools.product order: greedy and lm over
    (dtype, embedding, H, layers, V), device_ok over all seven axes.  Eng: the class whose unbound methods answer."""
    out = dict(greedy=[], lm=[], device_ok=[])
    for dtype, emb, H, nl, V in itertools.product(*(AXES[k] for k in ("dtype", "embedding", "H", "layers", "V"))):
        eng = _engine(dtype, emb, H, nl, V)
        eng.rnnt_beam_lm_why_not = lambda lm, eng=eng: Eng.rnnt_beam_lm_why_not(eng, lm)
        lm = SimpleNamespace(lm_type="rnn", compute_dtype=_DTYPES[dtype], f32_split=False, E=emb, H=H, L=nl, V=V)
        out["greedy"].append(Eng.rnnt_greedy_batch_why_not(eng) is None)
        out["lm"].append(Eng.rnnt_beam_lm_why_not(eng, lm) is None)
        out["device_ok"] += [bool(Eng.rnnt_beam_device_ok(eng, W, E)) for W in AXES["W"] for E in AXES["E"]]
    return {k: "".join("01"[v] for v in vals) for k, vals in out.items()}


def test_admission_predicates_answer_as_recorded():
    """tests/golden/rnnt_limits.json: the answers of the predicates as they stood in engine/rnnt.py before the limits table (recorded
    by _answers over that class), including where they disagree with each other about the same kernel"""
    from emoasr_amd.engine.rnnt import RNNTDecoder
    with open(os.path.join(HERE, "golden", "rnnt_limits.json")) as f:
        golden = json.load(f)
    assert golden["axes"] == AXES
    got = _answers(RNNTDecoder)
    for name in ("greedy", "lm", "device_ok"):
        want = golden[name]
        assert "0" in want and "1" in want, name          # every predicate both admits and refuses on this table
        assert len(got[name]) == len(want) and got[name] == want, (name, [i for i, (a, b) in enumerate(zip(got[name], want)) if a != b][:8])
    assert len(golden["greedy"]) == len(golden["lm"]) == 2 * 3 * 6 * 3 * 5 and len(golden["device_ok"]) == 540 * 16


def test_limit_terms():
    """the table's own terms at their edges: 1904 / 2368 columns, H = 1024 (64 KiB of joint rows), V = 15360 (60 KiB row)"""
    from emoasr_amd.engine import rnnt_search as S
    f32, bf16 = torch.float32, torch.bfloat16
    assert S.lstm_rows_fits(bf16, [952], 952) and not S.lstm_rows_fits(bf16, [960], 952) and not S.lstm_rows_fits(bf16, [12], 8)
    assert S.lstm_rows_fits(f32, [1184], 1184) and not S.lstm_rows_fits(f32, [1188], 1184) and S.lstm_rows_fits(f32, [12], 8)
    assert not S.lstm_rows_fits(f32, [8], 12)          # H % 8 in either dtype
    assert S.joint_rows_fits(1024) and not S.joint_rows_fits(1025)
    assert S.pick_row_fits(15360) and not S.pick_row_fits(15361)
    assert S.round_fits(f32, 40, 1344, 1024) and not S.round_fits(f32, 40, 1345, 1024) and S.round_fits(bf16, 40, 4000, 1024)
    assert not S.round_fits(bf16, 15361, 8, 8) and not S.round_fits(bf16, 40, 8, 1025)


# ---- rnnt_len_expand ------------------------------------------------------------------------------------------------------------------
def _len_expand_before(hyps, scores, len_weight):
    sc = [float(s) + float(len_weight) * float(len(h)) for h, s in zip(hyps, scores)]
    order = sorted(range(len(sc)), key=lambda i: -sc[i])
    return [hyps[i] for i in order], [sc[i] for i in order]


def test_len_expand_keeps_its_values_and_the_order_of_ties():
    from emoasr_amd import lockstep
    from emoasr_amd.engine.rnnt import RNNTDecoder
    hyps = [[2, 5], [2], [2, 7, 7], [2, 3], [2, 9, 9, 9], [2, 4]]
    for scores in ([-1.0] * 6, [-1.0, -0.5, -1.5, -1.0, -2.0, -1.0], [-3.0, -2.5, -3.5, -3.0, -4.0, -3.0], [0.1 * i for i in range(6)]):
        for w in (0.0, 0.5, 0.25, -0.5, 1e-17):          # 0.5: the length term cancels the score steps, every hypothesis ties
            got = RNNTDecoder.rnnt_len_expand(hyps, scores, w)
            assert got == _len_expand_before(hyps, scores, w), (scores, w)
    assert RNNTDecoder.rnnt_len_expand([], [], 0.3) == ([], [])
    # the default offset of the lockstep searches stays 2
    assert lockstep.expand_len_weights([[5]], [-1.0], [0.5]) == [([[5]], [-1.0 + 0.5 * 3.0])]
    assert lockstep.expand_len_weights([[5]], [-1.0], [0.5], 0) == [([[5]], [-1.0 + 0.5 * 1.0])]
