"""CPU checks of RNN-LM shallow fusion in the transducer beam search (no GPU): the restatement of
tests/rnnt_fusion_ref.py reduces to tests/rnnt_beam_ref.search at mu = 0, its case set really holds searches that fusion and the
length weight change, the host expansion of the grid equals one search per cell, and the interface is declared and routed."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnnt_beam_ref as R
from tests import rnnt_fusion_ref as F


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_mu_zero_is_the_unfused_search(case):
    """hypotheses, order and doubles of rnnt_beam_ref.search on its 35 cases (the tie cases included: 0 * lq adds nothing)"""
    seed, V, W, T, E, tie = case
    want = R.search(R.scorer_of(case), T, W, E)
    for V_lm in (V, V + 3):
        got = F.search(F.hash_rows(seed, V, tie), F.hash_lm_rows(seed + 5000, V_lm, tie), 0.0, T, W, E)
        assert got[0] == want[0] and got[1] == want[1]


_RESULTS = {}


def _run(case):
    if case not in _RESULTS:
        seed, V, V_lm, W, T, E, mu, lw = case
        sc, lm = F.scorers_of(case)
        fused = F.search(sc, lm, mu, T, W, E)          # (rnnt_beam_ref.search asserts inside that no grown candidates fold)
        plain = F.search(sc, lm, 0.0, T, W, E)
        _RESULTS[case] = (fused, plain, F.finish(fused[0], fused[1], lw))
    return _RESULTS[case]


@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_fused_search_is_well_formed(case):
    seed, V, V_lm, W, T, E, mu, lw = case
    (hyps, scores, ev), _, (fh, fs) = _run(case)
    assert 1 <= len(hyps) <= W and all(h[0] == F.EOS and all(1 <= v < V for v in h[1:]) for h in hyps)
    assert all(a >= b for a, b in zip(fs, fs[1:]))      # (the search's own order can be bent by a merge; the finish sorts)
    assert sorted(map(tuple, fh)) == sorted(map(tuple, hyps))
    if T == 0:
        assert hyps == [[F.EOS]] and scores == [0.0] and fs == [lw * 1.0]
    if E == 1:      # a single round grows nothing: the LM cannot matter
        assert hyps == [[F.EOS]]
    print(f"min gap {ev.min_gap:.3g}")


def test_case_set_covers_the_shapes_and_holds_its_events():
    cs = F.CASES
    assert {c[3] for c in cs} == {1, 2, 4, 16} and {c[4] for c in cs} == {0, 1, 2, 12} and {c[5] for c in cs} == {1, 3}
    assert any(c[1] - 1 == c[3] for c in cs) and any(c[1] - 1 > c[3] for c in cs)
    assert {c[2] - c[1] for c in cs} == {0, 3}
    differs = sum(int(_run(c)[0][0][0] != _run(c)[1][0][0]) for c in cs)
    len_moves = sum(int(_run(c)[2][0][0] != _run(c)[0][0][0]) for c in cs)
    assert differs >= 10 and len_moves >= 5, (differs, len_moves)
    close = [F.case_id(c) for c in cs if _run(c)[0][2].min_gap <= F.GAP_TOL]
    assert len(close) <= len(cs) // 10, close          # at most 10 % of the cases are too close to compare across forms


def test_fuse_is_two_f32_roundings_with_ties_to_the_lowest_index():
    lp = np.float32([-1.5, -2.0, -2.0, -0.5, -3.0])
    lq = np.float32([-0.5, -1.0, -1.0, -2.5, -1.0, -9.0, -9.0])
    blank, vals, ids = F.fuse(lp, lq, 1.0, 3)
    assert blank == np.float32(-1.5) and ids.tolist() == [0, 1, 2] and vals.tolist() == [-3.0, -3.0, -3.0]
    t = torch.from_numpy(lp)[1:] + torch.tensor(0.3, dtype=torch.float32) * torch.from_numpy(lq)[1:5]
    _, vals, ids = F.fuse(lp, lq, 0.3, 4)
    assert vals.tolist() == t[torch.from_numpy(ids)].tolist()          # a torch f32 expression reproduces it bit for bit
    assert F.fuse(lp, lq, 0.0, 4)[1].tolist() == sorted(lp[1:].tolist(), reverse=True)


def test_host_grid_expansion_equals_one_search_per_cell():
    from emoasr_amd.engine.rnnt import RNNTDecoder as Eng
    from emoasr_amd.modeling.beam_search_device import grid_cell_plan
    lm_weights, len_weights = [0.0, 0.3, 1.0, 0.3], [0.0, 0.7, 3.0]
    for case in [c for c in F.CASES if c[4] == 12 and c[5] == 3][:6]:
        seed, V, V_lm, W, T, E, _, _ = case
        sc, lm = F.scorers_of(case)
        weights, cells = grid_cell_plan(lm_weights, len_weights, True)
        assert weights == [0.0, 0.3, 1.0] and len(cells) == 12
        found = [F.search(sc, lm, a, T, W, E)[:2] for a in weights]
        for (k, j), (a, b) in zip(cells, [(a, b) for a in lm_weights for b in len_weights]):
            got = Eng.rnnt_len_expand(*found[k], len_weights[j]) if weights[k] > 0 else found[k]
            h, s, _ = F.search(sc, lm, a, T, W, E)
            want = F.finish(h, s, b) if a > 0 else (h, s)          # without fusion the length weight is not read
            assert (list(got[0]), list(got[1])) == (list(want[0]), list(want[1])), (case, a, b)


def test_chunk_capacity_counts_the_lm_pools():
    from emoasr_amd.engine.rnnt import RNNTDecoder as Eng
    eng = SimpleNamespace(dtype=torch.bfloat16, r_nl=2, r_H=512, _BEAM_BATCH_CAP=64, _BEAM_POOL_BUDGET=256 << 20)
    lm = SimpleNamespace(L=2, H=512)
    assert Eng.rnnt_beam_chunk_capacity(eng, 16, 3, None) == 64
    assert Eng.rnnt_beam_chunk_capacity(eng, 16, 3, lm) == 64          # 64 slots x 6 bytes x 2048 values = 768 KiB per search
    eng._BEAM_POOL_BUDGET = 5 * 64 * 6 * 2048 + 1
    assert Eng.rnnt_beam_chunk_capacity(eng, 16, 3, lm) == 5
    eng._BEAM_POOL_BUDGET = 1
    assert Eng.rnnt_beam_chunk_capacity(eng, 16, 3, lm) == 1 and Eng.rnnt_beam_chunk_capacity(eng, 16, 3, None) == 64


def test_entry_points_are_declared():
    from emoasr_amd import lib, ops
    h = lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "emoasr_hip.h")).read()
    for name in ("emoasr_rnnt_beam_pick_lm", "emoasr_rnnt_beam_gather_rows"):
        assert hasattr(h, name) and name in lib.SIGNATURES and name + "(" in header, name
    assert len(lib.SIGNATURES["emoasr_rnnt_beam_pick_lm"]) == 16 and len(lib.SIGNATURES["emoasr_rnnt_beam_gather_rows"]) == 9
    assert callable(ops.rnnt_beam_pick_lm) and callable(ops.rnnt_beam_gather_rows)


def _decoder():
    from emoasr_amd.modeling.decoders.rnn_transducer import RNNTDecoder
    return RNNTDecoder(SimpleNamespace(blank_id=0, eos_id=2, vocab_size=8, enc_hidden_size=4, kd_weight=0, dec_num_layers=1,
                                       dec_hidden_size=8, embedding_size=8, joint_hidden_size=8, mtl_ctc_weight=0))


def test_decoder_routing(monkeypatch):
    from emoasr_amd.modeling.decoders import rnn_transducer as mod
    from emoasr_amd.modeling.lm import _NO_PREDICT
    calls = []
    monkeypatch.setattr(mod, "rnnt_beam_apply", lambda dec, eouts, bw, *a: calls.append(("host", bw) + a) or [[2, 3]])

    def batch(dec, eouts, elens, bw, lm=None, lm_weights=None, len_weights=None, require_device=False):
        calls.append(("batch", bw, lm, lm_weights, len_weights, require_device))
        B = eouts.shape[0]
        if lm_weights is None:
            return [[[2, 3]]] * B, [[-1.0]] * B
        return [[[[2, 4]]]] * B, [[[-2.0]]] * B
    monkeypatch.setattr(mod, "rnnt_beam_batch_apply", batch)
    dec = _decoder()
    rnn, trf = SimpleNamespace(lm_type="rnn"), SimpleNamespace(lm_type="transformer")
    one, two = torch.zeros(1, 3, 4), torch.zeros(2, 3, 4)
    # without fusion: today's calls, whatever the weights say
    assert dec.decode(one, [3], beam_width=4, len_weight=2.0) == ([[2, 3]], None, None, None)
    assert dec.decode(one, [3], beam_width=4, lm=rnn, lm_weight=0, len_weight=2.0) == ([[2, 3]], None, None, None)
    assert dec.decode(two, [3, 3], beam_width=4, lm=rnn, lm_weight=0.0)[:2] == ([[[2, 3]]] * 2, [[-1.0]] * 2)
    assert calls == [("host", 4, None, 0, 2.0), ("host", 4, rnn, 0, 2.0), ("batch", 4, None, None, None, False)]
    del calls[:]
    # with fusion: one utterance on the host form, several (or "device") on the device form, in today's shapes
    assert dec.decode(one, [3], beam_width=4, lm=trf, lm_weight=0.3, len_weight=1.0) == ([[2, 3]], None, None, None)
    assert dec.decode(two, [3, 3], beam_width=4, lm=rnn, lm_weight=0.3, len_weight=1.0) == ([[[2, 4]]] * 2, [[-2.0]] * 2, None, None)
    dec.rnnt_beam_impl = "device"
    assert dec.decode(one, [3], beam_width=4, lm=rnn, lm_weight=0.3) == ([[2, 4]], [-2.0], None, None)
    assert calls == [("host", 4, trf, 0.3, 1.0), ("batch", 4, rnn, [0.3], [1.0], False), ("batch", 4, rnn, [0.3], [0.0], True)]
    del calls[:]
    # "device" with an LM the device form cannot take: by name, before any work
    for eouts, elens in ((one, [3]), (two, [3, 3])):
        with pytest.raises(ValueError, match="lm_type 'transformer'"):
            dec.decode(eouts, elens, beam_width=4, lm=trf, lm_weight=0.3)
    dec.decode(one, [3], beam_width=4, lm=trf, lm_weight=0.0)          # (not fused: nothing to refuse)
    assert calls == [("batch", 4, None, None, None, False)]
    # a masked LM has no next-token distribution
    with pytest.raises(NotImplementedError) as info:
        dec.decode(one, [3], beam_width=4, lm=SimpleNamespace(lm_type="bert"), lm_weight=0.3)
    assert str(info.value) == _NO_PREDICT


def test_grid_dispatch_and_pinned_refusals():
    from emoasr_amd import fusion_grid as fg
    assert fg.grid_of("rnn_transducer") is fg.rnnt_fusion_grid
    assert fg.grid_of("ctc") is fg.ctc_fusion_grid and fg.grid_of("transformer") is fg.joint_fusion_grid
    for kind in ("rnnt", "las", None):
        with pytest.raises(NotImplementedError, match="'ctc' and 'transformer'"):
            fg.grid_of(kind)
    for kind in ("ctc", "transformer", "las"):
        with pytest.raises(NotImplementedError, match="decoder_type == 'rnn_transducer'"):
            fg.rnnt_fusion_grid(SimpleNamespace(decoder_type=kind), [], None, 4, object(), [0.1], [0.0], "cpu")
    with pytest.raises(NotImplementedError, match="decoder_type == 'transformer'"):
        fg.joint_fusion_grid(SimpleNamespace(decoder_type="rnn_transducer"), [], None, 4, object(), [0.1], [0.0], "cpu")
    assert "rnnt_fusion_grid" in fg.__doc__
