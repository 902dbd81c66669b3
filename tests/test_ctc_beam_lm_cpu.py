"""CPU checks of the fused (LM) batched CTC prefix beam search's reference and interface (no GPU): the kernel's organisation of the
search in Python (tests/ctc_beam_lm_ref.py: node ids, LM rows in slots with a free list and a one-frame delay, records, the LM term
as a running sum) equals the oracle with a table LM on every case the GPU tests use, the cases really contain what they are for,
the slot bound 2 W holds, and the routing decisions that need no device.

Counts on these cases with the table LM (scale 2.0), lm_weight 0.3 / 1.0, measured here:
  FOLD_CASES  (6 searches at V=5 W=3, 6 at V=6 W=8): folds with the stay first 3-64, with the extension first 8-79 per search (365 /
              445 in all), the two sides carrying different LM terms in 8-119 of them (651 in all), a prefix formed again while its
              old slot waited in 9 of the 12 searches (38 in all)
  LEN_CASES   every search has folds of both kinds; high-water mark 2 W = 8 at lm_weight 0.3
  SIZE_CASES  V=1000 W=10: no folds, 446 / 232 records, high-water 20 = 2 W / 18; V=40 W=32: high-water 64 = 2 W / 59; V=5 W=8 T=1: 5
              records, 5 hypotheses
  TIE_CASES   with the LM the ties are gone (prefixes that tied carry different LM rows): 0 ties, smallest gap 6.8e-4; at
              lm_weight = 0 the same rows hold dozens of exact ties, and the search is that of tests/ctc_beam_ref.py bit for bit
  smallest non-zero gap between adjacent totals over all cases: 1.3e-4 (V=6 W=8 seed 8, lm_weight 0.3)
"""
import numpy as np
import pytest

from oracle import ctc_beam as ob
from tests import ctc_beam_lm_ref as M
from tests import ctc_beam_ref as R

LM_WEIGHTS = (0.3, 1.0)
_ID = lambda c: "V%d-W%d-T%d-s%d" % (c[0], c[1], c[2], c[5])
_RUNS = {}


def _run(case, lmw):
    """one search by slots, computed once and shared"""
    if (case, lmw) not in _RUNS:
        V, W, T, scale, lw, seed, tie = case
        lp, top = R.make_rows(seed, T, V, scale, W, tie)
        _RUNS[(case, lmw)] = (lp, top) + M.search_by_slots(lp, top, W, lw, lmw, M.table_lm(V))
    return _RUNS[(case, lmw)]


@pytest.mark.parametrize("lmw", LM_WEIGHTS)
@pytest.mark.parametrize("case", R.expand(R.ALL_CASES), ids=_ID)
def test_search_by_slots_equals_the_oracle(case, lmw):
    V, W, T, scale, lw, seed, tie = case
    lp, top, hyps, scores, ev = _run(case, lmw)
    want_h, want_s = ob.ctc_prefix_beam_search(lp, R.BLANK, R.EOS, W, lw, lm_predict=M.table_lm(V).batch, lm_weight=lmw)
    print(f"stay first {ev.folds_stay_first} extension first {ev.folds_ext_first} LM terms differ {ev.folds_lm_differ} formed again "
          f"{ev.reformed_waiting} high water {ev.slot_high} records {ev.records} ties {ev.ties} min gap {ev.min_gap:.3g}")
    assert hyps == want_h
    np.testing.assert_allclose(scores, want_s, rtol=0, atol=1e-12)
    assert all(h[0] == R.EOS for h in hyps)
    assert ev.slot_high <= 2 * W                    # the slot bound: <= W live after the previous frame + <= W taken now
    assert ev.min_gap > 1e-7                        # exact order may be demanded (with the LM the tie cases hold no ties either)


def test_table_lm_is_a_function_of_the_prefix():
    row = M.table_lm(40)
    a, b = row((2, 5, 7)), row((2, 5, 7))
    assert a.dtype == np.float32 and a.shape == (40,) and np.array_equal(a, b) and not np.array_equal(a, row((2, 5, 8)))
    assert abs(float(np.sum(np.exp(a.astype(np.float64)))) - 1.0) < 1e-5
    batch = np.array([[2, 5, 7, 0], [2, 9, 0, 0], [2, 5, 7, 3]])
    got = row.batch(batch, [3, 2, 4])
    assert np.array_equal(got[0], a) and np.array_equal(got[1], row((2, 9))) and np.array_equal(got[2], row((2, 5, 7, 3)))


def test_fold_cases_hold_their_events():
    stay = ext = differ = again = searches_again = 0
    for case in R.expand(R.FOLD_CASES):
        for lmw in LM_WEIGHTS:
            ev = _run(case, lmw)[4]
            assert ev.folds_stay_first >= 3 and ev.folds_ext_first >= 8 and ev.folds_lm_differ >= 8, (case, lmw)
            stay, ext, differ = stay + ev.folds_stay_first, ext + ev.folds_ext_first, differ + ev.folds_lm_differ
            again += ev.reformed_waiting
            searches_again += ev.reformed_waiting > 0
    assert (stay, ext, differ, again, searches_again) == (365, 445, 651, 38, 9)


def test_len_and_size_cases_hold_their_events():
    for case in R.expand(R.LEN_CASES):
        for lmw in LM_WEIGHTS:
            ev = _run(case, lmw)[4]
            assert ev.folds_stay_first >= 9 and ev.folds_ext_first >= 5, (case, lmw)
        assert _run(case, 0.3)[4].slot_high == 2 * case[1]
    big, wide, one = R.expand(R.SIZE_CASES)
    assert [_run(big, w)[4].slot_high for w in LM_WEIGHTS] == [20, 18] and [_run(big, w)[4].records for w in LM_WEIGHTS] == [446, 232]
    assert [_run(wide, w)[4].slot_high for w in LM_WEIGHTS] == [64, 59]
    for lmw in LM_WEIGHTS:
        _, _, hyps, _, ev = _run(one, lmw)
        assert len(hyps) == 5 < 8 and ev.records == 5


def test_tie_cases():
    """the LM separates the prefixes that tie without it; without it (lm_weight = 0, the cell that must equal the search of
    csrc/ctc_beam.hip) the ties are there and the slot organisation is the node-id search bit for bit"""
    for case in R.expand(R.TIE_CASES):
        V, W, T, scale, lw, seed, tie = case
        for lmw in LM_WEIGHTS:
            ev = _run(case, lmw)[4]
            assert ev.ties == 0 and ev.min_gap > 1e-7
        lp, top, hyps, scores, ev = _run(case, 0.0)
        assert ev.ties >= 24 and ev.min_gap > 1e-7
        assert (hyps, scores) == R.search_by_ids(lp, top, W, lw)


def test_an_exhausted_free_list_is_reported():
    V, W, T, scale, lw, seed, tie = R.expand(R.FOLD_CASES)[3]
    lp, top = R.make_rows(seed, T, V, scale, W, tie)
    with pytest.raises(M.SlotsExhausted):
        M.search_by_slots(lp, top, W, lw, 0.3, M.table_lm(V), nslot=2)
    assert M.search_by_slots(lp, top, W, lw, 0.3, M.table_lm(V), nslot=2 * W)[0] == _run((V, W, T, scale, lw, seed, tie), 0.3)[2]


def test_entry_points_are_declared_and_sized():
    from emoasr_amd import lib, ops
    h = lib.load()
    for name in ("emoasr_ctc_beam_lm_init", "emoasr_ctc_beam_lm_frame", "emoasr_ctc_beam_lm_finish", "emoasr_ctc_beam_lm_ws_bytes",
                 "emoasr_ctc_beam_lm_slots"):
        assert hasattr(h, name)
    assert len(lib.SIGNATURES["emoasr_ctc_beam_lm_frame"]) == 25
    assert [ops.ctc_beam_lm_slots(W) for W in (1, 10, 32, 33, 0)] == [4, 22, 66, -1, -1]
    q = lambda *a: lib.size_query("emoasr_ctc_beam_lm_ws_bytes", *a)
    state = q(1, 0, 1) - 32                          # one search, no frames: its state block and a one-node trie share
    assert state > 0 and state % 8 == 0
    assert q(6, 48, 10) == 6 * (state + 32 * (10 * 48 + 1)) and q(0, 48, 10) == 0
    assert q(1, 10, 33) == -1 and q(1, 10, 0) == -1 and q(1, -1, 4) == -1
    assert ops.CTC_BEAM_STATUS[16] and ops.CTC_BEAM_STATUS[32] and "pool" in ops.ctc_beam_status_text(32)


def test_routing_without_a_gpu():
    """with ctc_beam_impl = "host" (the default) an LM with several utterances is still refused; "device" sends it to the fused
    search, which refuses a beam over the limit and a masked LM before touching the device"""
    from types import SimpleNamespace

    import torch

    from emoasr_amd.modeling.decoders.ctc import CTCDecoder
    dec = CTCDecoder(SimpleNamespace(blank_id=0, eos_id=2, vocab_size=8, enc_hidden_size=4, kd_weight=0))
    eouts = torch.zeros(2, 3, 4)
    assert dec.ctc_beam_impl == "host"
    with pytest.raises(NotImplementedError, match="one utterance at a time"):
        dec.decode(eouts, [3, 3], beam_width=4, lm=object(), lm_weight=0.3)
    dec.ctc_beam_impl = "device"
    with pytest.raises(ValueError, match="outside 1..32"):
        dec.decode(eouts, [3, 3], beam_width=33, lm=object(), lm_weight=0.3)
    with pytest.raises(NotImplementedError):
        dec.decode(eouts, [3, 3], beam_width=4, lm=SimpleNamespace(lm_type="bert"), lm_weight=0.3)


def test_fusion_grid_weights_and_refusals():
    from types import SimpleNamespace

    from emoasr_amd import fusion_grid as fg
    args = fg.build_parser().parse_args(["-conf", "a.yaml", "-ep", "3"])
    lm_w, len_w = fg.weight_lists(args.lm_min, args.lm_max, args.lm_step, args.len_min, args.len_max, args.len_step)
    assert np.array_equal(lm_w, np.arange(0, 1 + 1e-5, 0.1)) and np.array_equal(len_w, np.arange(0, 5 + 1e-5, 1))
    assert len(lm_w) == 11 and len(len_w) == 6 and lm_w.dtype == np.float64
    assert lm_w[3] == 0.1 * 3 and lm_w[3] != 0.3                     # unrounded: 0.30000000000000004
    lm_w, len_w = fg.weight_lists(0.2, 0.6, 0.2, 0.0, 1.0, 0.5)
    assert np.array_equal(lm_w, np.arange(0.2, 0.6 + 1e-5, 0.2)) and np.array_equal(len_w, np.arange(0.0, 1.0 + 1e-5, 0.5))
    for kind in ("transformer", "rnn_transducer", "las"):
        with pytest.raises(NotImplementedError, match="CTC models only"):
            fg.ctc_fusion_grid(SimpleNamespace(decoder_type=kind), [], None, 4, object(), [0.1], [0.0], "cpu")
    with pytest.raises(NotImplementedError, match="decode_ctc_weight"):
        fg.ctc_fusion_grid(SimpleNamespace(decoder_type="ctc"), [], None, 4, object(), [0.1], [0.0], "cpu", decode_ctc_weight=0.3)
    for flag in ("--data", "--data_tag", "--beam_width", "--lm_min", "--lm_max", "--lm_step", "--len_min", "--len_max", "--len_step",
                 "--lm_conf", "--lm_ep", "--lm_tag"):
        assert flag in fg.build_parser().format_help()
