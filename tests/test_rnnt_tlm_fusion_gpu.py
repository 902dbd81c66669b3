"""Transformer-LM shallow fusion in the batched transducer beam search on the device, over a prefix tree (csrc/lm_tree.hip,
engine.rnnt_beam_search_batch under decoder.rnnt_tlm_fusion = "device"), end to end on the l4_tiny golden model
with the Transformer LM of the ctcbeam fixture: against the host form (_rnnt_beam_search_chain with the same LM), mu = 0 against the
unfused search, the grid against single cells, bf16 against f32, the routing of the switch and the grid tool."""
from types import SimpleNamespace

import pytest
import torch

from tests import lm_tree_ref as T
from tests import rnnt_fusion_ref as F
from tests.test_rnnt_fusion_gpu import _models
from tests.util import LM_CFG, load_ctc_beam_golden, load_golden

pytestmark = pytest.mark.gpu

ELENS, MUS, WIDTHS = T.ELENS, T.MUS, T.WIDTHS
LEN_W = 0.7
_REF = {}


def _cases(dev):
    """{(b, W, mu): (min_gap, oracle hyps, oracle plain hyps)} of the oracle restatement (tests/rnnt_fusion_ref.search with
    oracle.decoder.lm_predict as the LM) over the f32 model's encoder outputs"""
    if "cases" not in _REF:
        _, _, _, eouts, (cfg, sd) = _models(torch.float32, dev)
        lm_sd = {k: v.float() for k, v in load_ctc_beam_golden()[2].items()}
        _REF["cases"] = T.gap_cases(sd, cfg, lm_sd, SimpleNamespace(**LM_CFG), eouts.float().cpu())
    return _REF["cases"]


def _gap_checked(dev):
    cases = _cases(dev)
    keep = [k for k, v in cases.items() if v[0] > F.GAP_TOL]
    assert len(keep) >= len(cases) - len(cases) // 10, sorted(cases.items())          # at most 10 % may be left out
    return keep


class _switch:
    """decoder.rnnt_tlm_fusion (and rnnt_beam_impl) set inside the block, back to the defaults after it"""

    def __init__(self, dec, tlm="device", impl="host"):
        self.dec, self.tlm, self.impl = dec, tlm, impl

    def __enter__(self):
        self.dec.rnnt_tlm_fusion, self.dec.rnnt_beam_impl = self.tlm, self.impl

    def __exit__(self, *exc):
        self.dec.rnnt_tlm_fusion, self.dec.rnnt_beam_impl = "host", "host"


def _host(eng, dec, lm, eouts, b, W, mu, lw=0.0):
    return eng._rnnt_beam_search_chain(eouts[b:b + 1, :ELENS[b]], W, dec.blank_id, dec.eos_id, 3, True, lm, mu, lw)


def _close(a, b, tol=F.GAP_TOL):
    return len(a) == len(b) and all(abs(p - q) < tol for p, q in zip(a, b))


def test_device_form_equals_the_host_form_f32(dev):
    """hypotheses and order equal, scores within GAP_TOL on the gap-checked cases (len_weight 0.7); an utterance in the batch returns
    what it returns alone; fusion moves at least two results; the empty utterance returns [[eos]] with score len_weight"""
    model, _, tlm, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    checked = _gap_checked(dev)
    moved, compared, bit_equal, alone = 0, 0, 0, 0
    with torch.no_grad():
        for W in WIDTHS:
            plain, _, _, _ = dec.decode(eouts, list(ELENS), beam_width=W)
            for mu in MUS:
                with _switch(dec):
                    hyps, scores, logits, aligns = dec.decode(eouts, list(ELENS), beam_width=W, lm=tlm, lm_weight=mu, len_weight=LEN_W)
                assert logits is None and aligns is None and hyps[2] == [[dec.eos_id]] and scores[2] == [LEN_W]
                for b in (0, 1):
                    moved += int(hyps[b] != plain[b])
                    if (b, W, mu) in checked:
                        h, s = _host(eng, dec, tlm, eouts, b, W, mu, LEN_W)
                        assert hyps[b] == h and _close(scores[b], s), (b, W, mu, hyps[b], h, scores[b], s)
                        compared += 1
                    with _switch(dec, impl="device"):
                        h1, s1, _, _ = dec.decode(eouts[b:b + 1, :ELENS[b]], [ELENS[b]], beam_width=W, lm=tlm, lm_weight=mu,
                                                  len_weight=LEN_W)
                    assert h1 == hyps[b] and _close(s1, scores[b]), (b, W, mu, h1, hyps[b], s1, scores[b])
                    alone += 1
                    bit_equal += int(s1 == scores[b])
    print(f"[measured] {compared} of 8 cases compared with the host form; alone == in the batch bit for bit in {bit_equal} of {alone}; "
          f"fusion moved {moved} of 8 results; nodes used {eng.rnnt_tlm_stats}")
    assert moved >= 2 and compared >= 7


def test_mu_zero_through_the_fused_chain_is_the_unfused_search(dev):
    """the tree's launches run, weighted 0: hypotheses and doubles of the search without the LM, bit for bit; weights <= 0 in a grid
    call are that search too and do not read the length weight"""
    model, _, tlm, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    with torch.no_grad():
        for W in WIDTHS:
            want = eng.rnnt_beam_search_batch(eouts, list(ELENS), W, dec.blank_id, dec.eos_id)
            got = eng._rnnt_beam_search_device(eouts, list(ELENS), W, dec.blank_id, dec.eos_id, 3, tlm, [0.0] * 3)
            assert got[0] == want[0] and got[1] == want[1]
            grid = eng.rnnt_beam_search_batch(eouts, list(ELENS), W, dec.blank_id, dec.eos_id, lm=tlm, lm_weights=[0.0, -1.0],
                                              len_weights=[2.0], tlm_fusion="device")
            assert [h[0] for h in grid[0]] == want[0] == [h[1] for h in grid[0]] and [s[0] for s in grid[1]] == want[1]


def test_grid_call_equals_single_cell_calls(dev):
    """a 3 x 2 grid (one weight <= 0) against six decode calls of one cell each: hypotheses and doubles"""
    model, _, tlm, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    lm_weights, len_weights = [0.0, 0.3, 1.0], [0.0, 1.5]
    with torch.no_grad(), _switch(dec):
        hyps, scores = eng.rnnt_beam_search_batch(eouts, list(ELENS), 4, dec.blank_id, dec.eos_id, lm=tlm, lm_weights=lm_weights,
                                                  len_weights=len_weights, tlm_fusion="device")
        c = 0
        for a in lm_weights:
            for w in len_weights:
                h1, s1, _, _ = dec.decode(eouts, list(ELENS), beam_width=4, lm=tlm, lm_weight=a, len_weight=w)
                assert [h[c] for h in hyps] == h1 and [s[c] for s in scores] == s1, (a, w)
                c += 1
    assert len(hyps[0]) == 6


def test_bf16(dev):
    """well formed (sorted, finite, a leading <sos>); mu = 0 is the unfused bf16 search bit for bit; the best hypothesis equals the f32
    device search's wherever the oracle's smallest cut gap exceeds 2 x (longest oracle hypothesis) x mu x eps, eps = the bf16 tree
    step's measured distance from f64 (tests/test_lm_tree_kernels_gpu.py); at least 2 of the 8 cases remain"""
    import math

    from tests.test_lm_tree_kernels_gpu import tree_walk_distance
    model, _, tlm, eouts, _ = _models(torch.bfloat16, dev)
    m32, _, tlm32, e32, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    eps = tree_walk_distance(torch.bfloat16, dev)[0]
    cases = _cases(dev)
    bar = {k: 2.0 * max(len(h) for h in v[1]) * k[2] * eps for k, v in cases.items()}
    keep = [k for k, v in cases.items() if v[0] > bar[k]]
    print(f"[measured] bf16 step eps {eps:.3e}; cases above their bar: {sorted(keep)} of {len(cases)}")
    assert len(keep) >= 2, (eps, {k: (v[0], bar[k]) for k, v in cases.items()})
    with torch.no_grad():
        for W in WIDTHS:
            want0 = eng.rnnt_beam_search_batch(eouts, list(ELENS), W, dec.blank_id, dec.eos_id)
            got0 = eng._rnnt_beam_search_device(eouts, list(ELENS), W, dec.blank_id, dec.eos_id, 3, tlm, [0.0] * 3)
            assert got0[0] == want0[0] and got0[1] == want0[1]
            for mu in MUS:
                with _switch(dec):
                    hyps, scores, _, _ = dec.decode(eouts, list(ELENS), beam_width=W, lm=tlm, lm_weight=mu, len_weight=LEN_W)
                with _switch(m32.decoder):
                    want = m32.decoder.decode(e32, list(ELENS), beam_width=W, lm=tlm32, lm_weight=mu, len_weight=LEN_W)[0]
                assert hyps[2] == [[dec.eos_id]] and scores[2] == [LEN_W]
                for b in (0, 1):
                    assert 1 <= len(hyps[b]) <= W and all(h[0] == dec.eos_id and all(1 <= v < 40 for v in h[1:]) for h in hyps[b])
                    assert all(math.isfinite(s) for s in scores[b]) and all(p >= q for p, q in zip(scores[b], scores[b][1:]))
                    if (b, W, mu) in keep:
                        assert hyps[b][0] == want[b][0], (b, W, mu, hyps[b], want[b])


def test_routing_of_the_switch(dev):
    """"host" (the default): a Transformer LM takes the host form, as ever; "device": the prefix tree for several utterances and, under
    rnnt_beam_impl = "device", for one; an LM outside the plan is a ValueError naming the reason; a bad value is a ValueError"""
    model, rlm, tlm, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    assert dec.rnnt_tlm_fusion == "host"
    with torch.no_grad():
        eng.rnnt_tlm_stats = None
        hyps, scores, _, _ = dec.decode(eouts, list(ELENS), beam_width=4, lm=tlm, lm_weight=0.5, len_weight=0.2)
        for b in (0, 1):
            h, s = _host(eng, dec, tlm, eouts, b, 4, 0.5, 0.2)
            assert hyps[b] == h and scores[b] == [float(v) for v in s]
        assert eng.rnnt_tlm_stats is None          # no tree was built
        with _switch(dec):
            dev_hyps, dev_scores, _, _ = dec.decode(eouts, list(ELENS), beam_width=4, lm=tlm, lm_weight=0.5, len_weight=0.2)
            used = eng.rnnt_tlm_stats
            # nodes: at most W per fused round, E - 1 = 2 fused rounds per frame; the pool is sized for 64 frames
            assert len(used["nodes"]) == 3 and used["nodes"][2] == 0 and used["node_cap"] == 4 * 2 * 64 + 1 and used["lcap"] == 64
            assert all(0 < used["nodes"][b] <= 4 * 2 * ELENS[b] for b in (0, 1)), used
            # one utterance on rnnt_beam_impl = "host": the host form, no scores
            one = dec.decode(eouts[:1, :ELENS[0]], [ELENS[0]], beam_width=4, lm=tlm, lm_weight=0.5, len_weight=0.2)
            assert one == (_host(eng, dec, tlm, eouts, 0, 4, 0.5, 0.2)[0], None, None, None)
            # the RNN LM goes where it went
            r1 = dec.decode(eouts, list(ELENS), beam_width=4, lm=rlm, lm_weight=0.5, len_weight=0.2)
        r0 = dec.decode(eouts, list(ELENS), beam_width=4, lm=rlm, lm_weight=0.5, len_weight=0.2)
        assert r0 == r1 and dev_hyps[2] == [[dec.eos_id]] and dev_scores[2] == [0.2]
        with _switch(dec, impl="device"):
            h1, s1, _, _ = dec.decode(eouts[:1, :ELENS[0]], [ELENS[0]], beam_width=4, lm=tlm, lm_weight=0.5, len_weight=0.2)
            assert h1 == dev_hyps[0] and _close(s1, dev_scores[0])
            for bad, what in ((dict(num_attention_heads=32), "heads"), (dict(vocab_size=39), "vocabulary"), (dict(max_seq_len=9000), "LDS")):
                p = dict(LM_CFG)
                p.update(bad)
                fake = SimpleNamespace(lm_type="transformer", causal=True, compute_dtype=torch.float32, f32_split=False,
                                       params=SimpleNamespace(**p))
                for e, el in ((eouts, list(ELENS)), (eouts[:1, :ELENS[0]], [ELENS[0]])):
                    with pytest.raises(ValueError, match="rnnt_tlm_fusion = 'device' cannot fuse this LM.*" + what):
                        dec.decode(e, el, beam_width=4, lm=fake, lm_weight=0.5)
        with _switch(dec, tlm="gpu"):
            with pytest.raises(ValueError, match="rnnt_tlm_fusion is 'host' or 'device'"):
                dec.decode(eouts, list(ELENS), beam_width=4, lm=tlm, lm_weight=0.5)


@pytest.mark.parametrize("what,W", [("list_cap", 3), ("node_cap", 5)])
def test_a_raised_status_bit_is_an_error_naming_the_search(dev, monkeypatch, what, W):
    """a tree too small for the search (the capacity functions patched down; a width of its own, so that the small tree is built
    afresh): a RuntimeError that names the search and the limit, not a swallowed bit"""
    from emoasr_amd import lm_tree
    model, _, tlm, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    if what == "list_cap":
        monkeypatch.setattr(lm_tree, "list_cap", lambda E, longest, max_seq_len: 2)
        match = r"search 0 \(utterance 0, lm_weight 0.5\): a hypothesis outgrew the prefix capacity of 2 tokens"
    else:
        monkeypatch.setattr(lm_tree, "node_cap", lambda W_, E, longest: 7)
        match = r"search 0 \(utterance 0, lm_weight 0.5\): the node pool is full \(7 nodes per search\)"
    with torch.no_grad(), pytest.raises(RuntimeError, match=match):
        eng.rnnt_beam_search_batch(eouts, list(ELENS), W, dec.blank_id, dec.eos_id, lm=tlm, lm_weights=[0.5], tlm_fusion="device")


def test_kept_tree_records_stay_inside_the_pool_budget(dev, monkeypatch):
    """the records the engine keeps per (searches, width, LM) hold node pools: with a budget that fits one of them the older record
    is dropped when the next is built, and the results are what they were"""
    model, _, tlm, eouts, _ = _models(torch.float32, dev)
    eng, dec = model.engine(), model.decoder
    search = lambda W: eng.rnnt_beam_search_batch(eouts, list(ELENS), W, dec.blank_id, dec.eos_id, lm=tlm, lm_weights=[0.5],
                                                  tlm_fusion="device")
    with torch.no_grad():
        want = {W: search(W) for W in WIDTHS}
        tab = eng._beam_batch_static
        pools = lambda: sorted(v.tbytes for v in tab.values() if getattr(v, "tbytes", 0))
        one = {W: 2 * 2 * 3 * (W * 2 * 64 + 1) * 128 * 4 for W in WIDTHS}          # K and V, 2 layers, 3 searches, d = 128, f32
        assert set(one.values()) <= set(pools())
        monkeypatch.setattr(eng, "_TLM_POOL_BUDGET", one[4] + one[2] // 2)
        for k in [k for k, v in tab.items() if getattr(v, "tbytes", 0)]:
            del tab[k]
        assert search(4) == want[4] and pools() == [one[4]]
        assert search(2) == want[2] and pools() == [one[2]]
        assert search(4) == want[4] and pools() == [one[4]]


class _Vocab:
    def ids2text(self, ids):
        return " ".join(f"w{i}" for i in ids)


def test_grid_tool_with_the_switch_set(dev):
    """fusion_grid.set_rnnt_tlm_fusion sets "device" for this model and LM (and keeps "host", logging why, for an LM outside the
    plan); grid_of("rnn_transducer") then returns cells that equal decode calls of one cell each"""
    from emoasr_amd import fusion_grid as fg
    from emoasr_amd.decode import strip_eos
    model, rlm, tlm, _, _ = _models(torch.float32, dev)
    dec = model.decoder
    g = load_golden("l4_tiny")[2]
    xs, xlens = g["xs"], g["xlens"]
    pairs = []
    for a in (0, 2):
        n = int(xlens[a:a + 2].max())
        pairs.append({"utt_ids": [f"utt{a}", f"utt{a + 1}"], "texts": [f"w12 w{a}", "w35"], "xs": xs[a:a + 2, :n], "xlens": xlens[a:a + 2]})
    try:
        assert fg.set_rnnt_tlm_fusion(dec, 4, rlm) == "host" and fg.set_rnnt_tlm_fusion(dec, 4, tlm) == "device"
        assert dec.rnnt_tlm_fusion == "device"
        texts = []
        lm_weights, len_weights = [0.0, 1.0], [0.0, 0.5]
        results, _ = fg.grid_of("rnn_transducer")(model, pairs, _Vocab(), 4, tlm, lm_weights, len_weights, dev, texts_out=texts)
        assert [(r[0], r[1]) for r in results] == [(0.0, 0.0), (0.0, 0.5), (1.0, 0.0), (1.0, 0.5)] and len(texts) == 4
        c = 0
        with torch.no_grad():
            for a in lm_weights:
                for w in len_weights:
                    want = []
                    for data in pairs:
                        eouts, elens, _ = model.encoder(data["xs"].to(dev), data["xlens"])
                        hyps = dec.decode(eouts, elens, beam_width=4, lm=tlm, lm_weight=a, len_weight=w)[0]
                        want += [_Vocab().ids2text(strip_eos(h[0], dec.eos_id)) for h in hyps]
                    assert texts[c] == want, (a, w)
                    c += 1
        used = model.engine().rnnt_tlm_stats          # (the cells with lm_weight 1.0 really went over the tree)
        assert len(used["nodes"]) == 2 and min(used["nodes"]) > 0
    finally:
        dec.rnnt_tlm_fusion = "host"
