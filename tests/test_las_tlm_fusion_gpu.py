"""Transformer-LM shallow fusion in the LAS beam search on the device: LASDecoder.decode under
las_lm_fusion = "fuse" and las_tlm_fusion = "device" against the reference's modules (tests/golden/las_tlm_fusion_tiny.npz, written by
tests/golden/make_golden_las_tlm_fusion.py), the device and host forms against each other, chunks, the (lm_weight, len_weight) grid,
the tree's limits, the refusals and bf16."""
from types import SimpleNamespace

import pytest
import torch

from tests import las_beam_util as UB
from tests import las_tlm_fusion_util as U
from tests.test_las_fusion_gpu import _asr, _padded, _same
from tests.util import LM_CFG, load_ctc_beam_golden

pytestmark = pytest.mark.gpu

_CACHE = {}


def _pair(dev, mode):
    """the las_tiny model (eval mode) and the Transformer LM of LM_CFG / ctcbeam_tiny in the same compute dtype, one pair per dtype"""
    if mode not in _CACHE:
        from emoasr_amd.modeling.lm import LM
        lm = LM(SimpleNamespace(**LM_CFG), compute_dtype=mode)
        lm.load_state_dict(load_ctc_beam_golden()[2])
        _CACHE[mode] = (_asr(dev, mode), lm.to(dev).eval())
    return _CACHE[mode]


@pytest.fixture
def fused(dev):
    """(f32 model with las_lm_fusion = "fuse" and las_tlm_fusion = "device" for the test, the LM)"""
    model, lm = _pair(dev, torch.float32)
    dec = model.decoder
    dec.las_lm_fusion, dec.las_tlm_fusion = "fuse", "device"
    yield model, lm
    dec.las_lm_fusion, dec.las_tlm_fusion, dec.las_beam_impl = "ignore", "host", "single"


@pytest.fixture(scope="module")
def gold():
    return U.load_las_tlm_fusion_golden()[1]


@pytest.fixture(scope="module")
def gold_unfused():
    return UB.load_las_beam_golden()[1]


def _count(monkeypatch, model, lm):
    """-> (utterances of every batched search of the engine, host LM calls) from here on"""
    from emoasr_amd.modeling.functions import _engine_of
    eng = _engine_of(model.decoder)
    calls, host = [], []
    orig = eng.las_beam_search_batch
    monkeypatch.setattr(eng, "las_beam_search_batch", lambda *a, **k: (calls.append(len(a[1])), orig(*a, **k))[1])
    for name in ("predict", "predict_device"):
        f = getattr(lm, name)
        monkeypatch.setattr(lm, name, lambda *a, _f=f, **k: (host.append(1), _f(*a, **k))[1])
    return calls, host


_E2E = [(a, W, lw) for a, W in U.CASES for lw in U.LEN_WEIGHTS]


@pytest.mark.parametrize("a,W,lw", _E2E, ids=[f"lm{a}-W{W}-lw{lw}" for a, W, lw in _E2E])
def test_groups_against_the_reference_f32(dev, fused, gold, gold_unfused, a, W, lw, monkeypatch):
    """every recorded group as ONE decode call on the five searches of set A, padded with 50 * randn (the 1-frame utterance among
    them): the fixture's hypotheses in order, scores within 1e-3 |score|, exactly one batched search and no lm.predict /
    predict_device call; the same call under las_tlm_fusion = "host" returns the same lists through the host form, scores within
    1e-4; under las_lm_fusion = "ignore" the unfused lists of las_beam_tiny come back"""
    model, lm = fused
    dec = model.decoder
    eouts, elens = _padded(U.SEARCHES, dev)
    calls, host = _count(monkeypatch, model, lm)
    hyps, scores, logits, aligns = dec.decode(eouts, torch.tensor(elens), None, W, lw, lm=lm, lm_weight=a, decode_ctc_weight=0.3)
    assert calls == [len(U.SEARCHES)] and host == [] and logits is None and aligns is None
    assert len(hyps) == len(scores) == len(U.SEARCHES)
    for b, (u, t) in enumerate(U.SEARCHES):
        want, wscores = U.fused_nbest(gold, u, t, W, lw, a)
        assert hyps[b] == want, (b, hyps[b], want)
        assert len(scores[b]) == len(wscores)
        assert all(abs(s - w) <= 1e-3 * abs(w) for s, w in zip(scores[b], wscores)), (b, scores[b], wscores)
    dec.las_tlm_fusion = "host"
    h2, s2, _, _ = dec.decode(eouts, torch.tensor(elens), None, W, lw, lm=lm, lm_weight=a, decode_ctc_weight=0.3)
    assert calls == [len(U.SEARCHES)] and len(host) >= len(U.SEARCHES), "the host form steps the LM itself, utterance by utterance"
    assert h2 == hyps and all(_same(x, y, 1e-4) for x, y in zip(s2, scores)), (h2, hyps, s2, scores)
    dec.las_lm_fusion, dec.las_tlm_fusion = "ignore", "device"
    host.clear()
    h3, s3, _, _ = dec.decode(eouts, torch.tensor(elens), None, W, lw, lm=lm, lm_weight=a, decode_ctc_weight=0.3)
    assert calls == [len(U.SEARCHES)] * 2 and host == []
    for b, (u, t) in enumerate(U.SEARCHES):
        want, wscores = UB.golden_nbest(gold_unfused, u, t, W, lw)
        assert h3[b] == want, (b, h3[b], want)
        assert all(abs(s - w) <= 1e-3 * abs(w) for s, w in zip(s3[b], wscores)), (b, s3[b], wscores)


@pytest.mark.parametrize("lw", U.LEN_WEIGHTS)
def test_forms_against_each_other(dev, fused, gold, lw, monkeypatch):
    """W = 3, lm_weight = 0.3, set A: one utterance through las_beam_impl = "batch" (one under "single" stays the host form), and
    chunks [2, 2, 1] -- equal hypotheses, scores within 1e-4"""
    from emoasr_amd.engine import las as eng_las
    from emoasr_amd.modeling.functions import _engine_of
    model, lm = fused
    dec = model.decoder
    W, a = 3, 0.3
    eouts, elens = _padded(U.SEARCHES, dev)
    hyps, scores, _, _ = dec.decode(eouts, elens, None, W, lw, lm=lm, lm_weight=a)
    assert hyps == [U.fused_nbest(gold, u, t, W, lw, a)[0] for u, t in U.SEARCHES]
    calls, host = _count(monkeypatch, model, lm)
    for b, n in enumerate(elens):
        h, s, _, _ = dec.decode(eouts[b:b + 1, :n].contiguous(), [n], None, W, lw, lm=lm, lm_weight=a)
        assert calls == [] and len(host) >= 1, "one utterance under 'single' is the host form"
        assert h == hyps[b] and _same(s, scores[b], 1e-4), (b, h, hyps[b], s, scores[b])
        host.clear()
        dec.las_beam_impl = "batch"
        h2, s2, l2, a2 = dec.decode(eouts[b:b + 1], [n], None, W, lw, lm=lm, lm_weight=a)     # (its padding still attached)
        dec.las_beam_impl = "single"
        assert calls == [1] and host == [] and l2 is None and a2 is None
        calls.clear()
        assert h2 == hyps[b] and isinstance(s2, list) and _same(s2, scores[b], 1e-4)
    eng = _engine_of(dec)
    chunks, orig = [], eng._las_beam_chunk
    monkeypatch.setattr(eng_las, "las_beam_chunk_capacity", lambda *a_, **k: 2)
    monkeypatch.setattr(eng, "_las_beam_chunk", lambda *a_, **k: (chunks.append((len(a_[1]), a_[6] is lm, a_[7], k)), orig(*a_, **k))[1])
    parts = dec.decode(eouts, elens, None, W, lw, lm=lm, lm_weight=a)
    assert chunks == [(2, True, a, dict(first=0)), (2, True, a, dict(first=2)), (1, True, a, dict(first=4))] and host == []
    assert parts[0] == hyps and all(_same(x, y, 1e-4) for x, y in zip(parts[1], scores))


@pytest.mark.parametrize("W,lm_weights", [(3, [0.0, 0.3, 0.5]), (8, [0.0, 0.2, 2.0])], ids=["W3", "W8"])
def test_grid(dev, fused, gold, gold_unfused, W, lm_weights, monkeypatch):
    """lm_weights x len_weights [0, 0.1] on set A in ONE call: every cell against the fixtures at the end-to-end bar and against one
    batched decode per cell (hypotheses equal, scores within 1e-4); the cells of one lm_weight come from one search (two chunks:
    the unfused searches, and ten fused ones over five utterances' frames, each with its own node share); the lm_weight = 0 cells
    are bit-equal to the unfused batched search"""
    from emoasr_amd.modeling.functions import _engine_of, las_fusion_grid_apply
    model, lm = fused
    dec = model.decoder
    eng = _engine_of(dec)
    len_weights = [0.0, 0.1]
    eouts, elens = _padded(U.SEARCHES, dev)
    chunks, orig = [], eng._las_beam_chunk

    def spy(*a, **k):
        grid = k.get("grid")
        chunks.append((len(a[1]), None if grid is None else (list(grid[0]), list(grid[1]))))
        return orig(*a, **k)

    monkeypatch.setattr(eng, "_las_beam_chunk", spy)
    _, host = _count(monkeypatch, model, lm)
    hyps, scores = las_fusion_grid_apply(dec, eouts, elens, W, lm, lm_weights, len_weights)
    assert chunks == [(5, None), (5, ([0, 0, 1, 1, 2, 2, 3, 3, 4, 4], lm_weights[1:] * 5))] and host == []
    assert eng._las_beam_bufs[1].tree.S == 10 and eng._las_beam_bufs[1].tree.nnodes.min().item() >= 1
    monkeypatch.setattr(eng, "_las_beam_chunk", orig)
    assert len(hyps) == len(scores) == 5 and all(len(h) == 6 for h in hyps)
    cells = [(a, lw) for a in lm_weights for lw in len_weights]
    for c, (a, lw) in enumerate(cells):
        dec.las_lm_fusion = "fuse" if a > 0 else "ignore"
        h1, s1, _, _ = dec.decode(eouts, elens, None, W, lw, lm=lm, lm_weight=a)
        for b, (u, t) in enumerate(U.SEARCHES):
            want, wscores = U.fused_nbest(gold, u, t, W, lw, a) if a > 0 else UB.golden_nbest(gold_unfused, u, t, W, lw)
            assert hyps[b][c] == want, (a, lw, b, hyps[b][c], want)
            assert len(scores[b][c]) == len(wscores)
            assert all(abs(s - w) <= 1e-3 * abs(w) for s, w in zip(scores[b][c], wscores)), (a, lw, b)
            assert h1[b] == hyps[b][c] and _same(s1[b], scores[b][c], 1e-4), (a, lw, b, s1[b], scores[b][c])
            if a == 0:
                assert s1[b] == scores[b][c], (lw, b, s1[b], scores[b][c])       # bit-equal
    assert host == []


def test_a_tree_too_small_names_the_search_and_the_limit(dev, fused, monkeypatch):
    """the capacities patched down: a node share of 7 is used up by the third step of a width-4 search, a list of 2 tokens is
    outgrown by the third -- a RuntimeError naming the utterance (and the weight, in a grid) and the limit, not a wrong result"""
    from emoasr_amd import lm_tree
    from emoasr_amd.modeling.functions import las_fusion_grid_apply
    model, lm = fused
    dec = model.decoder
    eouts, elens = _padded(U.SEARCHES[:3], dev)
    monkeypatch.setattr(lm_tree, "las_node_cap", lambda W, max_len: 7)
    with pytest.raises(RuntimeError, match=r"las_tlm_fusion = 'device'\): utterance 0: the node pool is full \(7 nodes per search\) "
                                           r"\[POOL_FULL\]; utterance 1: .*; utterance 2: "):
        dec.decode(eouts, elens, None, 4, 0.0, lm=lm, lm_weight=0.3)
    with pytest.raises(RuntimeError, match=r"utterance 1 at lm_weight 0.5: the node pool is full"):
        las_fusion_grid_apply(dec, eouts, elens, 4, lm, [0.3, 0.5], [0.0])
    monkeypatch.undo()
    monkeypatch.setattr(lm_tree, "las_list_cap", lambda max_len, max_seq_len: 2)
    with pytest.raises(RuntimeError, match=r"utterance 0: a hypothesis outgrew the prefix capacity of 2 tokens \[OVERLEN\]"):
        dec.decode(eouts, elens, None, 4, 0.0, lm=lm, lm_weight=0.3)
    monkeypatch.undo()
    hyps, _, _, _ = dec.decode(eouts, elens, None, 4, 0.0, lm=lm, lm_weight=0.3)          # and with its own capacities it runs
    assert all(len(h) >= 1 for h in hyps)


def test_device_refuses_what_the_tree_cannot_take(dev, fused, monkeypatch):
    """V_lm != V, a non-causal LM and width 33 under "device": a ValueError with las_tlm_why_not's reason before any search (under
    "host" the same calls fall back to the host form, as tests/test_las_fusion_gpu.py pins)"""
    from emoasr_amd.modeling.lm import LM
    model, lm = fused
    dec = model.decoder
    eouts, elens = _padded(U.SEARCHES[:3], dev)
    calls, host = _count(monkeypatch, model, lm)
    torch.manual_seed(1)
    wide = LM(SimpleNamespace(**dict(LM_CFG, vocab_size=LM_CFG["vocab_size"] + 8)), compute_dtype=torch.float32).to(dev).eval()
    with pytest.raises(ValueError, match=r"las_tlm_fusion = 'device' cannot fuse this LM: the LM's vocabulary \(48\) is not the model's \(40\)"):
        dec.decode(eouts, elens, None, 3, 0.1, lm=wide, lm_weight=0.5)
    with pytest.raises(ValueError, match="cannot fuse this LM: beam_width 33"):
        dec.decode(eouts, elens, None, 33, 0.1, lm=lm, lm_weight=0.5)
    monkeypatch.setattr(lm, "causal", False)
    with pytest.raises(ValueError, match="cannot fuse this LM: there is no causal LM"):
        dec.decode(eouts, elens, None, 3, 0.1, lm=lm, lm_weight=0.5)
    assert calls == [] and host == []
    dec.las_tlm_fusion = "gpu"
    with pytest.raises(ValueError, match="las_tlm_fusion is 'host' or 'device', not 'gpu'"):
        dec.decode(eouts, elens, None, 3, 0.1, lm=lm, lm_weight=0.5)


@pytest.mark.parametrize("a,W,lw", [(1.0, 1, 0.0), (1.0, 1, 0.1), (0.3, 4, 0.0), (1.0, 4, 0.1)])
def test_fused_bf16(dev, gold, a, W, lw):
    """test_las_fusion_gpu.py's bf16 rule on the three uncut utterances: well-formed lists; width 1 (margin 8.9e-2) gives the fixture's
    hypothesis; the best score within 2e-2 |w| + 2e-2"""
    model, lm = _pair(dev, torch.bfloat16)
    dec = model.decoder
    dec.las_lm_fusion, dec.las_tlm_fusion = "fuse", "device"
    try:
        searches = U.SEARCHES[:3]
        eouts, elens = _padded(searches, dev)
        hyps, scores, _, _ = dec.decode(eouts, elens, None, W, lw, lm=lm, lm_weight=a)
    finally:
        dec.las_lm_fusion, dec.las_tlm_fusion = "ignore", "host"
    for b, (u, t) in enumerate(searches):
        want, wscores = U.fused_nbest(gold, u, t, W, lw, a)
        assert hyps[b] and scores[b] and len(hyps[b]) == len(scores[b]) <= W and scores[b] == sorted(scores[b], reverse=True)
        assert all(len(h) >= 1 and all(0 <= v < 40 and v != 2 for v in h) for h in hyps[b])
        if W == 1:
            assert hyps[b] == want, (b, hyps[b], want)
        assert abs(scores[b][0] - wscores[0]) <= 2e-2 * abs(wscores[0]) + 2e-2, (b, scores[b], wscores)
