"""The host scaffold of the lockstep searches (emoasr_amd/lockstep.py) without a GPU: the grid driver and its
chunk generator with fake searches, the builder of the pair of RnnlmRows under both parities, the shared admission reasons, and
fusion_grid's one pass against the values the four separate bodies returned."""
import ctypes
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from emoasr_amd import lockstep

A3 = 0.1 + 0.2      # 0.30000000000000004: another double than 0.3, another search
LM_WEIGHTS = [0.0, 0.3, -1.0, 0.5, 0.3, A3]
LEN_WEIGHTS = [0.0, 0.1]
ELENS = [9, 4, 2]


# ------------------------------------------------------------------------------------------------ the grid driver
def test_grid_chunks():
    # everything fits one chunk: utterance-major, the weights of one utterance consecutive
    assert list(lockstep.grid_chunks(3, 3, 64, ELENS)) == [([0, 1, 2], [9, 4, 2], [0, 0, 0, 1, 1, 1, 2, 2, 2], [0, 1, 2, 0, 1, 2, 0, 1, 2])]
    # two searches per chunk: an utterance with more searches than a chunk is cut by weight, its index inside the chunk is 0
    assert list(lockstep.grid_chunks(3, 3, 2, ELENS)) == [([0], [9], [0, 0], [0, 1]), ([0], [9], [0], [2]), ([1], [4], [0, 0], [0, 1]),
                                                         ([1], [4], [0], [2]), ([2], [2], [0, 0], [0, 1]), ([2], [2], [0], [2])]
    # whole utterances while they fit
    assert list(lockstep.grid_chunks(3, 2, 4, ELENS)) == [([0, 1], [9, 4], [0, 0, 1, 1], [0, 1, 0, 1]), ([2], [2], [0, 0], [0, 1])]
    assert list(lockstep.grid_chunks(3, 1, 2, ELENS)) == [([0, 1], [9, 4], [0, 1], [0, 0]), ([2], [2], [0], [0])]


def _run(cap, expand, calls):
    """the driver over fake searches: a search's two results come worse-first, so that the expansion has to sort them"""
    result = lambda b, a: ([[5], [6, 6, 6]], [-3.0 - a - b, -2.95 - a - b])

    def search_plain():
        calls.append(("plain",))
        found = [result(b, 0.0) for b in range(3)]
        return [f[0] for f in found], [f[1] for f in found]

    def search_fused(positive, weights, found):
        calls.append(("fused", list(positive), list(weights)))
        for utts, n, sutt, k_local in lockstep.grid_chunks(3, len(positive), cap, ELENS):
            ks = [positive[j] for j in k_local]
            calls.append(("chunk", utts, n, sutt, [weights[k] for k in ks]))
            for u, k in zip(sutt, ks):
                found[utts[u]][k] = result(utts[u], weights[k])

    return lockstep.run_fusion_grid(3, LM_WEIGHTS, LEN_WEIGHTS, True, search_plain, search_fused, expand)


@pytest.mark.parametrize("cap", [2, 64])
def test_run_fusion_grid_with_the_attention_searches_expansion(cap):
    """expand_len_weights: score + w * (len(hyp) + 2) in double for every search, the one without the LM too, re-sorted stably"""
    calls = []
    hyps, scores = _run(cap, lambda f, a: lockstep.expand_len_weights(*f, LEN_WEIGHTS), calls)
    assert calls[0] == ("plain",) and calls[1] == ("fused", [1, 2, 3], [0.0, 0.3, 0.5, A3])
    if cap == 64:
        assert calls[2:] == [("chunk", [0, 1, 2], [9, 4, 2], [0, 0, 0, 1, 1, 1, 2, 2, 2], [0.3, 0.5, A3] * 3)]
    else:
        assert calls[2:] == [("chunk", [b], [t], sutt, ws) for b, t in enumerate(ELENS) for sutt, ws in (([0, 0], [0.3, 0.5]), ([0], [A3]))]
    assert len(hyps) == len(scores) == 3 and all(len(h) == 12 for h in hyps)
    for b in range(3):
        for c, a in enumerate([0.0, 0.3, 0.0, 0.5, 0.3, A3]):      # (-1.0 folds into the search without the LM)
            s_short, s_long = -3.0 - a - b, -2.95 - a - b
            # len_weight 0.0: the longer hypothesis leads by its score
            assert hyps[b][2 * c] == [[6, 6, 6], [5]] and scores[b][2 * c] == [s_long, s_short]
            # len_weight 0.1: + 0.1 * 5 against + 0.1 * 3
            assert hyps[b][2 * c + 1] == [[6, 6, 6], [5]] and scores[b][2 * c + 1] == [s_long + 0.1 * 5.0, s_short + 0.1 * 3.0]
    assert scores[1][3] == [-2.95 - 0.3 - 1 + 0.1 * 5.0, -3.0 - 0.3 - 1 + 0.1 * 3.0]
    assert hyps[0][2] is hyps[0][8]                                 # one search, one expansion: the cells of a weight share it


@pytest.mark.parametrize("cap", [2, 64])
def test_run_fusion_grid_with_the_transducers_expansion(cap):
    """rnnt_len_expand: score + w * len(hyp) for the fused searches; the search without the LM is handed through unexpanded"""
    from emoasr_amd.engine.rnnt import RNNTDecoder
    calls = []
    expand = lambda f, a: [RNNTDecoder.rnnt_len_expand(*f, w) if a > 0 else f for w in LEN_WEIGHTS]
    hyps, scores = _run(cap, expand, calls)
    assert [c[0] for c in calls] == ["plain", "fused"] + ["chunk"] * (1 if cap == 64 else 6)
    for b in range(3):
        for c, a in enumerate([0.0, 0.3, 0.0, 0.5, 0.3, A3]):
            s_short, s_long = -3.0 - a - b, -2.95 - a - b
            if a == 0.0:       # as the search returned them: worse first, no len_weight
                for j in (0, 1):
                    assert hyps[b][2 * c + j] == [[5], [6, 6, 6]] and scores[b][2 * c + j] == [s_short, s_long]
            else:
                assert hyps[b][2 * c] == [[6, 6, 6], [5]] and scores[b][2 * c] == [s_long, s_short]
                assert hyps[b][2 * c + 1] == [[6, 6, 6], [5]] and scores[b][2 * c + 1] == [s_long + 0.1 * 3.0, s_short + 0.1 * 1.0]


def test_run_fusion_grid_calls_only_what_the_weights_need():
    calls = []
    plain = lambda: (calls.append("plain"), ([[[1]]] * 2, [[-1.0]] * 2))[1]

    def fused(positive, weights, found):
        calls.append(("fused", positive, weights))
        for b in range(2):
            for k in positive:
                found[b][k] = ([[2]], [-2.0])

    expand = lambda f, a: lockstep.expand_len_weights(*f, [0.0])
    lockstep.run_fusion_grid(2, [0.0, -0.5], [0.0], True, plain, fused, expand)
    assert calls == ["plain"]
    calls.clear()
    hyps, _ = lockstep.run_fusion_grid(2, [0.3, 0.5], [0.0], False, plain, fused, expand)      # without an LM every weight is the plain search
    assert calls == ["plain"] and hyps == [[[[1]], [[1]]]] * 2
    calls.clear()
    lockstep.run_fusion_grid(2, [0.3, 0.5], [0.0], True, plain, fused, expand)
    assert calls == [("fused", [0, 1], [0.3, 0.5])]


# ------------------------------------------------------------------------------------------------ the RnnlmRows pair
@pytest.mark.parametrize("even_src", [0, 1])
def test_rnnlm_rows_pair(even_src):
    from emoasr_amd import lib
    L, E, H, V, nb = 2, 48, 64, 40, 12
    w = [(torch.zeros(4 * H, E if l == 0 else H), torch.zeros(4 * H, H)) for l in range(L)]
    named = {"lm.embed.weight": torch.zeros(V, E), "lm.output.weight": torch.zeros(V, H), "lm.output.bias": torch.zeros(V)}
    lm = SimpleNamespace(L=L, E=E, H=H, _w=lambda l: w[l], _bias=[torch.zeros(4 * H) for _ in range(L)])
    LA = SimpleNamespace(w=named.__getitem__, p=named.__getitem__)
    Bf = SimpleNamespace(lm_h=torch.zeros(L, 2 * nb, H), lm_c=torch.zeros(L, 2 * nb, H), lm_logits=torch.zeros(nb, V))
    rows, tabs, ws = lockstep.rnnlm_rows_pair(lm, LA, Bf, nb, V, lib.F32, even_src)
    even, odd = rows
    # the even step reads half even_src and writes the other one, the odd step the reverse
    assert (even.src_base, even.dst_base) == (even_src * nb, (1 - even_src) * nb)
    assert (odd.src_base, odd.dst_base) == ((1 - even_src) * nb, even_src * nb)
    for rl in rows:
        assert rl.slots == 2 * nb and (rl.L, rl.E, rl.H, rl.V, rl.R) == (L, E, H, V, nb)
        assert rl.ph == Bf.lm_h.data_ptr() and rl.pc == Bf.lm_c.data_ptr()
        assert rl.logits == Bf.lm_logits.data_ptr() and rl.ldl == V
        assert rl.emb == named["lm.embed.weight"].data_ptr() and rl.w_out == named["lm.output.weight"].data_ptr()
        assert rl.b_out == named["lm.output.bias"].data_ptr()
    # one workspace and one set of tables for both
    assert even.ws == odd.ws == ws.data_ptr() and even.ws_bytes == odd.ws_bytes == ws.numel()
    assert ws.numel() == lib.size_query("emoasr_rnnlm_step_rows_ws_bytes", lib.F32, nb, H)
    for field, tab in zip(("w_ih", "w_hh", "bias"), tabs):
        assert getattr(even, field) == getattr(odd, field) == ctypes.addressof(tab)
    assert list(tabs[0]) == [w[l][0].data_ptr() for l in range(L)] and list(tabs[1]) == [w[l][1].data_ptr() for l in range(L)]
    assert list(tabs[2]) == [b.data_ptr() for b in lm._bias]


# ------------------------------------------------------------------------------------------------ the shared reasons
def _rnnlm(dtype=torch.float32, **over):
    lm = SimpleNamespace(lm_type="rnn", stateful=True, V=40, E=48, H=64, L=2, compute_dtype=dtype, f32_split=False)
    for k, v in over.items():
        setattr(lm, k, v)
    return lm


REASONS = [     # (the LM, the engine's dtype) -> the reason, as the two searches worded it before they shared it
    (SimpleNamespace(lm_type="transformer"), torch.float32,
     "lm_type 'transformer' is not 'rnn' (no per-hypothesis state the slot pools could hold)"),
    (SimpleNamespace(), torch.float32, "lm_type None is not 'rnn' (no per-hypothesis state the slot pools could hold)"),
    (_rnnlm(V=48), torch.float32, "the LM's vocabulary (48) is not the model's (40)"),
    (_rnnlm(torch.bfloat16), torch.float32,
     "the LM computes in torch.bfloat16 (split products: False), the model in torch.float32 (False)"),
    (_rnnlm(f32_split=True), torch.float32, "the LM computes in torch.float32 (split products: True), the model in torch.float32 (False)"),
    (_rnnlm(E=50), torch.float32, "the LM's sizes (embedding 50, hidden 64, layers 2) are outside emoasr_rnnlm_step_rows' shape plan"),
    (_rnnlm(torch.bfloat16, E=36), torch.bfloat16,
     "the LM's sizes (embedding 36, hidden 64, layers 2) are outside emoasr_rnnlm_step_rows' shape plan"),
]


@pytest.mark.parametrize("lm,dtype,want", REASONS)
def test_both_searches_give_the_shared_reasons(lm, dtype, want, monkeypatch):
    from emoasr_amd.modeling import beam_search_device as bsd
    from emoasr_amd.modeling import functions as F
    monkeypatch.delenv("EMOASR_DEVICE_BEAM", raising=False)
    monkeypatch.delenv("EMOASR_CPP_DECODE", raising=False)
    eng = SimpleNamespace(dtype=dtype, split=False)
    dec = SimpleNamespace(vocab_size=40, _owner=[SimpleNamespace(engine=lambda: eng)])
    assert lockstep.rnnlm_rows_why_not(eng, 40, lm) == want
    assert bsd.batch_rnnlm_why_not(dec, 4, lm, 0.3) == want
    assert F.las_rnnlm_why_not(dec, 4, lm) == want


def test_the_searches_keep_their_own_reasons(monkeypatch):
    from emoasr_amd.modeling import beam_search_device as bsd
    from emoasr_amd.modeling import functions as F
    monkeypatch.delenv("EMOASR_DEVICE_BEAM", raising=False)
    monkeypatch.delenv("EMOASR_CPP_DECODE", raising=False)
    eng = SimpleNamespace(dtype=torch.float32, split=False)
    dec = SimpleNamespace(vocab_size=40, _owner=[SimpleNamespace(engine=lambda: eng)])
    assert lockstep.rnnlm_rows_why_not(eng, 40, _rnnlm()) is None
    assert bsd.batch_rnnlm_why_not(dec, 4, _rnnlm(), 0.3) is None and F.las_rnnlm_why_not(dec, 4, _rnnlm()) is None
    assert bsd.batch_rnnlm_why_not(dec, 22, _rnnlm(), 0.3) == ("beam_width 22 (candidate width 33, vocabulary 40) is outside the device "
                                                              "bookkeeping's 32 beams x 32 candidates")
    assert F.las_rnnlm_why_not(dec, 33, _rnnlm()) == "beam_width 33 (vocabulary 40) is outside the device bookkeeping's 32 beams"
    monkeypatch.setenv("EMOASR_CPP_DECODE", "0")
    assert bsd.batch_rnnlm_why_not(dec, 4, _rnnlm(), 0.3) == "EMOASR_CPP_DECODE=0 forces the host bookkeeping"
    assert F.las_rnnlm_why_not(dec, 4, _rnnlm()) is None


def test_log_once(caplog):
    from emoasr_amd.modeling import functions as F
    logger = logging.getLogger("emoasr_amd.test_lockstep")
    F._LAS_FUSION_LOGGED.clear()         # (the name the LAS tests reset: the same set)
    with caplog.at_level(logging.INFO):
        for _ in range(3):
            lockstep.log_once(logger, "a reason")
        lockstep.log_once(logger, "another reason")
    assert [r.getMessage() for r in caplog.records] == ["a reason", "another reason"]


def test_the_moved_names_stay_importable():
    from emoasr_amd.modeling import beam_search_device as bsd
    for name in ("batch_pack_sizes", "batch_step_reported", "batch_nbest_from_pack", "grid_cell_plan", "grid_chunk_plan", "expand_len_weights"):
        assert getattr(bsd, name) is getattr(lockstep, name), name
    assert lockstep.batch_pack_sizes(3, 4, 6) == [24, 12, 12, 12, 72, 72]


# ------------------------------------------------------------------------------------------------ fusion_grid's one pass
REFS = [[3, 4, 5], [6, 7], [8]]          # the reference ids of the three utterances: two batches, (0, 1) and (2,)
GRID_LM, GRID_LEN = [0.0, 0.5, 1.0], [0.0, 1.0]


def _cell_hyps(u, c):
    """the N-best list of utterance u in cell c: an insertion, a deletion (an empty hypothesis for the one-word utterance), the
    reference with <eos> = 2 in it, the reference, an empty N-best list, the reference reversed"""
    r = REFS[u]
    return [[r + [9], [1]], [r[:-1]], [[2] + r + [2], r], [r], [], [r[::-1]]][c]


class _Xs:
    def __init__(self, utts):
        self.utts = utts

    def to(self, device):
        return self


def _grid_fakes(kind):
    words = lambda ids: " ".join(f"w{i}" for i in ids)
    loader = [{"xs": _Xs(u), "xlens": [10 + i for i in u], "texts": [words(REFS[i]) for i in u]} for u in ((0, 1), (2,))]
    decoder = SimpleNamespace(decode=lambda eouts, elens, inter, bw, decode_ctc_weight=0: ([[REFS[u][0]] for u in eouts], None, None, None))
    model = SimpleNamespace(decoder_type=kind, decoder=decoder, encoder=lambda xs, xlens: (xs.utts, xlens, "inter"))
    return model, loader, SimpleNamespace(ids2text=words)


def _fake_searches(monkeypatch, seen):
    from emoasr_amd.modeling import beam_search_device as bsd
    from emoasr_amd.modeling import ctc_beam_search as cbs
    from emoasr_amd.modeling import functions as F
    nbest = lambda eouts: [[_cell_hyps(u, c) for c in range(6)] for u in eouts]

    def ctc(dec, eouts, elens, bw, lm, cells):
        seen.append(("ctc", eouts, list(elens), bw, [(float(a), float(b)) for a, b in cells]))
        return nbest(eouts), None, None

    def joint(dec, eouts, elens, bw, lm, lm_weights, len_weights, ctc_weight):
        seen.append(("joint", eouts, list(elens), bw, list(lm_weights), list(len_weights), ctc_weight))
        return nbest(eouts), None

    def apply(name):
        def fn(dec, eouts, elens, bw, lm, lm_weights, len_weights):
            seen.append((name, eouts, list(elens), bw, list(lm_weights), list(len_weights)))
            return nbest(eouts), None
        return fn

    monkeypatch.setattr(cbs, "ctc_prefix_beam_search_batch_lm", ctc)
    monkeypatch.setattr(bsd, "joint_beam_search_device_grid", joint)
    monkeypatch.setattr(F, "rnnt_fusion_grid_apply", apply("rnnt"))
    monkeypatch.setattr(F, "las_fusion_grid_apply", apply("las"))


# what the four separate bodies returned for these fakes before they became one pass
WANT_RESULTS = [(0.0, 0.0, 50.0, "WER: 50.00 [D=0, S=0, I=3, N=6]"),
                (0.0, 1.0, 50.0, "WER: 50.00 [D=2, S=1, I=0, N=6]"),        # a tie with the first cell: best does not move
                (0.5, 0.0, 0.0, "WER: 0.00 [D=0, S=0, I=0, N=6]"),
                (0.5, 1.0, 0.0, "WER: 0.00 [D=0, S=0, I=0, N=6]"),          # a tie again
                (1.0, 0.0, 100.0, "WER: 100.00 [D=3, S=3, I=0, N=6]"),
                (1.0, 1.0, 66.66666666666667, "WER: 66.67 [D=1, S=2, I=1, N=6]")]
WANT_BEST = (0.5, 0.0, 0.0, "WER: 0.00 [D=0, S=0, I=0, N=6]")
WANT_TEXTS = [["w3 w4 w5 w9", "w6 w7 w9", "w8 w9"], ["w3 w4", "w6", ""], ["w3 w4 w5", "w6 w7", "w8"], ["w3 w4 w5", "w6 w7", "w8"],
              ["", "", ""], ["w5 w4 w3", "w7 w6", "w8"]]
WANT_GREEDY_RESULTS = [(a, b, 50.0, "WER: 50.00 [D=3, S=0, I=0, N=6]") for a in GRID_LM for b in GRID_LEN]
WANT_GREEDY_TEXTS = [["w3", "w6", "w8"]] * 6

KINDS = [("ctc", "ctc_fusion_grid"), ("transformer", "joint_fusion_grid"), ("rnn_transducer", "rnnt_fusion_grid"), ("las", "las_fusion_grid")]


@pytest.mark.parametrize("kind,name", KINDS)
def test_grid_pass_equals_the_separate_bodies(kind, name, monkeypatch):
    from emoasr_amd import fusion_grid as fg
    seen = []
    _fake_searches(monkeypatch, seen)
    model, loader, vocab = _grid_fakes(kind)
    texts = []
    results, best = getattr(fg, name)(model, loader, vocab, 4, "lm", GRID_LM, GRID_LEN, None, texts_out=texts)
    assert results == WANT_RESULTS and best == WANT_BEST and texts == WANT_TEXTS
    assert all(type(r[0]) is np.float64 and type(r[1]) is np.float64 for r in results)
    # one search call per batch, with what the body handed over before
    tag = {"ctc": "ctc", "transformer": "joint", "rnn_transducer": "rnnt", "las": "las"}[kind]
    cells = [(a, b) for a in GRID_LM for b in GRID_LEN]
    tail = {"ctc": (cells,), "transformer": (GRID_LM, GRID_LEN, 0)}.get(kind, (GRID_LM, GRID_LEN))
    assert seen == [(tag, (0, 1), [10, 11], 4) + tail, (tag, (2,), [12], 4) + tail]


@pytest.mark.parametrize("kind,name", KINDS)
def test_grid_pass_at_ctc_weight_one(kind, name, monkeypatch):
    """decode_ctc_weight == 1: greedy CTC once per batch for every cell -- but the CTC grid refuses any decode_ctc_weight > 0"""
    from emoasr_amd import fusion_grid as fg
    seen = []
    _fake_searches(monkeypatch, seen)
    model, loader, vocab = _grid_fakes(kind)
    texts = []
    if kind == "ctc":
        with pytest.raises(NotImplementedError, match="decode_ctc_weight > 0 is the joint CTC / attention search"):
            fg.ctc_fusion_grid(model, loader, vocab, 4, "lm", GRID_LM, GRID_LEN, None, decode_ctc_weight=1)
        return
    results, best = getattr(fg, name)(model, loader, vocab, 4, "lm", GRID_LM, GRID_LEN, None, decode_ctc_weight=1, texts_out=texts)
    assert seen == [] and results == WANT_GREEDY_RESULTS and best == WANT_GREEDY_RESULTS[0] and texts == WANT_GREEDY_TEXTS


@pytest.mark.parametrize("kind,name", KINDS)
def test_grid_functions_refuse_the_other_decoders(kind, name):
    from emoasr_amd import fusion_grid as fg
    other = "las" if kind != "las" else "ctc"
    want = (f"emoasr_amd.fusion_grid handles CTC models only (decoder_type == 'ctc'), not {other!r}" if kind == "ctc" else
            f"emoasr_amd.fusion_grid.{name} handles decoder_type == {kind!r}, not {other!r}")
    with pytest.raises(NotImplementedError) as info:
        getattr(fg, name)(SimpleNamespace(decoder_type=other), [], None, 4, object(), [0.1], [0.0], "cpu")
    assert str(info.value) == want
