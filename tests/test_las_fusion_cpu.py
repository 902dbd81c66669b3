"""RNN-LM shallow fusion in the LAS beam search without a GPU: the fixture, the header / binding tables of
emoasr_las_attend_cells, the routing of LASDecoder.decode under both values of las_lm_fusion, every reason of las_rnnlm_why_not,
the command-line tool's dispatch and the grid's de-duplication plan."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import las_beam_util as UB
from tests import las_fusion_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def fx():
    return U.load_las_fusion_golden()


def test_fixture_is_complete(fx):
    groups, g = fx
    assert groups == U.GROUPS
    assert g["searches"].tolist() == U.SEARCHES and tuple(g["len_weights"].tolist()) == U.LEN_WEIGHTS
    want = {f"{U.fusion_key(u, t, W, lw, a)}/{part}" for a, W in U.CASES for u, t in U.SEARCHES for lw in U.LEN_WEIGHTS
            for part in ("hyps", "lens", "scores", "margin")}
    assert set(g) - {"searches", "len_weights"} == want
    for a, W in U.CASES:
        for u, t in U.SEARCHES:
            for lw in U.LEN_WEIGHTS:
                hyps, scores = U.fused_nbest(g, u, t, W, lw, a)
                assert 1 <= len(hyps) <= W and len(scores) == len(hyps) and all(len(h) >= 1 for h in hyps)
                assert scores == sorted(scores, reverse=True)
                assert all(0 <= v < 40 and v != 2 for h in hyps for v in h)     # (<eos> = 2 is stripped)


def test_every_margin_exceeds_the_bar(fx):
    _, g = fx
    margins = {k: float(v) for k, v in g.items() if k.endswith("/margin")}
    assert len(margins) == len(U.CASES) * len(U.SEARCHES) * len(U.LEN_WEIGHTS)
    assert min(margins.values()) > U.MARGIN, min(margins.items(), key=lambda kv: kv[1])


def test_every_group_differs_from_the_unfused_search(fx):
    """the LM decides something in every (W, lm_weight) group: a search that ignores it cannot return the fixture"""
    _, g = fx
    _, unfused = UB.load_las_beam_golden()
    for a, W in U.CASES:
        changed = sum(U.fused_nbest(g, u, t, W, 0.0, a)[0] != UB.golden_nbest(unfused, u, t, W, 0.0)[0] for u, t in U.SEARCHES)
        assert changed >= 1, (a, W)


# ------------------------------------------------------------------------------------------------ header and bindings
def _struct_fields(header, name):
    """the field names of `typedef struct ... { ... } name;` in declaration order"""
    body = re.search(r"typedef struct \w+ \{([^}]*)\} " + name + ";", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            names.append(re.search(r"(\w+)\s*$", part.strip()).group(1))
    return names


def test_new_entry_points_are_declared_and_bound():
    from emoasr_amd import lib
    header = open(os.path.join(ROOT, "include", "emoasr_hip.h")).read()
    for name in ("emoasr_las_attend_cells", "emoasr_las_cells_check"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES, name
        assert hasattr(lib.load(), name), name
    want = ["g", "U", "sutt"]
    assert _struct_fields(header, "emoasr_las_attend_cells_t") == want
    assert [f[0] for f in lib.LasAttendCells._fields_] == want
    assert lib.LasAttendCells._fields_[0][1] is lib.LasAttendGroup
    assert lib.SIGNATURES["emoasr_las_attend_cells"] == [ctypes.c_int, ctypes.POINTER(lib.LasAttendCells), ctypes.c_void_p]
    assert lib.SIGNATURES["emoasr_las_cells_check"] == [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    # the group form keeps its layout
    assert _struct_fields(header, "emoasr_las_attend_group_t") == [f[0] for f in lib.LasAttendGroup._fields_]


def test_the_host_check_of_the_map():
    """emoasr_las_cells_check runs on the host: utterances 0 .. U - 1 in order, the searches of one consecutive, none missing"""
    from emoasr_amd import lib
    check = lambda sutt, U_: lib.call("emoasr_las_cells_check", len(sutt), (ctypes.c_int * len(sutt))(*sutt), U_)
    check([0], 1)
    check([0, 1, 1, 1, 2, 2], 3)
    check([0, 0, 0], 1)
    for sutt, U_, what in (([1, 1], 2, "starts at utterance 0"), ([0, 2, 2], 3, "after utterance 0"), ([0, 1, 0], 2, "after utterance 1"),
                           ([0, 1, 1], 3, "ends at utterance 1 of 3"), ([0, 1], 1, "ends at utterance 1 of 1"), ([0, -1], 1, "after utterance 0"),
                           ([0], 2, "2 utterances for 1 searches")):
        with pytest.raises(lib.EmoasrHipError, match=what):
            check(sutt, U_)


# ------------------------------------------------------------------------------------------------ routing
class _LMNext:          # a next-token Transformer LM as far as the routing looks
    stateful = False
    lm_type = "transformer"


def _rnnlm(dtype=torch.float32, **over):
    lm = SimpleNamespace(lm_type="rnn", stateful=True, V=40, E=48, H=64, L=2, compute_dtype=dtype, f32_split=False)
    for k, v in over.items():
        setattr(lm, k, v)
    return lm


def _decoder(vocab=40, dtype=torch.float32, split=False):
    from emoasr_amd.modeling.decoders.las import LASDecoder
    p = SimpleNamespace(vocab_size=vocab, embedding_size=8, enc_hidden_size=8, dec_hidden_size=8, dec_num_layers=1, attn_dim=8,
                        dec_intermediate_size=8, dropout_dec_rate=0.0, lsm_prob=0.0, loss_normalize_length=False,
                        loss_normalize_batch=True, kd_weight=0, mtl_ctc_weight=0.0, eos_id=2, max_decode_ylen=5)
    dec = LASDecoder(p)
    calls = []

    class _Eng:
        def las_beam_search(self, eouts, bw, lw, eos, max_len, lm=None, lm_weight=0):
            calls.append(("host", tuple(eouts.shape), lm, lm_weight))
            return [[7, int(eouts.shape[1])]] * min(bw, 2), [-1.0, -2.0][:min(bw, 2)]

        def las_beam_search_batch(self, eouts, elens, bw, lw, eos, max_len, lm=None, lm_weight=0, lm_weights=None, len_weights=None):
            calls.append(("batch", tuple(eouts.shape), [int(n) for n in elens], lm, lm_weight if lm_weights is None else list(lm_weights)))
            if lm_weights is not None:
                n = len(lm_weights) * len(len_weights)
                return [[[[7, b]]] * n for b in range(len(elens))], [[[-1.0]] * n for _ in elens]
            hyps = [[[7, int(n)]] * min(bw, 2) for n in elens]
            return hyps, [[-1.0, -2.0][:len(h)] for h in hyps]

    eng = _Eng()
    eng.dtype, eng.split = dtype, split
    dec._owner = [SimpleNamespace(engine=lambda: eng)]
    return dec, calls


def test_default_is_ignore_and_a_bad_value_raises():
    dec, calls = _decoder()
    assert dec.las_lm_fusion == "ignore"
    dec.las_lm_fusion = "on"
    for eouts, elens in ((torch.zeros(3, 9, 8), [9, 4, 2]), (torch.zeros(1, 9, 8), [9])):
        with pytest.raises(ValueError, match="las_lm_fusion is 'ignore' or 'fuse', not 'on'"):
            dec.decode(eouts, elens, beam_width=4, lm=_rnnlm(), lm_weight=0.3)
        with pytest.raises(ValueError, match="las_lm_fusion"):
            dec.decode(eouts, elens, beam_width=4)
    assert calls == []


def test_routing_of_decode_under_both_values(caplog):
    import logging
    from emoasr_amd.modeling import functions as F
    from emoasr_amd.modeling.lm import _NO_PREDICT
    F._LAS_FUSION_LOGGED.clear()
    dec, calls = _decoder()
    one, three = torch.zeros(1, 9, 8), torch.zeros(3, 9, 8)
    lm = _rnnlm()
    kw = dict(beam_width=4, lm=lm, lm_weight=0.3, decode_ctc_weight=0.3)
    # "ignore": today's searches, the LM never reaches the engine -- not even a masked one is looked at
    dec.decode(three, [9, 4, 2], **kw)
    dec.decode(one, [9], **kw)
    dec.decode(one, [9], beam_width=4, lm=SimpleNamespace(lm_type="bert"), lm_weight=0.3)
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], None, 0), ("host", (1, 9, 8), None, 0), ("host", (1, 9, 8), None, 0)]
    # "fuse": several utterances -> the device form; one utterance -> the host form, or the device form under "batch"
    calls.clear()
    dec.las_lm_fusion = "fuse"
    h, s, _, _ = dec.decode(three, [9, 4, 2], **kw)
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], lm, 0.3)]
    assert h == [[[7, 9], [7, 9]], [[7, 4], [7, 4]], [[7, 2], [7, 2]]] and s == [[-1.0, -2.0]] * 3
    calls.clear()
    h, s, _, _ = dec.decode(one, [9], **kw)
    assert calls == [("host", (1, 9, 8), lm, 0.3)] and h == [[7, 9], [7, 9]] and s == [-1.0, -2.0]
    calls.clear()
    dec.las_beam_impl = "batch"
    h, s, _, _ = dec.decode(one, [9], **kw)
    assert calls == [("batch", (1, 9, 8), [9], lm, 0.3)] and h == [[7, 9], [7, 9]] and s == [-1.0, -2.0]
    dec.las_beam_impl = "single"
    # no LM, or a weight <= 0: the unfused search
    calls.clear()
    dec.decode(three, [9, 4, 2], beam_width=4, lm=lm, lm_weight=0.0)
    dec.decode(three, [9, 4, 2], beam_width=4, lm=None, lm_weight=0.3)
    dec.decode(three, [9, 4, 2], beam_width=4, lm=lm, lm_weight=-1.0)
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], None, 0)] * 3
    # an LM the device form cannot take, and beams wider than 32 / than V: the host form per utterance, the reason logged ONCE
    calls.clear()
    with caplog.at_level(logging.INFO):
        for _ in range(2):
            h, s, _, _ = dec.decode(three, [9, 4, 2], beam_width=4, lm=_LMNext(), lm_weight=0.3)
    assert [c[:2] for c in calls] == [("host", (1, 9, 8)), ("host", (1, 4, 8)), ("host", (1, 2, 8))] * 2
    assert all(isinstance(c[2], _LMNext) and c[3] == 0.3 for c in calls)
    assert h == [[[7, 9], [7, 9]], [[7, 4], [7, 4]], [[7, 2], [7, 2]]] and s == [[-1.0, -2.0]] * 3
    assert sum("lm_type 'transformer'" in r.getMessage() for r in caplog.records) == 1
    for bad, bw in ((_rnnlm(V=48), 4), (lm, 33), (_rnnlm(torch.bfloat16), 4)):
        calls.clear()
        h, s, _, _ = dec.decode(three, [9, 4, 2], beam_width=bw, lm=bad, lm_weight=0.3)
        assert [c[:2] for c in calls] == [("host", (1, 9, 8)), ("host", (1, 4, 8)), ("host", (1, 2, 8))] and all(c[2] is bad for c in calls)
        assert len(h) == len(s) == 3
    # the unfused search's own fall-back for wide beams stays (no LM in it)
    calls.clear()
    dec.decode(three, [9, 4, 2], beam_width=33, lm=lm, lm_weight=0.0)
    assert calls == [("host", (1, 9, 8), None, 0), ("host", (1, 4, 8), None, 0), ("host", (1, 2, 8), None, 0)]
    # a masked LM is refused with the other searches' message; decode_ctc_weight == 1 stays CTC greedy (no LM is looked at)
    calls.clear()
    for eouts, elens in ((three, [9, 4, 2]), (one, [9])):
        with pytest.raises(NotImplementedError) as info:
            dec.decode(eouts, elens, beam_width=4, lm=SimpleNamespace(lm_type="bert"), lm_weight=0.3)
        assert str(info.value) == _NO_PREDICT
    dec.decode(three, [9, 4, 2], beam_width=4, lm=SimpleNamespace(lm_type="bert"), lm_weight=0.0)     # (not fused: nothing to refuse)
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], None, 0)]
    with pytest.raises(ValueError, match="1 <= elens"):
        dec.decode(three, [9, 0, 2], **kw)


def test_every_reason_of_las_rnnlm_why_not():
    from emoasr_amd.modeling.functions import las_rnnlm_why_not
    why = lambda lm, bw=4, d=None: las_rnnlm_why_not((d or _decoder())[0], bw, lm)
    assert why(_rnnlm()) is None and why(_rnnlm(), 32) is None and why(_rnnlm(), 1) is None
    assert why(_rnnlm(torch.bfloat16, E=64), d=_decoder(dtype=torch.bfloat16)) is None
    assert why(_rnnlm(f32_split=True), d=_decoder(split=True)) is None
    assert "lm_type 'transformer'" in why(_LMNext()) and "lm_type None" in why(SimpleNamespace())
    assert "vocabulary (48)" in why(_rnnlm(V=48)) and "vocabulary (32)" in why(_rnnlm(V=32))
    assert "computes in" in why(_rnnlm(torch.bfloat16)) and "computes in" in why(_rnnlm(), d=_decoder(dtype=torch.bfloat16))
    assert "split products" in why(_rnnlm(f32_split=True)) and "split products" in why(_rnnlm(), d=_decoder(split=True))
    assert "shape plan" in why(_rnnlm(E=50)) and "shape plan" in why(_rnnlm(H=36)) and "shape plan" in why(_rnnlm(L=0))
    assert "beam_width 33" in why(_rnnlm(), 33) and "beam_width 0" in why(_rnnlm(), 0)
    assert "beam_width 12" in why(_rnnlm(V=10), 12, _decoder(vocab=10))          # more beams than tokens


# ------------------------------------------------------------------------------------------------ the grid
def test_grid_routes_and_the_host_expansion(caplog):
    import logging
    from emoasr_amd.modeling import functions as F
    F._LAS_FUSION_LOGGED.clear()
    dec, calls = _decoder()
    three = torch.zeros(3, 9, 8)
    lm = _rnnlm()
    hyps, scores = F.las_fusion_grid_apply(dec, three, [9, 4, 2], 4, lm, [0.0, 0.3], [0.0, 1.0])
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], lm, [0.0, 0.3])] and len(hyps) == 3 and len(hyps[0]) == 4
    # without a positive weight the LM is not handed over
    calls.clear()
    F.las_fusion_grid_apply(dec, three, [9, 4, 2], 4, SimpleNamespace(lm_type="bert"), [0.0, -0.5], [0.0])
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], None, [0.0, -0.5])]
    with pytest.raises(NotImplementedError):
        F.las_fusion_grid_apply(dec, three, [9, 4, 2], 4, SimpleNamespace(lm_type="bert"), [0.0, 0.5], [0.0])
    # an LM the device form cannot take: one host search per utterance and DISTINCT weight at len_weight 0, expanded in double
    calls.clear()
    tlm = _LMNext()
    with caplog.at_level(logging.INFO):
        hyps, scores = F.las_fusion_grid_apply(dec, three, [9, 4, 2], 4, tlm, [0.0, 0.3, -1.0, 0.3], [0.0, 0.1])
    assert [(c[0], c[1][1], c[2], c[3]) for c in calls] == [("host", t, m, a) for t in (9, 4, 2) for m, a in ((None, 0.0), (tlm, 0.3))]
    assert any("lm_type 'transformer'" in r.getMessage() for r in caplog.records)
    assert len(hyps) == 3 and all(len(h) == 8 for h in hyps)
    for b, t in enumerate((9, 4, 2)):
        for c in range(8):
            assert hyps[b][c] == [[7, t], [7, t]]
            lw = (0.0, 0.1)[c % 2]
            assert scores[b][c] == [-1.0 + lw * 4.0, -2.0 + lw * 4.0]      # len(hyp) + 2 = 4, formed in double


def test_the_dedup_plan_of_the_engine_grid(monkeypatch):
    """engine.las_beam_search_batch(lm_weights=...): distinct positive weights searched once over shared frames, weights <= 0 folded
    into ONE search without the LM, the len_weights expanded on the host in double, a chunk cut by weight"""
    from emoasr_amd.engine import las as eng_las
    calls = []

    class Eng(eng_las.LASDecoder):
        dtype = torch.float32

        def __init__(self):
            self.arena = SimpleNamespace(p=lambda name: torch.zeros(40))

        def _las_beam_chunk(self, eouts, elens, W, len_weight, eos, max_len, lm=None, lm_weight=0, grid=None, sort=True):
            calls.append((tuple(eouts.shape), list(elens), len_weight, lm, None if grid is None else (list(grid[0]), list(grid[1])), sort))
            S = len(grid[0]) if grid else len(elens)
            mus = grid[1] if grid else [0.0] * S
            # two results per search, found worse-first: the expansion must sort them, stably
            return [[[5], [6, 6, 6]] for _ in range(S)], [[-3.0 - m, -2.95 - m] for m in mus]

    eng = Eng()
    lm = SimpleNamespace(L=2, H=64)
    three = torch.zeros(3, 9, 8)
    a3 = 0.1 + 0.2      # 0.30000000000000004: another double than 0.3, another search
    hyps, scores = eng.las_beam_search_batch(three, [9, 4, 2], 4, 0.7, 2, 5, lm=lm, lm_weights=[0.0, 0.3, -1.0, 0.5, 0.3, a3],
                                             len_weights=[0.0, 0.1])
    assert calls == [((3, 9, 8), [9, 4, 2], 0, None, None, False),
                     ((3, 9, 8), [9, 4, 2], 0, lm, ([0, 0, 0, 1, 1, 1, 2, 2, 2], [0.3, 0.5, a3] * 3), False)]
    assert len(hyps) == 3 and all(len(h) == 12 for h in hyps)
    for b in range(3):
        for c, a in enumerate([0.0, 0.3, 0.0, 0.5, 0.3, a3]):
            for j, lw in enumerate((0.0, 0.1)):
                raw = [(-3.0 - a) + lw * 3.0, (-2.95 - a) + lw * 5.0]      # score + lw * (len(hyp) + 2), in double
                want = sorted(zip(raw, [[5], [6, 6, 6]]), key=lambda r: r[0], reverse=True)
                assert scores[b][2 * c + j] == [r[0] for r in want] and hyps[b][2 * c + j] == [r[1] for r in want]
    # without an LM every weight is the one search without it
    calls.clear()
    hyps, _ = eng.las_beam_search_batch(three, [9, 4, 2], 4, 0.0, 2, 5, lm=None, lm_weights=[0.0, 0.3], len_weights=[0.0])
    assert [c[3:5] for c in calls] == [(None, None)] and len(hyps[0]) == 2
    # a capacity of two searches: whole utterances while they fit, an utterance with more searches than a chunk cut by weight
    calls.clear()
    monkeypatch.setattr(eng_las, "las_beam_chunk_capacity", lambda *a, **k: 2)
    eng.las_beam_search_batch(three, [9, 4, 2], 4, 0.0, 2, 5, lm=lm, lm_weights=[0.3, 0.5, 0.7], len_weights=[0.0])
    assert [(c[1], c[4]) for c in calls] == [([9], ([0, 0], [0.3, 0.5])), ([9], ([0], [0.7])), ([4], ([0, 0], [0.3, 0.5])),
                                             ([4], ([0], [0.7])), ([2], ([0, 0], [0.3, 0.5])), ([2], ([0], [0.7]))]


def test_chunk_capacity_counts_the_lm_pools():
    from emoasr_amd.engine.las import las_beam_chunk_capacity, las_beam_pool_bytes, las_lm_row_bytes
    lm = SimpleNamespace(L=2, H=512)
    assert las_lm_row_bytes(None, 2) == 0 and las_lm_row_bytes(lm, 2) == 2 * 512 * 6 and las_lm_row_bytes(lm, 4) == 2 * 512 * 8
    assert las_beam_pool_bytes(10, 64) == 2 * 10 * 64 * 4 and las_beam_pool_bytes(10, 64, 100) == 2 * 10 * (64 * 4 + 100)
    assert las_beam_chunk_capacity(4, 448) == las_beam_chunk_capacity(4, 448, lm_row_bytes=0) == 256
    budget = las_beam_pool_bytes(4 * 7, 448, 6144)
    assert las_beam_chunk_capacity(4, 448, budget=budget, lm_row_bytes=6144) == 7
    assert las_beam_chunk_capacity(4, 448, budget=budget - 1, lm_row_bytes=6144) == 6
    assert las_beam_chunk_capacity(4, 448, budget=budget) > 7        # (the same budget holds more searches without the LM)


# ------------------------------------------------------------------------------------------------ the command-line tool
def test_grid_dispatch_and_pinned_refusals():
    from emoasr_amd import fusion_grid as fg
    assert fg.grid_for("las") is fg.las_fusion_grid
    for kind in ("ctc", "transformer", "rnn_transducer"):
        assert fg.grid_for(kind) is fg.grid_of(kind)
    with pytest.raises(NotImplementedError, match="'ctc' and 'transformer'"):      # grid_of does not change
        fg.grid_of("las")
    with pytest.raises(NotImplementedError, match="'ctc' and 'transformer'"):
        fg.grid_for("rnnt")
    for kind in ("ctc", "transformer", "rnn_transducer"):
        with pytest.raises(NotImplementedError, match="decoder_type == 'las'"):
            fg.las_fusion_grid(SimpleNamespace(decoder_type=kind), [], None, 4, object(), [0.1], [0.0], "cpu")
    assert "las_fusion_grid" in fg.__doc__ and "rnnt_fusion_grid" in fg.__doc__


def test_the_grid_tool_sets_the_switch(caplog):
    import logging
    from emoasr_amd import fusion_grid as fg
    dec, _ = _decoder()
    assert fg.set_las_lm_fusion(dec, 10, _rnnlm()) is None and dec.las_lm_fusion == "fuse"
    dec.las_lm_fusion = "ignore"
    with caplog.at_level(logging.INFO):
        assert "vocabulary (48)" in fg.set_las_lm_fusion(dec, 10, _rnnlm(V=48)) and dec.las_lm_fusion == "fuse"
    assert any("vocabulary (48)" in r.getMessage() for r in caplog.records)


def test_main_sends_las_to_its_grid(monkeypatch, tmp_path):
    """main with everything heavy replaced: decoder_type 'las' reaches las_fusion_grid with the switch set, and grid_of is never asked"""
    from emoasr_amd import datasets, fusion_grid as fg, rescore
    from emoasr_amd.modeling import asr, lm as lm_mod
    dec, _ = _decoder()
    params = SimpleNamespace(decoder_type="las", test_path="test.tsv", beam_width=4, eos_id=2, vocab_path="vocab.txt")

    class _Model:
        decoder = dec

        def __init__(self, *a, **k):
            pass

        def load_state_dict(self, sd):
            pass

        def to(self, device):
            return self

        def eval(self):
            return self

    seen = {}

    def grid(model, loader, vocab, bw, lm, lm_weights, len_weights, device, eos_id=2, decode_ctc_weight=0):
        seen.update(switch=model.decoder.las_lm_fusion, bw=bw, cells=(len(lm_weights), len(len_weights)), lm=lm)
        return [(0.0, 0.0, 50.0, "wer")], (0.0, 0.0, 50.0, "wer")

    rn = _rnnlm()
    rn.load_state_dict, rn.to, rn.eval = (lambda sd: None), (lambda d: rn), (lambda: rn)
    monkeypatch.setattr(rescore, "load_config", lambda path: params)
    monkeypatch.setattr(rescore, "model_path", lambda conf, ep: "x.pt")
    monkeypatch.setattr(torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(asr, "ASR", _Model)
    monkeypatch.setattr(lm_mod, "LM", lambda *a, **k: rn)
    monkeypatch.setattr(datasets, "ASRDataset", lambda *a, **k: [])
    monkeypatch.setattr(datasets, "Vocab", lambda path: None)
    monkeypatch.setattr(fg, "las_fusion_grid", grid)
    monkeypatch.setattr(fg, "grid_of", lambda kind: (_ for _ in ()).throw(AssertionError("grid_of asked for " + repr(kind))))
    args = fg.build_parser().parse_args(["-conf", "asr.yaml", "-ep", "1", "--lm_conf", "lm.yaml", "--lm_ep", "1", "--save_dir", str(tmp_path)])
    results, best = fg.main(args)
    assert seen == dict(switch="fuse", bw=4, cells=(11, 6), lm=rn) and best[2] == 50.0
