"""Transformer-LM shallow fusion in the batched LAS beam search without a GPU: the fixture, the header / binding
tables of emoasr_lm_tree_advance_beam, its numpy restatement (tests/las_tree_ref.py) on a random lockstep walk, every reason of
las_tlm_why_not, the routing of LASDecoder.decode under both values of las_tlm_fusion, the command-line tool's dispatch and the
chunk capacity with the tree's bytes."""
import ctypes
import logging
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import las_beam_util as UB
from tests import las_tlm_fusion_util as U
from tests import las_tree_ref as R
from tests.test_las_fusion_cpu import _decoder, _rnnlm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def fx():
    return U.load_las_tlm_fusion_golden()


def test_fixture_is_complete(fx):
    groups, g = fx
    assert groups == U.GROUPS and len(U.CASES) == 12
    assert g["searches"].tolist() == U.SEARCHES and tuple(g["len_weights"].tolist()) == U.LEN_WEIGHTS == (0.0, 0.1)
    want = {f"{U.fusion_key(u, t, W, lw, a)}/{part}" for a, W in U.CASES for u, t in U.SEARCHES for lw in U.LEN_WEIGHTS
            for part in ("hyps", "lens", "scores", "margin")}
    assert set(g) - {"searches", "len_weights"} == want
    longest = 0
    for a, W in U.CASES:
        for u, t in U.SEARCHES:
            for lw in U.LEN_WEIGHTS:
                hyps, scores = U.fused_nbest(g, u, t, W, lw, a)
                assert 1 <= len(hyps) <= W and len(scores) == len(hyps) and all(len(h) >= 1 for h in hyps)
                assert scores == sorted(scores, reverse=True)
                assert all(0 <= v < 40 and v != 2 for h in hyps for v in h)     # (<eos> = 2 is stripped)
                longest = max([longest] + [len(h) for h in hyps])
    assert longest == U.LONGEST


def test_every_margin_exceeds_the_bar_and_is_the_recorded_one(fx):
    _, g = fx
    margins = {k: float(v) for k, v in g.items() if k.endswith("/margin")}
    assert len(margins) == len(U.CASES) * len(U.SEARCHES) * len(U.LEN_WEIGHTS)
    assert min(margins.values()) > U.MARGIN, min(margins.items(), key=lambda kv: kv[1])
    for (a, W), want in U.MARGINS.items():
        worst = min(float(g[U.fusion_key(u, t, W, lw, a) + "/margin"]) for u, t in U.SEARCHES for lw in U.LEN_WEIGHTS)
        assert abs(worst - want) <= 0.05 * want, (a, W, worst, want)          # (two recorded digits)


def test_every_group_differs_from_the_unfused_search(fx):
    """the LM decides something in every (W, lm_weight) group: a search that ignores it cannot return the fixture"""
    _, g = fx
    _, unfused = UB.load_las_beam_golden()
    for a, W in U.CASES:
        changed = sum(U.fused_nbest(g, u, t, W, 0.0, a)[0] != UB.golden_nbest(unfused, u, t, W, 0.0)[0] for u, t in U.SEARCHES)
        assert changed >= 1, (a, W)


# ------------------------------------------------------------------------------------------------ header and bindings
def test_the_new_entry_point_is_declared_bound_and_exported():
    from emoasr_amd import lib
    header = open(os.path.join(ROOT, "include", "emoasr_hip.h")).read()
    name = "emoasr_lm_tree_advance_beam"
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert decl, name
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["const emoasr_lm_tree_t* t", "const int* ids", "const int* parent", "const emoasr_beam_state_t* state",
                    "int src_base", "int dst_base", "long long* lab", "long long* dst", "void* stream"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert lib.SIGNATURES[name] == [ctypes.POINTER(lib.LmTree), P, P, P, I, I, P, P, P]
    assert hasattr(lib.load(), name)
    assert header.index("} emoasr_beam_state_t;") < decl.start()          # declared after the state record it names
    from emoasr_amd import lm_tree
    assert callable(lm_tree.TreeState.advance_beam)
    src = open(os.path.join(ROOT, "emoasr_amd", "csrc", "lm_tree.hip")).read()
    kernel = src.split("void lm_tree_advance_beam_kernel(")[1].split("\n}\n")[0]
    assert "__ballot" in kernel and "atomic" not in kernel, "the beam advance takes its nodes by ballot: no atomics"


# ------------------------------------------------------------------------------------------------ the restatement
def _walk_and_check(S, W, Lcap, cap, steps, seed, **kw):
    walk, tree = R.BookWalk(seed, S, W, 50, **kw), R.BeamTree(S, W, Lcap, cap)
    nb, node_label = S * W, {}
    for i in range(steps):
        ids, parent, state = walk.next_step()
        src_base, dst_base = R.halves(i, nb)
        before = (tree.llen.copy(), tree.lanc.copy())
        row_node, row_pos, lab, dst = tree.advance_beam(ids, parent, state, src_base, dst_base)
        for r in range(nb):
            s, w = divmod(r, W)
            live = not state[s][3] and w < min(max(int(state[s][1]), 0), W)
            if row_node[r] >= 0:
                assert live and lab[r] == ids[r] and dst[r] == dst_base + r and s * cap <= row_node[r] < (s + 1) * cap
                assert int(row_node[r]) not in node_label
                node_label[int(row_node[r])] = int(ids[r])
            else:
                assert lab[r] == 0 and dst[r] == -1 and row_pos[r] == 0
                assert tree.llen[dst_base + r] == before[0][dst_base + r] and np.array_equal(tree.lanc[dst_base + r], before[1][dst_base + r])
        assert np.array_equal(tree.llen[src_base:src_base + nb], before[0][src_base:src_base + nb])      # the source half is only read
        walk.commit(row_node)
        for half in (0, 1):
            for r, seq in walk.seq[half].items():
                assert R.labels(tree, half * nb + r, node_label) == seq, (i, half, r)
    return walk, tree


def test_restatement_reproduces_the_label_sequences_of_a_random_walk():
    """20 steps over 4 searches of width 5 with random parents inside the search and n_alive shrinking from step 12: every slot
    of either half reads back, through its node list, the labels the walk appended along its parents"""
    walk, tree = _walk_and_check(4, 5, 32, 5 * 20 + 1, 20, seed=7, shrink_from=12)
    assert not tree.status.any() and max(len(q) for h in walk.seq for q in h.values()) >= 8


def test_restatement_limits_and_liveness():
    """a finished search and rows past n_alive take no node; a parent outside the search reads row 0; counts outside 0 .. W are
    clamped; p = Lcap raises OVERLEN, a used-up share POOL_FULL, each for its own search alone"""
    full = lambda i, s: 3
    walk, tree = _walk_and_check(3, 3, 4, 100, 7, seed=1, done=(1,), alive=full, bad={2: [(0, 5), (7, -1)], 3: [(1, 1 << 30)]})
    assert tree.status.tolist() == [R.OVERLEN, 0, R.OVERLEN] and tree.nnodes[1] == 0 and int(tree.llen.max()) == 4
    walk, tree = _walk_and_check(2, 3, 16, 5, 4, seed=2, alive=lambda i, s: (9, -2)[s] if i == 1 else 3)
    assert tree.status.tolist() == [R.POOL_FULL, 0] and tree.nnodes.tolist() == [5, 4]       # 1 + 3 + 1 of 3, and 1 + 0 + 3


# ------------------------------------------------------------------------------------------------ las_tlm_why_not and the switch
def _tlm(dtype=torch.float32, causal=True, **over):
    p = dict(vocab_size=40, hidden_size=128, num_attention_heads=2, num_layers=2, intermediate_size=256, max_seq_len=64)
    p.update(over)
    return SimpleNamespace(lm_type="transformer", stateful=False, causal=causal, compute_dtype=dtype, f32_split=False,
                           params=SimpleNamespace(**p))


def test_every_reason_of_las_tlm_why_not():
    from emoasr_amd.modeling.functions import las_tlm_why_not
    why = lambda lm, bw=4, d=None: las_tlm_why_not((d or _decoder())[0], bw, lm)
    assert why(_tlm()) is None and why(_tlm(), 32) is None and why(_tlm(), 1) is None
    assert why(_tlm(torch.bfloat16)) is None                                   # the LM's own dtype: the model stays f32
    assert why(_tlm(), d=_decoder(dtype=torch.bfloat16)) is None
    assert "lm_type 'rnn' is not 'transformer'" in why(_rnnlm()) and "lm_type None" in why(SimpleNamespace())
    assert "no causal LM" in why(_tlm(causal=False))
    assert "computes in torch.float16" in why(_tlm(torch.float16))
    assert "vocabulary (48) is not the model's (40)" in why(_tlm(vocab_size=48))     # not >=: the score kernel soft-maxes V columns
    assert "vocabulary (32) is not the model's (40)" in why(_tlm(vocab_size=32))
    assert "heads (128 over 32)" in why(_tlm(num_attention_heads=32)) and "heads (128 over 3)" in why(_tlm(num_attention_heads=3))
    # the LDS bound is taken on the search's own longest prefix, min(max_decode_ylen, max_seq_len): a long LM under a short search fits
    assert why(_tlm(max_seq_len=100000)) is None
    long_dec = _decoder()
    long_dec[0].max_decode_ylen = 9000
    assert "prefixes of 9000 tokens need 73536 bytes of LDS" in why(_tlm(max_seq_len=100000), d=long_dec)
    assert why(_tlm(max_seq_len=8000), d=long_dec) is None                      # 8 * 8000 + 1536 = 65536
    assert "beam_width 33" in why(_tlm(), 33) and "beam_width 0" in why(_tlm(), 0)
    assert "beam_width 12" in why(_tlm(vocab_size=10), 12, _decoder(vocab=10))


def test_default_is_host_and_a_bad_value_raises():
    from emoasr_amd.modeling import functions as F
    dec, calls = _decoder()
    assert dec.las_tlm_fusion == "host" and F.las_tlm_fusion_of(dec) == "host"
    assert F.las_tlm_fusion_of(SimpleNamespace()) == "host"
    dec.las_lm_fusion, dec.las_tlm_fusion = "fuse", "gpu"
    with pytest.raises(ValueError, match="las_tlm_fusion is 'host' or 'device', not 'gpu'"):
        dec.decode(torch.zeros(3, 9, 8), [9, 4, 2], beam_width=4, lm=_tlm(), lm_weight=0.3)
    with pytest.raises(ValueError, match="las_tlm_fusion"):
        F.las_fusion_grid_apply(dec, torch.zeros(3, 9, 8), [9, 4, 2], 4, _tlm(), [0.3], [0.0])
    assert calls == []


def test_routing_of_decode_under_both_values(caplog):
    from emoasr_amd.modeling import functions as F
    from emoasr_amd.modeling.lm import _NO_PREDICT
    F._LAS_FUSION_LOGGED.clear()
    dec, calls = _decoder()
    one, three = torch.zeros(1, 9, 8), torch.zeros(3, 9, 8)
    lm, rn = _tlm(), _rnnlm()
    kw = dict(beam_width=4, lm=lm, lm_weight=0.3)
    per_utt = [("host", (1, 9, 8), lm, 0.3), ("host", (1, 4, 8), lm, 0.3), ("host", (1, 2, 8), lm, 0.3)]
    # "host" (the default): exactly today's calls -- one host search per utterance, the reason logged once
    dec.las_lm_fusion = "fuse"
    with caplog.at_level(logging.INFO):
        dec.decode(three, [9, 4, 2], **kw)
        dec.decode(three, [9, 4, 2], **kw)
    assert calls == per_utt * 2
    assert sum("lm_type 'transformer' is not 'rnn'" in r.getMessage() for r in caplog.records) == 1
    calls.clear()
    dec.decode(one, [9], **kw)
    dec.las_beam_impl = "batch"
    dec.decode(one, [9], **kw)
    dec.las_beam_impl = "single"
    assert calls == [("host", (1, 9, 8), lm, 0.3)] * 2
    # "device": several utterances, and one under "batch", are ONE batched search with the LM; one under "single" stays the host form
    calls.clear()
    caplog.clear()
    dec.las_tlm_fusion = "device"
    with caplog.at_level(logging.INFO):
        h, s, _, _ = dec.decode(three, [9, 4, 2], **kw)
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], lm, 0.3)] and not caplog.records
    assert h == [[[7, 9], [7, 9]], [[7, 4], [7, 4]], [[7, 2], [7, 2]]] and s == [[-1.0, -2.0]] * 3
    calls.clear()
    dec.decode(one, [9], **kw)
    dec.las_beam_impl = "batch"
    h, s, _, _ = dec.decode(one, [9], **kw)
    dec.las_beam_impl = "single"
    assert calls == [("host", (1, 9, 8), lm, 0.3), ("batch", (1, 9, 8), [9], lm, 0.3)] and h == [[7, 9], [7, 9]] and s == [-1.0, -2.0]
    # the switch is not read for another LM: the RNN LM keeps its own device form
    calls.clear()
    dec.decode(three, [9, 4, 2], beam_width=4, lm=rn, lm_weight=0.3)
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], rn, 0.3)]
    # lm_weight <= 0, no LM, or "ignore" never reach the tree: the unfused search
    calls.clear()
    dec.decode(three, [9, 4, 2], beam_width=4, lm=lm, lm_weight=0.0)
    dec.decode(three, [9, 4, 2], beam_width=4, lm=None, lm_weight=0.3)
    dec.las_lm_fusion = "ignore"
    dec.decode(three, [9, 4, 2], beam_width=33 - 29, lm=_tlm(vocab_size=48), lm_weight=0.3)     # (not even looked at)
    dec.las_lm_fusion = "fuse"
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], None, 0)] * 3
    # an LM the tree cannot take is a ValueError with the reason, before any search; a masked LM is refused as before
    calls.clear()
    for bad, bw, what in ((_tlm(vocab_size=48), 4, r"vocabulary \(48\)"), (_tlm(causal=False), 4, "no causal LM"), (lm, 33, "beam_width 33")):
        for eouts, elens in ((three, [9, 4, 2]), (one, [9])):
            with pytest.raises(ValueError, match="las_tlm_fusion = 'device' cannot fuse this LM: .*" + what):
                dec.decode(eouts, elens, beam_width=bw, lm=bad, lm_weight=0.3)
    with pytest.raises(NotImplementedError) as info:
        dec.decode(three, [9, 4, 2], beam_width=4, lm=SimpleNamespace(lm_type="bert"), lm_weight=0.3)
    assert str(info.value) == _NO_PREDICT and calls == []


def test_grid_routes_under_both_values(caplog):
    from emoasr_amd.modeling import functions as F
    F._LAS_FUSION_LOGGED.clear()
    dec, calls = _decoder()
    three, lm = torch.zeros(3, 9, 8), _tlm()
    with caplog.at_level(logging.INFO):
        F.las_fusion_grid_apply(dec, three, [9, 4, 2], 4, lm, [0.0, 0.3], [0.0, 0.1])
    assert [(c[0], c[1][1], c[2], c[3]) for c in calls] == [("host", t, m, a) for t in (9, 4, 2) for m, a in ((None, 0.0), (lm, 0.3))]
    assert any("lm_type 'transformer'" in r.getMessage() for r in caplog.records)
    calls.clear()
    dec.las_tlm_fusion = "device"
    hyps, _ = F.las_fusion_grid_apply(dec, three, [9, 4, 2], 4, lm, [0.0, 0.3], [0.0, 0.1])
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], lm, [0.0, 0.3])] and len(hyps) == 3 and len(hyps[0]) == 4
    calls.clear()
    F.las_fusion_grid_apply(dec, three, [9, 4, 2], 4, _tlm(vocab_size=48), [0.0, -0.5], [0.0])      # no positive weight: no LM, no refusal
    assert calls == [("batch", (3, 9, 8), [9, 4, 2], None, [0.0, -0.5])]
    calls.clear()
    with pytest.raises(ValueError, match=r"cannot fuse this LM: the LM's vocabulary \(48\)"):
        F.las_fusion_grid_apply(dec, three, [9, 4, 2], 4, _tlm(vocab_size=48), [0.0, 0.5], [0.0])
    with pytest.raises(ValueError, match="beam_width 33"):
        F.las_fusion_grid_apply(dec, three, [9, 4, 2], 33, lm, [0.5], [0.0])
    assert calls == []


# ------------------------------------------------------------------------------------------------ the engine's plan
def test_the_engine_hands_the_chunks_their_first_utterance(monkeypatch):
    """engine.las_beam_search_batch with a Transformer LM: the chunks carry `first` (the RuntimeError of a full tree names the
    utterance), the capacity counts the tree; the RNN LM's calls are what they were"""
    from emoasr_amd.engine import las as eng_las
    calls, caps = [], []

    class Eng(eng_las.LASDecoder):
        dtype = torch.float32

        def __init__(self):
            self.arena = SimpleNamespace(p=lambda name: torch.zeros(40))

        def _las_beam_chunk(self, eouts, elens, W, len_weight, eos, max_len, lm=None, lm_weight=0, grid=None, sort=True, **more):
            calls.append((list(elens), lm_weight, None if grid is None else (list(grid[0]), list(grid[1])), more))
            S = len(grid[0]) if grid else len(elens)
            return [[[5]] for _ in range(S)], [[-3.0] for _ in range(S)]

    orig = eng_las.las_beam_chunk_capacity
    monkeypatch.setattr(eng_las, "las_beam_chunk_capacity", lambda *a, **k: (caps.append(k), 2)[1])
    eng, lm, three = Eng(), _tlm(), torch.zeros(3, 9, 8)
    eng.las_beam_search_batch(three, [9, 4, 2], 4, 0.1, 2, 5, lm=lm, lm_weight=0.3)
    tree = eng_las.las_tlm_search_bytes(lm, 4, 5, 40)
    assert calls == [([9, 4], 0.3, None, dict(first=0)), ([2], 0.3, None, dict(first=2))] and caps == [dict(tree_bytes=tree)]
    calls.clear(), caps.clear()
    eng.las_beam_search_batch(three, [9, 4, 2], 4, 0.0, 2, 5, lm=lm, lm_weights=[0.3, 0.5, 0.7], len_weights=[0.0])
    assert [(c[0], c[2], c[3]) for c in calls] == [([9], ([0, 0], [0.3, 0.5]), dict(first=0)), ([9], ([0], [0.7]), dict(first=0)),
                                                   ([4], ([0, 0], [0.3, 0.5]), dict(first=1)), ([4], ([0], [0.7]), dict(first=1)),
                                                   ([2], ([0, 0], [0.3, 0.5]), dict(first=2)), ([2], ([0], [0.7]), dict(first=2))]
    assert caps == [dict(tree_bytes=tree)]
    calls.clear(), caps.clear()
    rn = SimpleNamespace(L=2, H=64)
    eng.las_beam_search_batch(three, [9, 4, 2], 4, 0.1, 2, 5, lm=rn, lm_weight=0.3)
    assert calls == [([9, 4], 0.3, None, {}), ([2], 0.3, None, {})] and caps == [dict(lm_row_bytes=2 * 64 * 8)]
    assert orig(4, 448) == 256


def test_chunk_capacity_counts_the_tree():
    from emoasr_amd import lm_tree
    from emoasr_amd.engine.las import las_beam_chunk_capacity, las_beam_pool_bytes, las_tlm_dims, las_tlm_search_bytes
    assert lm_tree.las_list_cap(20, 64) == 20 and lm_tree.las_list_cap(100, 64) == 64 and lm_tree.las_list_cap(0, 64) == 1
    assert lm_tree.las_node_cap(4, 20) == 81 and lm_tree.las_node_cap(1, 0) == 1
    lm = _tlm()
    assert las_tlm_dims(lm, 4, 20) == (20, 81) and las_tlm_dims(lm, 4, 100) == (64, 401)
    # both pools of every layer, the lists and lengths of 2 W slots, the logits in the LM's dtype and the f32 rows
    want = 2 * 2 * 81 * 128 * 4 + 2 * 4 * 21 * 4 + 4 * 40 * 8
    assert las_tlm_search_bytes(lm, 4, 20, 40) == want == lm_tree.las_search_bytes(4, 20, 81, 2, 128, 40, 4)
    assert las_tlm_search_bytes(_tlm(torch.bfloat16), 4, 20, 40) == 2 * 2 * 81 * 128 * 2 + 2 * 4 * 21 * 4 + 4 * 40 * 6
    assert las_tlm_search_bytes(None, 4, 20, 40) == 0
    assert las_beam_chunk_capacity(4, 448, tree_bytes=0) == las_beam_chunk_capacity(4, 448) == 256
    budget = 7 * (las_beam_pool_bytes(4, 448) + want)
    assert las_beam_chunk_capacity(4, 448, budget=budget, tree_bytes=want) == 7
    assert las_beam_chunk_capacity(4, 448, budget=budget - 1, tree_bytes=want) == 6
    assert las_beam_chunk_capacity(4, 448, budget=budget) > 7


# ------------------------------------------------------------------------------------------------ the command-line tool
def test_the_grid_tool_sets_both_switches(caplog):
    from emoasr_amd import fusion_grid as fg
    dec, _ = _decoder()
    assert fg.set_las_lm_fusion(dec, 10, _tlm()) is None and dec.las_lm_fusion == "fuse" and dec.las_tlm_fusion == "device"
    with caplog.at_level(logging.INFO):
        why = fg.set_las_lm_fusion(dec, 10, _tlm(vocab_size=48))
    assert "lm_type 'transformer'" in why and dec.las_lm_fusion == "fuse" and dec.las_tlm_fusion == "host"
    assert any("las_tlm_fusion stays 'host'" in r.getMessage() and "vocabulary (48)" in r.getMessage() for r in caplog.records)
    dec.las_tlm_fusion = "host"
    assert fg.set_las_lm_fusion(dec, 10, _rnnlm()) is None and dec.las_tlm_fusion == "host"     # (not touched for another LM)
    assert "las_tlm_fusion" in fg.__doc__


def test_main_sets_the_switch_for_a_transformer_lm(monkeypatch, tmp_path):
    """main with everything heavy replaced: a LAS model with a Transformer LM reaches las_fusion_grid with both switches set"""
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
        seen.update(switch=model.decoder.las_lm_fusion, tlm=model.decoder.las_tlm_fusion, bw=bw, lm=lm)
        return [(0.0, 0.0, 50.0, "wer")], (0.0, 0.0, 50.0, "wer")

    tl = _tlm()
    tl.load_state_dict, tl.to, tl.eval = (lambda sd: None), (lambda d: tl), (lambda: tl)
    monkeypatch.setattr(rescore, "load_config", lambda path: params)
    monkeypatch.setattr(rescore, "model_path", lambda conf, ep: "x.pt")
    monkeypatch.setattr(torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(asr, "ASR", _Model)
    monkeypatch.setattr(lm_mod, "LM", lambda *a, **k: tl)
    monkeypatch.setattr(datasets, "ASRDataset", lambda *a, **k: [])
    monkeypatch.setattr(datasets, "Vocab", lambda path: None)
    monkeypatch.setattr(fg, "las_fusion_grid", grid)
    args = fg.build_parser().parse_args(["-conf", "asr.yaml", "-ep", "1", "--lm_conf", "lm.yaml", "--lm_ep", "1", "--save_dir", str(tmp_path)])
    fg.main(args)
    assert seen == dict(switch="fuse", tlm="device", bw=4, lm=tl)
