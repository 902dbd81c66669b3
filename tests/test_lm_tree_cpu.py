"""CPU checks of the Transformer-LM fusion over a prefix tree (no GPU): the restatement of advance against the
label sequences a random walk keeps on the host, every reason of rnnt_beam_tlm_why_not, the routing of decoder.rnnt_tlm_fusion through
the decoder, the apply functions and the grid tool with fake engines, the chunk capacity, and the gap condition of the end-to-end
cases (tests/test_rnnt_tlm_fusion_gpu.py) on the oracle's encoder outputs."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import lm_tree_ref as T
from tests import rnnt_fusion_ref as F
from tests.util import LM_CFG, load_ctc_beam_golden, load_golden


# ---- the restatement against itself -----------------------------------------------------------------------------------------------
def test_advance_ref_keeps_the_label_sequences_of_a_random_walk():
    """40 rounds, 10 searches of 4 rows with slot reuse: every live slot's list reads back the labels the walk appended, nodes are
    handed out compactly per search in row order, a node is never given twice, the lengths outgrow Lcap = 16 (the refused rows
    change nothing)"""
    S, W, per, Lcap, cap = 10, 4, 16, 16, 170
    tree = T.Tree(S, W, S * per, Lcap, cap)
    walk = T.Walk(5, S, W, per, 40, off=(0, 3, 4, 15, 16, 21, 30, 33, 36), rows=37, keep=3,
                  bad={2: [(1, "src", -1), (2, "dst", S * per)], 3: [(5, "dst", 1 << 40)]})
    node_label, seen = {}, set()
    for _ in range(40):
        lab, src, dst, act = walk.next_round()
        before = (tree.llen.copy(), tree.lanc.copy(), tree.nnodes.copy())
        node, pos = tree.advance(src, dst, act)
        for s in range(S):
            got = [int(n) for n in node[s * W:(s + 1) * W] if n >= 0]
            assert got == list(range(s * cap + before[2][s], s * cap + before[2][s] + len(got)))          # compact, in row order
            assert tree.nnodes[s] == before[2][s] + len(got)
        for r in range(S * W):
            if node[r] >= 0:
                assert act[r] and node[r] not in seen and pos[r] == before[0][src[r]] and tree.llen[dst[r]] == pos[r] + 1
                seen.add(int(node[r]))
                node_label[int(node[r])] = int(lab[r])
            elif act[r] and 0 <= src[r] < S * per and 0 <= dst[r] < S * per:      # refused: over length (the pool is large enough)
                assert before[0][src[r]] >= Lcap and tree.status[r // W] & T.OVERLEN
                assert tree.llen[dst[r]] == before[0][dst[r]] and np.array_equal(tree.lanc[dst[r]], before[1][dst[r]])
        walk.commit(node)
        for s in range(S):
            for slot in walk.live[s]:
                assert T.labels_of(tree, slot, node_label) == walk.seq[slot], (s, slot)
    assert walk.round == 40 and int(tree.llen.max()) == Lcap and bool((tree.status & T.OVERLEN).any())
    assert not bool((tree.status & T.POOL_FULL).any()) and int(tree.nnodes.max()) < cap and len(seen) == int(tree.nnodes.sum())


def test_advance_ref_refuses_at_the_list_and_the_pool_capacity():
    tree = T.Tree(2, 4, 16, 3, 5)
    one = lambda v: np.asarray(v, np.int64)
    act = one([1, 1, 0, 1, 1, 1, 1, 1])
    # round 1: search 0 takes nodes 0, 1, 2 (row 2 is inactive: no node), search 1 takes 5 .. 8
    node, pos = tree.advance(one([0, 0, 0, 0, 8, 8, 8, 8]), one([1, 2, 3, 4, 9, 10, 11, 12]), act)
    assert node.tolist() == [0, 1, -1, 2, 5, 6, 7, 8] and pos.tolist() == [0] * 8 and tree.nnodes.tolist() == [3, 4]
    # round 2: search 0 has two nodes left for three rows; search 1 one for four
    node, pos = tree.advance(one([1, 2, 0, 4, 9, 9, 10, 11]), one([5, 6, 7, 3, 13, 14, 15, 8]), act)
    assert node.tolist() == [3, 4, -1, -1, 9, -1, -1, -1] and tree.status.tolist() == [T.POOL_FULL, T.POOL_FULL]
    assert tree.nnodes.tolist() == [5, 5] and tree.llen[[5, 6, 3, 13, 14]].tolist() == [2, 2, 0, 2, 0]
    assert tree.lanc[5, :2].tolist() == [0, 3] and tree.lanc[13, :2].tolist() == [5, 9]
    # a prefix at Lcap = 3: the bit, and nothing else
    tree = T.Tree(1, 2, 8, 3, 50)
    a2 = one([1, 1])
    for k in range(3):
        node, _ = tree.advance(one([k, k]), one([k + 1, 7]), a2)
        assert (node >= 0).all() and tree.status[0] == 0
    keep = (tree.llen.copy(), tree.lanc.copy(), tree.nnodes.copy())
    node, _ = tree.advance(one([3, 0]), one([4, 5]), a2)
    assert node.tolist() == [-1, 6] and tree.status[0] == T.OVERLEN and tree.llen[4] == keep[0][4] and tree.nnodes[0] == keep[2][0] + 1
    assert np.array_equal(tree.lanc[4], keep[1][4])


def test_gathered_attention_ref_is_the_dense_reference_over_gathered_rows():
    from tests.decode_step_ref import attn_step_ref
    rs = np.random.RandomState(3)
    d, H, nodes = 32, 2, 20
    tree = T.Tree(1, 2, 4, 8, nodes)
    kp, vp = rs.randn(nodes, d), rs.randn(nodes, d)
    one = lambda v: np.asarray(v, np.int64)
    tree.advance(one([0, 0]), one([1, 2]), one([1, 1]))
    node, _ = tree.advance(one([1, 1]), one([3, 0]), one([1, 0]))          # slot 3: nodes [0, 2]
    qkv = rs.randn(2, 3 * d)
    out, k2, v2 = T.gathered_attn_ref(qkv, kp, vp, tree.lanc, tree.llen, node, one([3, 0]), H)
    assert node.tolist() == [2, -1] and np.isnan(out[1]).all() and np.array_equal(k2[2], qkv[0, d:2 * d]) and np.array_equal(v2[3:], vp[3:])
    dense_k, dense_v = np.stack([kp[0], kp[7]])[None], np.stack([vp[0], vp[7]])[None]
    want = attn_step_ref(qkv[:1], dense_k, dense_v, 1, H)[0]
    assert np.array_equal(out[0], want[0])


# ---- rnnt_beam_tlm_why_not ----------------------------------------------------------------------------------------------------------
def _engine(dtype=torch.float32, split=False, V=40):
    from emoasr_amd.engine.rnnt import RNNTDecoder as Eng
    eng = SimpleNamespace(dtype=dtype, split=split, arena=SimpleNamespace(w=lambda name: torch.zeros(V, 4)), r_nl=2, r_H=64,
                          _BEAM_BATCH_CAP=64, _TLM_POOL_BUDGET=8 << 30)
    eng._tlm_frames = Eng._tlm_frames
    return Eng, eng


def _tlm(**over):
    p = dict(LM_CFG)
    p.update({k: over.pop(k) for k in list(over) if k in p and k != "lm_type"})
    lm = dict(lm_type="transformer", causal=True, compute_dtype=torch.float32, f32_split=False, params=SimpleNamespace(**p))
    lm.update(over)
    return SimpleNamespace(**lm)


def test_every_reason_of_tlm_why_not():
    Eng, eng = _engine()
    why = lambda lm, e=eng: Eng.rnnt_beam_tlm_why_not(e, lm)
    assert why(_tlm()) is None and why(_tlm(vocab_size=43)) is None
    assert "is not 'transformer'" in why(_tlm(lm_type="rnn")) and "is not 'transformer'" in why(SimpleNamespace())
    assert "no causal LM" in why(_tlm(causal=False))
    assert "computes in" in why(_tlm(compute_dtype=torch.bfloat16)) and "computes in" in why(_tlm(f32_split=True))
    assert "computes in" in why(_tlm(compute_dtype=torch.float16), _engine(torch.float16)[1])
    assert why(_tlm(compute_dtype=torch.bfloat16), _engine(torch.bfloat16)[1]) is None
    assert "vocabulary (39) is smaller than the model's (40)" in why(_tlm(vocab_size=39))
    for d, H in ((128, 32), (128, 3), (520, 2), (256, 1)):          # 4 wide, no divisor, 260 wide, 256 wide
        assert "heads" in why(_tlm(hidden_size=d, num_attention_heads=H)), (d, H)
    for d, H in ((64, 8), (256, 2), (128, 4)):
        assert why(_tlm(hidden_size=d, num_attention_heads=H)) is None
    assert why(_tlm(max_seq_len=8000)) is None and "bytes of LDS" in why(_tlm(max_seq_len=8001))
    # the RNN form's answer for a Transformer LM stays what it was
    assert "is not 'rnn'" in Eng.rnnt_beam_lm_why_not(eng, _tlm())


def test_plan_and_chunk_capacity():
    from emoasr_amd import lm_tree
    Eng, eng = _engine(torch.bfloat16)
    assert lm_tree.list_cap(3, 12, 64) == 25 and lm_tree.list_cap(3, 300, 512) == 512 and lm_tree.list_cap(1, 300, 512) == 1
    assert lm_tree.node_cap(4, 3, 12) == 97 and lm_tree.node_cap(16, 1, 300) == 1
    assert lm_tree.attn_lds_bytes(8000) == 65536 and Eng._tlm_frames(0) == 64 and Eng._tlm_frames(65) == 128
    lm = _tlm(hidden_size=512, num_layers=6, max_seq_len=1024, compute_dtype=torch.bfloat16)
    cap = Eng.rnnt_beam_tlm_chunk_capacity(eng, 16, 3, lm, 300)          # 320 frames: 10241 nodes x 6 x 512 x 2 x 2 bytes = 126 MB
    assert cap == 64
    eng._TLM_POOL_BUDGET = 1 << 30
    per = 2 * 6 * 10241 * 512 * 2 + 64 * 642 * 4 + 64 * 6 * 2 * 64
    assert Eng.rnnt_beam_tlm_chunk_capacity(eng, 16, 3, lm, 300) == (1 << 30) // per == 8
    eng._TLM_POOL_BUDGET = 1
    assert Eng.rnnt_beam_tlm_chunk_capacity(eng, 16, 3, lm, 300) == 1


def test_entry_points_are_declared():
    from emoasr_amd import lib
    h = lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "emoasr_hip.h")).read()
    for name, n in (("emoasr_lm_tree_advance", 5), ("emoasr_lm_tree_attn", 10), ("emoasr_lm_tree_step", 6)):
        assert hasattr(h, name) and len(lib.SIGNATURES[name]) == n and name + "(" in header, name
    assert hasattr(h, "emoasr_lm_tree_step_ws_bytes") and "emoasr_lm_tree_step_ws_bytes(" in header
    assert (lib.LM_TREE_OVERLEN, lib.LM_TREE_POOL_FULL) == (T.OVERLEN, T.POOL_FULL)
    assert "#define EMOASR_LM_TREE_OVERLEN 1" in header and "#define EMOASR_LM_TREE_POOL_FULL 2" in header


# ---- routing ----------------------------------------------------------------------------------------------------------------------
def _decoder():
    from emoasr_amd.modeling.decoders.rnn_transducer import RNNTDecoder
    return RNNTDecoder(SimpleNamespace(blank_id=0, eos_id=2, vocab_size=8, enc_hidden_size=4, kd_weight=0, dec_num_layers=1,
                                       dec_hidden_size=8, embedding_size=8, joint_hidden_size=8, mtl_ctc_weight=0))


def test_decoder_routing_under_both_switch_values(monkeypatch):
    from emoasr_amd.modeling.decoders import rnn_transducer as mod
    calls = []
    monkeypatch.setattr(mod, "rnnt_beam_apply", lambda dec, eouts, bw, *a: calls.append(("host", bw) + a) or [[2, 3]])

    def batch(dec, eouts, elens, bw, lm=None, lm_weights=None, len_weights=None, require_device=False, **kw):
        calls.append(("batch", bw, lm, lm_weights, len_weights, require_device, kw))
        B = eouts.shape[0]
        if lm_weights is None:
            return [[[2, 3]]] * B, [[-1.0]] * B
        return [[[[2, 4]]]] * B, [[[-2.0]]] * B
    monkeypatch.setattr(mod, "rnnt_beam_batch_apply", batch)
    dec = _decoder()
    rnn, trf = SimpleNamespace(lm_type="rnn"), SimpleNamespace(lm_type="transformer")
    one, two = torch.zeros(1, 3, 4), torch.zeros(2, 3, 4)
    assert dec.rnnt_tlm_fusion == "host" and "rnnt_tlm_fusion" not in dec.state_dict()

    def today():
        del calls[:]
        assert dec.decode(one, [3], beam_width=4, lm=trf, lm_weight=0.3, len_weight=1.0) == ([[2, 3]], None, None, None)
        assert dec.decode(two, [3, 3], beam_width=4, lm=trf, lm_weight=0.3, len_weight=1.0)[0] == [[[2, 4]]] * 2
        assert dec.decode(two, [3, 3], beam_width=4, lm=rnn, lm_weight=0.3, len_weight=1.0)[0] == [[[2, 4]]] * 2
        assert dec.decode(two, [3, 3], beam_width=4, lm=trf, lm_weight=0.0)[0] == [[[2, 3]]] * 2
        return list(calls)
    # "host": exactly today's calls -- no new keyword reaches the apply function
    assert today() == [("host", 4, trf, 0.3, 1.0), ("batch", 4, trf, [0.3], [1.0], False, {}), ("batch", 4, rnn, [0.3], [1.0], False, {}),
                       ("batch", 4, None, None, None, False, {})]
    dec.rnnt_beam_impl = "device"
    with pytest.raises(ValueError, match="lm_type 'transformer'"):
        dec.decode(one, [3], beam_width=4, lm=trf, lm_weight=0.3)
    dec.rnnt_beam_impl = "host"
    # "device": the Transformer LM goes to the batched search with the keyword; everything else is unchanged
    dec.rnnt_tlm_fusion = "device"
    dev_kw = {"tlm_fusion": "device"}
    assert today() == [("host", 4, trf, 0.3, 1.0), ("batch", 4, trf, [0.3], [1.0], False, dev_kw), ("batch", 4, rnn, [0.3], [1.0], False, {}),
                       ("batch", 4, None, None, None, False, {})]
    dec.rnnt_beam_impl = "device"
    del calls[:]
    assert dec.decode(one, [3], beam_width=4, lm=trf, lm_weight=0.3) == ([[2, 4]], [-2.0], None, None)
    assert dec.decode(one, [3], beam_width=4, lm=rnn, lm_weight=0.3) == ([[2, 4]], [-2.0], None, None)
    assert calls == [("batch", 4, trf, [0.3], [0.0], True, dev_kw), ("batch", 4, rnn, [0.3], [0.0], True, {})]
    with pytest.raises(NotImplementedError):          # a masked LM has no next-token distribution, whatever the switch says
        dec.decode(one, [3], beam_width=4, lm=SimpleNamespace(lm_type="bert"), lm_weight=0.3)
    dec.rnnt_beam_impl = "host"
    for value in ("gpu", None, "Device"):
        dec.rnnt_tlm_fusion = value
        with pytest.raises(ValueError, match="rnnt_tlm_fusion is 'host' or 'device'"):
            dec.decode(two, [3, 3], beam_width=4, lm=trf, lm_weight=0.3)


class _FakeEngine:
    """records the engine calls of the apply functions; the batch search takes exactly today's arguments unless told otherwise"""

    def __init__(self, why=None, tlm_why=None):
        self.calls, self.why, self.tlm_why = [], why, tlm_why

    def rnnt_beam_lm_why_not(self, lm):
        return self.why

    def rnnt_beam_tlm_why_not(self, lm):
        return self.tlm_why

    def rnnt_beam_device_ok(self, W, E=3, lm=None):
        return True

    def rnnt_beam_search_batch(self, eouts, elens, bw, blank, eos, num_expands=3, lm=None, lm_weights=None, len_weights=None, **kw):
        self.calls.append((list(elens), bw, blank, eos, lm, lm_weights, len_weights, kw))
        return "hyps", "scores"


def test_apply_functions_pass_the_switch_down(monkeypatch):
    from emoasr_amd.modeling import functions as fn
    eng = _FakeEngine(why="is not 'rnn'")
    monkeypatch.setattr(fn, "_engine_of", lambda dec: eng)
    dec = SimpleNamespace(blank_id=0, eos_id=2)
    trf, eouts = SimpleNamespace(lm_type="transformer"), torch.zeros(2, 3, 4)
    assert fn.rnnt_beam_batch_apply(dec, eouts, [3, 2], 4, trf, [0.3], [1.0]) == ("hyps", "scores")
    assert fn.rnnt_fusion_grid_apply(dec, eouts, [3, 2], 4, trf, [0.3, 0.0], [1.0]) == ("hyps", "scores")
    assert eng.calls == [([3, 2], 4, 0, 2, trf, [0.3], [1.0], {}), ([3, 2], 4, 0, 2, trf, [0.3, 0.0], [1.0], {})]          # today's calls
    with pytest.raises(ValueError, match="rnnt_beam_impl = 'device' cannot fuse this LM: is not 'rnn'"):
        fn.rnnt_beam_batch_apply(dec, eouts, [3, 2], 4, trf, [0.3], [1.0], require_device=True)
    del eng.calls[:]
    # "device": the keyword reaches the engine, and the RNN form's refusal does not stand in the way of a Transformer LM
    fn.rnnt_beam_batch_apply(dec, eouts, [3, 2], 4, trf, [0.3], [1.0], require_device=True, tlm_fusion="device")
    fn.rnnt_fusion_grid_apply(dec, eouts, [3, 2], 4, trf, [0.3], [1.0], tlm_fusion="device")
    assert [c[-1] for c in eng.calls] == [{"tlm_fusion": "device"}] * 2
    rnn = SimpleNamespace(lm_type="rnn")
    with pytest.raises(ValueError, match="rnnt_beam_impl = 'device' cannot fuse this LM"):
        fn.rnnt_beam_batch_apply(dec, eouts, [3, 2], 4, rnn, [0.3], [1.0], require_device=True, tlm_fusion="device")
    for value in ("gpu", None):
        with pytest.raises(ValueError, match="rnnt_tlm_fusion is 'host' or 'device'"):
            fn.rnnt_beam_batch_apply(dec, eouts, [3, 2], 4, trf, [0.3], [1.0], tlm_fusion=value)
    assert fn.rnnt_tlm_fusion_of(SimpleNamespace()) == "host" and fn.rnnt_tlm_fusion_of(SimpleNamespace(rnnt_tlm_fusion="device")) == "device"
    with pytest.raises(ValueError, match="rnnt_tlm_fusion"):
        fn.rnnt_tlm_fusion_of(SimpleNamespace(rnnt_tlm_fusion="both"))


def test_engine_refuses_by_name_under_device(monkeypatch):
    """rnnt_beam_search_batch(tlm_fusion="device") with an LM outside the plan: a ValueError carrying rnnt_beam_tlm_why_not's reason,
    before any search; a bad value of the switch is a ValueError too"""
    Eng, eng = _engine()
    eng._scope = lambda: __import__("contextlib").nullcontext()
    eng.arena.refresh_shadow = lambda: None
    eng.rnnt_beam_tlm_why_not = lambda lm: Eng.rnnt_beam_tlm_why_not(eng, lm)
    eng.rnnt_beam_device_ok = lambda W, E=3, lm=None: True
    eng._rnnt_beam_search_grid = lambda *a: Eng._rnnt_beam_search_grid(eng, *a)
    eouts = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="rnnt_tlm_fusion = 'device' cannot fuse this LM: the LM's heads"):
        Eng.rnnt_beam_search_batch(eng, eouts, [3, 2], 4, 0, 2, lm=_tlm(num_attention_heads=32), lm_weights=[0.3], tlm_fusion="device")
    with pytest.raises(ValueError, match="vocabulary"):
        Eng.rnnt_beam_search_batch(eng, eouts, [3, 2], 4, 0, 2, lm=_tlm(vocab_size=12), lm_weights=[0.0, 0.3], tlm_fusion="device")
    with pytest.raises(ValueError, match="rnnt_tlm_fusion is 'host' or 'device'"):
        Eng.rnnt_beam_search_batch(eng, eouts, [3, 2], 4, 0, 2, tlm_fusion="gpu")


def test_grid_tool_sets_the_switch_and_logs_the_reason(monkeypatch, caplog):
    import logging

    from emoasr_amd import fusion_grid as fg
    from emoasr_amd.modeling import functions as fn
    dec = SimpleNamespace(rnnt_tlm_fusion="host")
    monkeypatch.setattr(fn, "_engine_of", lambda d: _FakeEngine())
    assert fg.set_rnnt_tlm_fusion(dec, 4, _tlm()) == "device" and dec.rnnt_tlm_fusion == "device"
    assert fg.set_rnnt_tlm_fusion(dec, 4, SimpleNamespace(lm_type="rnn")) == "host" and dec.rnnt_tlm_fusion == "host"
    monkeypatch.setattr(fn, "_engine_of", lambda d: _FakeEngine(tlm_why="the LM's heads are too wide"))
    dec.rnnt_tlm_fusion = "device"
    with caplog.at_level(logging.INFO):
        assert fg.set_rnnt_tlm_fusion(dec, 4, _tlm()) == "host" and dec.rnnt_tlm_fusion == "host"
    assert "rnnt_tlm_fusion stays 'host'" in caplog.text and "heads are too wide" in caplog.text
    # the grid function hands the switch to the apply function only when it is set
    seen = []
    monkeypatch.setattr(fn, "rnnt_fusion_grid_apply", lambda d, e, el, bw, lm, a, b, **kw: seen.append(kw) or ([[[[2]]] * 2] * len(e), None))
    for value, want in (("host", {}), ("device", {"tlm_fusion": "device"})):
        model = SimpleNamespace(decoder_type="rnn_transducer", decoder=SimpleNamespace(rnnt_tlm_fusion=value),
                                encoder=lambda xs, xlens: (xs, xlens, None))
        model.decoder.decode = lambda *a, **k: None
        loader = [{"xs": torch.zeros(1, 3, 4), "xlens": [3], "texts": ["w2"]}]
        fg.rnnt_fusion_grid(model, loader, SimpleNamespace(ids2text=lambda ids: " ".join(f"w{i}" for i in ids)), 4, "lm", [0.5], [0.0, 1.0],
                            None)
        assert seen[-1] == want


# ---- the gap condition of the end-to-end cases ------------------------------------------------------------------------------------------
def test_gap_condition_of_the_end_to_end_cases():
    """tests/rnnt_fusion_ref.search with the oracle transducer on the oracle's encoder outputs of l4_tiny and oracle.decoder.lm_predict
    as the LM: at most 10 % of the eight cases have a cut closer than GAP_TOL, fusion changes at least two results, the longest
    hypothesis is short (tree depth is the kernel tests' job)"""
    from oracle import model as om
    cfg, sd, g = load_golden("l4_tiny")
    lm_sd = {k: v.float() for k, v in load_ctc_beam_golden()[2].items()}
    with torch.no_grad():
        outs = []
        for b in range(2):
            n = int(g["xlens"][b])
            e, el = om.encoder_forward(sd, cfg, g["xs"][b:b + 1, :n], g["xlens"][b:b + 1])
            assert int(el[0]) >= T.ELENS[b]
            outs.append(e[0, :T.ELENS[0]])
    cases = T.gap_cases(sd, cfg, lm_sd, SimpleNamespace(**LM_CFG), torch.stack(outs).float())
    assert len(cases) == 8
    for key, (gap, hyps, plain) in sorted(cases.items()):
        print(f"b={key[0]} W={key[1]} mu={key[2]}: min gap {gap:.3g}, longest {max(map(len, hyps))}, moved {hyps != plain}")
    close = [k for k, v in cases.items() if v[0] <= F.GAP_TOL]
    assert len(close) <= len(cases) // 10, close
    assert sum(int(v[1] != v[2]) for v in cases.values()) >= 2
    assert max(len(h) for v in cases.values() for h in v[1]) <= 1 + 2 * T.ELENS[0]
