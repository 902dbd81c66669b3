"""The batched joint CTC / attention beam search without a GPU: the numpy restatement of the batched update against the oracle's
search, the header / binding tables, the routing of TransformerDecoder.decode and the chunk capacity."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import joint_beam_ref as ref
from tests.util import DECODE_SETTINGS, LM_CFG, load_golden, lm_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["emoasr_attn_step_group", "emoasr_group_offsets_check", "emoasr_beam_update_batch",
                    "emoasr_ctc_prefix_init_ragged", "emoasr_ctc_prefix_score_ragged", "emoasr_transformer_decoder_step_group",
                    "emoasr_joint_beam_batch_step"]


# ------------------------------------------------------------------------------------------------ the update against the oracle
def _oracle_tables(sd, cfg, lm, eouts, hyp, ctc, W, cw, lm_weight):
    """the candidate table of ONE hypothesis as oracle/decoder.py:joint_beam_search computes it: (vals, cands, psi, lm_at, states)"""
    from oracle import decoder as od
    V = cfg.vocab_size
    ys_in, ylens_in = torch.tensor([hyp]), torch.tensor([len(hyp)])
    scores = torch.log_softmax(od.forward_one_step(sd, cfg, ys_in, ylens_in, eouts), -1)
    lm_lp = None
    if lm_weight > 0:
        lm_lp = od.lm_predict(lm[0], lm[1], ys_in, ylens_in)[:, :V]
        scores = scores + lm_weight * lm_lp
    vals, idx = torch.topk(scores, k=cw, dim=1)
    psi = states = lm_at = None
    if ctc is not None:
        scorer, state = ctc
        psi, states = scorer(hyp, idx[0].numpy(), state)
        if lm_lp is not None:
            lm_at = lm_lp[0, idx[0]].numpy()
    return vals[0].numpy(), idx[0].numpy().astype(np.int32), psi, lm_at, states


@pytest.mark.parametrize("si", range(len(DECODE_SETTINGS)))
def test_reference_update_reproduces_the_oracle_search(si):
    """both golden utterances as ONE batch of two searches (they finish at different steps): joint_beam_ref.update driven with
    the oracle's candidate tables gives oracle/decoder.py:joint_beam_search's hypotheses and scores"""
    from oracle import decoder as od
    from oracle import model as om
    cfg, sd, g = load_golden("l3_tiny")
    lm = (lm_state(g), SimpleNamespace(**LM_CFG))
    st_ = DECODE_SETTINGS[si]
    W, lw, mu, lam = st_["beam_width"], st_["len_weight"], st_["lm_weight"], st_["decode_ctc_weight"]
    V, eos, blank = cfg.vocab_size, cfg.eos_id, cfg.blank_id
    cw = min(V, int(W * 1.5)) if lam > 0 else W
    S = 2
    with torch.no_grad():
        enc, want = [], []
        for b in range(S):
            n = int(g["xlens"][b])
            eouts, elens = om.encoder_forward(sd, cfg, g["xs"][b:b + 1, :n], g["xlens"][b:b + 1])
            enc.append(eouts)
            want.append(od.joint_beam_search(sd, cfg, eouts, elens, W, lw, lm, mu, lam))
        scorers = [None] * S
        if lam > 0:
            for b in range(S):
                x = torch.log_softmax(od.linear(sd, "decoder.ctc.output", enc[b]), -1)[0].numpy()
                scorers[b] = od.CTCPrefixScorer(x, blank, eos)
        st = ref.new_state(S, W, cfg.max_decode_ylen, eos)
        hyps = [[[eos]] for _ in range(S)]                                       # the live hypotheses of every search, by slot
        cstates = [[sc.initial_state() if sc is not None else None] for sc in scorers]
        for _ in range(cfg.max_decode_ylen):
            nb = S * W
            vals, cands = np.zeros((nb, cw), np.float32), np.zeros((nb, cw), np.int32)
            psi = np.zeros((nb, cw), np.float32) if lam > 0 else None
            lm_at = np.zeros((nb, cw), np.float32) if (lam > 0 and mu > 0) else None
            new_states = [[None] * W for _ in range(S)]
            for s in range(S):
                if st["state"][s, 3]:
                    continue
                for m in range(int(st["state"][s, 1])):
                    ctc = (scorers[s], cstates[s][m]) if lam > 0 else None
                    v, c, p, la, ns = _oracle_tables(sd, cfg, lm, enc[s], hyps[s][m], ctc, W, cw, mu)
                    vals[s * W + m], cands[s * W + m] = v, c
                    if psi is not None:
                        psi[s * W + m] = p
                    if lm_at is not None:
                        lm_at[s * W + m] = la
                    new_states[s][m] = ns
            live = [not st["state"][s, 3] for s in range(S)]
            ref.update(st, vals, cands, psi, lm_at, cw, eos, lam, mu, lw)
            for s in range(S):
                if not live[s]:
                    continue
                nh, nc = [], []
                for a in range(int(st["state"][s, 1])):
                    par = int(st["parent"][s * W + a]) - s * W
                    nh.append(hyps[s][par] + [int(st["ids"][s * W + a])])
                    nc.append(new_states[s][par][int(st["pcand"][s * W + a])] if lam > 0 else None)
                hyps[s], cstates[s] = nh, nc
            if st["all_done"]:
                break
    got_h, got_s = ref.results(st)
    for b in range(S):
        assert got_h[b] == want[b][0], (si, b, got_h[b], want[b][0])
        assert np.allclose(got_s[b], want[b][1], rtol=0, atol=1e-4), (si, b, got_s[b], want[b][1])
    assert st["pos"] == st["mirror"][0] and st["mirror"][1] == S


def test_reference_update_replay_after_the_end_changes_nothing():
    eos, W, cw = 2, 2, 2
    st = ref.new_state(1, W, 8, eos)
    vals = np.array([[0.0, -1.0], [0.0, 0.0]], np.float32)
    cands = np.array([[5, eos], [0, 0]], np.int32)
    ref.update(st, vals, cands, None, None, cw, eos, 0.0, 0.0, 0.0)
    assert st["state"][0].tolist() == [1, 1, 0, 0]          # <eos> at position 0: an empty hypothesis, dropped
    cands = np.array([[eos, 7], [0, 0]], np.int32)
    ref.update(st, vals, cands, None, None, cw, eos, 0.0, 0.0, 0.5)
    ref.update(st, np.array([[0.0, -1.0], [0.0, 0.0]], np.float32), np.array([[eos, eos], [0, 0]], np.int32), None, None, cw, eos,
               0.0, 0.0, 0.5)
    assert st["all_done"] == 1 and st["pos"] == 3
    snap = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    ref.update(st, vals, cands, None, None, cw, eos, 0.0, 0.0, 0.5)
    for k, v in snap.items():
        assert np.array_equal(st[k], v), k
    h, s = ref.results(st)
    assert h == [[[5], [5, 7]]] and s[0][0] == 0.5 * 3 and s[0][1] == 0.5 * 4 - 1.0


# ------------------------------------------------------------------------------------------------ header and bindings
def test_new_entry_points_are_declared_and_bound():
    from emoasr_amd import lib
    header = open(os.path.join(ROOT, "include", "emoasr_hip.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES, name
    assert re.search(r"size_t\s+emoasr_decode_step_group_ws_bytes\s*\(", header)
    for struct, mirror in (("emoasr_beam_update_batch_t", "BeamUpdateBatch"), ("emoasr_decoder_step_group_t", "DecoderStepGroup"),
                           ("emoasr_joint_batch_step_t", "JointBatchStep")):
        assert struct in header and hasattr(lib, mirror), struct
    # the existing structs keep their layout: the new ones embed them
    assert lib.BeamUpdateBatch._fields_[0] == ("u", lib.BeamUpdate)
    assert lib.DecoderStepGroup._fields_[0] == ("d", lib.DecoderStep)
    for src in ("decode_batch.hip",):
        from emoasr_amd import build
        assert src in build.SOURCES


# ------------------------------------------------------------------------------------------------ routing
class _LMNext:          # a next-token Transformer LM as far as the routing looks
    def predict_device(self, *a):
        raise AssertionError("not called")


class _LMStateful:      # the RNN LM: no predict_device
    stateful = True


def _decoder(vocab=40):
    from emoasr_amd.modeling.decoders.transformer import TransformerDecoder
    p = SimpleNamespace(vocab_size=vocab, dec_hidden_size=8, dec_num_layers=1, dec_num_attention_heads=2, dec_intermediate_size=16,
                        mtl_ctc_weight=0.0, kd_weight=0, blank_id=0, eos_id=2, max_decode_ylen=5)
    return TransformerDecoder(p)


@pytest.fixture
def routed(monkeypatch):
    """the three searches replaced by recorders that return recognisable results"""
    from emoasr_amd.modeling import beam_search as bs
    from emoasr_amd.modeling import beam_search_device as bsd
    calls = []

    def single(dec, eouts, elens, bw, *a, **k):
        calls.append(("single", tuple(eouts.shape), [int(n) for n in elens]))
        return [[7, int(eouts.shape[1])]] * min(bw, 2), [-1.0, -2.0][:min(bw, 2)], None, None

    def batch(dec, eouts, elens, bw, *a, **k):
        calls.append(("batch", tuple(eouts.shape), [int(n) for n in elens]))
        hyps = [[[7, int(n)]] * min(bw, 2) if n > 1 else [] for n in elens]
        return hyps, [[-1.0, -2.0][:len(h)] for h in hyps], None, None

    monkeypatch.setattr(bs, "joint_beam_search", single)
    monkeypatch.setattr(bsd, "joint_beam_search_device_batch", batch)
    monkeypatch.delenv("EMOASR_DEVICE_BEAM", raising=False)
    monkeypatch.delenv("EMOASR_CPP_DECODE", raising=False)
    return calls


def test_routing_single_batch_fallback(routed, monkeypatch):
    dec = _decoder()
    one, three = torch.zeros(1, 9, 8), torch.zeros(3, 9, 8)
    # one utterance: the single search, today's return value
    h, s, _, _ = dec.decode(one, [9], beam_width=4)
    assert routed == [("single", (1, 9, 8), [9])] and h == [[7, 9], [7, 9]] and s == [-1.0, -2.0]
    # ... unless joint_beam_impl = "batch": the batched search, the same return shape
    routed.clear()
    dec.joint_beam_impl = "batch"
    h, s, _, _ = dec.decode(one, [9], beam_width=4)
    assert routed == [("batch", (1, 9, 8), [9])] and h == [[7, 9], [7, 9]] and s == [-1.0, -2.0]
    dec.joint_beam_impl = "single"
    # several utterances, beam_width >= 2: the batched search, lists per utterance
    routed.clear()
    h, s, _, _ = dec.decode(three, [9, 4, 1], beam_width=4, lm=_LMNext(), lm_weight=0.3, decode_ctc_weight=0.3)
    assert routed == [("batch", (3, 9, 8), [9, 4, 1])]
    assert h == [[[7, 9], [7, 9]], [[7, 4], [7, 4]], []] and s == [[-1.0, -2.0], [-1.0, -2.0], []]
    # beam_width == 1 on a batch: one hypothesis (or none) per utterance
    routed.clear()
    h, s, _, _ = dec.decode(three, [9, 4, 1], beam_width=1)
    assert routed[0][0] == "batch" and h == [[7, 9], [7, 4], []] and s == [-1.0, -1.0, None]
    # the RNN LM, width 33, the host-bookkeeping switches: utterance by utterance through joint_beam_search, the same return shape
    for kw, env in ((dict(beam_width=4, lm=_LMStateful(), lm_weight=0.3), None), (dict(beam_width=33), None),
                    (dict(beam_width=22, decode_ctc_weight=0.3), None),              # candidate width 33
                    (dict(beam_width=4), "EMOASR_DEVICE_BEAM"), (dict(beam_width=4), "EMOASR_CPP_DECODE")):
        routed.clear()
        if env:
            monkeypatch.setenv(env, "0")
        h, s, _, _ = dec.decode(three, [9, 4, 2], **kw)
        if env:
            monkeypatch.delenv(env)
        assert routed == [("single", (1, 9, 8), [9]), ("single", (1, 4, 8), [4]), ("single", (1, 2, 8), [2])], (kw, env, routed)
        assert h == [[[7, 9], [7, 9]], [[7, 4], [7, 4]], [[7, 2], [7, 2]]] and s == [[-1.0, -2.0]] * 3
    # an LM weight of zero does not count as an RNN LM in the way
    routed.clear()
    dec.decode(three, [9, 4, 2], beam_width=4, lm=_LMStateful(), lm_weight=0.0)
    assert routed[0][0] == "batch"


def test_routing_refusals(routed):
    dec = _decoder()
    three = torch.zeros(3, 9, 8)
    with pytest.raises(ValueError, match="at least one"):
        dec.decode(three, [9, 0, 3], beam_width=4)
    with pytest.raises(ValueError, match="at least one"):
        dec.decode(three, [9, 0, 3], beam_width=33)          # the fallback refuses it as well
    assert routed == []
    dec.joint_beam_impl = "both"
    with pytest.raises(ValueError, match="joint_beam_impl"):
        dec.decode(three, [9, 4, 3], beam_width=4)

    class Masked:      # a masked LM is refused by require_next_token_lm as before
        lm_type = "bert"
    dec.joint_beam_impl = "single"
    with pytest.raises(NotImplementedError):
        dec.decode(three, [9, 4, 3], beam_width=4, lm=Masked(), lm_weight=0.3)
    assert routed == []


def test_ctc_weight_one_is_unchanged(routed, monkeypatch):
    dec = _decoder()
    seen = []
    dec.ctc = SimpleNamespace(decode=lambda eouts, elens, beam_width: seen.append(beam_width) or "ctc", _owner=None)
    assert dec.decode(torch.zeros(3, 9, 8), [9, 4, 3], beam_width=4, decode_ctc_weight=1) == "ctc"
    assert seen == [1] and routed == []


# ------------------------------------------------------------------------------------------------ chunk capacity
def test_chunk_capacity_keeps_to_its_two_bounds():
    from emoasr_amd.modeling import beam_search_device as bsd
    for W in (1, 3, 4, 10, 32):
        for Lmax in (21, 101, 257):
            for (dnl, dd, lnl, ld) in ((2, 128, 0, 0), (6, 256, 12, 512), (6, 512, 12, 768)):
                for esz in (2, 4):
                    for budget in (None, 1 << 20, 1 << 28):
                        cap = bsd.batch_chunk_capacity(W, Lmax, dnl, dd, lnl, ld, esz, budget)
                        b = bsd.CACHE_BUDGET_BYTES if budget is None else budget
                        assert cap >= 1
                        assert cap * W <= bsd.MAX_ROWS
                        one = bsd.batch_cache_bytes(W, Lmax, dnl, dd, lnl, ld, esz)
                        assert one == 2 * 2 * W * Lmax * (dnl * dd + lnl * ld) * esz
                        assert cap == 1 or bsd.batch_cache_bytes(cap * W, Lmax, dnl, dd, lnl, ld, esz) <= b
                        # and it is the largest such number
                        more = cap + 1
                        assert more * W > bsd.MAX_ROWS or bsd.batch_cache_bytes(more * W, Lmax, dnl, dd, lnl, ld, esz) > b
    assert bsd.MAX_ROWS == 1024
