"""The RNN LM in the batched joint CTC / attention search without a GPU: the header / binding tables, the
routing of TransformerDecoder.decode, joint_beam_search_batch and joint_beam_search_device_grid under both values of
decoder.joint_rnnlm_impl, and every reason of batch_rnnlm_why_not."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["emoasr_rnnlm_step_rows", "emoasr_joint_beam_batch_step_rnnlm", "emoasr_joint_beam_grid_step_rnnlm"]


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
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES, name
        assert hasattr(lib.load(), name), name
    assert re.search(r"\bint\s+emoasr_rnnlm_step_rows_supported\s*\(", header)
    assert re.search(r"\blong\s+emoasr_rnnlm_step_rows_ws_bytes\s*\(", header)
    want = ["L", "E", "H", "V", "R", "emb", "w_ih", "w_hh", "bias", "w_out", "b_out", "ph", "pc", "slots", "src_base", "dst_base",
            "logits", "ldl", "ws", "ws_bytes"]
    assert _struct_fields(header, "emoasr_rnnlm_rows_t") == want
    assert [f[0] for f in lib.RnnlmRows._fields_] == want
    P = ctypes.POINTER
    assert lib.SIGNATURES["emoasr_joint_beam_batch_step_rnnlm"][1:3] == [P(lib.JointBatchStep), P(lib.RnnlmRows)]
    assert lib.SIGNATURES["emoasr_joint_beam_grid_step_rnnlm"][1:3] == [P(lib.JointGridStep), P(lib.RnnlmRows)]
    # the existing structs keep their layout
    assert _struct_fields(header, "emoasr_joint_grid_step_t") == [f[0] for f in lib.JointGridStep._fields_]
    assert _struct_fields(header, "emoasr_joint_batch_step_t") == [f[0] for f in lib.JointBatchStep._fields_]


def test_shape_plan_and_workspace_queries():
    from emoasr_amd import lib
    q = lambda *a: lib.size_query("emoasr_rnnlm_step_rows_supported", *a)
    for code in (lib.F32, lib.BF16, lib.F32X3):
        assert q(code, 2, 512, 512) == 1 and q(code, 2, 48, 64) == 1
        assert q(code, 2, 512, 512) == lib.size_query("emoasr_rnnlm_step_supported", code, 32, 2, 512, 512)
    assert q(lib.BF16, 2, 36, 64) == 0 and q(lib.F32, 2, 64, 36) == 0 and q(lib.F32, 0, 64, 64) == 0 and q(7, 2, 64, 64) == 0
    ws = lambda *a: lib.size_query("emoasr_rnnlm_step_rows_ws_bytes", *a)
    assert ws(lib.F32, 70, 64) >= 70 * 64 * 4 and ws(lib.BF16, 70, 64) >= 70 * 64 * 2 and ws(lib.F32X3, 1, 8) >= 32
    assert ws(lib.BF16, 640, 512) < 2 * 640 * 512 * 2


# ------------------------------------------------------------------------------------------------ routing
class _LMNext:          # a next-token Transformer LM as far as the routing looks
    stateful = False

    def predict_device(self, *a):
        raise AssertionError("not called")


def _rnnlm(dtype=torch.float32, **over):
    """the RNN LM as far as the routing and batch_rnnlm_why_not look"""
    lm = SimpleNamespace(lm_type="rnn", stateful=True, V=40, E=48, H=64, L=2, compute_dtype=dtype, f32_split=False)
    for k, v in over.items():
        setattr(lm, k, v)
    return lm


def _decoder(vocab=40, dtype=torch.float32, split=False):
    from emoasr_amd.modeling.decoders.transformer import TransformerDecoder
    p = SimpleNamespace(vocab_size=vocab, dec_hidden_size=8, dec_num_layers=1, dec_num_attention_heads=2, dec_intermediate_size=16,
                        mtl_ctc_weight=0.0, kd_weight=0, blank_id=0, eos_id=2, max_decode_ylen=5)
    dec = TransformerDecoder(p)
    eng = SimpleNamespace(dtype=dtype, split=split, dnl=1, dd=8)
    dec._owner = [SimpleNamespace(engine=lambda: eng)]
    return dec


@pytest.fixture
def routed(monkeypatch):
    """the searches replaced by recorders that return recognisable results"""
    from emoasr_amd.modeling import beam_search as bs
    from emoasr_amd.modeling import beam_search_device as bsd
    calls = []

    def single(dec, eouts, elens, bw, *a, **k):
        calls.append(("single", tuple(eouts.shape), [int(n) for n in elens]))
        return [[7, int(eouts.shape[1])]] * min(bw, 2), [-1.0, -2.0][:min(bw, 2)], None, None

    def batch(dec, eouts, elens, bw, *a, **k):
        calls.append(("batch", tuple(eouts.shape), [int(n) for n in elens]))
        hyps = [[[7, int(n)]] * min(bw, 2) for n in elens]
        return hyps, [[-1.0, -2.0][:len(h)] for h in hyps], None, None

    def chunk(dec, eng, eouts, elens, bw, len_weight, lm, lm_weight, ctc_weight, grid=None, sort=True):
        calls.append(("chunk", [int(n) for n in elens], None if lm is None else "lm", None if grid is None else (list(grid[0]), list(grid[1]))))
        S = len(grid[0]) if grid else len(elens)
        return [[[7, s]] for s in range(S)], [[-1.0 - s] for s in range(S)]

    monkeypatch.setattr(bs, "joint_beam_search", single)
    monkeypatch.setattr(bsd, "joint_beam_search_device_batch", batch)
    monkeypatch.setattr(bsd, "_batch_search_chunk", chunk)
    monkeypatch.delenv("EMOASR_DEVICE_BEAM", raising=False)
    monkeypatch.delenv("EMOASR_CPP_DECODE", raising=False)
    return calls


def test_default_is_host_and_a_bad_value_raises(routed):
    dec = _decoder()
    assert dec.joint_rnnlm_impl == "host"
    three = torch.zeros(3, 9, 8)
    dec.joint_rnnlm_impl = "gpu"
    with pytest.raises(ValueError, match="joint_rnnlm_impl"):
        dec.decode(three, [9, 4, 2], beam_width=4)
    with pytest.raises(ValueError, match="joint_rnnlm_impl"):
        dec.decode(three[:1], [9], beam_width=4, lm=_rnnlm(), lm_weight=0.3)
    from emoasr_amd.modeling import beam_search_device as bsd
    with pytest.raises(ValueError, match="joint_rnnlm_impl"):
        bsd.batch_device_ok(dec, 4, _rnnlm(), 0.3, 0.0)
    assert routed == []


def test_routing_of_decode_under_both_values(routed):
    dec = _decoder()
    one, three = torch.zeros(1, 9, 8), torch.zeros(3, 9, 8)
    kw = dict(beam_width=4, lm=_rnnlm(), lm_weight=0.3, decode_ctc_weight=0.3)
    # "host": one single search per utterance, as before the switch existed
    h, s, _, _ = dec.decode(three, [9, 4, 2], **kw)
    assert routed == [("single", (1, 9, 8), [9]), ("single", (1, 4, 8), [4]), ("single", (1, 2, 8), [2])]
    assert h == [[[7, 9], [7, 9]], [[7, 4], [7, 4]], [[7, 2], [7, 2]]] and s == [[-1.0, -2.0]] * 3
    # "device": the batched device search, lists per utterance
    routed.clear()
    dec.joint_rnnlm_impl = "device"
    h, s, _, _ = dec.decode(three, [9, 4, 2], **kw)
    assert routed == [("batch", (3, 9, 8), [9, 4, 2])]
    assert h == [[[7, 9], [7, 9]], [[7, 4], [7, 4]], [[7, 2], [7, 2]]] and s == [[-1.0, -2.0]] * 3
    # one utterance: the single search unless joint_beam_impl = "batch"; then the batched search, the single search's return shape
    routed.clear()
    h, s, _, _ = dec.decode(one, [9], **kw)
    assert routed == [("single", (1, 9, 8), [9])]
    routed.clear()
    dec.joint_beam_impl = "batch"
    h, s, _, _ = dec.decode(one, [9], **kw)
    assert routed == [("batch", (1, 9, 8), [9])] and h == [[7, 9], [7, 9]] and s == [-1.0, -2.0]
    dec.joint_rnnlm_impl = "host"
    routed.clear()
    h, s, _, _ = dec.decode(one, [9], **kw)
    assert routed == [("single", (1, 9, 8), [9])] and h == [[7, 9], [7, 9]]
    dec.joint_beam_impl = "single"
    # a Transformer LM is not touched by the switch; neither is an LM weight of zero
    for impl in ("host", "device"):
        dec.joint_rnnlm_impl = impl
        routed.clear()
        dec.decode(three, [9, 4, 2], beam_width=4, lm=_LMNext(), lm_weight=0.3)
        dec.decode(three, [9, 4, 2], beam_width=4, lm=_rnnlm(V=99), lm_weight=0.0)
        dec.decode(three, [9, 4, 2], beam_width=33, lm=_LMNext(), lm_weight=0.3)      # (the quiet fallback of a Transformer LM stays)
        assert [c[0] for c in routed] == ["batch", "batch", "single", "single", "single"], (impl, routed)


def test_device_refuses_by_name_and_never_detours(routed, monkeypatch):
    from emoasr_amd.modeling import beam_search as bs
    from emoasr_amd.modeling import beam_search_device as bsd
    dec = _decoder()
    dec.joint_rnnlm_impl = "device"
    three = torch.zeros(3, 9, 8)
    for kw, what in ((dict(beam_width=33, lm=_rnnlm()), "beam_width 33"), (dict(beam_width=22, lm=_rnnlm(), decode_ctc_weight=0.3), "candidate width 33"),
                     (dict(beam_width=4, lm=_rnnlm(V=48)), "vocabulary"), (dict(beam_width=4, lm=_rnnlm(torch.bfloat16)), "computes in")):
        with pytest.raises(ValueError, match="joint_rnnlm_impl = 'device' cannot fuse this LM.*" + what):
            dec.decode(three, [9, 4, 2], lm_weight=0.3, **kw)
        with pytest.raises(ValueError, match=what):
            bs.joint_beam_search_batch(dec, three, [9, 4, 2], kw["beam_width"], 0, kw["lm"], 0.3, kw.get("decode_ctc_weight", 0))
        with pytest.raises(ValueError, match=what):
            bsd.joint_beam_search_device_grid(dec, three, [9, 4, 2], kw["beam_width"], kw["lm"], [0.0, 0.3], [0.0], kw.get("decode_ctc_weight", 0))
    monkeypatch.setenv("EMOASR_DEVICE_BEAM", "0")
    with pytest.raises(ValueError, match="EMOASR_DEVICE_BEAM=0"):
        dec.decode(three, [9, 4, 2], beam_width=4, lm=_rnnlm(), lm_weight=0.3)
    assert routed == []
    # "host" with the same configurations: the quiet per-utterance search, as before
    dec.joint_rnnlm_impl = "host"
    dec.decode(three, [9, 4, 2], beam_width=4, lm=_rnnlm(V=48), lm_weight=0.3)
    assert [c[0] for c in routed] == ["single"] * 3


def test_routing_of_the_grid_under_both_values(routed):
    from emoasr_amd.modeling import beam_search_device as bsd
    dec = _decoder()
    three = torch.zeros(3, 9, 8)
    lm = _rnnlm()
    # "host": one joint_beam_search_batch per distinct weight, each one single search per utterance
    hyps, scores = bsd.joint_beam_search_device_grid(dec, three, [9, 4, 2], 4, lm, [0.0, 0.3, 0.5], [0.0, 1.0], 0.3)
    assert [c[0] for c in routed] == ["batch"] + ["single"] * 6       # (weight 0: no LM in the way, the batched search)
    assert len(hyps) == 3 and len(hyps[0]) == 6
    # "device": the search without the LM once, every positive weight as a search of ONE grid chunk over shared frames
    routed.clear()
    dec.joint_rnnlm_impl = "device"
    hyps, scores = bsd.joint_beam_search_device_grid(dec, three, [9, 4, 2], 4, lm, [0.0, 0.3, 0.5, -1.0, 0.3], [0.0, 1.0], 0.3)
    assert routed == [("chunk", [9, 4, 2], None, None), ("chunk", [9, 4, 2], "lm", ([0, 0, 1, 1, 2, 2], [0.3, 0.5] * 3))], routed
    assert len(hyps) == 3 and all(len(h) == 10 for h in hyps)
    for b in range(3):      # cells: lm_weight outer, len_weight inner; the searches' results by weight, len_weight * (len + 2) added
        assert hyps[b][0] == hyps[b][6] == [[7, b]] and hyps[b][2] == hyps[b][8] == [[7, 2 * b]] and hyps[b][4] == [[7, 2 * b + 1]]
        assert scores[b][2] == [-1.0 - 2 * b] and scores[b][3] == [-1.0 - 2 * b + 1.0 * 4]


# ------------------------------------------------------------------------------------------------ the reasons
def test_every_reason_of_batch_rnnlm_why_not(monkeypatch):
    from emoasr_amd.modeling import beam_search_device as bsd
    monkeypatch.delenv("EMOASR_DEVICE_BEAM", raising=False)
    monkeypatch.delenv("EMOASR_CPP_DECODE", raising=False)
    dec = _decoder()
    why = lambda lm, bw=4, ctc=0.3, d=dec: bsd.batch_rnnlm_why_not(d, bw, lm, ctc)
    assert why(_rnnlm()) is None
    assert why(_rnnlm(), 32, 0.0) is None and why(_rnnlm(), 21, 0.3) is None
    assert why(_rnnlm(torch.bfloat16, E=64), d=_decoder(dtype=torch.bfloat16)) is None
    assert why(_rnnlm(f32_split=True), d=_decoder(split=True)) is None
    assert "lm_type" in why(_LMNext()) and "lm_type 'transformer'" in why(SimpleNamespace(lm_type="transformer"))
    assert "vocabulary (48)" in why(_rnnlm(V=48)) and "vocabulary (32)" in why(_rnnlm(V=32))
    assert "computes in" in why(_rnnlm(torch.bfloat16)) and "computes in" in why(_rnnlm(), d=_decoder(dtype=torch.bfloat16))
    assert "split products" in why(_rnnlm(f32_split=True)) and "split products" in why(_rnnlm(), d=_decoder(split=True))
    assert "shape plan" in why(_rnnlm(E=50)) and "shape plan" in why(_rnnlm(H=36)) and "shape plan" in why(_rnnlm(L=0))
    assert "shape plan" in why(_rnnlm(torch.bfloat16, E=36), d=_decoder(dtype=torch.bfloat16))
    assert "beam_width 33" in why(_rnnlm(), 33, 0.0) and "candidate width 33" in why(_rnnlm(), 22, 0.3)
    assert "beam_width 12" in why(_rnnlm(V=10), 12, 0.0, _decoder(vocab=10))          # more beams than tokens
    for env in ("EMOASR_DEVICE_BEAM", "EMOASR_CPP_DECODE"):
        monkeypatch.setenv(env, "0")
        assert env + "=0" in why(_rnnlm())
        monkeypatch.delenv(env)
    assert why(_rnnlm()) is None


def test_the_grid_tool_sets_the_switch(monkeypatch, caplog):
    import logging
    from emoasr_amd import fusion_grid as fg
    monkeypatch.delenv("EMOASR_DEVICE_BEAM", raising=False)
    monkeypatch.delenv("EMOASR_CPP_DECODE", raising=False)
    dec = _decoder()
    assert fg.set_joint_rnnlm_impl(dec, 10, _rnnlm(), 0.3) == "device" and dec.joint_rnnlm_impl == "device"
    assert fg.set_joint_rnnlm_impl(dec, 10, _LMNext(), 0.3) == "host" and dec.joint_rnnlm_impl == "host"
    with caplog.at_level(logging.INFO):
        assert fg.set_joint_rnnlm_impl(dec, 10, _rnnlm(V=48), 0.3) == "host" and dec.joint_rnnlm_impl == "host"
    assert any("vocabulary (48)" in r.getMessage() for r in caplog.records)
